"""`Swing` (`libreco/algorithms/swing.py`, engine `rust/src/swing.rs`, `graph.rs`, `inference.rs`): the item-to-item
scores of the Swing graph algorithm on the device (csrc/swing.hip), ranked by the ItemCF kernels (csrc/cf_rank.hip).  After
`fit` the model is an item x item score CSR used like ItemCF's similarity, so it shares `CfBase`'s device CSRs, top-k view,
consumed-CSR plumbing and recommend batching.

Deliberate differences from the reference:
  (a) ties in a row and in the recommendations are broken by ascending item id (the reference's unstable sorts leave them
      arbitrary);
  (b) `max_cache_num` and `num_threads` are accepted and ignored;
  (c) a checkpoint is `*_hyper_parameters.json` plus three npz files (scores, user and item interactions), not the
      reference's bincode dump `model_name.gz`;
  (d) `predict` returns a float for one pair and an ndarray for several;
  (e) the scores are summed in a fixed order of their own, within (P + 16) * 2^-24 relative of the exact sum of P pairs.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch
from scipy.sparse import load_npz as load_sparse
from scipy.sparse import save_npz as save_sparse

from .. import ops
from ..bases.base import hip_device
from ..bases.cf_base import CfBase, _DeviceCsr, _resized, merge_interactions  # noqa: F401  (both are this module's names too)
from ..evaluation.evaluate import print_metrics
from ..recommendation import popular_recommendations
from ..utils.misc import time_block
from ..utils.validate import check_fitting


class Swing(CfBase):
    _warn_all_consumed = False

    def __init__(self, task, data_info, top_k=20, alpha=1.0, max_cache_num=100_000_000, num_threads=1, seed=42):
        assert task == "ranking", "`Swing` is only suitable for ranking task."
        super().__init__(task, data_info, "item_cf", k_sim=top_k, num_threads=num_threads, seed=seed)
        self.all_args = locals()
        self.top_k = top_k
        self.alpha = alpha
        self.max_cache_num = max_cache_num
        self.incremental = False
        self._topk_csr = None

    swing_scores = CfBase.sim_matrix

    def _set(self, name, m):
        super()._set(name, m)
        if name == "sim":
            self._topk_csr = None

    def _predict_rows(self):
        return "user", False

    # ---- fit -----------------------------------------------------------------------------------------------------
    def fit(self, train_data, neg_sampling, verbose=1, eval_data=None, metrics=None, k=10, eval_batch_size=8192,
            eval_user_num=None):
        check_fitting(self, train_data, eval_data, neg_sampling, k)
        from .. import distributed as D

        if D.active() is not None:
            raise RuntimeError(f"{self.model_name}: multi-GPU `fit` (torch.distributed is initialised with more than one "
                               "rank) is implemented for TwoTower, LightGCN, FM / DeepFM with plain sparse columns and DIN "
                               "on pure ids; run this model in a single process")
        self.show_start_time()
        dev = hip_device("cuda")
        user_host, user, item = self._interactions(train_data, dev)
        prev, old_user = None, None
        if self.incremental:
            # `update_swing`: the new interactions alone, every row starting from its previous scores
            assert self._host["sim"] is not None or self._dev["sim"] is not None
            p = self._device("sim")
            prev, old_user = (p.ptr, p.col, p.val), self.user_interaction
        with time_block("update swing" if self.incremental else "swing computing", verbose=1):
            ptr, col, val = ops.swing_scores(user.ptr, user.col, item.ptr, item.col, self.alpha, prev=prev)
            torch.cuda.synchronize(dev)
        if old_user is not None:
            merged = merge_interactions(_resized(old_user, user_host.shape), user_host, user_host.shape)
            self._set("user", merged)
            self._set("item", merged.T.tocsr())
        else:
            self._set("user", user_host)
            self._set("item", None)
            self._dev["user"], self._dev["item"] = user, item
        self._set("sim", None)
        self._dev["sim"] = _DeviceCsr(ptr, col, val, (self.n_items, self.n_items))
        self.topk_sim = None
        num = int(col.numel())
        density_ratio = 100 * num / (self.n_items * self.n_items)
        print(f"swing num_elements: {num}, density: {density_ratio:5.4f} %")
        if verbose > 1:
            print_metrics(model=self, neg_sampling=neg_sampling, eval_data=eval_data, metrics=metrics,
                          eval_batch_size=eval_batch_size, k=k, sample_user_num=eval_user_num, seed=self.seed)
            print("=" * 30)

    # ---- predict ---------------------------------------------------------------------------------------------------
    def _topk_rows(self):
        """The top-k lists as a CSR with ascending columns: Swing cuts a row to `top_k` before it intersects it with the
        user's items (`swing.rs:167-173`), so the CF predict kernel reads this instead of the full rows."""
        if self._topk_csr is None:
            ids, sims, lens = self._topk()
            n, kk = ids.shape
            dev = ids.device
            keep = torch.arange(kk, device=dev)[None, :] < lens[:, None]
            rows = torch.arange(n, device=dev)[:, None].expand(n, kk)[keep]
            order = torch.argsort(rows * max(self.n_items, 1) + ids[keep].to(torch.int64))
            ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            ptr[1:] = torch.cumsum(lens.to(torch.int64), 0)
            self._topk_csr = (ptr, ids[keep][order].contiguous(), sims[keep][order].contiguous())
        return self._topk_csr

    def predict(self, user, item, cold_start="popular", inner_id=False):
        user_arr, item_arr = self.pre_predict_check(user, item, inner_id, cold_start)
        user_arr = np.asarray(user_arr, dtype=np.int64)
        item_arr = np.asarray(item_arr, dtype=np.int64)
        preds = np.full(len(user_arr), self.default_pred, dtype=np.float32)
        known = np.flatnonzero((user_arr != self.n_users) & (item_arr != self.n_items))
        if len(known):
            ptr, col, val = self._topk_rows()
            inter = self._device("user")
            dev = ptr.device
            to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)  # noqa: E731
            # any stored label counts (`get_intersect_neighbors` ignores it for ranking): the kernel sees ones
            ones = torch.ones_like(inter.val)
            p, _ = ops.cf_predict(to(item_arr[known]), to(user_arr[known]), ptr, col, val, inter.ptr, inter.col, ones,
                                  max(int(self.top_k), 1), False, 0.0, 0.0, self.default_pred)
            preds[known] = p.cpu().numpy()
        return preds[0] if len(user_arr) == 1 else preds

    # ---- recommend -------------------------------------------------------------------------------------------------
    def _recommend_batch(self, user_ids, n_rec, filter_consumed, random_rec):
        recs = super()._recommend_batch(user_ids, n_rec, filter_consumed, random_rec)
        out = []
        for rec in recs:   # a short list is padded with popular items (`swing.py:150-155`)
            rec = np.asarray(rec, dtype=np.int64)
            if len(rec) < n_rec:
                extra = popular_recommendations(self.data_info, inner_id=True, n_rec=n_rec - len(rec))
                rec = np.concatenate([rec, np.asarray(extra, dtype=np.int64)])
            out.append(rec)
        return out

    # ---- persistence -----------------------------------------------------------------------------------------------
    def save(self, path, model_name, **kwargs):
        if not os.path.isdir(path):
            print(f"file folder {path} doesn't exists, creating a new one...")
            os.makedirs(path)
        with open(os.path.join(path, f"{model_name}_hyper_parameters.json"), "w") as f:
            json.dump(self._hparams(), f, separators=(",", ":"), indent=4)
        model_path = os.path.join(path, model_name)
        save_sparse(f"{model_path}_swing_scores", self.sim_matrix)
        save_sparse(f"{model_path}_user_inter", self.user_interaction)
        save_sparse(f"{model_path}_item_inter", self.item_interaction)

    def _load_matrices(self, path, model_name):
        if not os.path.exists(path):
            raise OSError(f"file folder {path} doesn't exists...")
        model_path = os.path.join(path, model_name)
        shape = (self.n_users, self.n_items)
        self.sim_matrix = _resized(load_sparse(f"{model_path}_swing_scores.npz"), (self.n_items, self.n_items))
        self.user_interaction = _resized(load_sparse(f"{model_path}_user_inter.npz"), shape)
        self.item_interaction = _resized(load_sparse(f"{model_path}_item_inter.npz"), shape[::-1])

    @classmethod
    def load(cls, path, model_name, data_info, **kwargs):
        if not os.path.exists(path):
            raise OSError(f"file folder {path} doesn't exists...")
        with open(os.path.join(path, f"{model_name}_hyper_parameters.json")) as f:
            hparams = json.load(f)
        model = cls(data_info=data_info, **hparams)
        model._load_matrices(path, model_name)
        model.loaded = True
        return model

    def rebuild_model(self, path, model_name):
        """Take the saved scores and interactions into this newly initialised model (whose `data_info` holds the merged
        ids and consumed items) before retraining on new data: the next `fit` adds the new data's scores to them."""
        self._load_matrices(path, model_name)
        self.incremental = True
