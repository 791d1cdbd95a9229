"""`RsCfBase` (`libreco/bases/cf_base_rs.py`, engine `rust/src/{item_cf,user_cf,similarities,incremental,inference}.rs`):
the neighbourhood models that can be retrained on new interactions alone, RsUserCF and RsItemCF.  Write `x` for the side
that gets similarities (items for RsItemCF, users for RsUserCF) and `y` for the other side; cosine is the only similarity.

The model keeps, on the device, what the Rust engine keeps: `sumsq` (f32 per x) and the pair state, a symmetric CSR of every
pair with a common y that carries the accumulated product `prod`, the count `cnt` and the cosine `sim` of the pair's last
refresh (csrc/cf_sim.hip, csrc/cf_state.hip).  `fit` is an update of the empty state, and `rebuild_model` followed by `fit`
on new interactions is an update of the saved one:

  1. `sumsq` is extended with zeros and every row's f32 sum of squares over the new data is added to it;
  2. the delta holds, for every pair that co-occurs in one y of the NEW data, the f32 sum of the products over ascending y
     and the count.  Old and new interactions of the same y are not crossed, and an interaction that reappears in the new
     data is counted again: both are what the reference does, and they are kept;
  3. a pair of the delta gets prod = old + delta, cnt = old + delta and sim = prod / (sqrt(sumsq[x1]) * sqrt(sumsq[x2])),
     0 if prod or either sum is 0;
  4. a pair that is not in the delta keeps its three values bit for bit, also when a `sumsq` of one of its rows has changed:
     this staleness is the reference's scheme, and what makes the update cheap;
  5. the interactions are merged, the new labels winning.

A pair is visible to ranking and prediction iff cnt >= min_common (counts only grow, so this is `sort_by_sims` /
`update_by_sims`); a visible pair may have sim 0 and is kept, unlike in UserCF / ItemCF.  A row's neighbour list is its
first `k_sim` visible entries by (sim descending, id ascending).  `predict` cuts the row to that list BEFORE it intersects
it with the other side's interaction row, uses every hit whatever its label, and clips nothing; the recommendation scores
are those of UserCF / ItemCF, a user without candidates gets the popular items without a warning, and short lists are not
padded.  The device CSRs, the top-k view, the consumed-CSR plumbing and the recommend batching are `CfBase`'s.

Deliberate differences from the reference (DESIGN, section "RsUserCF / RsItemCF"):
  (a) the pair state is keyed by the pair itself.  The reference keys it by `i32(x1 * n_x + x2)` with the current n_x, so
      after the id space has grown a pair's key names another pair's entry (and the key overflows from n_x = 46,341); the
      neighbour lists asserted by the Rust unit tests `test_*_cf_incremental_training` depend on that aliasing
      (tests/test_rs_cf_cpu.py shows both);
  (b) ties in a neighbour list and in the recommendations are broken by ascending id (the reference's unstable sorts leave
      them arbitrary);
  (c) `num_threads` and `mode` are accepted; `mode` is validated and both values give the same result;
  (d) `min_common` below 1 acts as 1;
  (e) a checkpoint is `*_hyper_parameters.json` plus three npz files (state, user and item interactions), not the
      reference's bincode dump `model_name.gz`;
  (f) `predict` returns a float for one pair and an ndarray for several;
  (g) under a process group of more than one rank `fit` raises, as `CfBase.fit` does.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch
from scipy.sparse import load_npz as load_sparse
from scipy.sparse import save_npz as save_sparse

from .. import ops
from ..evaluation.evaluate import print_metrics
from ..utils.misc import time_block
from ..utils.validate import check_fitting
from .base import hip_device
from .cf_base import CfBase, _DeviceCsr, _resized, merge_interactions

_STATE_KEYS = ("ptr", "col", "prod", "cnt", "sim")


class RsCfBase(CfBase):
    _warn_all_consumed = False
    _cf_type = None              # "user_cf" / "item_cf", set by the two models

    def __init__(self, task, data_info, k_sim=20, num_threads=1, min_common=1, mode="invert", seed=42,
                 lower_upper_bound=None):
        if mode not in ("forward", "invert"):
            raise ValueError("mode must either be 'forward' or 'invert'")
        super().__init__(task, data_info, self._cf_type, "cosine", k_sim, True, None, num_threads, min_common, mode, seed,
                         lower_upper_bound)
        self.incremental = False
        self._state = None       # ops.CfState on the device
        self._sumsq = None       # f32 [n_x] on the device
        self._state_host = None  # the same as numpy arrays, after `load` / `rebuild_model` until first use

    @property
    def n_x(self):
        return self.n_users if self.cf_type == "user_cf" else self.n_items

    def _predict_rows(self):
        return ("item", True) if self.cf_type == "user_cf" else ("user", False)

    # ---- the state -------------------------------------------------------------------------------------------------
    def _state_on(self, dev):
        """(state, sumsq) on the device, rows padded to this model's n_x."""
        if self._state is None:
            if self._state_host is None:
                raise RuntimeError(f"{self.model_name} has no similarity state: call `fit` or `load` first")
            h = self._state_host
            to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
            self._state = ops.CfState(*(to(h[k]) for k in _STATE_KEYS))
            self._sumsq = to(h["sumsq"])
            self._state_host = None
        return self._state, self._sumsq

    def _publish(self, state, sumsq):
        """Take a new state: the visible pairs become the `sim` matrix that `CfBase` ranks."""
        self._state, self._sumsq, self._state_host = state, sumsq, None
        n = state.ptr.numel() - 1
        self._set("sim", None)
        self._dev["sim"] = _DeviceCsr(*ops.cf_state_visible(state, self.min_common), (n, n))
        self.topk_sim = None

    def _device(self, name):
        if name == "sim" and self._dev["sim"] is None and self._host["sim"] is None:
            self._publish(*self._state_on(hip_device("cuda")))
        return super()._device(name)

    def _get(self, name):
        if name == "sim" and self._dev["sim"] is None and self._host["sim"] is None and \
                (self._state is not None or self._state_host is not None):
            self._device("sim")
        return super()._get(name)

    def pair_state(self):
        """The state as numpy arrays: `ptr`, `col`, `prod`, `cnt`, `sim` of the symmetric pair CSR and `sumsq`."""
        if self._state is None and self._state_host is not None:
            return dict(self._state_host)
        if self._state is None:
            raise RuntimeError(f"{self.model_name} has no similarity state: call `fit` or `load` first")
        out = {k: t.cpu().numpy() for k, t in zip(_STATE_KEYS, self._state)}
        out["sumsq"] = self._sumsq.cpu().numpy()
        return out

    # ---- fit -------------------------------------------------------------------------------------------------------
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
        X, Y = (user, item) if self.cf_type == "user_cf" else (item, user)
        n_x = X.shape[0]
        sumsq = torch.zeros(n_x, dtype=torch.float32, device=dev)
        old_user = None
        if self.incremental:
            old, old_sumsq = self._state_on(dev)
            sumsq[: old_sumsq.numel()] = old_sumsq
            old_user = self.user_interaction
        else:
            old = ops.cf_state_empty(n_x, dev)
        with time_block("update similarity" if self.incremental else "similarity", verbose=1):
            ops.cf_sumsq(X.ptr, X.val, out=sumsq)
            delta = ops.cf_pair_state(X.ptr, X.col, X.val, Y.ptr, Y.col, Y.val)
            state = ops.cf_state_update(old, delta, sumsq)
            torch.cuda.synchronize(dev)
        if old_user is not None:
            merged = merge_interactions(_resized(old_user, user_host.shape), user_host, user_host.shape)
            self._set("user", merged)
            self._set("item", merged.T.tocsr())
        else:
            self._set("user", user_host)
            self._set("item", None)
            self._dev["user"], self._dev["item"] = user, item
        self._publish(state, sumsq)
        self.compute_top_k()
        num = int(self._device("sim").col.numel())
        density_ratio = 100 * num / (n_x * n_x)
        print(f"similarity num_elements: {num}, density: {density_ratio:5.4f} %")
        if verbose > 1:
            print_metrics(model=self, neg_sampling=neg_sampling, eval_data=eval_data, metrics=metrics,
                          eval_batch_size=eval_batch_size, k=k, sample_user_num=eval_user_num, seed=self.seed)
            print("=" * 30)

    # ---- predict ---------------------------------------------------------------------------------------------------
    def predict(self, user, item, cold_start="popular", inner_id=False):
        user_arr, item_arr = self.pre_predict_check(user, item, inner_id, cold_start)
        user_arr = np.asarray(user_arr, dtype=np.int64)
        item_arr = np.asarray(item_arr, dtype=np.int64)
        preds = np.full(len(user_arr), self.default_pred, dtype=np.float32)
        known = np.flatnonzero((user_arr != self.n_users) & (item_arr != self.n_items))
        if len(known):
            ids, sims, lens = self._topk()
            inter_name, by_user = self._predict_rows()
            inter = self._device(inter_name)
            s_rows = user_arr[known] if by_user else item_arr[known]
            i_rows = item_arr[known] if by_user else user_arr[known]
            to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(ids.device)  # noqa: E731
            p, _ = ops.cf_predict_topk(to(s_rows), to(i_rows), ids, sims, lens, inter.ptr, inter.col, inter.val,
                                       max(int(self.k_sim), 1), self.task == "rating", self.default_pred)
            preds[known] = p.cpu().numpy()
        return preds[0] if len(user_arr) == 1 else preds

    # ---- persistence -----------------------------------------------------------------------------------------------
    def save(self, path, model_name, **kwargs):
        if not os.path.isdir(path):
            print(f"file folder {path} doesn't exists, creating a new one...")
            os.makedirs(path)
        with open(os.path.join(path, f"{model_name}_hyper_parameters.json"), "w") as f:
            json.dump(self._hparams(), f, separators=(",", ":"), indent=4)
        model_path = os.path.join(path, model_name)
        np.savez(f"{model_path}_cf_state.npz", **self.pair_state())
        save_sparse(f"{model_path}_user_inter", self.user_interaction)
        save_sparse(f"{model_path}_item_inter", self.item_interaction)

    def _load_state(self, path, model_name):
        """The saved state and interactions, resized to this model's `n_users` / `n_items` (new rows are empty)."""
        if not os.path.exists(path):
            raise OSError(f"file folder {path} doesn't exists...")
        model_path = os.path.join(path, model_name)
        with np.load(f"{model_path}_cf_state.npz") as z:
            h = {k: z[k] for k in (*_STATE_KEYS, "sumsq")}
        n_old, n_x = len(h["sumsq"]), self.n_x
        if n_old > n_x:
            raise ValueError(f"the saved state has {n_old} rows, this model's `data_info` only {n_x}")
        h["ptr"] = np.concatenate([h["ptr"], np.full(n_x - n_old, h["ptr"][-1], dtype=np.int64)])
        h["sumsq"] = np.concatenate([h["sumsq"], np.zeros(n_x - n_old, dtype=np.float32)])
        self._state, self._sumsq, self._state_host = None, None, h
        self._set("sim", None)
        self.topk_sim = None
        shape = (self.n_users, self.n_items)
        self.user_interaction = _resized(load_sparse(f"{model_path}_user_inter.npz"), shape)
        self.item_interaction = _resized(load_sparse(f"{model_path}_item_inter.npz"), shape[::-1])

    @classmethod
    def load(cls, path, model_name, data_info, **kwargs):
        if not os.path.exists(path):
            raise OSError(f"file folder {path} doesn't exists...")
        with open(os.path.join(path, f"{model_name}_hyper_parameters.json")) as f:
            hparams = json.load(f)
        model = cls(data_info=data_info, **hparams)
        model._load_state(path, model_name)
        model.loaded = True
        return model

    def rebuild_model(self, path, model_name):
        """Take the saved state and interactions into this newly initialised model (whose `data_info` holds the merged
        ids and consumed items) before retraining on new data: the next `fit` updates them with the new data alone."""
        self._load_state(path, model_name)
        self.incremental = True
