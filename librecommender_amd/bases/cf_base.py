"""`CfBase` (`libreco/bases/cf_base.py`): the neighbourhood collaborative-filtering models UserCF and ItemCF with the
reference's constructor, `fit` signature, prints, checks, fallbacks and checkpoint files.  The similarity matrix, its
per-row top-k, the recommendation scores and the predictions run on the device (csrc/cf_sim.hip, csrc/cf_rank.hip); the
per-row statistics of the similarity are computed on the host as the reference does (`utils/similarities.py:206-240`),
since the result's bits rest on them.

Deliberate differences from the reference:
  (a) ties in the recommendation order are broken by ascending item id (the reference uses numpy's unstable argsort);
  (b) `predict` returns a float for one pair and an ndarray for several (the reference returns a list);
  (c) `block_size` and `num_threads` are accepted and ignored, and `min_common` below 1 acts as 1;
  (d) the interaction CSRs have shape (n_users, n_items) even when the last ids have no training interaction;
  (e) under a process group of more than one rank `fit` raises;
  (f) the sums of `predict` run in a wave-reduction order (within 1e-6 relative of the reference's).
`sim_matrix`, `user_interaction` and `item_interaction` are scipy CSRs made from the device copies on first access;
`topk_sim` is a read-only mapping with the reference's layout (row -> list of (id, sim), or None for an empty row).
"""
from __future__ import annotations

import abc
import os
import random
from collections.abc import Mapping

import numpy as np
import torch
from scipy.sparse import csr_matrix
from scipy.sparse import load_npz as load_sparse
from scipy.sparse import save_npz as save_sparse
from scipy.sparse.linalg import norm as spnorm

from .. import ops
from ..evaluation.evaluate import print_metrics
from ..prediction.predict import convert_id
from ..recommendation import construct_rec, popular_recommendations
from ..utils.misc import colorize, time_block
from ..utils.validate import check_fitting, check_unknown, check_unknown_user
from .base import Base, hip_device


# ---- per-row statistics (`utils/similarities.py:206-240`), computed the same way on the host --------------------------
def row_norm(csr) -> np.ndarray:
    """The row 2-norms as f32 (`compute_sparse_norm`)."""
    return np.asarray(spnorm(csr, axis=1)).astype(np.float32)


def row_mean(csr) -> np.ndarray:
    """The f32 row sum over the stored entries divided by their number, as f32 (`compute_sparse_mean`)."""
    total = np.asarray(csr.sum(axis=1)).ravel()
    count = np.diff(csr.indptr)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (total / count).astype(np.float32)


def row_centred_norm(csr) -> np.ndarray:
    """The norms of the rows after subtracting each row's numpy mean (`compute_sparse_mean_centered_norm`)."""
    data = np.array(csr.data, copy=True)
    ptr = csr.indptr
    for r in range(csr.shape[0]):
        b, e = ptr[r], ptr[r + 1]
        if e > b:
            data[b:e] -= np.mean(data[b:e])
    return row_norm(csr_matrix((data, csr.indices.copy(), ptr.copy()), shape=csr.shape))


def row_count(csr) -> np.ndarray:
    return np.diff(csr.indptr)


def merge_interactions(old, new, shape):
    """The union of two interaction CSRs with the labels of `new` winning (`CsrMatrix::merge`), shaped `shape`: what the
    models that retrain on new data alone (Swing, RsUserCF, RsItemCF) keep for inference."""
    old, new = old.tocoo(), new.tocoo()
    ko = old.row.astype(np.int64) * shape[1] + old.col
    kn = new.row.astype(np.int64) * shape[1] + new.col
    keep = ~np.isin(ko, kn)
    key = np.concatenate([ko[keep], kn])
    val = np.concatenate([old.data[keep], new.data]).astype(np.float32)
    m = csr_matrix((val, (key // shape[1], key % shape[1])), shape=shape, dtype=np.float32)
    m.sort_indices()
    return m


def _resized(m, shape):
    m = m.tocsr().copy()
    m.resize(shape)
    return m


class _DeviceCsr:
    """A CSR on the device: rowptr int64, col int32 (ascending per row), val f32."""

    def __init__(self, ptr, col, val, shape):
        self.ptr, self.col, self.val, self.shape = ptr, col, val, tuple(shape)

    @classmethod
    def from_scipy(cls, m, device):
        m = m.tocsr()
        if not m.has_sorted_indices:
            m = m.sorted_indices()
        to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)  # noqa: E731
        return cls(to(m.indptr, np.int64), to(m.indices, np.int32), to(m.data, np.float32), m.shape)

    def to_scipy(self):
        return csr_matrix((self.val.cpu().numpy(), self.col.cpu().numpy(), self.ptr.cpu().numpy()), shape=self.shape)

    def transpose(self):
        """The transpose, built on the device (columns ascending, values carried along)."""
        rows, cols = self.shape
        nnz = self.col.numel()
        dev = self.ptr.device
        r = torch.repeat_interleave(torch.arange(rows, device=dev, dtype=torch.int64), self.ptr[1:] - self.ptr[:-1],
                                    output_size=nnz)
        order = torch.argsort(self.col.to(torch.int64) * max(rows, 1) + r)
        ptr = torch.zeros(cols + 1, dtype=torch.int64, device=dev)
        ptr[1:] = torch.cumsum(torch.bincount(self.col.to(torch.int64), minlength=cols), 0)
        return _DeviceCsr(ptr, r[order].to(torch.int32).contiguous(), self.val[order].contiguous(), (cols, rows))


class _TopkView(Mapping):
    """`topk_sim` with the reference's layout, read from the device top-k on first access."""

    def __init__(self, ids, sims, lens):
        self._dev = (ids, sims, lens)
        self._host = None

    def _load(self):
        if self._host is None:
            ids, sims, lens = self._dev
            self._host = (ids.cpu().numpy(), sims.cpu().numpy(), lens.cpu().numpy())
        return self._host

    def __getitem__(self, i):
        ids, sims, lens = self._load()
        if not 0 <= i < len(lens):
            raise KeyError(i)
        n = int(lens[i])
        if n == 0:
            return None
        return list(zip(ids[i, :n].tolist(), sims[i, :n].tolist()))

    def __iter__(self):
        return iter(range(len(self._load()[2])))

    def __len__(self):
        return len(self._load()[2])


class CfBase(Base):
    _warn_all_consumed = True     # UserCF / ItemCF say so when every candidate of a user was consumed; Swing does not

    def __init__(self, task, data_info, cf_type, sim_type="cosine", k_sim=20, store_top_k=True, block_size=None,
                 num_threads=1, min_common=1, mode="invert", seed=42, lower_upper_bound=None):
        super().__init__(task, data_info, lower_upper_bound)
        assert cf_type in ("user_cf", "item_cf")
        self.cf_type = cf_type
        self.k_sim = k_sim
        self.sim_type = sim_type
        self.store_top_k = store_top_k
        self.block_size = block_size
        self.num_threads = num_threads
        self.min_common = min_common
        self.mode = mode
        self.seed = seed
        self._host = {"sim": None, "user": None, "item": None}
        self._dev = {"sim": None, "user": None, "item": None}
        self._topk_dev = None
        self.topk_sim = None
        self.print_count = 0
        self._caution_sim_type()

    def _caution_sim_type(self):
        if self.task == "ranking" and self.sim_type == "pearson":
            print(f"{colorize('Warning: pearson is not suitable for implicit data', 'red')}")
        if self.task == "rating" and self.sim_type == "jaccard":
            print(f"{colorize('Warning: jaccard is not suitable for explicit data', 'red')}")

    # ---- host / device copies of the three matrices ------------------------------------------------------------
    def _get(self, name):
        if self._host[name] is None and self._dev[name] is not None:
            self._host[name] = self._dev[name].to_scipy()
        return self._host[name]

    def _set(self, name, m):
        self._host[name] = m
        self._dev[name] = None
        if name == "sim":
            self._topk_dev = None

    def _device(self, name):
        if self._dev[name] is None:
            if self._host[name] is None:
                raise RuntimeError(f"{self.model_name} has no {name} matrix: call `fit` or `load` first")
            self._dev[name] = _DeviceCsr.from_scipy(self._host[name], hip_device("cuda"))
        return self._dev[name]

    sim_matrix = property(lambda self: self._get("sim"), lambda self, m: self._set("sim", m))
    user_interaction = property(lambda self: self._get("user"), lambda self, m: self._set("user", m))
    item_interaction = property(lambda self: self._get("item"), lambda self, m: self._set("item", m))

    def build_model(self):
        pass

    def train_on_batch(self, batch):
        raise NotImplementedError(f"{self.model_name} computes its similarity matrix in one pass, not by batches")

    def state_arrays(self):
        return {}

    def load_state_arrays(self, arrays):
        pass

    # ---- fit -----------------------------------------------------------------------------------------------------
    def _check_sim_args(self):
        if self.sim_type not in ops.CF_SIM_TYPES:
            raise ValueError("sim_type must be one of (`cosine`, `pearson`, `jaccard`)")
        if self.mode not in ("forward", "invert"):
            raise ValueError("mode must either be 'forward' or 'invert'")

    def _interactions(self, train_data, device):
        """The user x item CSR padded to (n_users, n_items) on the device, and its transpose."""
        m = train_data.sparse_interaction.tocsr()
        indptr = np.asarray(m.indptr, dtype=np.int64)
        ptr = np.full(self.n_users + 1, indptr[-1] if len(indptr) else 0, dtype=np.int64)
        ptr[: len(indptr)] = indptr
        m = csr_matrix((np.asarray(m.data, dtype=np.float32), np.asarray(m.indices, dtype=np.int32), ptr),
                       shape=(self.n_users, self.n_items))
        user = _DeviceCsr.from_scipy(m, device)
        return m if m.has_sorted_indices else m.sorted_indices(), user, user.transpose()

    def _similarity(self, x_host, X, Y):
        """The similarity CSR of the rows of X (forward CSR on the device, `x_host` its host copy) against Y = X^T."""
        dev = X.ptr.device
        n_x = X.shape[0]
        if self.sim_type == "jaccard":
            cnt = torch.from_numpy(row_count(x_host).astype(np.int32)).to(dev)
            ptr, col, val = ops.cf_similarity(X.ptr, X.col, None, Y.ptr, Y.col, None, "jaccard", self.min_common, cnt=cnt)
        elif self.sim_type == "cosine":
            norm = torch.from_numpy(row_norm(x_host)).to(dev)
            ptr, col, val = ops.cf_similarity(X.ptr, X.col, X.val, Y.ptr, Y.col, Y.val, "cosine", self.min_common,
                                              norm=norm)
        else:
            mean = torch.from_numpy(row_mean(x_host)).to(dev)
            norm = torch.from_numpy(row_centred_norm(x_host)).to(dev)
            rows = torch.repeat_interleave(torch.arange(n_x, device=dev), X.ptr[1:] - X.ptr[:-1],
                                           output_size=X.col.numel())
            xc = (X.val - mean[rows]).contiguous()
            yc = (Y.val - mean[Y.col.to(torch.int64)]).contiguous()
            ptr, col, val = ops.cf_similarity(X.ptr, X.col, xc, Y.ptr, Y.col, yc, "pearson", self.min_common, norm=norm)
        return _DeviceCsr(ptr, col, val, (n_x, n_x))

    def fit(self, train_data, neg_sampling, verbose=1, eval_data=None, metrics=None, k=10, eval_batch_size=8192,
            eval_user_num=None):
        check_fitting(self, train_data, eval_data, neg_sampling, k)
        self._check_sim_args()
        from .. import distributed as D

        if D.active() is not None:
            raise RuntimeError(f"{self.model_name}: multi-GPU `fit` (torch.distributed is initialised with more than one "
                               "rank) is implemented for TwoTower, LightGCN, FM / DeepFM with plain sparse columns and DIN "
                               "on pure ids; run this model in a single process")
        self.show_start_time()
        dev = hip_device("cuda")
        user_host, user, item = self._interactions(train_data, dev)
        self._set("user", user_host)
        self._set("item", None)
        self._dev["user"], self._dev["item"] = user, item
        with time_block("sim_matrix", verbose=1):
            if self.cf_type == "user_cf":
                sim = self._similarity(user_host, user, item)
            else:
                sim = self._similarity(self.item_interaction, item, user)
            torch.cuda.synchronize(dev)
        self._set("sim", None)
        self._dev["sim"] = sim
        self.topk_sim = None
        n_elements = int(sim.col.numel())
        n = self.n_users if self.cf_type == "user_cf" else self.n_items
        print(f"sim_matrix, shape: {sim.shape}, num_elements: {n_elements}, density: {100 * n_elements / (n * n):5.4f} %")
        if self.store_top_k:
            self.compute_top_k()
        if verbose > 1:
            print_metrics(model=self, neg_sampling=neg_sampling, eval_data=eval_data, metrics=metrics,
                          eval_batch_size=eval_batch_size, k=k, sample_user_num=eval_user_num, seed=self.seed)
            print("=" * 30)

    # ---- top-k -----------------------------------------------------------------------------------------------------
    def _topk(self):
        if self._topk_dev is None:
            s = self._device("sim")
            self._topk_dev = ops.cf_topk(s.ptr, s.col, s.val, self.k_sim)
        return self._topk_dev

    def compute_top_k(self):
        self.topk_sim = _TopkView(*self._topk())

    def get_top_k_sims(self, ui_id):
        ids, sims, lens = self._topk()
        n = int(lens[ui_id])
        if n == 0:
            return None
        return list(zip(ids[ui_id, :n].tolist(), sims[ui_id, :n].tolist()))

    # ---- predict ---------------------------------------------------------------------------------------------------
    def pre_predict_check(self, user, item, inner_id, cold_start):
        user_arr, item_arr = convert_id(self, user, item, inner_id)
        unknown_num, _, user_arr, item_arr = check_unknown(self, user_arr, item_arr)
        if unknown_num > 0 and cold_start != "popular":
            raise ValueError(f"{self.model_name} only supports popular strategy")
        return user_arr, item_arr

    @abc.abstractmethod
    def _predict_rows(self):
        """(sim rows from (u, i), the interaction side) of the model."""

    def predict(self, user, item, cold_start="popular", inner_id=False):
        user_arr, item_arr = self.pre_predict_check(user, item, inner_id, cold_start)
        user_arr = np.asarray(user_arr, dtype=np.int64)
        item_arr = np.asarray(item_arr, dtype=np.int64)
        preds = np.full(len(user_arr), self.default_pred, dtype=np.float32)
        known = np.flatnonzero((user_arr != self.n_users) & (item_arr != self.n_items))
        if len(known):
            sim = self._device("sim")
            inter_name, by_user = self._predict_rows()
            inter = self._device(inter_name)
            dev = sim.ptr.device
            s_rows = user_arr[known] if by_user else item_arr[known]
            i_rows = item_arr[known] if by_user else user_arr[known]
            to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)  # noqa: E731
            rating = self.task == "rating"
            lo, hi = (self.lower_bound, self.upper_bound) if rating else (0.0, 0.0)
            p, none = ops.cf_predict(to(s_rows), to(i_rows), sim.ptr, sim.col, sim.val, inter.ptr, inter.col, inter.val,
                                     self.k_sim, rating, lo, hi, self.default_pred)
            preds[known] = p.cpu().numpy()
            for q in np.flatnonzero(none.cpu().numpy()).tolist():
                self.print_count += 1
                if self.print_count < 7:
                    no_str = (f"No common interaction or similar neighbor for user {user_arr[known[q]]} and item "
                              f"{item_arr[known[q]]}, proceed with default prediction")
                    print(f"{colorize(no_str, 'red')}")
        return preds[0] if len(user_arr) == 1 else preds

    # ---- recommend -------------------------------------------------------------------------------------------------
    def recommend_user(self, user, n_rec, cold_start="popular", inner_id=False, filter_consumed=True, random_rec=False):
        result_recs = dict()
        user_ids, unknown_users = check_unknown_user(self.data_info, user, inner_id)
        if unknown_users:
            if cold_start != "popular":
                raise ValueError(f"{self.model_name} only supports `popular` cold start strategy")
            for u in unknown_users:
                result_recs[u] = popular_recommendations(self.data_info, inner_id, n_rec)
        if user_ids:
            computed_recs = self._recommend_batch(user_ids, n_rec, filter_consumed, random_rec)
            result_recs.update(construct_rec(self.data_info, user_ids, computed_recs, inner_id))
        return result_recs

    def _consumed_csr(self, users, device):
        idx = self.consumed_index
        u = np.asarray(users, dtype=np.int64)
        lens = idx.ptr[u + 1] - idx.ptr[u]
        ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        total = int(ptr[-1])
        items = idx.items[np.repeat(idx.ptr[u] - ptr[:-1], lens) + np.arange(total, dtype=np.int64)] if total else \
            np.zeros(1, dtype=np.int32)
        to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)  # noqa: E731
        return to(ptr, np.int64), to(items, np.int32)

    def _recommend_batch(self, user_ids, n_rec, filter_consumed, random_rec):
        ui = self._device("user")
        tk = self._topk()
        dev = ui.ptr.device
        users = torch.from_numpy(np.asarray(user_ids, dtype=np.int32)).to(dev)
        cons_ptr, cons_idx = self._consumed_csr(user_ids, dev)
        user_cf = self.cf_type == "user_cf"

        def run(users_t, cp, ci, n):
            return [t.cpu().numpy() for t in ops.cf_recommend(users_t, user_cf, ui.ptr, ui.col, ui.val, *tk,
                                                               self.n_items, cp, ci, filter_consumed, n)]

        ids, _, lens, ncand, fallback = run(users, cons_ptr, cons_idx, n_rec)
        wide = np.flatnonzero((fallback == 0) & (ncand > n_rec)) if random_rec else np.zeros(0, dtype=np.int64)
        every = {}
        if len(wide):    # random_rec draws from every candidate: select them all
            sel_ptr, sel_idx = self._consumed_csr([user_ids[b] for b in wide.tolist()], dev)
            all_ids, _, all_lens, _, _ = run(users[torch.from_numpy(wide).to(dev)], sel_ptr, sel_idx,
                                             int(ncand[wide].max()))
            every = {int(b): all_ids[j, : all_lens[j]] for j, b in enumerate(wide.tolist())}
        recs = []
        for b, u in enumerate(user_ids):
            if fallback[b] == 1:
                recs.append(popular_recommendations(self.data_info, inner_id=True, n_rec=n_rec))
            elif fallback[b] == 2:
                self.print_count += self._warn_all_consumed
                if self._warn_all_consumed and self.print_count < 11:
                    no_str = f"no suitable recommendation for user {u}, return default recommendation"
                    print(f"{colorize(no_str, 'red')}")
                recs.append(popular_recommendations(self.data_info, inner_id=True, n_rec=n_rec))
            elif b in every:
                recs.append(np.asarray(random.sample(every[b].tolist(), k=n_rec)))
            else:
                recs.append(ids[b, : lens[b]].astype(np.int64))
        return recs

    # ---- persistence -----------------------------------------------------------------------------------------------
    def save(self, path, model_name, **kwargs):
        if not os.path.isdir(path):
            print(f"file folder {path} doesn't exists, creating a new one...")
            os.makedirs(path)
        import json

        with open(os.path.join(path, f"{model_name}_hyper_parameters.json"), "w") as f:
            json.dump(self._hparams(), f, separators=(",", ":"), indent=4)
        model_path = os.path.join(path, model_name)
        save_sparse(f"{model_path}_sim_matrix", self.sim_matrix)
        save_sparse(f"{model_path}_user_inter", self.user_interaction)
        save_sparse(f"{model_path}_item_inter", self.item_interaction)

    @classmethod
    def load(cls, path, model_name, data_info, **kwargs):
        import json

        if not os.path.exists(path):
            raise OSError(f"file folder {path} doesn't exists...")
        with open(os.path.join(path, f"{model_name}_hyper_parameters.json")) as f:
            hparams = json.load(f)
        model = cls(data_info=data_info, **hparams)
        model_path = os.path.join(path, model_name)
        model.sim_matrix = load_sparse(f"{model_path}_sim_matrix.npz").tocsr()
        model.user_interaction = load_sparse(f"{model_path}_user_inter.npz").tocsr()
        model.item_interaction = load_sparse(f"{model_path}_item_inter.npz").tocsr()
        model.loaded = True
        return model
