"""IVF-Flat index over trained embeddings: the approximate search behind `EmbedServer(use_index=True)` and
`EmbedBase.init_knn(nlist=...)`, the counterpart of the reference's faiss `IndexIVFFlat(IndexFlatIP, d, nlist,
METRIC_INNER_PRODUCT)` (`libserving/serialization/embed.py:42-54`, searched in `sanic_serving/embed_deploy.py:36-56`).

Inner-product metric only (cosine = inner product over unit-normalised rows, which the caller normalises).  Training is a
deterministic k-means without RNG; assignment, list build, centroid means and the list scan are HIP kernels (`csrc/ivf.hip`) and
there is no CPU path.  The file format is this library's own (`ivf_index.npz`); faiss's binary format is neither written nor
read.

`_IVFIndex` holds what every list format shares (checks, training, the lists, persistence); a format adds its payload."""
from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch

from .. import ops

INDEX_FILE = "ivf_index.npz"
TRAIN_CAP = 256                 # training rows per list at most (faiss's cap)


def timed(t: Optional[dict], name: str, fn):
    """`fn()`.  With a dict `t`, the call's device time in ms (HIP events, then a synchronise) is ADDED to `t[name]`: legs
    that share a name accumulate."""
    if t is None:
        return fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    t[name] = t.get(name, 0.0) + a.elapsed_time(b)
    return out


class _IVFIndex:
    """`centroids` [nlist, D] f32, `list_ptr` [nlist + 1] int64 (CSR of the lists) and `list_ids` [N] int32 (global ids, ascending
    within a list); `nprobe` is the default of `search`.  A subclass names its file, the extra integer fields it stores
    (`EXTRA`: field -> its check; constructor arguments between `nprobe` and `d`) and builds its payload in `_payload` (the
    constructor arguments between `list_ids` and `nprobe`)."""

    FILE = None
    EXTRA = {}
    LISTS_MS = "lists_ms"           # the `timings` key of the list build

    def __init__(self, centroids, list_ptr, list_ids, nprobe: int, d: int):
        self.centroids, self.list_ptr, self.list_ids = centroids, list_ptr, list_ids
        self.d = int(d)                                  # width of the caller's rows (the stored ones are padded to 4)
        self.nlist = int(centroids.shape[0])
        self.ntotal = int(list_ids.numel())
        self.nprobe = int(nprobe)
        self.timings = {}

    @classmethod
    def _payload(cls, rows_p: torch.Tensor, list_ids: torch.Tensor, t: Optional[dict]) -> tuple:
        raise NotImplementedError

    # ---- build ------------------------------------------------------------------------------------------------------
    @staticmethod
    def check_train_args(N: int, D: int, nlist: int, niter: int, nprobe: int) -> None:
        """Argument errors of `train_add`, raised before a device is needed."""
        if nlist < 1:
            raise ValueError(f"nlist must be >= 1, got {nlist}")
        if nlist > N:
            raise ValueError(f"nlist {nlist} exceeds the number of rows {N}")
        if nlist > ops.IVF_MAX_NLIST or D < 1 or D > 256 or N >= 2 ** 31:
            raise ValueError(f"IVFFlatIndex: shape not supported (N={N} D={D} nlist={nlist})")
        if niter < 0:
            raise ValueError(f"niter must be >= 0, got {niter}")
        if not 1 <= int(nprobe) <= nlist:
            raise ValueError(f"nprobe must be in 1..nlist ({nlist}), got {nprobe}")

    @classmethod
    def _check_rows(cls, rows, nlist, niter, nprobe) -> None:
        if not isinstance(rows, torch.Tensor) or rows.dim() != 2:
            raise ValueError("rows must be a 2-d tensor")
        cls.check_train_args(rows.shape[0], rows.shape[1], int(nlist), int(niter), nprobe)

    @classmethod
    def train_lists(cls, rows_p: torch.Tensor, nlist: int, niter: int, t: Optional[dict] = None):
        """(centroids, list_ptr, list_ids) of padded rows: k-means on at most `256 * nlist` rows (ids floor(j N / n_train);
        initial centroids the training rows at floor(j n_train / nlist); `niter` rounds of assign + mean, an empty list keeps
        its centroid), then every row is assigned and the lists are built."""
        def kmeans():
            N, dev = rows_p.shape[0], rows_p.device
            n_train = min(N, TRAIN_CAP * nlist)
            if n_train == N:
                tr = rows_p
            else:
                tr = rows_p.index_select(0, (torch.arange(n_train, dtype=torch.int64, device=dev) * N) // n_train).contiguous()
            cent = tr.index_select(0, (torch.arange(nlist, dtype=torch.int64, device=dev) * n_train) // nlist).contiguous()
            for _ in range(niter):
                ptr, ids = ops.ivf_build_lists(ops.ivf_assign(tr, cent), nlist)
                ops.ivf_centroids(tr, ptr, ids, cent)
            return cent

        cent = timed(t, "train_ms", kmeans)
        list_of = timed(t, "assign_ms", lambda: ops.ivf_assign(rows_p, cent))
        list_ptr, list_ids = timed(t, cls.LISTS_MS, lambda: ops.ivf_build_lists(list_of, nlist))
        return cent, list_ptr, list_ids

    @classmethod
    def _build(cls, rows: torch.Tensor, nlist: int, niter: int, nprobe: int, timings: bool, *extra):
        """`train_add` after its argument checks."""
        ops._req(rows, torch.float32, "rows", 2)
        (rows_p,) = ops._ivf_pad(rows)
        t = {} if timings else None
        cent, list_ptr, list_ids = cls.train_lists(rows_p, int(nlist), int(niter), t)
        index = cls(cent, list_ptr, list_ids, *cls._payload(rows_p, list_ids, t), nprobe, *extra, rows.shape[1])
        index.timings = t or {}
        return index

    # ---- search -----------------------------------------------------------------------------------------------------
    def _search_args(self, queries, k, nprobe, check=ops.ivf_check_search_args, *extra):
        """The checks of `search` that need no device (`check` with the format's `extra` arguments): (the padded queries,
        nprobe)."""
        nprobe = self.nprobe if nprobe is None else int(nprobe)
        if not isinstance(queries, torch.Tensor) or queries.dim() != 2:
            raise ValueError("queries must be a 2-d tensor")
        check(queries.shape[0], self.ntotal, self.d, queries.shape[1], int(k), nprobe, self.nlist, *extra)
        return ops._ivf_pad(queries)[0], nprobe

    # ---- persistence ------------------------------------------------------------------------------------------------
    def save(self, path: str) -> str:
        """`<path>/<FILE>`: centroids, list_ptr, list_ids, nprobe, the `EXTRA` fields, d.  Neither the rows nor anything derived
        from them is stored: `load` takes the rows from the catalogue they index and builds the payload again, which gives the
        same bits."""
        os.makedirs(path, exist_ok=True)
        file = os.path.join(path, self.FILE)
        np.savez(file, centroids=self.centroids[:, : self.d].cpu().numpy(), list_ptr=self.list_ptr.cpu().numpy(),
                 list_ids=self.list_ids.cpu().numpy(), nprobe=np.int64(self.nprobe),
                 **{name: np.int64(getattr(self, name)) for name in self.EXTRA}, d=np.int64(self.d))
        return file

    @classmethod
    def load(cls, path: str, device="cuda", rows: Optional[torch.Tensor] = None):
        """The index of `save` over `rows`, the same [N, d] catalogue (default: `item_embed.json` of the same serving
        directory, as `serving.save_embed` writes it)."""
        with np.load(os.path.join(path, cls.FILE)) as z:
            extra = [int(z[name]) for name in cls.EXTRA]
            cent, ptr, ids = z["centroids"], z["list_ptr"], z["list_ids"]
            nprobe, d = int(z["nprobe"]), int(z["d"])
        if rows is None:
            import json

            with open(os.path.join(path, "item_embed.json")) as f:
                ie = json.load(f)
            rows = torch.tensor([ie[str(i)] for i in range(len(ie))], dtype=torch.float32)
        if rows.dim() != 2 or rows.shape[1] != d or rows.shape[0] != ids.shape[0] or cent.shape[1] != d:
            raise ValueError(f"{cls.FILE} does not describe these rows")
        if (ptr.shape[0] != cent.shape[0] + 1 or int(ptr[0]) != 0 or int(ptr[-1]) != ids.shape[0] or (np.diff(ptr) < 0).any()
                or (ids.size and (ids.min() < 0 or ids.max() >= ids.shape[0]))):
            raise ValueError(f"{cls.FILE} is inconsistent")
        for check, value in zip(cls.EXTRA.values(), extra):
            check(value)
        dev = torch.device(device)
        rows = ops._req(rows.to(dev), torch.float32, "rows", 2)
        cent_t, rows_p = ops._ivf_pad(torch.from_numpy(np.ascontiguousarray(cent, dtype=np.float32)).to(dev))[0], ops._ivf_pad(rows)[0]
        list_ptr = torch.from_numpy(np.ascontiguousarray(ptr, dtype=np.int64)).to(dev)
        list_ids = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).to(dev)
        return cls(cent_t.contiguous(), list_ptr, list_ids, *cls._payload(rows_p, list_ids, None), nprobe, *extra, d)


class IVFFlatIndex(_IVFIndex):
    """The lists as f32 rows: `list_rows` [N, D], the rows in list order (a list is one contiguous stream)."""

    FILE = INDEX_FILE
    LISTS_MS = "permute_ms"         # list build + row permutation

    def __init__(self, centroids, list_ptr, list_ids, list_rows, nprobe: int, d: int):
        super().__init__(centroids, list_ptr, list_ids, nprobe, d)
        self.list_rows = list_rows

    @classmethod
    def _payload(cls, rows_p, list_ids, t):
        return (timed(t, cls.LISTS_MS, lambda: ops.embed_gather(rows_p, list_ids)),)

    @classmethod
    def train_add(cls, rows: torch.Tensor, nlist: int, niter: int = 20, nprobe: int = 1, timings: bool = False) -> "IVFFlatIndex":
        """`train_lists` over `rows`, then the rows are permuted into list order."""
        cls._check_rows(rows, nlist, niter, nprobe)
        return cls._build(rows, nlist, niter, nprobe, timings)

    def search(self, queries: torch.Tensor, k: int, nprobe: Optional[int] = None, consumed_ptr: Optional[torch.Tensor] = None,
               consumed_idx: Optional[torch.Tensor] = None, filter_flag: Optional[torch.Tensor] = None):
        """([B, k] f32 scores, [B, k] int64 global ids) by (score desc, id asc) among the rows of the `nprobe` best lists; slots
        beyond the surviving candidates hold id -1 / score -inf.  The consumed CSR is `ops.score_topk`'s."""
        q, nprobe = self._search_args(queries, k, nprobe)
        return ops.ivf_search(q, self.centroids, self.list_ptr, self.list_ids, self.list_rows, k, nprobe, consumed_ptr,
                              consumed_idx, filter_flag)
