"""IVF-Flat index over trained embeddings: the approximate search behind `EmbedServer(use_index=True)` and
`EmbedBase.init_knn(nlist=...)`, the counterpart of the reference's faiss `IndexIVFFlat(IndexFlatIP, d, nlist,
METRIC_INNER_PRODUCT)` (`libserving/serialization/embed.py:42-54`, searched in `sanic_serving/embed_deploy.py:36-56`).

Inner-product metric only (cosine = inner product over unit-normalised rows, which the caller normalises).  Training is a
deterministic k-means without RNG; assignment, list build, centroid means and the list scan are HIP kernels (`csrc/ivf.hip`) and
there is no CPU path.  The file format is this library's own (`ivf_index.npz`); faiss's binary format is neither written nor
read."""
from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch

from .. import ops

INDEX_FILE = "ivf_index.npz"
TRAIN_CAP = 256                 # training rows per list at most (faiss's cap)


def check_train_args(N: int, D: int, nlist: int, niter: int) -> None:
    """Argument errors of `train_add`, raised before a device is needed."""
    if nlist < 1:
        raise ValueError(f"nlist must be >= 1, got {nlist}")
    if nlist > N:
        raise ValueError(f"nlist {nlist} exceeds the number of rows {N}")
    if nlist > ops.IVF_MAX_NLIST or D < 1 or D > 256 or N >= 2 ** 31:
        raise ValueError(f"IVFFlatIndex: shape not supported (N={N} D={D} nlist={nlist})")
    if niter < 0:
        raise ValueError(f"niter must be >= 0, got {niter}")


class IVFFlatIndex:
    """`centroids` [nlist, D] f32, `list_ptr` [nlist + 1] int64 (CSR of the lists), `list_ids` [N] int32 (global ids, ascending
    within a list) and `list_rows` [N, D] (the rows in list order: a list is one contiguous stream); `nprobe` is the default of
    `search`."""

    def __init__(self, centroids, list_ptr, list_ids, list_rows, nprobe: int, d: int):
        self.centroids, self.list_ptr, self.list_ids, self.list_rows = centroids, list_ptr, list_ids, list_rows
        self.d = int(d)                                  # width of the caller's rows (the stored ones are padded to 4)
        self.nlist = int(centroids.shape[0])
        self.ntotal = int(list_ids.numel())
        self.nprobe = int(nprobe)
        self.timings = {}

    # ---- build ------------------------------------------------------------------------------------------------------
    @staticmethod
    def train_centroids(rows_p: torch.Tensor, nlist: int, niter: int) -> torch.Tensor:
        """The k-means of `train_add` over padded rows (shared with `IVFSQ8Index`): centroids [nlist, D]."""
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

    @classmethod
    def train_add(cls, rows: torch.Tensor, nlist: int, niter: int = 20, nprobe: int = 1, timings: bool = False) -> "IVFFlatIndex":
        """k-means on at most `256 * nlist` rows (ids floor(j N / n_train); initial centroids the training rows at
        floor(j n_train / nlist); `niter` rounds of assign + mean, an empty list keeps its centroid), then all rows are added."""
        if not isinstance(rows, torch.Tensor) or rows.dim() != 2:
            raise ValueError("rows must be a 2-d tensor")
        N, D = rows.shape
        nlist, niter = int(nlist), int(niter)
        check_train_args(N, D, nlist, niter)
        if not 1 <= int(nprobe) <= nlist:
            raise ValueError(f"nprobe must be in 1..nlist ({nlist}), got {nprobe}")
        ops._req(rows, torch.float32, "rows", 2)
        (rows_p,) = ops._ivf_pad(rows)
        t = {}

        def timed(name, fn):
            if not timings:
                return fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            torch.cuda.synchronize()
            t[name] = t.get(name, 0.0) + a.elapsed_time(b)
            return out

        cent = timed("train_ms", lambda: cls.train_centroids(rows_p, nlist, niter))
        list_of = timed("assign_ms", lambda: ops.ivf_assign(rows_p, cent))
        list_ptr, list_ids, list_rows = timed("permute_ms", lambda: ops.ivf_build_lists(list_of, nlist, rows_p))
        index = cls(cent, list_ptr, list_ids, list_rows, nprobe, D)
        index.timings = t
        return index

    # ---- search -----------------------------------------------------------------------------------------------------
    def search(self, queries: torch.Tensor, k: int, nprobe: Optional[int] = None, consumed_ptr: Optional[torch.Tensor] = None,
               consumed_idx: Optional[torch.Tensor] = None, filter_flag: Optional[torch.Tensor] = None):
        """([B, k] f32 scores, [B, k] int64 global ids) by (score desc, id asc) among the rows of the `nprobe` best lists; slots
        beyond the surviving candidates hold id -1 / score -inf.  The consumed CSR is `ops.score_topk`'s."""
        nprobe = self.nprobe if nprobe is None else int(nprobe)
        if not isinstance(queries, torch.Tensor) or queries.dim() != 2:
            raise ValueError("queries must be a 2-d tensor")
        ops.ivf_check_search_args(queries.shape[0], self.ntotal, self.d, queries.shape[1], int(k), nprobe, self.nlist)
        (q,) = ops._ivf_pad(queries)
        return ops.ivf_search(q, self.centroids, self.list_ptr, self.list_ids, self.list_rows, k, nprobe, consumed_ptr,
                              consumed_idx, filter_flag)

    # ---- persistence ------------------------------------------------------------------------------------------------
    def save(self, path: str) -> str:
        """`<path>/ivf_index.npz`: centroids, list_ptr, list_ids, nprobe, d.  The rows are not stored: `load` takes them from
        the catalogue they index."""
        os.makedirs(path, exist_ok=True)
        file = os.path.join(path, INDEX_FILE)
        np.savez(file, centroids=self.centroids[:, : self.d].cpu().numpy(), list_ptr=self.list_ptr.cpu().numpy(),
                 list_ids=self.list_ids.cpu().numpy(), nprobe=np.int64(self.nprobe), d=np.int64(self.d))
        return file

    @classmethod
    def load(cls, path: str, device="cuda", rows: Optional[torch.Tensor] = None) -> "IVFFlatIndex":
        """The index of `save` over `rows`, the same [N, d] catalogue (default: `item_embed.json` of the same serving
        directory, as `serving.save_embed` writes it)."""
        with np.load(os.path.join(path, INDEX_FILE)) as z:
            cent_t, list_ptr, list_ids, rows_p, nprobe, d = cls.read_lists(z, path, device, rows, INDEX_FILE)
        list_rows = ops.embed_gather(rows_p, list_ids)
        return cls(cent_t, list_ptr, list_ids, list_rows, nprobe, d)

    @staticmethod
    def read_lists(z, path: str, device, rows: Optional[torch.Tensor], name: str):
        """What `load` reads and checks of an opened index file `z` (shared with `IVFSQ8Index`): (centroids, list_ptr, list_ids,
        the padded rows on the device, nprobe, d)."""
        cent, ptr, ids = z["centroids"], z["list_ptr"], z["list_ids"]
        nprobe, d = int(z["nprobe"]), int(z["d"])
        if rows is None:
            import json

            with open(os.path.join(path, "item_embed.json")) as f:
                ie = json.load(f)
            rows = torch.tensor([ie[str(i)] for i in range(len(ie))], dtype=torch.float32)
        if rows.dim() != 2 or rows.shape[1] != d or rows.shape[0] != ids.shape[0] or cent.shape[1] != d:
            raise ValueError(f"{name} does not describe these rows")
        if (ptr.shape[0] != cent.shape[0] + 1 or int(ptr[0]) != 0 or int(ptr[-1]) != ids.shape[0] or (np.diff(ptr) < 0).any()
                or (ids.size and (ids.min() < 0 or ids.max() >= ids.shape[0]))):
            raise ValueError(f"{name} is inconsistent")
        dev = torch.device(device)
        rows = ops._req(rows.to(dev), torch.float32, "rows", 2)
        cent_t, rows_p = ops._ivf_pad(torch.from_numpy(np.ascontiguousarray(cent, dtype=np.float32)).to(dev))[0], ops._ivf_pad(rows)[0]
        list_ids = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).to(dev)
        return (cent_t.contiguous(), torch.from_numpy(np.ascontiguousarray(ptr, dtype=np.int64)).to(dev), list_ids, rows_p,
                nprobe, d)
