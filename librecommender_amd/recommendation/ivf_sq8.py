"""IVF-SQ8 index over trained embeddings: the lists of `IVFFlatIndex` stored as int8 codes with one f32 scale per
row instead of a second f32 copy of the catalogue, and an exact re-rank of a short candidate list from the f32 rows the caller
holds anyway.  The counterpart of faiss's `IndexIVFScalarQuantizer` (QT_8bit) under `IndexRefineFlat`, with a per-row symmetric
scale in place of faiss's trained per-dimension range.

Training, assignment and the list build are `IVFFlatIndex.train_add`'s, through the same kernels: `centroids`, `list_ptr` and
`list_ids` are bit-identical to the Flat index's.  Encoding, the code scan and the re-rank are HIP kernels (`csrc/ivf_sq8.hip`)
and there is no CPU path.  The file (`ivf_sq8_index.npz`) stores no codes: encoding is deterministic and `load` redoes it."""
from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch

from .. import ops
from .ivf import IVFFlatIndex, check_train_args

INDEX_FILE = "ivf_sq8_index.npz"


def check_refine(refine: int) -> None:
    if not 0 <= int(refine) <= ops.IVF_SQ8_MAX_REFINE:
        raise ValueError(f"refine must be in 0..{ops.IVF_SQ8_MAX_REFINE}, got {refine}")


class IVFSQ8Index:
    """`centroids`, `list_ptr`, `list_ids` as in `IVFFlatIndex`; `codes` int8 [N, stride] and `scales` f32 [N] in list order
    (stride = the width rounded up to 16, padding code 0); `rows` the caller's own f32 catalogue [N, d], read by the re-rank: a
    reference, not a copy (a width that is no multiple of 4 is zero-padded once, as everywhere in this library, and that is a
    copy).  `nprobe` and `refine` are the defaults of `search`."""

    def __init__(self, centroids, list_ptr, list_ids, codes, scales, rows, nprobe: int, refine: int, d: int):
        self.centroids, self.list_ptr, self.list_ids = centroids, list_ptr, list_ids
        self.codes, self.scales, self.rows = codes, scales, rows
        self.d = int(d)
        self.nlist = int(centroids.shape[0])
        self.ntotal = int(list_ids.numel())
        self.nprobe = int(nprobe)
        self.refine = int(refine)
        self.timings = {}

    @property
    def nbytes(self) -> int:
        """Device bytes of the index itself: codes, scales, ids, ptr and centroids (the caller's `rows` are not counted)."""
        return sum(t.numel() * t.element_size() for t in (self.codes, self.scales, self.list_ids, self.list_ptr, self.centroids))

    # ---- build ------------------------------------------------------------------------------------------------------
    @classmethod
    def train_add(cls, rows: torch.Tensor, nlist: int, niter: int = 20, nprobe: int = 1, refine: int = 4,
                  timings: bool = False) -> "IVFSQ8Index":
        """`IVFFlatIndex.train_add`'s k-means and lists, then one gather-and-encode pass; no f32 rows in list order exist at
        any time."""
        if not isinstance(rows, torch.Tensor) or rows.dim() != 2:
            raise ValueError("rows must be a 2-d tensor")
        N, D = rows.shape
        nlist, niter = int(nlist), int(niter)
        check_train_args(N, D, nlist, niter)
        if not 1 <= int(nprobe) <= nlist:
            raise ValueError(f"nprobe must be in 1..nlist ({nlist}), got {nprobe}")
        check_refine(refine)
        ops._req(rows, torch.float32, "rows", 2)
        t = {}

        def timed(name, fn):
            if not timings:
                return fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            torch.cuda.synchronize()
            t[name] = a.elapsed_time(b)
            return out

        (rows_p,) = ops._ivf_pad(rows)
        cent = timed("train_ms", lambda: IVFFlatIndex.train_centroids(rows_p, nlist, niter))
        list_of = timed("assign_ms", lambda: ops.ivf_assign(rows_p, cent))
        list_ptr, list_ids = timed("lists_ms", lambda: ops.ivf_build_lists(list_of, nlist))
        codes, scales = timed("encode_ms", lambda: ops.ivf_sq8_encode(rows_p, list_ids))
        index = cls(cent, list_ptr, list_ids, codes, scales, rows_p, nprobe, refine, D)
        index.timings = t
        return index

    # ---- search -----------------------------------------------------------------------------------------------------
    def search(self, queries: torch.Tensor, k: int, nprobe: Optional[int] = None, consumed_ptr: Optional[torch.Tensor] = None,
               consumed_idx: Optional[torch.Tensor] = None, filter_flag: Optional[torch.Tensor] = None,
               refine: Optional[int] = None):
        """([B, k] f32 scores, [B, k] int64 global ids) among the rows of the `nprobe` best lists.  The code scan keeps
        kk = min(max(k, k * refine), 1024) candidates by (scale * dot(q, codes) desc, id asc); with `refine >= 1` they are
        re-scored as f32 inner products with their catalogue rows and the k best by (score desc, id asc) returned; with
        `refine == 0` the scan's own k best and their approximate scores.  Fill and consumed CSR as `IVFFlatIndex.search`."""
        nprobe = self.nprobe if nprobe is None else int(nprobe)
        refine = self.refine if refine is None else int(refine)
        if not isinstance(queries, torch.Tensor) or queries.dim() != 2:
            raise ValueError("queries must be a 2-d tensor")
        B, k = queries.shape[0], int(k)
        ops.ivf_sq8_check_search_args(B, self.ntotal, self.d, queries.shape[1], k, nprobe, self.nlist, refine)
        kk = ops.ivf_sq8_kk(k, refine)
        (q,) = ops._ivf_pad(queries)
        s, i = ops.ivf_sq8_search(q, self.centroids, self.list_ptr, self.list_ids, self.codes, self.scales, kk, nprobe, consumed_ptr,
                                  consumed_idx, filter_flag)
        if refine == 0:
            return s, i
        return ops.ivf_rerank(q, self.rows, i, k)

    # ---- persistence ------------------------------------------------------------------------------------------------
    def save(self, path: str) -> str:
        """`<path>/ivf_sq8_index.npz`: centroids, list_ptr, list_ids, nprobe, refine, d.  Neither rows nor codes are stored:
        `load` takes the rows from the catalogue they index and encodes them again, which gives the same bits."""
        os.makedirs(path, exist_ok=True)
        file = os.path.join(path, INDEX_FILE)
        np.savez(file, centroids=self.centroids[:, : self.d].cpu().numpy(), list_ptr=self.list_ptr.cpu().numpy(),
                 list_ids=self.list_ids.cpu().numpy(), nprobe=np.int64(self.nprobe), refine=np.int64(self.refine), d=np.int64(self.d))
        return file

    @classmethod
    def load(cls, path: str, device="cuda", rows: Optional[torch.Tensor] = None) -> "IVFSQ8Index":
        """The index of `save` over `rows`, the same [N, d] catalogue (default: `item_embed.json` of the same serving
        directory); the consistency checks are `IVFFlatIndex.load`'s."""
        with np.load(os.path.join(path, INDEX_FILE)) as z:
            refine = int(z["refine"])
            parts = IVFFlatIndex.read_lists(z, path, device, rows, INDEX_FILE)
        check_refine(refine)
        cent, list_ptr, list_ids, rows_p, nprobe, d = parts
        codes, scales = ops.ivf_sq8_encode(rows_p, list_ids)
        return cls(cent, list_ptr, list_ids, codes, scales, rows_p, nprobe, refine, d)
