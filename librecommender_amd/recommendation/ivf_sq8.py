"""IVF-SQ8 index over trained embeddings: the lists of `IVFFlatIndex` stored as int8 codes with one f32 scale per
row instead of a second f32 copy of the catalogue, and an exact re-rank of a short candidate list from the f32 rows the caller
holds anyway.  The counterpart of faiss's `IndexIVFScalarQuantizer` (QT_8bit) under `IndexRefineFlat`, with a per-row symmetric
scale in place of faiss's trained per-dimension range.

Training, assignment and the list build are the shared `_IVFIndex.train_lists`, through the same kernels: `centroids`,
`list_ptr` and `list_ids` are bit-identical to the Flat index's.  Encoding, the code scan and the re-rank are HIP kernels (`csrc/ivf_sq8.hip`)
and there is no CPU path.  The file (`ivf_sq8_index.npz`) stores no codes: encoding is deterministic and `load` redoes it."""
from __future__ import annotations

from typing import Optional

import torch

from .. import ops
from .ivf import _IVFIndex, timed

INDEX_FILE = "ivf_sq8_index.npz"


def check_refine(refine: int) -> None:
    if not 0 <= int(refine) <= ops.IVF_SQ8_MAX_REFINE:
        raise ValueError(f"refine must be in 0..{ops.IVF_SQ8_MAX_REFINE}, got {refine}")


class IVFSQ8Index(_IVFIndex):
    """`centroids`, `list_ptr`, `list_ids` as in `IVFFlatIndex`; `codes` int8 [N, stride] and `scales` f32 [N] in list order
    (stride = the width rounded up to 16, padding code 0); `rows` the caller's own f32 catalogue [N, d], read by the re-rank: a
    reference, not a copy (a width that is no multiple of 4 is zero-padded once, as everywhere in this library, and that is a
    copy).  `nprobe` and `refine` are the defaults of `search`.  The file stores `refine` and no codes."""

    FILE = INDEX_FILE
    EXTRA = {"refine": check_refine}

    def __init__(self, centroids, list_ptr, list_ids, codes, scales, rows, nprobe: int, refine: int, d: int):
        super().__init__(centroids, list_ptr, list_ids, nprobe, d)
        self.codes, self.scales, self.rows = codes, scales, rows
        self.refine = int(refine)

    @property
    def nbytes(self) -> int:
        """Device bytes of the index itself: codes, scales, ids, ptr and centroids (the caller's `rows` are not counted)."""
        return sum(t.numel() * t.element_size() for t in (self.codes, self.scales, self.list_ids, self.list_ptr, self.centroids))

    @classmethod
    def _payload(cls, rows_p, list_ids, t):
        return (*timed(t, "encode_ms", lambda: ops.ivf_sq8_encode(rows_p, list_ids)), rows_p)

    @classmethod
    def train_add(cls, rows: torch.Tensor, nlist: int, niter: int = 20, nprobe: int = 1, refine: int = 4,
                  timings: bool = False) -> "IVFSQ8Index":
        """`train_lists` over `rows`, then one gather-and-encode pass; no f32 rows in list order exist at any time."""
        cls._check_rows(rows, nlist, niter, nprobe)
        check_refine(refine)
        return cls._build(rows, nlist, niter, nprobe, timings, refine)

    def search(self, queries: torch.Tensor, k: int, nprobe: Optional[int] = None, consumed_ptr: Optional[torch.Tensor] = None,
               consumed_idx: Optional[torch.Tensor] = None, filter_flag: Optional[torch.Tensor] = None,
               refine: Optional[int] = None):
        """([B, k] f32 scores, [B, k] int64 global ids) among the rows of the `nprobe` best lists.  The code scan keeps
        kk = min(max(k, k * refine), 1024) candidates by (scale * dot(q, codes) desc, id asc); with `refine >= 1` they are
        re-scored as f32 inner products with their catalogue rows and the k best by (score desc, id asc) returned; with
        `refine == 0` the scan's own k best and their approximate scores.  Fill and consumed CSR as `IVFFlatIndex.search`."""
        refine = self.refine if refine is None else int(refine)
        q, nprobe = self._search_args(queries, k, nprobe, ops.ivf_sq8_check_search_args, refine)
        s, i = ops.ivf_sq8_search(q, self.centroids, self.list_ptr, self.list_ids, self.codes, self.scales,
                                  ops.ivf_sq8_kk(k, refine), nprobe, consumed_ptr, consumed_idx, filter_flag)
        return (s, i) if refine == 0 else ops.ivf_rerank(q, self.rows, i, int(k))
