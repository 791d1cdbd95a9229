"""Tensor-level wrappers over the C-ABI (``include/libreco_hip.h``).

PyTorch is plumbing here: it owns device memory and the HIP stream; every function below
validates its arguments, passes raw device pointers + the current stream to the shared
library, and raises if the tensors are not on a HIP device (no CPU path exists).
"""
from __future__ import annotations

import os

from dataclasses import dataclass
from typing import NamedTuple, Optional

import torch

from . import _lib
from ._lib import AdamHP, COMBINERS, check


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class KernelTimer:
    """Optional HIP-event timing of selected C-ABI launches on the stream they are enqueued on
    (bench.py's roofline leg).  Disabled by default: zero overhead on the product path."""

    def __init__(self):
        self.names = set()
        self.events = {}

    def enable(self, *names):
        self.names = set(names)
        self.events = {n: [] for n in names}

    def disable(self):
        self.names = set()

    def summary(self):
        """name -> (launches, mean_ms); call after torch.cuda.synchronize()."""
        out = {}
        for n, evs in self.events.items():
            if evs:
                ms = [a.elapsed_time(b) for a, b in evs]
                out[n] = (len(ms), sum(ms) / len(ms))
        return out


TIMER = KernelTimer()


def _call(name: str, *args) -> None:
    fn = getattr(_lib.load(), name)
    if name in TIMER.names:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = fn(*args)
        b.record()
        TIMER.events[name].append((a, b))
    else:
        rc = fn(*args)
    check(rc, name)


def _ptr(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.data_ptr()


def _req(t: torch.Tensor, dtype: torch.dtype, name: str, ndim: Optional[int] = None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(
            f"{name} is on {t.device}: the libreco HIP kernels only run on an MI355X device "
            "tensor (there is no CPU fallback)"
        )
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"{name} must be {ndim}-d, got shape {tuple(t.shape)}")
    return t


def adam_hp(lr: float, step: int, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-5,
            weight_decay: float = 0.0, tf_style: bool = True) -> AdamHP:
    if step < 1:
        raise ValueError("Adam step counts from 1")
    return AdamHP(lr, beta1, beta2, eps, weight_decay, int(step), 1 if tf_style else 0)


# --------------------------------------------------------------------------------------
# gather / pooling
# --------------------------------------------------------------------------------------
def embed_gather(table: torch.Tensor, idx: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[..., :] = table[idx[...], :]`` (layers/embedding.py:23)."""
    _req(table, torch.float32, "table")
    _req(idx, torch.int32, "idx")
    t2 = table if table.dim() == 2 else table.reshape(table.shape[0], -1)
    V, K = t2.shape
    n = idx.numel()
    if out is None:
        out = torch.empty((*idx.shape, K), dtype=torch.float32, device=table.device)
    else:
        _req(out, torch.float32, "out")
        if out.numel() != n * K:
            raise ValueError("out has the wrong size")
    _call("lr_embed_gather_f32", _ptr(t2), V, K, _ptr(idx), n, _ptr(out), _stream())
    return out


def embed_bag_pool(table: torch.Tensor, idx: torch.Tensor, combiner: str, oov: int) -> torch.Tensor:
    """Fixed-length bag pooling with OOV->0 (tfops/features.py:90-118)."""
    _req(table, torch.float32, "table", 2)
    _req(idx, torch.int32, "idx", 2)
    V, K = table.shape
    nbags, bag_len = idx.shape
    out = torch.empty((nbags, K), dtype=torch.float32, device=table.device)
    _call("lr_embed_bag_pool_f32", _ptr(table), V, K, _ptr(idx), nbags, bag_len,
                                            COMBINERS[combiner], int(oov), _ptr(out), _stream())
    return out


def embed_bag_pool_bwd(gout: torch.Tensor, idx: torch.Tensor, V: int, combiner: str, oov: int) -> torch.Tensor:
    _req(gout, torch.float32, "gout", 2)
    _req(idx, torch.int32, "idx", 2)
    nbags, bag_len = idx.shape
    K = gout.shape[1]
    gentry = torch.empty((nbags * bag_len, K), dtype=torch.float32, device=gout.device)
    _call("lr_embed_bag_pool_bwd_f32", _ptr(gout), K, _ptr(idx), V, nbags, bag_len,
                                                COMBINERS[combiner], int(oov), _ptr(gentry),
                                                _stream())
    return gentry


def pair_dot(U: torch.Tensor, I: torch.Tensor, user: torch.Tensor, item: torch.Tensor) -> torch.Tensor:
    """``out[i] = <U[user[i]], I[item[i]]>`` (prediction/predict.py:36-40)."""
    _req(U, torch.float32, "U", 2)
    _req(I, torch.float32, "I", 2)
    _req(user, torch.int32, "user", 1)
    _req(item, torch.int32, "item", 1)
    if U.shape[1] != I.shape[1] or user.numel() != item.numel():
        raise ValueError("shape mismatch")
    out = torch.empty(user.numel(), dtype=torch.float32, device=U.device)
    _call("lr_pair_dot_f32", _ptr(U), U.shape[0], _ptr(I), I.shape[0], U.shape[1],
                                      _ptr(user), _ptr(item), user.numel(), _ptr(out), _stream())
    return out


# --------------------------------------------------------------------------------------
# segments ("CSR by touched row") + gradient scatter
# --------------------------------------------------------------------------------------
@dataclass
class Segments:
    """Device-side grouping of batch positions by table row (see lr_segments_build)."""

    pos: torch.Tensor      # int32 [n]
    rows: torch.Tensor     # int32 [n]      (first n_seg valid)
    start: torch.Tensor    # int32 [n + 1]  (first n_seg + 1 valid)
    n_seg: torch.Tensor    # int32 [1], device
    n: int
    V: int
    slots: Optional[torch.Tensor] = None   # int32 [n]: run number of every position (on request)
    slotT: Optional[torch.Tensor] = None   # int32 [F,B]: index of position (b,f) in `pos` (FieldSegmentBuilder)
    runT: Optional[torch.Tensor] = None    # int32 [F,B]: run number of position (b,f) (FieldSegmentBuilder(want_runs=True))
    owner: Optional[object] = None         # the builder: keeps the long-run workspaces of the scatter kernels

    def long_ws(self, K: int) -> Optional[torch.Tensor]:
        """Persistent workspace for the long-run (Zipf head) path of the scatter kernels (see lr_embed_scatter_ws_bytes)."""
        return self.owner.long_ws(K) if self.owner is not None and hasattr(self.owner, "long_ws") else None

    def ftrl_ws(self) -> Optional[torch.Tensor]:
        """Persistent workspace for the long-run path of `ftrl_rows` (see lr_ftrl_rows_ws_bytes)."""
        return self.owner.ftrl_ws() if self.owner is not None and hasattr(self.owner, "ftrl_ws") else None

    def count(self) -> int:
        """Host sync — for tests and logging only."""
        return int(self.n_seg.item())


class SegmentBuilder:
    """Reusable workspace for ``lr_segments_build`` (no per-step allocation)."""

    def __init__(self, n_max: int, V: int, device: torch.device):
        self.n_max, self.V, self.device = int(n_max), int(V), device
        nbytes = _lib.load().lr_segments_ws_bytes(self.n_max, self.V)
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.pos = torch.empty(self.n_max, dtype=torch.int32, device=device)
        self.rows = torch.empty(self.n_max, dtype=torch.int32, device=device)
        self.start = torch.empty(self.n_max + 1, dtype=torch.int32, device=device)
        self.n_seg = torch.zeros(1, dtype=torch.int32, device=device)
        self.slots = None
        self._long_ws = {}

    def long_ws(self, K: int) -> torch.Tensor:
        ws = self._long_ws.get(K)
        if ws is None:
            ws = self._long_ws[K] = torch.empty(max(_lib.load().lr_embed_scatter_ws_bytes(self.n_max, K), 256),
                                                dtype=torch.uint8, device=self.device)
        return ws

    def hist_ws(self, K: int) -> torch.Tensor:
        """Persistent workspace of `lr_svdpp_hist_grad_f32` for up to `n_max` entries (contents arbitrary between calls)."""
        ws = self._long_ws.get(("hist", K))
        if ws is None:
            ws = self._long_ws[("hist", K)] = torch.empty(max(_lib.load().lr_svdpp_hist_grad_ws_bytes(self.n_max, K), 256),
                                                          dtype=torch.uint8, device=self.device)
        return ws

    def ftrl_ws(self) -> torch.Tensor:
        """Persistent workspace of `lr_ftrl_rows_f32` for up to `n_max` positions (contents arbitrary between calls)."""
        ws = self._long_ws.get("ftrl")
        if ws is None:
            ws = self._long_ws["ftrl"] = torch.empty(max(_lib.load().lr_ftrl_rows_ws_bytes(self.n_max), 256),
                                                     dtype=torch.uint8, device=self.device)
        return ws

    def build(self, idx: torch.Tensor, want_slots: bool = False) -> Segments:
        """``want_slots``: also emit the run number of every position (``seg.slots``)."""
        _req(idx, torch.int32, "idx")
        n = idx.numel()
        if n > self.n_max:
            raise ValueError(f"idx has {n} entries, builder was sized for {self.n_max}")
        if want_slots and self.slots is None:
            self.slots = torch.empty(self.n_max, dtype=torch.int32, device=self.device)
        _call("lr_segments_build", _ptr(idx), n, self.V, _ptr(self.pos), _ptr(self.rows),
                                            _ptr(self.start), _ptr(self.n_seg),
                                            _ptr(self.slots) if want_slots else None, _ptr(self.ws),
                                            self.ws.numel(), _stream())
        seg = Segments(self.pos, self.rows, self.start, self.n_seg, n, self.V, owner=self)
        seg.slots = self.slots[:n] if want_slots else None
        return seg


def build_segments(idx: torch.Tensor, V: int) -> Segments:
    return SegmentBuilder(max(idx.numel(), 1), V, idx.device).build(idx)


class FieldSegmentBuilder:
    """Reusable buffers for ``lr_segments_build_fields`` (idx [B,F] whose column f only holds rows of
    field f): same `Segments` as `SegmentBuilder.build(idx.reshape(-1))`, plus ``seg.slotT`` [F,B] —
    the index of position (b,f) in ``seg.pos`` (-1 for dropped entries)."""

    MAX_B = 16384

    def __init__(self, B_max: int, F: int, V: int, device: torch.device, want_runs: bool = False):
        self.B_max, self.F, self.V, self.device = int(B_max), int(F), int(V), device
        n = self.B_max * self.F
        self.ws = torch.empty(_lib.load().lr_segments_fields_ws_bytes(self.B_max, self.F), dtype=torch.uint8, device=device)
        self.pos = torch.empty(n, dtype=torch.int32, device=device)
        self.rows = torch.empty(n, dtype=torch.int32, device=device)
        self.start = torch.empty(n + 1, dtype=torch.int32, device=device)
        self.n_seg = torch.zeros(1, dtype=torch.int32, device=device)
        self.slotT = torch.empty((self.F, self.B_max), dtype=torch.int32, device=device)
        self.runT = torch.empty((self.F, self.B_max), dtype=torch.int32, device=device) if want_runs else None

    def build(self, idxT: torch.Tensor, field_row_start: torch.Tensor) -> Segments:
        """``want_runs`` builders also set ``seg.runT`` [F,B]: the run number of every position (-1 if dropped)."""
        _req(idxT, torch.int32, "idxT", 2)
        _req(field_row_start, torch.int32, "field_row_start", 1)
        F, B = idxT.shape
        if F != self.F or B > self.B_max or field_row_start.numel() != F + 1:
            raise ValueError("idxT does not match this builder")
        cut = (lambda t: t if B == self.B_max else t.view(-1)[: F * B].view(F, B))
        slotT = cut(self.slotT)
        seg = Segments(self.pos, self.rows, self.start, self.n_seg, B * F, self.V)
        if self.runT is None:
            _call("lr_segments_build_fields", _ptr(idxT), B, F, _ptr(field_row_start), _ptr(self.pos), _ptr(self.rows),
                  _ptr(self.start), _ptr(self.n_seg), _ptr(slotT), _ptr(self.ws), self.ws.numel(), _stream())
        else:
            seg.runT = cut(self.runT)
            _call("lr_segments_build_fields_runs", _ptr(idxT), B, F, _ptr(field_row_start), _ptr(self.pos), _ptr(self.rows),
                  _ptr(self.start), _ptr(self.n_seg), _ptr(slotT), _ptr(seg.runT), _ptr(self.ws), self.ws.numel(), _stream())
        seg.slotT = slotT
        return seg


class OwnerPartition:
    """Reusable buffers for ``lr_owner_partition_i32``: the stable owner-major order of a batch's distinct rows under
    round-robin row sharding (owner = row % W).  `run(seg)` -> (perm [n_max] int32: place of run r, send_ids [n_max] int32:
    local rows in that order, counts [W + 1] int64 on the device: per owner, then the total)."""

    def __init__(self, n_max: int, W: int, device: torch.device):
        self.n_max, self.W = int(n_max), int(W)
        self.ws = torch.empty(max(_lib.load().lr_owner_partition_ws_bytes(self.n_max, self.W), 256), dtype=torch.uint8, device=device)
        self.perm = torch.empty(self.n_max, dtype=torch.int32, device=device)
        self.send_ids = torch.empty(self.n_max, dtype=torch.int32, device=device)
        self.counts = torch.zeros(self.W + 1, dtype=torch.int64, device=device)

    def run(self, rows: torch.Tensor, n_seg: torch.Tensor):
        _req(rows, torch.int32, "rows", 1)
        _req(n_seg, torch.int32, "n_seg", 1)
        if rows.numel() > self.n_max:
            raise ValueError("rows exceed this partition's capacity")
        _call("lr_owner_partition_i32", _ptr(rows), _ptr(n_seg), rows.numel(), self.W, _ptr(self.perm), _ptr(self.send_ids),
              _ptr(self.counts), _ptr(self.ws), self.ws.numel(), _stream())
        return self.perm, self.send_ids, self.counts


def idx_transpose(idx: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B,F] int32 -> [F,B] (the field-major id layout of the per-field kernels)."""
    _req(idx, torch.int32, "idx", 2)
    B, F = idx.shape
    if out is None:
        out = torch.empty((F, B), dtype=torch.int32, device=idx.device)
    _call("lr_idx_transpose_i32", _ptr(idx), B, F, _ptr(out), _stream())
    return out


def din_build_ids(users, items, sparse, cols, seqs, lens, user_off: int, item_off: int, sparse_off: int,
                  out: torch.Tensor) -> torch.Tensor:
    """The id stream of the fused DIN step in one launch (see lr_din_build_ids_i32).  `sparse` [B, n_sp] int32 or None, `cols`
    int32 [n_plain] (the plain sparse columns) or None = all of them."""
    for t_, n_ in ((users, "users"), (items, "items"), (seqs, "seqs"), (lens, "lens"), (out, "out")):
        _req(t_, torch.int32, n_)
    B, L = seqs.shape
    n_plain = 0
    if sparse is not None:
        _req(sparse, torch.int32, "sparse", 2)
        n_plain = int(cols.numel()) if cols is not None else sparse.shape[1]
        if cols is not None:
            _req(cols, torch.int32, "cols", 1)
    if out.numel() != (2 + n_plain + 2 + L) * B or not seqs.is_contiguous() or (sparse is not None and not sparse.is_contiguous()):
        raise ValueError("`out` must hold (2 + n_plain + 2 + L) * B ids; seqs / sparse contiguous")
    _call("lr_din_build_ids_i32", _ptr(users), _ptr(items), _ptr(sparse), sparse.shape[1] if sparse is not None else 0,
          _ptr(cols), n_plain, _ptr(seqs), _ptr(lens), B, L, int(user_off), int(item_off), int(sparse_off), _ptr(out), _stream())
    return out


def _din_order(order, B):
    if order is not None and (order.dtype != torch.int32 or not order.is_contiguous() or order.numel() != B):
        raise ValueError("order must be a contiguous int32 tensor of B elements")
    return order


def embed_segment_sum(grad: torch.Tensor, seg: Segments) -> torch.Tensor:
    _req(grad, torch.float32, "grad")
    K = grad.shape[-1]
    if grad.numel() != seg.n * K:
        raise ValueError("grad rows must match the segmented index count")
    grows = torch.zeros((max(seg.n, 1), K), dtype=torch.float32, device=grad.device)
    ws = seg.long_ws(K)
    _call("lr_embed_segment_sum_f32", _ptr(grad), K, _ptr(seg.pos), _ptr(seg.start), _ptr(seg.n_seg), seg.n, _ptr(grows),
          _ptr(ws), 0 if ws is None else ws.numel(), _stream())
    return grows


def embed_scatter_add(table: torch.Tensor, grad: torch.Tensor, seg: Segments, alpha: float = 1.0) -> None:
    _req(table, torch.float32, "table", 2)
    _req(grad, torch.float32, "grad")
    V, K = table.shape
    if grad.numel() != seg.n * K or V != seg.V:
        raise ValueError("shape mismatch")
    ws = seg.long_ws(K)
    _call("lr_embed_scatter_add_f32", _ptr(table), V, K, _ptr(grad), _ptr(seg.pos), _ptr(seg.rows), _ptr(seg.start),
          _ptr(seg.n_seg), seg.n, float(alpha), _ptr(ws), 0 if ws is None else ws.numel(), _stream())


def embed_scatter_adam(table: torch.Tensor, m: torch.Tensor, v: torch.Tensor, grad: torch.Tensor,
                       seg: Segments, hp) -> None:
    """`hp`: an `AdamHP` (by value) or an `AdamCoefBuffer` (device-resident coefficients, graph-capturable).
    `grad` may hold more rows than `seg.n` (a prefix of a larger buffer)."""
    _req(table, torch.float32, "table", 2)
    _req(m, torch.float32, "m", 2)
    _req(v, torch.float32, "v", 2)
    _req(grad, torch.float32, "grad")
    V, K = table.shape
    if grad.numel() < seg.n * K or V != seg.V or m.shape != table.shape or v.shape != table.shape:
        raise ValueError("shape mismatch")
    dc = isinstance(hp, AdamCoefBuffer)
    ws = seg.long_ws(K)
    _call("lr_embed_scatter_adam_dc_f32" if dc else "lr_embed_scatter_adam_f32", _ptr(table), _ptr(m), _ptr(v), V, K,
          _ptr(grad), _ptr(seg.pos), _ptr(seg.rows), _ptr(seg.start), _ptr(seg.n_seg), seg.n,
          _ptr(hp.dev) if dc else hp, _ptr(ws), 0 if ws is None else ws.numel(), _stream())


def embed_scatter_adam_lin(table, m, v, grad, lin, lin_m, lin_v, glin, seg: Segments, hp: AdamHP) -> None:
    """`embed_scatter_adam` on a table and on its per-row linear weight ([V,1]) in one pass over the segments."""
    for t_, n_ in ((table, "table"), (m, "m"), (v, "v"), (grad, "grad"), (lin, "lin"), (lin_m, "lin_m"), (lin_v, "lin_v"),
                   (glin, "glin")):
        _req(t_, torch.float32, n_)
    V, K = table.shape
    if grad.numel() != seg.n * K or glin.numel() != seg.n or V != seg.V or lin.numel() != V:
        raise ValueError("shape mismatch")
    dc = isinstance(hp, AdamCoefBuffer)
    _call("lr_embed_scatter_adam_lin_dc_f32" if dc else "lr_embed_scatter_adam_lin_f32", _ptr(table), _ptr(m), _ptr(v),
          V, K, _ptr(grad), _ptr(lin), _ptr(lin_m), _ptr(lin_v), _ptr(glin), _ptr(seg.pos), _ptr(seg.rows),
          _ptr(seg.start), _ptr(seg.n_seg), seg.n, _ptr(hp.dev) if dc else hp, _stream())


def embed_peer_adam(table, m, v, grad, ids, peer_counts, hp: AdamHP, lin=None, lin_m=None, lin_v=None, glin=None,
                    peer_tab: Optional[torch.Tensor] = None) -> None:
    """The owner-side update of the row-sharded tables from the peers' de-duplicated lists (`lr_embed_peer_adam_f32`):
    `ids` int32 [n] local rows (the W lists back to back, `peer_counts` a host list of W lengths), `grad` [n, K] and
    `glin` [n] their gradients, `peer_tab` int32 [V * W] zeros (W > 1)."""
    import ctypes as C

    for t_, n_ in ((table, "table"), (m, "m"), (v, "v"), (grad, "grad")):
        _req(t_, torch.float32, n_)
    _req(ids, torch.int32, "ids", 1)
    V, K = table.shape
    W = len(peer_counts)
    n = int(sum(peer_counts))
    if ids.numel() != n or grad.numel() != n * K or (glin is not None and glin.numel() != n):
        raise ValueError("shape mismatch")
    if W > 1 and (peer_tab is None or peer_tab.numel() < V * W or peer_tab.dtype != torch.int32):
        raise ValueError("peer_tab must be int32 [V * W]")
    counts = (C.c_int64 * W)(*[int(c) for c in peer_counts])
    _call("lr_embed_peer_adam_f32", _ptr(table), _ptr(m), _ptr(v), V, K, _ptr(grad), _ptr(lin), _ptr(lin_m), _ptr(lin_v),
          _ptr(glin), _ptr(ids), C.cast(counts, C.c_void_p), W, _ptr(peer_tab), hp, _stream())


def adam_dense(table: torch.Tensor, m: torch.Tensor, v: torch.Tensor, hp: AdamHP,
               grows: Optional[torch.Tensor] = None, seg: Optional[Segments] = None,
               row_slot: Optional[torch.Tensor] = None, l2: float = 0.0,
               vmax: Optional[torch.Tensor] = None) -> None:
    """Dense Adam over every row (TF1: training/tf_trainer.py:120; torch: torch_trainer.py:63-69).
    ``vmax`` (same shape as ``v``) switches on AMSGrad."""
    if vmax is not None:
        _req(vmax, torch.float32, "vmax")
    _req(table, torch.float32, "table")
    t2 = table.reshape(table.shape[0], -1) if table.dim() != 2 else table
    V, K = t2.shape
    n_max = 0
    if seg is None and grows is not None:  # full dense gradient (MLP / BN parameters)
        _req(grows, torch.float32, "grad")
        if grows.numel() != t2.numel():
            raise ValueError("dense gradient must have the parameter's size")
        _call("lr_adam_dense_f32", _ptr(t2), _ptr(m), _ptr(v), _ptr(vmax), V, K, _ptr(grows), 0, 0, 0,
                                            0, float(l2), hp, _stream())
        return
    if seg is not None and grows is not None and seg.n > 0:
        n_max = seg.n
        if row_slot is None:
            row_slot = torch.full((V,), -1, dtype=torch.int32, device=table.device)
        _req(row_slot, torch.int32, "row_slot", 1)
    _call("lr_adam_dense_f32", _ptr(t2), _ptr(m), _ptr(v), _ptr(vmax), V, K, _ptr(grows),
                                        _ptr(seg.rows) if n_max else 0,
                                        _ptr(seg.n_seg) if n_max else 0, n_max,
                                        _ptr(row_slot) if n_max else 0, float(l2), hp, _stream())


# --------------------------------------------------------------------------------------
# FTRL-proximal on scalar rows (csrc/ftrl.hip)
# --------------------------------------------------------------------------------------
FTRL_LONG_RUN = 32      # kFtrlLongRun / kFtrlChunk of csrc/ftrl.hip: a run of more positions than FTRL_LONG_RUN is cut into
FTRL_CHUNK = 256        # chunks of FTRL_CHUNK positions (tests/test_wide_deep_cpu.py compares both with the source)
FTRL_INIT_ACCUM = 0.1   # tf.train.FtrlOptimizer's initial_accumulator_value; the linear slot starts at 0
_FTRL_WS_AUTO = object()


def _ftrl_slots(var, accum, linear):
    _req(var, torch.float32, "var")
    _req(accum, torch.float32, "accum")
    _req(linear, torch.float32, "linear")
    if accum.numel() != var.numel() or linear.numel() != var.numel():
        raise ValueError("shape mismatch: var, accum and linear must have the same number of elements")


def _ftrl_hp(lr, l1, l2):
    if not lr > 0 or l1 < 0 or l2 < 0:
        raise ValueError(f"FTRL needs lr > 0, l1 >= 0 and l2 >= 0, got lr={lr}, l1={l1}, l2={l2}")
    return float(lr), float(l1), float(l2)


def ftrl_rows(var: torch.Tensor, accum: torch.Tensor, linear: torch.Tensor, grad: torch.Tensor, seg: Segments, lr: float,
              l1: float = 1e-3, l2: float = 0.0, ws=_FTRL_WS_AUTO) -> None:
    """Row-wise FTRL-proximal on a scalar-row table ([V] or [V, 1]) from the per-position gradients `grad` ([seg.n] or
    [seg.n, 1]): each distinct row takes the sum over its run and is read and written once (`lr_ftrl_rows_f32`).
    `ws`: the long-run workspace, by default the persistent one of the segments' builder; None walks every run with one lane."""
    _ftrl_slots(var, accum, linear)
    _req(grad, torch.float32, "grad")
    if var.dim() > 2 or (var.dim() == 2 and var.shape[1] != 1):
        raise ValueError(f"var must be a scalar-row table [V] or [V, 1], got shape {tuple(var.shape)}")
    if grad.numel() != seg.n or var.numel() != seg.V:
        raise ValueError("shape mismatch: one gradient per segmented position, one row per id of the segments")
    hp = _ftrl_hp(lr, l1, l2)
    if ws is _FTRL_WS_AUTO:
        ws = seg.ftrl_ws()
    if ws is not None:
        _req(ws, torch.uint8, "ws", 1)
    _call("lr_ftrl_rows_f32", _ptr(var), _ptr(accum), _ptr(linear), var.numel(), _ptr(grad), _ptr(seg.pos), _ptr(seg.rows),
          _ptr(seg.start), _ptr(seg.n_seg), seg.n, *hp, _ptr(ws), 0 if ws is None else ws.numel(), _stream())


def ftrl_dense(var: torch.Tensor, accum: torch.Tensor, linear: torch.Tensor, grad: torch.Tensor, lr: float, l1: float = 1e-3,
               l2: float = 0.0, l2_grad_coef: float = 0.0) -> None:
    """FTRL-proximal on every element of `var` with the gradient `grad + l2_grad_coef * var` (`lr_ftrl_dense_f32`)."""
    _ftrl_slots(var, accum, linear)
    _req(grad, torch.float32, "grad")
    if grad.numel() != var.numel():
        raise ValueError("shape mismatch: the dense gradient must have the parameter's size")
    hp = _ftrl_hp(lr, l1, l2)
    _call("lr_ftrl_dense_f32", _ptr(var), _ptr(accum), _ptr(linear), var.numel(), _ptr(grad), float(l2_grad_coef), *hp, _stream())


# --------------------------------------------------------------------------------------
# NCF: the two-field front / back of a step and the one-launch inference tower (csrc/ncf.hip)
# --------------------------------------------------------------------------------------
def _ncf_k(K: int) -> int:
    if K % 4 or not 4 <= K <= 128:
        raise ValueError(f"the NCF kernels take K % 4 == 0, 4 <= K <= 128, got K={K}")
    return int(K)


def ncf_pair_fwd(table: torch.Tensor, idx: torch.Tensor, x: Optional[torch.Tensor] = None, gmf: Optional[torch.Tensor] = None):
    """`idx` [B, 2] global (user row, item row) -> x [B, 2K] = [u | i] and gmf [B, K] = u * i, one f32 multiply per element; an
    id outside the table reads as a zero row (`lr_ncf_pair_fwd_f32`).  `x` / `gmf`: buffers of at least B rows to write into."""
    _req(table, torch.float32, "table", 2)
    _req(idx, torch.int32, "idx", 2)
    V, K = table.shape
    _ncf_k(K)
    B = idx.shape[0]
    if idx.shape[1] != 2:
        raise ValueError(f"shape mismatch: idx must be [B, 2], got {tuple(idx.shape)}")
    x = torch.empty((B, 2 * K), dtype=torch.float32, device=table.device) if x is None else _req(x, torch.float32, "x", 2)
    gmf = torch.empty((B, K), dtype=torch.float32, device=table.device) if gmf is None else _req(gmf, torch.float32, "gmf", 2)
    if x.shape[0] < B or x.shape[1] != 2 * K or gmf.shape[0] < B or gmf.shape[1] != K:
        raise ValueError("shape mismatch: x must be [>= B, 2K] and gmf [>= B, K]")
    _call("lr_ncf_pair_fwd_f32", _ptr(table), V, K, _ptr(idx), B, _ptr(x), _ptr(gmf), _stream())
    return x, gmf


def ncf_pair_bwd_(x: torch.Tensor, gl: torch.Tensor, wg: torch.Tensor, G: torch.Tensor, B: Optional[int] = None) -> torch.Tensor:
    """In place on the MLP's row gradient `G` [B, 2K]: G[b, :K] += gl[b] wg * x[b, K:], G[b, K:] += gl[b] wg * x[b, :K], one fma
    per element (`lr_ncf_pair_bwd_f32`).  `B`: the first B rows (default: all of `gl`)."""
    _req(x, torch.float32, "x", 2)
    _req(G, torch.float32, "G", 2)
    _req(gl, torch.float32, "gl", 1)
    _req(wg, torch.float32, "wg")
    K = _ncf_k(wg.numel())
    B = gl.numel() if B is None else int(B)
    if x.shape[1] != 2 * K or G.shape[1] != 2 * K or min(x.shape[0], G.shape[0], gl.numel()) < B:
        raise ValueError("shape mismatch: x and G must be [>= B, 2K], gl [>= B], wg [K]")
    _call("lr_ncf_pair_bwd_f32", _ptr(x), _ptr(gl), _ptr(wg), _ptr(G), B, K, _stream())
    return G


def _c_ints(values):
    import ctypes as C

    return (C.c_int * len(values))(*[int(v) for v in values])


def ncf_score_supported(K: int, widths) -> bool:
    """The envelope of `ncf_score` (`lr_ncf_score_supported`: K, the number of layers, the widths and the 160 KB of LDS)."""
    widths = [int(w) for w in widths]
    return bool(_lib.load().lr_ncf_score_supported(int(K), len(widths), _c_ints(widths)))


def ncf_score(table: torch.Tensor, users: torch.Tensor, items: torch.Tensor, W, b, s, t, wg: torch.Tensor, wd: torch.Tensor,
              c: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[p] = (u * i) . wg + h_L . wd + c for the pairs of global rows (users[p], items[p]) in one launch, with
    h_l = relu(h_{l-1} @ W[l] + b[l]) * s[l] + t[l] and a bare last layer (`lr_ncf_score_f32`).  `W`, `b`: one tensor per layer;
    `s`, `t`: None, or one entry per layer (None: identity).  Outside the envelope (`ncf_score_supported`): ValueError."""
    import ctypes as C

    _req(table, torch.float32, "table", 2)
    _req(users, torch.int32, "users", 1)
    _req(items, torch.int32, "items", 1)
    V, K = table.shape
    L, n = len(W), users.numel()
    if items.numel() != n or len(b) != L or (s is None) != (t is None) or (s is not None and (len(s) != L or len(t) != L)):
        raise ValueError("shape mismatch: one user and one item per pair, one W, b (and s, t) per layer")
    widths, d_in = [], 2 * K
    for l in range(L):
        _req(W[l], torch.float32, f"W[{l}]", 2)
        _req(b[l], torch.float32, f"b[{l}]", 1)
        if W[l].shape[0] != d_in or b[l].numel() != W[l].shape[1]:
            raise ValueError(f"shape mismatch: W[{l}] must be [{d_in}, width] and b[{l}] [width]")
        for name, a in (("s", s), ("t", t)):
            if a is not None and a[l] is not None and _req(a[l], torch.float32, f"{name}[{l}]", 1).numel() != W[l].shape[1]:
                raise ValueError(f"shape mismatch: {name}[{l}] must be [width]")
        if s is not None and (s[l] is None) != (t[l] is None):
            raise ValueError(f"s[{l}] and t[{l}] must be given together")
        d_in = W[l].shape[1]
        widths.append(d_in)
    _req(wg, torch.float32, "wg")
    _req(wd, torch.float32, "wd")
    if wg.numel() != K or wd.numel() != d_in:
        raise ValueError("shape mismatch: wg must be [K] and wd [widths[-1]]")
    out = torch.empty(n, dtype=torch.float32, device=table.device) if out is None else _req(out, torch.float32, "out", 1)
    if out.numel() < n:
        raise ValueError("shape mismatch: out must hold one score per pair")
    ptrs = lambda a: None if a is None else (C.c_void_p * L)(*[_ptr(x) or None for x in a])
    _call("lr_ncf_score_f32", _ptr(table), V, K, _ptr(users), _ptr(items), n, L, _c_ints(widths), ptrs(W), ptrs(b), ptrs(s), ptrs(t),
          _ptr(wg), _ptr(wd), float(c), _ptr(out), _stream())
    return out


# --------------------------------------------------------------------------------------
# FM
# --------------------------------------------------------------------------------------
def fm_pairwise_fwd(e: torch.Tensor, want_sum: bool = True):
    _req(e, torch.float32, "e", 3)
    B, F, K = e.shape
    pair = torch.empty((B, K), dtype=torch.float32, device=e.device)
    fsum = torch.empty((B, K), dtype=torch.float32, device=e.device) if want_sum else None
    _call("lr_fm_pairwise_fwd_f32", _ptr(e), B, F, K, _ptr(pair), _ptr(fsum), _stream())
    return pair, fsum


def fm_pairwise_bwd(e: torch.Tensor, fsum: torch.Tensor, gpair: torch.Tensor,
                    ge: Optional[torch.Tensor] = None) -> torch.Tensor:
    _req(e, torch.float32, "e", 3)
    _req(fsum, torch.float32, "fsum", 2)
    _req(gpair, torch.float32, "gpair", 2)
    B, F, K = e.shape
    acc = 1
    if ge is None:
        ge = torch.empty_like(e)
        acc = 0
    else:
        _req(ge, torch.float32, "ge", 3)
    _call("lr_fm_pairwise_bwd_f32", _ptr(e), _ptr(fsum), _ptr(gpair), B, F, K, _ptr(ge),
                                             acc, _stream())
    return ge


def fm_embed_fwd(table: torch.Tensor, idx: torch.Tensor, want_e: bool = True,
                 lin: Optional[torch.Tensor] = None):
    """Fused gather + pairwise interaction (deepfm.py:155-163 over tfops/features.py:40).
    Returns (e, pair, fsum) or, with `lin` (the linear-weight table), (e, pair, fsum, lin_out)."""
    _req(table, torch.float32, "table", 2)
    _req(idx, torch.int32, "idx", 2)
    V, K = table.shape
    B, F = idx.shape
    dev = table.device
    e = torch.empty((B, F, K), dtype=torch.float32, device=dev) if want_e else None
    pair = torch.empty((B, K), dtype=torch.float32, device=dev)
    fsum = torch.empty((B, K), dtype=torch.float32, device=dev)
    lin_out = None
    if lin is not None:
        _req(lin, torch.float32, "lin")
        if lin.numel() != V:
            raise ValueError("lin must hold one weight per table row")
        lin_out = torch.empty((B, F), dtype=torch.float32, device=dev)
    _call("lr_fm_embed_fwd_f32", _ptr(table), _ptr(lin), V, K, _ptr(idx), B, F, _ptr(e), _ptr(pair),
          _ptr(fsum), _ptr(lin_out), _stream())
    return (e, pair, fsum) if lin is None else (e, pair, fsum, lin_out)


def fm_embed_bwd_adam(table: torch.Tensor, m: torch.Tensor, v: torch.Tensor,
                      gdeep: Optional[torch.Tensor], gpair: torch.Tensor, fsum: torch.Tensor,
                      B: int, F: int, seg: Segments, hp: AdamHP, lin=None, lin_m=None, lin_v=None,
                      glin: Optional[torch.Tensor] = None, bn_a: Optional[torch.Tensor] = None,
                      bn_c: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> None:
    _req(table, torch.float32, "table", 2)
    _req(m, torch.float32, "m", 2)
    _req(v, torch.float32, "v", 2)
    _req(gpair, torch.float32, "gpair", 2)
    _req(fsum, torch.float32, "fsum", 2)
    if glin is not None:          # the C ABI takes the linear gradient field-major [F,B]
        glin = glin.reshape(B, F).t().contiguous()
    for t_, n_ in ((gdeep, "gdeep"), (glin, "glin"), (bn_a, "bn_a"), (bn_c, "bn_c"), (lin, "lin"),
                   (lin_m, "lin_m"), (lin_v, "lin_v")):
        if t_ is not None:
            _req(t_, torch.float32, n_)
    V, K = table.shape
    if seg.n != B * F or seg.V != V:
        raise ValueError("segments were not built over idx[B*F] of this table")
    need = _lib.load().lr_fm_embed_bwd_ws_bytes(B, F)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=table.device)
    _call("lr_fm_embed_bwd_adam_f32", _ptr(table), _ptr(m), _ptr(v), _ptr(lin), _ptr(lin_m),
          _ptr(lin_v), V, K, _ptr(gdeep), _ptr(gpair), _ptr(fsum), _ptr(glin), _ptr(bn_a), _ptr(bn_c),
          B, F, _ptr(seg.pos), _ptr(seg.rows), _ptr(seg.start), _ptr(seg.n_seg), hp, _ptr(ws),
          ws.numel(), _stream())


def fm_embed_bwd_rows(row_cache: torch.Tensor, gdeep: Optional[torch.Tensor], gpair: torch.Tensor,
                      fsum: torch.Tensor, B: int, F: int, seg: Segments,
                      glin: Optional[torch.Tensor] = None, bn_a: Optional[torch.Tensor] = None,
                      bn_c: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None):
    """Per-distinct-row gradients (run order) for row-sharded tables; see the header."""
    _req(row_cache, torch.float32, "row_cache", 2)
    _req(gpair, torch.float32, "gpair", 2)
    _req(fsum, torch.float32, "fsum", 2)
    U, K = row_cache.shape
    dev = row_cache.device
    grows = torch.empty((U, K), dtype=torch.float32, device=dev)
    if glin is not None:          # field-major [F,B] for the C ABI
        glin = glin.reshape(B, F).t().contiguous()
    glin_rows = torch.empty((U,), dtype=torch.float32, device=dev) if glin is not None else None
    need = _lib.load().lr_fm_embed_bwd_ws_bytes(B, F)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _call("lr_fm_embed_bwd_rows_f32", _ptr(row_cache), K, _ptr(gdeep), _ptr(gpair), _ptr(fsum),
          _ptr(glin), _ptr(bn_a), _ptr(bn_c), B, F, _ptr(seg.pos), _ptr(seg.start), _ptr(seg.n_seg),
          _ptr(grows), _ptr(glin_rows), _ptr(ws), ws.numel(), _stream())
    return grows, glin_rows


class AdamCoefBuffer:
    """Step-dependent Adam coefficients in device memory (see lr_adam_coef_store): what the `_dc`
    kernels of a hipGraph-captured training step read."""

    def __init__(self, device: torch.device):
        self.dev = torch.zeros(max(64, _lib.load().lr_adam_coef_bytes()), dtype=torch.uint8, device=device)

    def set(self, hp: AdamHP) -> None:
        """Enqueue (current stream) the write of step `hp.step`'s coefficients."""
        _call("lr_adam_coef_store", hp, _ptr(self.dev), _stream())


def adam_dense_dc(flat: torch.Tensor, m: torch.Tensor, v: torch.Tensor, grad: torch.Tensor, coef: AdamCoefBuffer) -> None:
    for t_, n_ in ((flat, "flat"), (m, "m"), (v, "v"), (grad, "grad")):
        _req(t_, torch.float32, n_)
    if not (flat.numel() == m.numel() == v.numel() == grad.numel()):
        raise ValueError("shape mismatch")
    _call("lr_adam_dense_dc_f32", _ptr(flat), _ptr(m), _ptr(v), flat.numel(), _ptr(grad), _ptr(coef.dev), _stream())


# --------------------------------------------------------------------------------------
# DeepFM: lookup fused with the first Dense layer (f32 MFMA) — see include/libreco_hip.h
# --------------------------------------------------------------------------------------
def deepfm_l1_supported(K: int, H1: int) -> bool:
    return bool(_lib.load().lr_deepfm_l1_supported(int(K), int(H1)))


# Arithmetic of the fused first layer's three contractions (csrc/deepfm_l1_sb.hip vs csrc/deepfm_l1.hip):
#   "split_bf16"  six-term split-bf16 MFMA products, f32 accumulation — the default where the shape is compiled (K = 64, H1 = 128);
#                 as close to f64 as the f32 chain (tests/test_l1_split_bf16_gpu.py), not bit-identical to it
#   "f32_chain"   v_mfma_f32_32x32x2_f32: the exact k-ordered f32 fma chain (every other shape; selectable everywhere)
# The packed-weight buffers carry the choice (uint8 planes vs float32 fragments): a net that allocated its buffers under one
# setting keeps it.  `LIBRECO_L1_ARITH` in the environment sets the initial value.
L1_ARITH = os.environ.get("LIBRECO_L1_ARITH", "split_bf16")
if L1_ARITH not in ("split_bf16", "f32_chain"):
    raise ValueError("LIBRECO_L1_ARITH must be split_bf16 or f32_chain")


def set_l1_arith(mode: str) -> str:
    """Select the arithmetic of first-layer buffers allocated from now on; returns the previous setting."""
    global L1_ARITH
    if mode not in ("split_bf16", "f32_chain"):
        raise ValueError("mode must be 'split_bf16' or 'f32_chain'")
    prev, L1_ARITH = L1_ARITH, mode
    return prev


def deepfm_l1_sb_supported(K: int, H1: int) -> bool:
    return bool(_lib.load().lr_deepfm_l1_sb_supported(int(K), int(H1)))


def deepfm_l1_use_sb(K: int, H1: int) -> bool:
    return L1_ARITH == "split_bf16" and deepfm_l1_sb_supported(K, H1)


def deepfm_l1_pack_bufs(F: int, K: int, H1: int, device, arith: Optional[str] = None):
    """Persistent (forward, row-gradient) packed-kernel buffers of a first layer [F*K, H1] under the current arithmetic."""
    sb = deepfm_l1_use_sb(K, H1) if arith is None else (arith == "split_bf16" and deepfm_l1_sb_supported(K, H1))
    if sb:
        n = _lib.load().lr_deepfm_l1_sb_pack_bytes(F, K, H1)
        return (torch.empty(n, dtype=torch.uint8, device=device), torch.empty(n, dtype=torch.uint8, device=device))
    return (torch.empty((F * K, H1), dtype=torch.float32, device=device),
            torch.empty((F * K, H1), dtype=torch.float32, device=device))


def _is_sb(buf: torch.Tensor) -> bool:
    return buf.dtype == torch.uint8


def deepfm_l1_pack(Wp: torch.Tensor, F: int, K: int, out=None, scale: Optional[torch.Tensor] = None, reduce=None):
    """First kernel Wp [F*K, H1] (optionally row-scaled: the BatchNorm fold, `diag(scale) Wp`) -> (WpA, WpB) in MFMA fragment
    order: f32 fragments for the f32 chain, three bf16 planes each (uint8 buffers) for the split-bf16 kernels — `out` from
    `deepfm_l1_pack_bufs` decides, the current `L1_ARITH` when `out` is None.  `reduce` = (partial [n, H1], out [H1]) with a
    scale: the launch also sums the folded bias's slab partials (no reduction launch of its own)."""
    red = (0, 0, 0)
    if reduce is not None:
        if scale is None:
            raise ValueError("`reduce` rides the scaled pack")
        rp, ro = reduce
        _req(rp, torch.float32, "reduce partial", 2)
        _req(ro, torch.float32, "reduce out", 1)
        if rp.shape[1] != Wp.shape[1] or ro.numel() != Wp.shape[1] or not rp.is_contiguous():
            raise ValueError("reduce = (partial [n, H1] contiguous, out [H1])")
        red = (_ptr(rp), rp.shape[0], _ptr(ro))
    _req(Wp, torch.float32, "Wp", 2)
    H1 = Wp.shape[1]
    if Wp.shape[0] != F * K:
        raise ValueError("Wp must be [F*K, H1]")
    if scale is not None:
        _req(scale, torch.float32, "scale", 1)
        if scale.numel() != F * K:
            raise ValueError("scale must be [F*K]")
    if out is None:
        out = deepfm_l1_pack_bufs(F, K, H1, Wp.device)
    if _is_sb(out[0]):
        n = _lib.load().lr_deepfm_l1_sb_pack_bytes(F, K, H1)
        if not deepfm_l1_sb_supported(K, H1) or out[0].numel() < n or out[1].numel() < n:
            raise ValueError(f"split-bf16 pack buffers do not fit K={K} H1={H1}")
        _call("lr_deepfm_l1_sb_pack", _ptr(Wp), _ptr(scale), F, K, H1, _ptr(out[0]), _ptr(out[1]), *red, _stream())
    elif scale is not None:
        _call("lr_deepfm_l1_pack_scaled_f32", _ptr(Wp), _ptr(scale), F, K, H1, _ptr(out[0]), _ptr(out[1]), *red, _stream())
    else:
        _call("lr_deepfm_l1_pack_f32", _ptr(Wp), F, K, H1, _ptr(out[0]), _ptr(out[1]), _stream())
    return out


_L1_WS: dict = {}     # persistent scratch of the split-bf16 kernels per (device, stream, purpose): addressed by captured graphs


def _l1_ws(device, key, nbytes: int) -> torch.Tensor:
    """One buffer per (device, stream, purpose, size), never released or replaced: a captured step keeps addressing it.  The
    STREAM is part of the key (round-5 advisor finding): launches on one stream are ordered and may share scratch, two nets whose
    captured steps replay on their own streams (`GraphRunner` has one per net) must not."""
    dev_i = device.index if device.index is not None else torch.cuda.current_device()
    k = (dev_i, int(torch.cuda.current_stream(dev_i).cuda_stream), key, int(nbytes))
    t = _L1_WS.get(k)
    if t is None:
        t = _L1_WS[k] = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)
    return t


def deepfm_l1_fwd(table: torch.Tensor, idx: torch.Tensor, WpA: torch.Tensor, bias: Optional[torch.Tensor],
                  H1: int, lin: Optional[torch.Tensor] = None, out=None):
    """(z1 [B,H1], pair [B,K], fsum [B,K], lin_out [B,F] | None).  `out` = (z1, pair, fsum) persistent buffers.
    `WpA` from `deepfm_l1_pack`: its kind selects the kernel (`lr_deepfm_l1_fwd_f32` / `lr_deepfm_l1_fwd_sb_f32`)."""
    _req(table, torch.float32, "table", 2)
    _req(idx, torch.int32, "idx", 2)
    V, K = table.shape
    B, F = idx.shape
    sb = _is_sb(WpA)
    if sb:
        if not deepfm_l1_sb_supported(K, H1) or WpA.numel() < _lib.load().lr_deepfm_l1_sb_pack_bytes(F, K, H1):
            raise ValueError("WpA must come from deepfm_l1_pack for this shape")
    else:
        _req(WpA, torch.float32, "WpA")
        if WpA.numel() != F * K * H1:
            raise ValueError("WpA has the wrong size")
    dev = table.device
    if out is not None:
        z1, pair, fsum = out
        if z1.shape != (B, H1) or pair.shape != (B, K) or fsum.shape != (B, K):
            raise ValueError("out buffers have the wrong shape")
    else:
        z1 = torch.empty((B, H1), dtype=torch.float32, device=dev)
        pair = torch.empty((B, K), dtype=torch.float32, device=dev)
        fsum = torch.empty((B, K), dtype=torch.float32, device=dev)
    lin_out = None
    if lin is not None:
        _req(lin, torch.float32, "lin")
        lin_out = torch.empty((B, F), dtype=torch.float32, device=dev)
    if bias is not None:
        _req(bias, torch.float32, "bias", 1)
    if sb:
        need = _lib.load().lr_deepfm_l1_fwd_sb_ws_bytes(B, F)
        ws = _l1_ws(dev, "fwd", need)
        _call("lr_deepfm_l1_fwd_sb_f32", _ptr(table), _ptr(lin), V, K, _ptr(idx), B, F, _ptr(WpA), _ptr(bias), H1,
              _ptr(z1), _ptr(pair), _ptr(fsum), _ptr(lin_out), _ptr(ws), ws.numel(), _stream())
    else:
        _call("lr_deepfm_l1_fwd_f32", _ptr(table), _ptr(lin), V, K, _ptr(idx), B, F, _ptr(WpA), _ptr(bias), H1,
              _ptr(z1), _ptr(pair), _ptr(fsum), _ptr(lin_out), _stream())
    return z1, pair, fsum, lin_out


def deepfm_l1_wgrad_chunks(B: int, F: int, K: int, H1: int, arith: Optional[str] = None) -> int:
    """Batch chunks of the weight-gradient kernel the current arithmetic would use for this shape."""
    sb = deepfm_l1_use_sb(K, H1) if arith is None else (arith == "split_bf16" and deepfm_l1_sb_supported(K, H1))
    return int(_lib.load().lr_deepfm_l1_wgrad_sb_chunks(B, F) if sb else _lib.load().lr_deepfm_l1_wgrad_chunks(B, F))


def deepfm_l1_wgrad(table: torch.Tensor, idxT: torch.Tensor, gz: torch.Tensor, n_chunks: Optional[int] = None,
                    out: Optional[torch.Tensor] = None, arith: Optional[str] = None) -> torch.Tensor:
    """partial [n_chunks, F*K, H1]; gather(table, idx)^T @ gz = partial.sum(0).  `arith` (default: `L1_ARITH`) selects
    `lr_deepfm_l1_wgrad_sb_f32` (gz split into bf16 planes first: `lr_deepfm_l1_sb_gz_pack`) or `lr_deepfm_l1_wgrad_f32`;
    an `out` buffer fixes the number of chunks (any value is valid for both kernels)."""
    _req(table, torch.float32, "table", 2)
    _req(idxT, torch.int32, "idxT", 2)
    _req(gz, torch.float32, "gz", 2)
    V, K = table.shape
    F, B = idxT.shape
    H1 = gz.shape[1]
    if gz.shape[0] != B:
        raise ValueError("gz must be [B, H1]")
    sb = deepfm_l1_use_sb(K, H1) if arith is None else (arith == "split_bf16" and deepfm_l1_sb_supported(K, H1))
    if out is not None:
        if out.numel() % (F * K * H1) != 0 or out.numel() == 0:
            raise ValueError("out has the wrong size")
        if n_chunks is None:
            n_chunks = out.numel() // (F * K * H1)
        elif out.numel() != n_chunks * F * K * H1:
            raise ValueError("out has the wrong size")
    if n_chunks is None:
        n_chunks = deepfm_l1_wgrad_chunks(B, F, K, H1, "split_bf16" if sb else "f32_chain")
    if out is None:
        out = torch.empty((n_chunks, F * K, H1), dtype=torch.float32, device=table.device)
    if B == 0:
        return out.zero_()
    if sb:
        gzp = _l1_ws(table.device, "gzp", _lib.load().lr_deepfm_l1_sb_gz_pack_bytes(B, H1))
        _call("lr_deepfm_l1_sb_gz_pack", _ptr(gz), B, H1, _ptr(gzp), _stream())
        _call("lr_deepfm_l1_wgrad_sb_f32", _ptr(table), V, K, _ptr(idxT), B, F, _ptr(gzp), H1, n_chunks, _ptr(out), _stream())
    else:
        _call("lr_deepfm_l1_wgrad_f32", _ptr(table), V, K, _ptr(idxT), B, F, _ptr(gz), H1, n_chunks, _ptr(out), _stream())
    return out


def deepfm_l1_dgrad(gz: torch.Tensor, WpB: torch.Tensor, K: int, F: int, slotT: torch.Tensor,
                    gl: Optional[torch.Tensor] = None, wp: Optional[torch.Tensor] = None,
                    fsum: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ge [B*F + 1, K]: per-position row gradients in run order; dropped positions land in the spare last row.
    `WpB` from `deepfm_l1_pack`: its kind selects the kernel (`lr_deepfm_l1_dgrad_f32` / `lr_deepfm_l1_dgrad_sb_f32`)."""
    _req(gz, torch.float32, "gz", 2)
    _req(slotT, torch.int32, "slotT", 2)
    B, H1 = gz.shape
    sb = _is_sb(WpB)
    if slotT.shape != (F, B):
        raise ValueError("shape mismatch")
    if sb:
        if not deepfm_l1_sb_supported(K, H1) or WpB.numel() < _lib.load().lr_deepfm_l1_sb_pack_bytes(F, K, H1):
            raise ValueError("WpB must come from deepfm_l1_pack for this shape")
    else:
        _req(WpB, torch.float32, "WpB")
        if WpB.numel() != F * K * H1:
            raise ValueError("shape mismatch")
    for t_, n_ in ((gl, "gl"), (wp, "wp"), (fsum, "fsum")):
        if t_ is not None:
            _req(t_, torch.float32, n_)
    if out is None:
        out = torch.empty((B * F + 1, K), dtype=torch.float32, device=gz.device)    # + the spare row of dropped positions
    elif out.numel() < (B * F + 1) * K:
        raise ValueError("ge must hold B*F + 1 rows")
    _call("lr_deepfm_l1_dgrad_sb_f32" if sb else "lr_deepfm_l1_dgrad_f32", _ptr(gz), H1, _ptr(WpB), K, F, B, _ptr(gl),
          _ptr(wp), _ptr(fsum), _ptr(slotT), _ptr(out), _stream())
    return out


def fm_rows_adam(table: torch.Tensor, m: torch.Tensor, v: torch.Tensor, ge: torch.Tensor, seg: Segments,
                 hp, B: int, F: int, gl=None, wp=None, lin=None, lin_m=None, lin_v=None, bn_a=None,
                 bn_c=None, lin_scale=None, ws: Optional[torch.Tensor] = None) -> None:
    """Adam over run-ordered per-position gradients (see lr_fm_rows_adam_f32).  `hp`: an `AdamHP`
    (by value) or an `AdamCoefBuffer` (device-resident coefficients, graph-capturable)."""
    _req(table, torch.float32, "table", 2)
    _req(m, torch.float32, "m", 2)
    _req(v, torch.float32, "v", 2)
    _req(ge, torch.float32, "ge", 2)
    for t_, n_ in ((gl, "gl"), (wp, "wp"), (lin, "lin"), (lin_m, "lin_m"), (lin_v, "lin_v"), (bn_a, "bn_a"),
                   (bn_c, "bn_c"), (lin_scale, "lin_scale")):
        if t_ is not None:
            _req(t_, torch.float32, n_)
    V, K = table.shape
    if seg.n != B * F or seg.V != V or ge.dim() != 2 or ge.shape[1] != K or ge.shape[0] < B * F:
        raise ValueError("segments / ge were not built over idx[B*F] of this table")
    need = _lib.load().lr_fm_embed_bwd_ws_bytes(B, F)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=table.device)
    dc = isinstance(hp, AdamCoefBuffer)
    _call("lr_fm_rows_adam_dc_f32" if dc else "lr_fm_rows_adam_f32", _ptr(table), _ptr(m), _ptr(v), _ptr(lin),
          _ptr(lin_m), _ptr(lin_v), V, K, _ptr(ge), _ptr(gl), _ptr(wp), _ptr(bn_a), _ptr(bn_c), _ptr(lin_scale), B, F,
          _ptr(seg.pos), _ptr(seg.rows), _ptr(seg.start), _ptr(seg.n_seg), _ptr(hp.dev) if dc else hp, _ptr(ws),
          ws.numel(), _stream())


def fm_rows_grad(cache: torch.Tensor, lin_cache: Optional[torch.Tensor], ge: torch.Tensor, seg: Segments, B: int,
                 F: int, slots: torch.Tensor, gl, wp, bn_a=None, bn_c=None, lin_scale=None,
                 ws: Optional[torch.Tensor] = None):
    """Row-sharded tables: per-row gradients of the run-ordered per-position gradients `ge` (the arithmetic of
    `fm_rows_adam` without the update), written at the rows' cache slots: returns (grows [n_cache, K],
    glin_rows [n_cache] or None).  `seg`: per-field runs of the GLOBAL ids, `slots` [B*F]: position -> cache row."""
    _req(cache, torch.float32, "cache", 2)
    _req(ge, torch.float32, "ge", 2)
    _req(slots, torch.int32, "slots")
    n_cache, K = cache.shape
    if seg.n != B * F or slots.numel() != B * F or ge.shape[1] != K or ge.shape[0] < B * F:
        raise ValueError("segments / slots / ge were not built over idx[B*F]")
    grows = torch.empty((n_cache, K), dtype=torch.float32, device=cache.device)
    glin = torch.empty(n_cache, dtype=torch.float32, device=cache.device) if lin_cache is not None else None
    need = _lib.load().lr_fm_embed_bwd_ws_bytes(B, F)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=cache.device)
    _call("lr_fm_rows_grad_f32", _ptr(cache), _ptr(lin_cache), n_cache, K, _ptr(ge), _ptr(gl), _ptr(wp), _ptr(bn_a),
          _ptr(bn_c), _ptr(lin_scale), B, F, _ptr(seg.pos), _ptr(seg.rows), _ptr(seg.start), _ptr(seg.n_seg),
          _ptr(slots), _ptr(grows), _ptr(glin), _ptr(ws), ws.numel(), _stream())
    return grows, glin


def fm_rows_grad_compact(table: torch.Tensor, lin: Optional[torch.Tensor], ge: torch.Tensor, seg: Segments, B: int, F: int,
                         gl, wp, bn_a=None, bn_c=None, lin_scale=None, ws: Optional[torch.Tensor] = None, out=None):
    """The per-row gradients of `fm_rows_adam` WITHOUT the update, rows read from the tables themselves, run s writing
    grows[s] / glin_rows[s]: the operand of the dense (TF1) table pass `adam_dense_rows`.  `out`: persistent
    (grows [>= B*F, K], glin_rows [>= B*F] or None) buffers of a captured step."""
    _req(table, torch.float32, "table", 2)
    _req(ge, torch.float32, "ge", 2)
    V, K = table.shape
    if seg.n != B * F or seg.V != V or ge.shape[1] != K or ge.shape[0] < B * F:
        raise ValueError("segments / ge were not built over idx[B*F] of this table")
    if out is None:
        out = (torch.empty((B * F, K), dtype=torch.float32, device=table.device),
               torch.empty(B * F, dtype=torch.float32, device=table.device) if lin is not None else None)
    grows, glin = out
    if grows.shape[0] < B * F or grows.shape[1] != K or (glin is None) != (lin is None) or (glin is not None and glin.numel() < B * F):
        raise ValueError("`out` must hold one row per position")
    need = _lib.load().lr_fm_embed_bwd_ws_bytes(B, F)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=table.device)
    _call("lr_fm_rows_grad_compact_f32", _ptr(table), _ptr(lin), V, K, _ptr(ge), _ptr(gl), _ptr(wp), _ptr(bn_a), _ptr(bn_c),
          _ptr(lin_scale), B, F, _ptr(seg.pos), _ptr(seg.rows), _ptr(seg.start), _ptr(seg.n_seg), _ptr(grows), _ptr(glin),
          _ptr(ws), ws.numel(), _stream())
    return grows, glin


def adam_dense_rows(table, m, v, hp, grows, seg: Segments, row_slot: torch.Tensor, lin=None, lin_m=None, lin_v=None,
                    glin_rows=None) -> None:
    """TF1's dense Adam over EVERY row of `table` [V, K] (and of `lin` [V]) in one streaming launch; the rows of
    `seg.rows[:n_seg]` take `grows[s]` / `glin_rows[s]`.  `row_slot`: int32 [V], all -1 (restored on return).
    `hp`: an `AdamHP` (by value) or an `AdamCoefBuffer` (graph-capturable)."""
    for t_, n_ in ((table, "table"), (m, "m"), (v, "v"), (grows, "grows")):
        _req(t_, torch.float32, n_, 2)
    _req(row_slot, torch.int32, "row_slot", 1)
    V, K = table.shape
    if row_slot.numel() != V or seg.V != V or grows.shape[1] != K or grows.shape[0] < seg.n:
        raise ValueError("row_slot / segments / grows do not belong to this table")
    dc = isinstance(hp, AdamCoefBuffer)
    _call("lr_adam_dense_rows_dc_f32" if dc else "lr_adam_dense_rows_f32", _ptr(table), _ptr(m), _ptr(v), _ptr(lin), _ptr(lin_m),
          _ptr(lin_v), V, K, _ptr(grows), _ptr(glin_rows), _ptr(seg.rows), _ptr(seg.n_seg), seg.n, _ptr(row_slot),
          _ptr(hp.dev) if dc else hp, _stream())


# --------------------------------------------------------------------------------------
# full-catalog scoring + top-k
# --------------------------------------------------------------------------------------
# Arithmetic of the score contraction: "f32_chain" = the exact k-ordered f32 fma chain on the f32 MFMA pipe; "split_bf16" = six
# bf16 MFMA products per f32 product with f32 accumulation (as close to fp64 as the chain, not bit-identical to it; the item
# planes are split on the fly).  An explicit argument of every call (no library-side state); `LIBRECO_TOPK_ARITH` only sets the
# default the Python callers pass.
# "filter" (the default) / "filter_f32_chain": lr_score_topk_filter_f32 — a one-product bf16 pass keeps k' > k candidates per
# user (ranked by an upper bound of the exact score), f32 scores of those, a PROOF per user that nothing outside the k' can be in
# the top k (its k-th exact score exceeds the k'-th bound), and the exact kernel (split-bf16 /
# f32 chain) for the users without a proof and for the shapes the filter does not take (below 2^20 items, k > 100, reduction
# widths outside 33..128).  44.5 ms per 1,024 users x 100 M items pass against 144 ms (split_bf16) and 209 ms (f32_chain); ids
# equal to the fp64 ranking wherever fp64 scores are separated by more than f32 rounding (tests/test_fullsize_parity_gpu.py, all
# three forms).  TOPK_FILTER_FORCE takes the filter below 2^20 items too (tests).
_TOPK_ARITHS = ("split_bf16", "f32_chain", "filter", "filter_f32_chain")
TOPK_ARITH = os.environ.get("LIBRECO_TOPK_ARITH", "filter")
if TOPK_ARITH not in _TOPK_ARITHS:
    raise ValueError(f"LIBRECO_TOPK_ARITH must be one of {_TOPK_ARITHS}")
TOPK_FILTER_FORCE = False


def score_topk(users: torch.Tensor, items: torch.Tensor, k: int,
               consumed_ptr: Optional[torch.Tensor] = None,
               consumed_idx: Optional[torch.Tensor] = None,
               filter_flag: Optional[torch.Tensor] = None, item_base: int = 0,
               ws: Optional[torch.Tensor] = None, arith: Optional[str] = None,
               failed_out: Optional[torch.Tensor] = None):
    """``users @ items.T`` + per-user top-k (recommendation/recommend.py:66-68 + ranking.py).  `failed_out` ([B] uint8, the
    filtered forms only): 1 where a user was not certified by the filter and was ranked by the exact kernel."""
    arith = TOPK_ARITH if arith is None else arith
    if arith not in _TOPK_ARITHS:
        raise ValueError(f"arith must be one of {_TOPK_ARITHS}")
    filt = arith.startswith("filter")
    _req(users, torch.float32, "users", 2)
    _req(items, torch.float32, "items", 2)
    B, D = users.shape
    N = items.shape[0]
    if items.shape[1] != D:
        raise ValueError("users and items must share the embedding width")
    if k > N:
        raise ValueError(f"`n_rec` {k} exceeds num of items {N}")
    if D % 4 != 0:  # the MFMA path needs 16-byte rows: pad the (tiny) reduction dim with zeros
        pad = 4 - D % 4
        users = torch.nn.functional.pad(users, (0, pad)).contiguous()
        items = torch.nn.functional.pad(items, (0, pad)).contiguous()
        D += pad
    lib = _lib.load()
    need = (lib.lr_score_topk_filter_ws_bytes if filt else lib.lr_score_topk_ws_bytes)(B, N, D, k)
    if need == 0 and B > 0 and N > 0:
        raise ValueError(f"unsupported score_topk shape B={B} N={N} D={D} k={k}")
    if ws is None or ws.numel() < need:
        ws = torch.empty(max(need, 8), dtype=torch.uint8, device=users.device)
    if consumed_ptr is not None:
        _req(consumed_ptr, torch.int64, "consumed_ptr", 1)
        _req(consumed_idx, torch.int32, "consumed_idx", 1)
    if filter_flag is not None:
        _req(filter_flag, torch.uint8, "filter_flag", 1)
    out_s = torch.empty((B, k), dtype=torch.float32, device=users.device)
    out_i = torch.empty((B, k), dtype=torch.int64, device=users.device)
    if filt:
        if failed_out is not None:
            _req(failed_out, torch.uint8, "failed_out", 1)
            if failed_out.numel() < B:
                raise ValueError("failed_out holds one byte per user")
        _call("lr_score_topk_filter_f32", _ptr(users), B, _ptr(items), N, D, _ptr(consumed_ptr), _ptr(consumed_idx),
              _ptr(filter_flag), k, item_base, _ptr(out_s), _ptr(out_i), _ptr(ws), ws.numel(),
              0 if arith == "filter_f32_chain" else 1, 1 if TOPK_FILTER_FORCE else 0, _ptr(failed_out), _stream())
        return out_s, out_i
    if failed_out is not None:
        raise ValueError("failed_out belongs to the filtered forms")
    _call("lr_score_topk_sb_f32" if arith == "split_bf16" else "lr_score_topk_f32", _ptr(users), B, _ptr(items), N, D, _ptr(consumed_ptr),
                                _ptr(consumed_idx), _ptr(filter_flag), k, item_base, _ptr(out_s),
                                _ptr(out_i), _ptr(ws), ws.numel(), _stream())
    return out_s, out_i


# --------------------------------------------------------------------------------------
# IVF-Flat index (csrc/ivf.hip): assignment, list build, centroid means, list scan with fused filter + top-k
# --------------------------------------------------------------------------------------
IVF_MAX_NLIST = 65536
IVF_MAX_K = 1024


def _ivf_pad(*mats: torch.Tensor):
    """Rows of a width that is no multiple of 4 are zero-padded (16-byte rows), as `score_topk` does."""
    D = mats[0].shape[1]
    if D % 4 == 0:
        return mats
    pad = 4 - D % 4
    return tuple(torch.nn.functional.pad(m, (0, pad)).contiguous() for m in mats)


def _ivf_check_width(D: int, what: str) -> None:
    if D < 1 or D > 256:
        raise ValueError(f"{what}: shape not supported (row width {D} outside 1..256)")


def _topk_out(out: Optional[tuple], B: int, k: int, dev, what: str):
    """The (scores [B, k] f32, ids [B, k] int64) pair a search writes: new tensors, or the caller's `out` after its checks (`what`
    is the name of k in the error)."""
    if out is None:
        return torch.empty((B, k), dtype=torch.float32, device=dev), torch.empty((B, k), dtype=torch.int64, device=dev)
    out_s, out_i = _req(out[0], torch.float32, "out scores", 2), _req(out[1], torch.int64, "out ids", 2)
    if tuple(out_s.shape) != (B, k) or tuple(out_i.shape) != (B, k):
        raise ValueError(f"out must be ([B, {what}] f32, [B, {what}] int64)")
    return out_s, out_i


def _ivf_search_common(queries, centroids, lists, list_ptr, list_ids, consumed_ptr, consumed_idx, filter_flag) -> None:
    """Device, dtype and rank checks of a search's tensors; `lists` is the format's own payload as (tensor, dtype, name, rank)."""
    _req(queries, torch.float32, "queries", 2)
    _req(centroids, torch.float32, "centroids", 2)
    for t, dtype, name, rank in lists:
        _req(t, dtype, name, rank)
    _req(list_ptr, torch.int64, "list_ptr", 1)
    _req(list_ids, torch.int32, "list_ids", 1)
    if consumed_ptr is not None:
        _req(consumed_ptr, torch.int64, "consumed_ptr", 1)
        _req(consumed_idx, torch.int32, "consumed_idx", 1)
    if filter_flag is not None:
        _req(filter_flag, torch.uint8, "filter_flag", 1)


def ivf_assign(rows: torch.Tensor, centroids: torch.Tensor, want_score: bool = False):
    """int32 [n]: for every row the centroid of largest inner product, ties to the lowest list id (`lr_ivf_assign_f32`);
    with `want_score` also that inner product."""
    if rows.dim() != 2 or centroids.dim() != 2 or rows.shape[1] != centroids.shape[1]:
        raise ValueError("rows and centroids must be 2-d and share the embedding width")
    n, D = rows.shape
    nlist = centroids.shape[0]
    if nlist < 1 or nlist > IVF_MAX_NLIST or n >= 2 ** 31:
        raise ValueError(f"ivf_assign: shape not supported (n={n}, nlist={nlist})")
    _ivf_check_width(D, "ivf_assign")
    _req(rows, torch.float32, "rows", 2)
    _req(centroids, torch.float32, "centroids", 2)
    rows, centroids = _ivf_pad(rows, centroids)
    out = torch.empty(n, dtype=torch.int32, device=rows.device)
    best = torch.empty(n, dtype=torch.float32, device=rows.device) if want_score else None
    _call("lr_ivf_assign_f32", _ptr(rows), n, _ptr(centroids), nlist, rows.shape[1], _ptr(out), _ptr(best), _stream())
    return (out, best) if want_score else out


def ivf_build_lists(list_of: torch.Tensor, nlist: int, rows: Optional[torch.Tensor] = None):
    """Stable counting sort of the assignment: `list_ptr` int64 [nlist + 1], `list_ids` int32 [n] ascending within a list and,
    when `rows` is given, `list_rows` = rows[list_ids] (`lr_ivf_build_lists` + `lr_embed_gather_f32`)."""
    if not 1 <= int(nlist) <= IVF_MAX_NLIST:
        raise ValueError(f"ivf_build_lists: shape not supported (nlist={nlist})")
    _req(list_of, torch.int32, "list_of", 1)
    n = list_of.numel()
    if rows is not None:
        _req(rows, torch.float32, "rows", 2)
        if rows.shape[0] != n:
            raise ValueError("rows and list_of must have one entry per row")
    dev = list_of.device
    list_ptr = torch.empty(nlist + 1, dtype=torch.int64, device=dev)
    list_ids = torch.empty(n, dtype=torch.int32, device=dev)
    ws = torch.empty(max(_lib.load().lr_ivf_build_ws_bytes(n, nlist), 256), dtype=torch.uint8, device=dev)
    _call("lr_ivf_build_lists", _ptr(list_of), n, int(nlist), _ptr(list_ptr), _ptr(list_ids), _ptr(ws), ws.numel(), _stream())
    if rows is None:
        return list_ptr, list_ids
    list_rows = embed_gather(rows, list_ids) if n else torch.empty((0, rows.shape[1]), dtype=torch.float32, device=dev)
    return list_ptr, list_ids, list_rows


def ivf_centroids(rows: torch.Tensor, list_ptr: torch.Tensor, list_ids: torch.Tensor, centroids: torch.Tensor) -> torch.Tensor:
    """In place: `centroids[l]` = f32 mean of `rows[list_ids[list_ptr[l]:list_ptr[l+1]]]` (fixed summation order, one division);
    an empty list keeps its centroid (`lr_ivf_centroids_f32`).  Widths that are no multiple of 4 are not taken here."""
    _req(rows, torch.float32, "rows", 2)
    _req(centroids, torch.float32, "centroids", 2)
    _req(list_ptr, torch.int64, "list_ptr", 1)
    _req(list_ids, torch.int32, "list_ids", 1)
    D = rows.shape[1]
    nlist = centroids.shape[0]
    if centroids.shape[1] != D or list_ptr.numel() != nlist + 1:
        raise ValueError("centroids must be [nlist, D] and list_ptr [nlist + 1]")
    if D % 4 != 0 or D > 256 or nlist > IVF_MAX_NLIST:
        raise ValueError(f"ivf_centroids: shape not supported (D={D}, nlist={nlist})")
    n = list_ids.numel()
    ws = torch.empty(max(_lib.load().lr_ivf_centroids_ws_bytes(n, D), 256), dtype=torch.uint8, device=rows.device)
    _call("lr_ivf_centroids_f32", _ptr(rows), rows.shape[0], D, _ptr(list_ptr), _ptr(list_ids), n, nlist, _ptr(centroids),
          _ptr(ws), ws.numel(), _stream())
    return centroids


def ivf_check_search_args(B: int, N: int, D: int, Dq: int, k: int, nprobe: int, nlist: int) -> None:
    """The argument errors of `ivf_search`, raised before a device is needed."""
    if D != Dq:
        raise ValueError(f"queries have width {Dq}, the index {D}")
    if k < 1:
        raise ValueError(f"k must be >= 1, got {k}")
    if nlist > N:
        raise ValueError(f"nlist {nlist} exceeds the number of rows {N}")
    if nprobe < 1 or nprobe > nlist:
        raise ValueError(f"nprobe must be in 1..nlist ({nlist}), got {nprobe}")


def ivf_search(queries: torch.Tensor, centroids: torch.Tensor, list_ptr: torch.Tensor, list_ids: torch.Tensor,
               list_rows: torch.Tensor, k: int, nprobe: int, consumed_ptr: Optional[torch.Tensor] = None,
               consumed_idx: Optional[torch.Tensor] = None, filter_flag: Optional[torch.Tensor] = None,
               out: Optional[tuple] = None):
    """Top-k by (score desc, global id asc) among the rows of the `nprobe` best lists of every query (`lr_ivf_search_f32`);
    the output contract is `score_topk`'s.  `out`: (scores [B, k] f32, ids [B, k] int64) to write into."""
    if queries.dim() != 2 or centroids.dim() != 2 or list_rows.dim() != 2:
        raise ValueError("queries, centroids and list_rows must be 2-d")
    B, Dq = queries.shape
    N, D = list_rows.shape
    nlist = centroids.shape[0]
    k, nprobe = int(k), int(nprobe)
    ivf_check_search_args(B, N, D, Dq, k, nprobe, nlist)
    if centroids.shape[1] != D or list_ptr.numel() != nlist + 1 or list_ids.numel() != N:
        raise ValueError("centroids / list_ptr / list_ids do not describe list_rows")
    _ivf_check_width(D, "ivf_search")
    Dp = (D + 3) // 4 * 4
    lib = _lib.load()
    if B > 0 and not lib.lr_ivf_supported(B, N, Dp, k, nprobe, nlist):
        raise ValueError(f"ivf_search: shape not supported (B={B} N={N} D={D} k={k} nprobe={nprobe} nlist={nlist})")
    _ivf_search_common(queries, centroids, [(list_rows, torch.float32, "list_rows", 2)], list_ptr, list_ids, consumed_ptr,
                       consumed_idx, filter_flag)
    queries, centroids, list_rows = _ivf_pad(queries, centroids, list_rows)
    dev = queries.device
    out_s, out_i = _topk_out(out, B, k, dev, "k")
    if B == 0:
        return out_s, out_i
    ws = torch.empty(lib.lr_ivf_search_ws_bytes(B, N, Dp, k, nprobe, nlist), dtype=torch.uint8, device=dev)
    _call("lr_ivf_search_f32", _ptr(queries), B, _ptr(centroids), nlist, _ptr(list_ptr), _ptr(list_ids), _ptr(list_rows), N, Dp,
          _ptr(consumed_ptr), _ptr(consumed_idx), _ptr(filter_flag), k, nprobe, _ptr(out_s), _ptr(out_i), _ptr(ws), ws.numel(),
          _stream())
    return out_s, out_i


# --------------------------------------------------------------------------------------
# IVF-SQ8 index (csrc/ivf_sq8.hip): int8 list codes with one f32 scale per row, scan with fused filter + top-kk, exact re-rank
# --------------------------------------------------------------------------------------
IVF_SQ8_MAX_REFINE = 64


def ivf_sq8_stride(D: int) -> int:
    """Bytes of a stored code row: the width rounded up to 16 (one 16-byte load per lane); the padding holds code 0."""
    return (int(D) + 15) // 16 * 16


def ivf_sq8_kk(k: int, refine: int) -> int:
    """Candidates the scan keeps per query: k without re-rank, else min(max(k, k * refine), 1024)."""
    return int(k) if int(refine) == 0 else min(max(int(k), int(k) * int(refine)), IVF_MAX_K)


def ivf_sq8_encode(rows: torch.Tensor, list_ids: Optional[torch.Tensor] = None):
    """(codes int8 [n, stride], scales f32 [n]): row j encodes `rows[list_ids[j]]` (`rows[j]` without `list_ids`), gather and
    encode in one pass (`lr_ivf_sq8_encode_f32`): scale = max|x| / 127, code = clamp(rint(x / scale), -127, 127), a zero row has
    scale 0."""
    if not isinstance(rows, torch.Tensor) or rows.dim() != 2:
        raise ValueError("rows must be a 2-d tensor")
    n_rows, D = rows.shape
    _ivf_check_width(D, "ivf_sq8_encode")
    if n_rows >= 2 ** 31:
        raise ValueError(f"ivf_sq8_encode: shape not supported (n_rows={n_rows})")
    _req(rows, torch.float32, "rows", 2)
    if list_ids is not None:
        _req(list_ids, torch.int32, "list_ids", 1)
    n = n_rows if list_ids is None else list_ids.numel()
    stride = ivf_sq8_stride(D)
    (rows,) = _ivf_pad(rows)
    dev = rows.device
    codes = torch.empty((n, stride), dtype=torch.int8, device=dev)
    scales = torch.empty(n, dtype=torch.float32, device=dev)
    _call("lr_ivf_sq8_encode_f32", _ptr(rows), n_rows, rows.shape[1], _ptr(list_ids), n, _ptr(codes), stride, _ptr(scales), _stream())
    return codes, scales


def ivf_sq8_check_search_args(B: int, N: int, D: int, Dq: int, k: int, nprobe: int, nlist: int, refine: int) -> None:
    """The argument errors of `ivf_sq8_search` and `IVFSQ8Index.search`, raised before a device is needed."""
    ivf_check_search_args(B, N, D, Dq, k, nprobe, nlist)
    if refine < 0:
        raise ValueError(f"refine must be >= 0, got {refine}")
    if refine > IVF_SQ8_MAX_REFINE or k > IVF_MAX_K:
        raise ValueError(f"ivf_sq8_search: shape not supported (k={k} refine={refine})")


def ivf_sq8_search(queries: torch.Tensor, centroids: torch.Tensor, list_ptr: torch.Tensor, list_ids: torch.Tensor,
                   codes: torch.Tensor, scales: torch.Tensor, kk: int, nprobe: int, consumed_ptr: Optional[torch.Tensor] = None,
                   consumed_idx: Optional[torch.Tensor] = None, filter_flag: Optional[torch.Tensor] = None,
                   out: Optional[tuple] = None):
    """Stage 1 of the SQ8 search (`lr_ivf_sq8_search_f32`): the `kk` largest `scale_j * dot(q, codes_j)` by (score desc, global
    id asc) among the rows of the `nprobe` best lists; filter and output contract as `ivf_search`."""
    if queries.dim() != 2 or centroids.dim() != 2 or codes.dim() != 2:
        raise ValueError("queries, centroids and codes must be 2-d")
    B, D = queries.shape
    N, stride = codes.shape
    nlist = centroids.shape[0]
    kk, nprobe = int(kk), int(nprobe)
    ivf_check_search_args(B, N, centroids.shape[1], D, kk, nprobe, nlist)
    _ivf_check_width(D, "ivf_sq8_search")
    if stride != ivf_sq8_stride(D) or list_ptr.numel() != nlist + 1 or list_ids.numel() != N or scales.numel() != N:
        raise ValueError("centroids / list_ptr / list_ids / scales do not describe codes")
    Dp = (D + 3) // 4 * 4
    lib = _lib.load()
    ws_bytes = lib.lr_ivf_sq8_search_ws_bytes(B, N, Dp, kk, nprobe, nlist) if B > 0 else 0
    if B > 0 and ws_bytes == 0:
        raise ValueError(f"ivf_sq8_search: shape not supported (B={B} N={N} D={D} kk={kk} nprobe={nprobe} nlist={nlist})")
    _ivf_search_common(queries, centroids, [(codes, torch.int8, "codes", 2), (scales, torch.float32, "scales", 1)], list_ptr,
                       list_ids, consumed_ptr, consumed_idx, filter_flag)
    queries, centroids = _ivf_pad(queries, centroids)
    dev = queries.device
    out_s, out_i = _topk_out(out, B, kk, dev, "kk")
    if B == 0:
        return out_s, out_i
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _call("lr_ivf_sq8_search_f32", _ptr(queries), B, _ptr(centroids), nlist, _ptr(list_ptr), _ptr(list_ids), _ptr(codes), stride,
          _ptr(scales), N, Dp, _ptr(consumed_ptr), _ptr(consumed_idx), _ptr(filter_flag), kk, nprobe, _ptr(out_s), _ptr(out_i),
          _ptr(ws), ws.numel(), _stream())
    return out_s, out_i


def ivf_rerank(queries: torch.Tensor, rows: torch.Tensor, cand_ids: torch.Tensor, k: int, out: Optional[tuple] = None):
    """Stage 2 (`lr_ivf_rerank_f32`): the candidates `cand_ids` [B, kk] int64 (global ids, -1 = none) re-scored as f32 inner
    products with `rows[id]`; the `k` largest by (score desc, id asc), id -1 / score -inf beyond them."""
    if queries.dim() != 2 or rows.dim() != 2 or cand_ids.dim() != 2 or cand_ids.shape[0] != queries.shape[0]:
        raise ValueError("queries [B, D], rows [N, D] and cand_ids [B, kk] must be 2-d")
    B, D = queries.shape
    N, kk, k = rows.shape[0], cand_ids.shape[1], int(k)
    if rows.shape[1] != D:
        raise ValueError(f"queries have width {D}, the rows {rows.shape[1]}")
    _ivf_check_width(D, "ivf_rerank")
    if not (1 <= k <= IVF_MAX_K and 1 <= kk <= IVF_MAX_K and 1 <= N < 2 ** 31):
        raise ValueError(f"ivf_rerank: shape not supported (N={N} kk={kk} k={k})")
    _req(queries, torch.float32, "queries", 2)
    _req(rows, torch.float32, "rows", 2)
    _req(cand_ids, torch.int64, "cand_ids", 2)
    queries, rows = _ivf_pad(queries, rows)
    out_s, out_i = _topk_out(out, B, k, queries.device, "k")
    if B == 0:
        return out_s, out_i
    _call("lr_ivf_rerank_f32", _ptr(queries), B, _ptr(rows), N, rows.shape[1], _ptr(cand_ids), kk, k, _ptr(out_s), _ptr(out_i),
          _stream())
    return out_s, out_i


# --------------------------------------------------------------------------------------
# evaluation metrics (csrc/eval_metrics.hip): sort keys, rank statistics, pointwise sums, listwise metrics, coverage
# --------------------------------------------------------------------------------------
EVAL_SCAN_TILE = 2048       # rows per workgroup of the rank-statistics scan (kScanTile of csrc/eval_metrics.hip)
EVAL_POINT_TILE = 4096      # rows per workgroup of the pointwise reduction's first stage (kPointTile)
EVAL_MAX_K = 1024
EVAL_MAX_ROWS = 2 ** 31 - 1


def _eval_rows(n: int, what: str) -> None:
    if n < 1 or n > EVAL_MAX_ROWS:
        raise ValueError(f"{what}: shape not supported ({n} rows; 1 .. 2^31 - 1 are)")


def eval_keys(score: torch.Tensor, group: Optional[torch.Tensor] = None):
    """(key int64 [N], bad int32 [1]): key = (group << 32) | the order-preserving image of the f32 score, -0.0 as +0.0
    (`lr_eval_keys_f32`); `bad` counts the NaN scores.  Groups are int32 >= 0."""
    _req(score, torch.float32, "score", 1)
    n = score.numel()
    _eval_rows(n, "eval_keys")
    if group is not None:
        _req(group, torch.int32, "group", 1)
        if group.numel() != n:
            raise ValueError("group must have one entry per score")
    key = torch.empty(n, dtype=torch.int64, device=score.device)
    bad = torch.empty(1, dtype=torch.int32, device=score.device)
    _call("lr_eval_keys_f32", _ptr(score), _ptr(group), n, _ptr(key), _ptr(bad), _stream())
    return key, bad


def eval_rank_stats(key_sorted: torch.Tensor, label_sorted: torch.Tensor):
    """(int64 [3] = num2, P, Nneg; f64 [2] = gauc, pr_auc) over keys sorted ascending with their labels (uint8, != 0 is a
    positive): `lr_eval_rank_stats`.  With one group ROC AUC = num2 / (2 P Nneg)."""
    _req(key_sorted, torch.int64, "key_sorted", 1)
    _req(label_sorted, torch.uint8, "label_sorted", 1)
    n = key_sorted.numel()
    _eval_rows(n, "eval_rank_stats")
    if label_sorted.numel() != n:
        raise ValueError("label_sorted must have one entry per key")
    dev = key_sorted.device
    out_i = torch.empty(3, dtype=torch.int64, device=dev)
    out_f = torch.empty(2, dtype=torch.float64, device=dev)
    ws = torch.empty(_lib.load().lr_eval_rank_ws_bytes(n), dtype=torch.uint8, device=dev)
    _call("lr_eval_rank_stats", _ptr(key_sorted), _ptr(label_sorted), n, _ptr(out_i), _ptr(out_f), _ptr(ws), ws.numel(), _stream())
    return out_i, out_f


def eval_point_sums(pred: torch.Tensor, label: torch.Tensor, mean: float = 0.0):
    """(f64 [5] = sum (y-p)^2, sum |y-p|, sum y, sum (y-mean)^2, log-loss sum; int64 [4] = TP, TN, P, N of the class rint(p)):
    `lr_eval_point_sums_f32`, a two-stage reduction in fp64 with a fixed order."""
    _req(pred, torch.float32, "pred", 1)
    _req(label, torch.float32, "label", 1)
    n = pred.numel()
    _eval_rows(n, "eval_point_sums")
    if label.numel() != n:
        raise ValueError("label must have one entry per prediction")
    dev = pred.device
    out_f = torch.empty(5, dtype=torch.float64, device=dev)
    out_i = torch.empty(4, dtype=torch.int64, device=dev)
    ws = torch.empty(_lib.load().lr_eval_point_ws_bytes(n), dtype=torch.uint8, device=dev)
    _call("lr_eval_point_sums_f32", _ptr(pred), _ptr(label), n, float(mean), _ptr(out_f), _ptr(out_i), _ptr(ws), ws.numel(),
          _stream())
    return out_f, out_i


def eval_listwise(reco: torch.Tensor, truth_ptr: torch.Tensor, truth_items: torch.Tensor, truth_len: torch.Tensor,
                  disc: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """f64 [4, U] = precision, recall, AP and NDCG at k of every user (`lr_eval_listwise`): `reco` int32 [U, k] padded with -1,
    the truth as a CSR of ascending distinct ids, `truth_len` the divisor of recall, `disc` f64 [k] = 1 / log2(j + 2)."""
    _req(reco, torch.int32, "reco", 2)
    U, k = reco.shape
    if not 1 <= k <= EVAL_MAX_K:
        raise ValueError(f"eval_listwise: shape not supported (k={k}; 1 .. {EVAL_MAX_K} are)")
    _eval_rows(U, "eval_listwise")
    _req(truth_ptr, torch.int64, "truth_ptr", 1)
    _req(truth_items, torch.int32, "truth_items", 1)
    _req(truth_len, torch.int32, "truth_len", 1)
    _req(disc, torch.float64, "disc", 1)
    if truth_ptr.numel() != U + 1 or truth_len.numel() != U or disc.numel() != k:
        raise ValueError("truth_ptr must be [U + 1], truth_len [U] and disc [k]")
    if out is None:
        out = torch.empty((4, U), dtype=torch.float64, device=reco.device)
    else:
        _req(out, torch.float64, "out", 2)
        if tuple(out.shape) != (4, U):
            raise ValueError("out must be [4, U] f64")
    _call("lr_eval_listwise", _ptr(reco), _ptr(truth_ptr), _ptr(truth_items), _ptr(truth_len), _ptr(disc), U, k, _ptr(out),
          _stream())
    return out


def eval_coverage(reco: torch.Tensor, n_items: int) -> torch.Tensor:
    """int64 [1]: the number of distinct ids of `reco` (int32, any shape) in [0, n_items); ids < 0 are padding
    (`lr_eval_coverage_i32`)."""
    _req(reco, torch.int32, "reco")
    n, n_items = reco.numel(), int(n_items)
    _eval_rows(n, "eval_coverage")
    _eval_rows(n_items, "eval_coverage (n_items)")
    flags = torch.empty(n_items, dtype=torch.int32, device=reco.device)
    count = torch.empty(1, dtype=torch.int64, device=reco.device)
    _call("lr_eval_coverage_i32", _ptr(reco), n, n_items, _ptr(flags), _ptr(count), _stream())
    return count


# --------------------------------------------------------------------------------------
# streaming in-batch softmax cross-entropy (two-tower retrieval loss)
# --------------------------------------------------------------------------------------
# Arithmetic of the two contractions of the streaming softmax cross-entropy: "split_bf16" (default) forms every f32 product as
# six bf16 MFMA products with f32 accumulation (error against f64 = that of the f32 fma chain: tests/test_softmax_ce_gpu.py runs
# every case under both); "f32_chain" is the exact f32 MFMA chain.  `LIBRECO_SCE_ARITH` sets the initial value.
SCE_ARITH = os.environ.get("LIBRECO_SCE_ARITH", "split_bf16")
if SCE_ARITH not in ("split_bf16", "f32_chain"):
    raise ValueError("LIBRECO_SCE_ARITH must be split_bf16 or f32_chain")


def set_sce_arith(mode: str) -> str:
    """Select the arithmetic of `softmax_ce_fwd` / `softmax_ce_bwd_cols` from now on; returns the previous setting."""
    global SCE_ARITH
    if mode not in ("split_bf16", "f32_chain"):
        raise ValueError("mode must be 'split_bf16' or 'f32_chain'")
    prev, SCE_ARITH = SCE_ARITH, mode
    return prev


def _sce_arith(arith: Optional[str] = None) -> int:
    """The arithmetic as the C ABI takes it (an explicit argument of the workspace query and of both launches: the library keeps
    no setting of its own, so callers with different settings cannot race) — `arith` or the module default `SCE_ARITH`."""
    arith = SCE_ARITH if arith is None else arith
    if arith not in ("split_bf16", "f32_chain"):
        raise ValueError("arith must be 'split_bf16' or 'f32_chain'")
    return 1 if arith == "split_bf16" else 0


def softmax_ce_supported(B: int, N: int, D: int) -> bool:
    return bool(_lib.load().lr_softmax_ce_supported(B, N, D))


def _sce_check(X, Y, col_bias, row_ids, col_ids, pos0):
    _req(X, torch.float32, "X", 2)
    _req(Y, torch.float32, "Y", 2)
    B, D = X.shape
    N = Y.shape[0]
    if Y.shape[1] != D:
        raise ValueError("X and Y must share the embedding width")
    if col_bias is not None:
        _req(col_bias, torch.float32, "col_bias", 1)
        if col_bias.numel() != N:
            raise ValueError("col_bias must hold one value per column")
    if (row_ids is None) != (col_ids is None):
        raise ValueError("row_ids and col_ids come together")
    if row_ids is not None:
        _req(row_ids, torch.int32, "row_ids", 1)
        _req(col_ids, torch.int32, "col_ids", 1)
        if row_ids.numel() != B or col_ids.numel() != N:
            raise ValueError("row_ids / col_ids must hold one id per row / column")
    if pos0 < 0 or pos0 + B > N:
        raise ValueError("the positives [pos0, pos0 + B) must be columns of Y")
    return B, N, D


def softmax_ce_fwd(X, Y, col_bias=None, row_ids=None, col_ids=None, pos0: int = 0, want_w: bool = True, arith: Optional[str] = None):
    """`softmax_cross_entropy` (tfops/loss.py:71-75) of logits = X @ Y.T + col_bias with the accidental-hit
    mask of `adjust_logits` (two_tower.py:458-479), without the B x N matrix: returns (lse, pos_logit, W)
    with W[i] = softmax(logits[i]) @ Y (None unless `want_w`)."""
    B, N, D = _sce_check(X, Y, col_bias, row_ids, col_ids, pos0)
    lse = torch.empty(B, dtype=torch.float32, device=X.device)
    pos = torch.empty(B, dtype=torch.float32, device=X.device)
    W = torch.empty((B, D), dtype=torch.float32, device=X.device) if want_w else None
    ar = _sce_arith(arith)
    need = _lib.load().lr_softmax_ce_fwd_ws_bytes(B, N, D, ar)
    ws = torch.empty(need, dtype=torch.uint8, device=X.device) if need else None
    _call("lr_softmax_ce_fwd_f32", _ptr(X), B, _ptr(Y), N, D, _ptr(col_bias), _ptr(row_ids), _ptr(col_ids), pos0,
          _ptr(lse), _ptr(pos), _ptr(W), _ptr(ws), need, ar, _stream())
    return lse, pos, W


def softmax_ce_bwd_cols(X, Y, lse, g, col_bias=None, row_ids=None, col_ids=None, pos0: int = 0, arith: Optional[str] = None):
    """V[j] = sum_i g[i] softmax(logits[i])[j] X[i] — the column-side gradient of `softmax_ce_fwd`'s loss
    (without the positives' -g[i] X[i])."""
    B, N, D = _sce_check(X, Y, col_bias, row_ids, col_ids, pos0)
    _req(lse, torch.float32, "lse", 1)
    _req(g, torch.float32, "g", 1)
    V = torch.empty((N, D), dtype=torch.float32, device=X.device)
    _call("lr_softmax_ce_bwd_cols_f32", _ptr(X), B, _ptr(Y), N, D, _ptr(col_bias), _ptr(row_ids), _ptr(col_ids), pos0,
          _ptr(lse), _ptr(g), _ptr(V), _sce_arith(arith), _stream())
    return V


class _SoftmaxCE(torch.autograd.Function):
    """loss_i = logsumexp_j logits[i][:] - logits[i][pos0 + i] on the streaming kernels; gradients w.r.t.
    X and Y (col_bias and the ids are constants of the reference's graph as well)."""

    @staticmethod
    def forward(ctx, X, Y, col_bias, row_ids, col_ids, pos0):
        X, Y = X.contiguous(), Y.contiguous()
        need = X.requires_grad or Y.requires_grad
        lse, pos, W = softmax_ce_fwd(X, Y, col_bias, row_ids, col_ids, pos0, want_w=need)
        ctx.save_for_backward(X, Y, lse, W if W is not None else lse)
        ctx.misc = (col_bias, row_ids, col_ids, pos0)
        return lse - pos

    @staticmethod
    def backward(ctx, g):
        X, Y, lse, W = ctx.saved_tensors
        col_bias, row_ids, col_ids, pos0 = ctx.misc
        g = g.contiguous()
        B = X.shape[0]
        dX = g[:, None] * (W - Y[pos0:pos0 + B])
        dY = softmax_ce_bwd_cols(X, Y, lse, g, col_bias, row_ids, col_ids, pos0)
        dY[pos0:pos0 + B] -= g[:, None] * X
        return dX, dY, None, None, None, None


def softmax_ce(X, Y, col_bias=None, row_ids=None, col_ids=None, pos0: int = 0) -> torch.Tensor:
    """Per-row in-batch softmax cross-entropy (differentiable w.r.t. X and Y), D <= 128 and D % 4 == 0."""
    return _SoftmaxCE.apply(X, Y, col_bias, row_ids, col_ids, pos0)


def pair_mlp_supported(H1: int, H2: int) -> bool:
    return bool(_lib.load().lr_pair_mlp_supported(H1, H2))


# Arithmetic of the pair MLP's H1 x H2 product: "split_bf16" (six bf16 MFMA products per f32 product, f32 accumulation; the default)
# or "f32_chain" — an explicit choice per call, `LIBRECO_PAIR_MLP_ARITH` only sets the default the Python callers pass.
PAIR_MLP_ARITH = os.environ.get("LIBRECO_PAIR_MLP_ARITH", "split_bf16")
if PAIR_MLP_ARITH not in ("split_bf16", "f32_chain"):
    raise ValueError("LIBRECO_PAIR_MLP_ARITH must be split_bf16 or f32_chain")


def pair_mlp(P: torch.Tensor, Q: torch.Tensor, W2: torch.Tensor, b2: torch.Tensor, v3: torch.Tensor, c3: float,
             out: torch.Tensor, accumulate: bool = True, arith: Optional[str] = None) -> torch.Tensor:
    """out[u, i] (+)= relu(relu(P[u] + Q[i]) @ W2 + b2) @ v3 + c3 — the MLP tail of every (user, item) pair of a
    DeepFM catalogue ranking (see lr_pair_mlp_f32 / lr_pair_mlp_sb_f32); `out` [B, N] may be a column slice of a wider matrix."""
    arith = PAIR_MLP_ARITH if arith is None else arith
    if arith not in ("split_bf16", "f32_chain"):
        raise ValueError("arith must be 'split_bf16' or 'f32_chain'")
    for t_, n_ in ((P, "P"), (Q, "Q"), (W2, "W2"), (b2, "b2"), (v3, "v3")):
        _req(t_.contiguous(), torch.float32, n_)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.dim() == 2):
        raise RuntimeError("out must be a 2-D float32 tensor on the MI355X device (there is no CPU fallback)")
    B, H1 = P.shape
    N, H2 = Q.shape[0], W2.shape[1]
    if Q.shape[1] != H1 or W2.shape[0] != H1 or b2.numel() != H2 or v3.numel() != H2 or out.shape != (B, N) or out.stride(1) != 1:
        raise ValueError("shape mismatch")
    _call("lr_pair_mlp_sb_f32" if arith == "split_bf16" else "lr_pair_mlp_f32", _ptr(P.contiguous()), B, _ptr(Q.contiguous()), N, H1,
          _ptr(W2.contiguous()), _ptr(b2.contiguous()), H2,
          _ptr(v3.contiguous()), float(c3), _ptr(out), out.stride(0), 1 if accumulate else 0, _stream())
    return out


def topk_merge(scores: torch.Tensor, ids: torch.Tensor):
    """Merge per-shard ``[S,B,k]`` candidates into the global top-k."""
    _req(scores, torch.float32, "scores", 3)
    _req(ids, torch.int64, "ids", 3)
    S, B, k = scores.shape
    out_s = torch.empty((B, k), dtype=torch.float32, device=scores.device)
    out_i = torch.empty((B, k), dtype=torch.int64, device=scores.device)
    _call("lr_topk_merge_f32", _ptr(scores), _ptr(ids), S, B, k, _ptr(out_s), _ptr(out_i),
                                        _stream())
    return out_s, out_i


# --------------------------------------------------------------------------------------
# SpMM
# --------------------------------------------------------------------------------------
class SpmmPlan:
    """Workspace of the degree-bucketed SpMM bound to ONE graph: the chunk lists of the long rows depend on `rowptr` alone,
    so they are built by the first product and reused by every later one (LightGCN: six products per step on a static
    graph, `lightgcn_module.py:66-88`; the classification pre-pass re-ran on each of them before round 4)."""

    def __init__(self, rowptr: torch.Tensor, nnz: int, K: int):
        self.rowptr_ptr, self.rows, self.nnz, self.K = rowptr.data_ptr(), rowptr.numel() - 1, int(nnz), int(K)
        need = _lib.load().lr_spmm_csr_ws_bytes(self.rows, self.nnz, self.K)
        self.ws = torch.empty(max(need, 256), dtype=torch.uint8, device=rowptr.device)
        self.ready = False

    def matches(self, rowptr, nnz, K) -> bool:
        return rowptr.data_ptr() == self.rowptr_ptr and rowptr.numel() - 1 == self.rows and nnz == self.nnz and K == self.K


def row_slots(seg: Segments, row_slot: torch.Tensor, set: bool = True) -> None:
    """row_slot[seg.rows[s]] = s for the segments of `seg` (`set`), or -1 again."""
    _req(row_slot, torch.int32, "row_slot", 1)
    if row_slot.numel() != seg.V:
        raise ValueError("row_slot must hold one entry per table row")
    _call("lr_row_slots_i32", _ptr(seg.rows), _ptr(seg.n_seg), seg.n, _ptr(row_slot), 1 if set else 0, _stream())


def spmm_csr_adam(rowptr, col, val, X, w, m, v, hp: AdamHP, plan: "SpmmPlan", vmax=None, row_slot=None, gsum=None,
                  alpha: float = 1.0) -> None:
    """One Adam step of (w, m, v[, vmax]) with the gradient g = A X (+ alpha * gsum[row_slot[r]] on the rows with a slot), the
    product's rows never written (see lr_spmm_csr_adam_f32).  Raises ValueError for widths the bucketed kernels do not take."""
    _req(rowptr, torch.int64, "rowptr", 1)
    _req(col, torch.int32, "col", 1)
    _req(val, torch.float32, "val", 1)
    for t_, n_ in ((X, "X"), (w, "w"), (m, "m"), (v, "v")):
        _req(t_, torch.float32, n_, 2)
    rows, K, nnz = rowptr.numel() - 1, X.shape[1], col.numel()
    if not plan.matches(rowptr, nnz, K) or w.shape != (rows, K) or m.shape != w.shape or v.shape != w.shape:
        raise ValueError("plan / parameter shapes do not belong to this graph")
    if (row_slot is None) != (gsum is None):
        raise ValueError("row_slot and gsum come together")
    if row_slot is not None:
        _req(row_slot, torch.int32, "row_slot", 1)
        _req(gsum, torch.float32, "gsum", 2)
    _call("lr_spmm_csr_adam_f32", _ptr(rowptr), _ptr(col), _ptr(val), rows, nnz, _ptr(X), K, _ptr(w), _ptr(m), _ptr(v),
          _ptr(vmax), _ptr(row_slot), _ptr(gsum), float(alpha), hp, _ptr(plan.ws), plan.ws.numel(), 1 if plan.ready else 0, _stream())
    plan.ready = True


class RowBitmap:
    """One bit per row (uint32 words) marking the rows of a batch: `set(ids)` / `clear(ids)` with the same id list."""

    def __init__(self, n_rows: int, device):
        self.n = int(n_rows)
        self.words = torch.zeros((self.n + 31) // 32 + 1, dtype=torch.int32, device=device)
        self._marked = False

    def set(self, ids: torch.Tensor) -> "RowBitmap":
        _req(ids, torch.int32, "ids", 1)
        if self._marked:            # a step that raised between `set` and `clear` left bits behind: start from an empty map
            self.words.zero_()
        self._marked = True
        _call("lr_bitmap_ids_i32", _ptr(ids), ids.numel(), self.n, _ptr(self.words), 1, _stream())
        return self

    def clear(self, ids: torch.Tensor) -> None:
        _req(ids, torch.int32, "ids", 1)
        _call("lr_bitmap_ids_i32", _ptr(ids), ids.numel(), self.n, _ptr(self.words), 0, _stream())
        self._marked = False


def spmm_csr(rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, X: torch.Tensor,
             out: Optional[torch.Tensor] = None, acc: Optional[torch.Tensor] = None,
             plan: Optional[SpmmPlan] = None, x_rows: Optional[RowBitmap] = None,
             y_rows: Optional[RowBitmap] = None, acc_only: bool = False) -> Optional[torch.Tensor]:
    """Y = A X.  `x_rows`: the rows of X outside the bitmap are zero and are not read; `y_rows`: only the rows of Y inside the
    bitmap are computed (the others keep what `out` held) — both need a `plan` and a compiled width (K in 16 / 32 / 64 / 128).
    `acc_only`: `acc += A X`, the product itself is not stored (returns None)."""
    _req(rowptr, torch.int64, "rowptr", 1)
    _req(col, torch.int32, "col", 1)
    _req(val, torch.float32, "val", 1)
    _req(X, torch.float32, "X", 2)
    rows = rowptr.numel() - 1
    K = X.shape[1]
    nnz = col.numel()
    if acc_only:
        if acc is None or out is not None:
            raise ValueError("`acc_only` adds the product to `acc` and stores nothing else: pass `acc`, no `out`")
    elif out is None:
        if y_rows is not None:
            raise ValueError("`y_rows` writes some rows only: pass the `out` buffer that holds the others")
        out = torch.empty((rows, K), dtype=torch.float32, device=X.device)
    if x_rows is not None or y_rows is not None:
        if plan is None or not plan.matches(rowptr, nnz, K):
            raise ValueError("row bitmaps need the graph's SpmmPlan")
        if (x_rows is not None and x_rows.n != X.shape[0]) or (y_rows is not None and y_rows.n != rows):
            raise ValueError("bitmap sizes must match the rows of X / Y")
        _call("lr_spmm_csr_masked_f32", _ptr(rowptr), _ptr(col), _ptr(val), rows, nnz, _ptr(X), K, _ptr(out), _ptr(acc),
              _ptr(x_rows.words) if x_rows is not None else 0, _ptr(y_rows.words) if y_rows is not None else 0,
              _ptr(plan.ws), plan.ws.numel(), 1 if plan.ready else 0, _stream())
        plan.ready = True
        return out
    if plan is not None:
        if not plan.matches(rowptr, nnz, K):
            raise ValueError("the SpmmPlan was made for another graph (rowptr / nnz / K differ)")
        _call("lr_spmm_csr_bucketed_f32", _ptr(rowptr), _ptr(col), _ptr(val), rows, nnz, _ptr(X), K,
              _ptr(out), _ptr(acc), _ptr(plan.ws), plan.ws.numel(), 1 if plan.ready else 0, _stream())
        plan.ready = True
        return out
    need = _lib.load().lr_spmm_csr_ws_bytes(rows, nnz, K)
    key = (X.device, "spmm")
    ws = _WS_CACHE.get(key)
    if ws is None or ws.numel() < need:
        ws = _WS_CACHE[key] = torch.empty(max(need, 256), dtype=torch.uint8, device=X.device)
    _call("lr_spmm_csr_bucketed_f32", _ptr(rowptr), _ptr(col), _ptr(val), rows, nnz, _ptr(X), K,
          _ptr(out), _ptr(acc), _ptr(ws), ws.numel(), 0, _stream())
    return out


_WS_CACHE = {}      # per-device scratch of the degree-bucketed SpMM (chunk lists + chunk sums)


# --------------------------------------------------------------------------------------
# DIN attention pooling
# --------------------------------------------------------------------------------------
def _din_params(W1, b1, W2, b2, K):
    _req(W1, torch.float32, "W1", 2)
    _req(b1, torch.float32, "b1", 1)
    _req(W2, torch.float32, "W2")
    _req(b2, torch.float32, "b2")
    H = W1.shape[1]
    if W1.shape[0] != 4 * K or b1.numel() != H or W2.numel() != H or b2.numel() != 1:
        raise ValueError("attention MLP must be [4K,H] -> [H] -> 1 (layers/attention.py:50-56)")
    return H


def din_path(K: int, L: int, backward: bool = False) -> int:
    """The kernels a DIN attention shape runs on (`lr_din_attn_path`, the dispatchers' own statement of the region):
    0 = none, 1 = the shuffle kernels (L > 2048 while their LDS fits), 2 = the MFMA kernels (the only ones that take
    `hid` / `order`).  The backward's region is the smaller one."""
    return int(_lib.load().lr_din_attn_path(int(K), int(L), int(bool(backward))))


def _din_require(K, L, backward, what, mfma_only=False):
    path = din_path(K, L, backward)
    side = "backward" if backward else "forward"
    if path == 0:
        raise ValueError(f"{what}: no DIN attention {side} kernel for K = {K}, L = {L} (ops.din_path)")
    if mfma_only and path != 2:
        raise ValueError(f"{what}: `hid` / `order` need the MFMA kernels, K = {K}, L = {L} runs the shuffle {side} (ops.din_path)")
    return path


def din_attn_pool_fwd(item_table: torch.Tensor, item: torch.Tensor, seq: torch.Tensor,
                      seq_len: torch.Tensor, W1, b1, W2, b2, out=None, attn=None, hid=None, order_out=None):
    """Fused gather + din_attention (algorithms/din.py:241-250, layers/attention.py:28-64).  `out` [B, K] / `attn`
    [B, L]: persistent output buffers (e.g. the attention plane of the MLP-input block).  `hid` [B * L, 16] (optional): the
    hidden activations of the attention MLP are kept there for `din_attn_pool_bwd(..., hid=hid)`.  `order_out` int32 [B]
    (optional): the launch also writes the balanced walk order of the backward kernels (`din_attn_pool_bwd(..., order=...)`)."""
    _req(item_table, torch.float32, "item_table", 2)
    _req(item, torch.int32, "item", 1)
    _req(seq, torch.int32, "seq", 2)
    _req(seq_len, torch.int32, "seq_len", 1)
    V, K = item_table.shape
    B, L = seq.shape
    H = _din_params(W1, b1, W2, b2, K)
    _din_require(K, L, False, "din_attn_pool_fwd", hid is not None or order_out is not None)
    if out is None:
        out = torch.empty((B, K), dtype=torch.float32, device=item_table.device)
    if attn is None:
        attn = torch.empty((B, L), dtype=torch.float32, device=item_table.device)
    if out.shape != (B, K) or attn.shape != (B, L) or not out.is_contiguous() or not attn.is_contiguous():
        raise ValueError("out / attn must be contiguous [B, K] / [B, L] tensors")
    _call("lr_din_attn_pool_fwd_f32", _ptr(item_table), V, K, _ptr(item), _ptr(seq),
                                               _ptr(seq_len), B, L, _ptr(W1), _ptr(b1), _ptr(W2),
                                               _ptr(b2), H, _ptr(out), _ptr(attn),
                                               _ptr(_din_hid(hid, B, L, K, order_out is not None)),
                                               _ptr(_din_order(order_out, B)), _stream())
    return out, attn


def din_hid_floats(B: int, L: int, K: int, with_order: bool = True) -> int:
    """Elements of the `hid` buffer of `din_attn_pool_fwd / _bwd`: the hidden activations [B * L, 16] and, when the balanced
    order is used too, the backward's transposed weight images behind them (see include/libreco_hip.h)."""
    return B * L * 16 + (3 * (K // 16) * 256 if with_order else 0)


def _din_hid(hid, B, L, K=0, with_order=False):
    need = din_hid_floats(B, L, K, with_order)
    if hid is not None and (hid.dtype != torch.float32 or not hid.is_contiguous() or hid.numel() < need):
        raise ValueError(f"hid must be a contiguous float32 buffer of at least {need} elements (ops.din_hid_floats)")
    return hid


def din_attn_pool_bwd(item_table, item, seq, seq_len, W1, b1, W2, b2, attn, gout, gq_out=None, gkey_out=None,
                      param_out=None, ws=None, parts=3, keep_pad_rows=False, hid=None, order=None):
    """`parts`: 1 = data half (gq, gkey), 2 = parameter half (needs the data half's spill in the same `ws`), 3 = both;
    `keep_pad_rows`: leave gkey rows past a sample's length untouched (caller drops those positions).
    `gq_out` [B, K] / `gkey_out` [B, L, K] (contiguous): write the query / key gradients there — e.g. straight into
    the combined gradient buffer of the table update instead of concatenating 210 MB afterwards.  `param_out` =
    (gW1, gb1, gW2, gb2) contiguous tensors shaped like the parameters (e.g. the `.grad` views of `DenseParams`);
    `ws`: persistent workspace of at least `lr_din_attn_ws_bytes` bytes."""
    _req(item_table, torch.float32, "item_table", 2)
    _req(attn, torch.float32, "attn", 2)
    _req(gout, torch.float32, "gout", 2)
    V, K = item_table.shape
    B, L = seq.shape
    H = _din_params(W1, b1, W2, b2, K)
    _din_require(K, L, True, "din_attn_pool_bwd", hid is not None or order is not None)
    dev = item_table.device
    lib = _lib.load()
    need = max(lib.lr_din_attn_ws_bytes(B, L, K, H), 8)
    if parts != 3 and (ws is None or ws.numel() < need or gkey_out is None or gq_out is None):
        raise ValueError("a split backward needs the caller's persistent `ws` and output buffers")
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    gq = torch.empty((B, K), dtype=torch.float32, device=dev) if gq_out is None else gq_out
    gkey = torch.empty((B, L, K), dtype=torch.float32, device=dev) if gkey_out is None else gkey_out
    if gq.shape != (B, K) or gkey.shape != (B, L, K) or not gq.is_contiguous() or not gkey.is_contiguous():
        raise ValueError("gq_out / gkey_out must be contiguous [B, K] / [B, L, K] tensors")
    if param_out is not None:
        gW1, gb1, gW2, gb2 = param_out
        for g_, p_ in ((gW1, W1), (gb1, b1), (gW2, W2), (gb2, b2)):
            if g_.numel() != p_.numel() or not g_.is_contiguous() or g_.dtype != torch.float32:
                raise ValueError("param_out tensors must be contiguous fp32 tensors shaped like the parameters")
    else:
        gW1, gb1 = torch.empty_like(W1), torch.empty_like(b1)
        gW2, gb2 = torch.empty_like(W2), torch.empty_like(b2)
    _call("lr_din_attn_pool_bwd_parts_f32", _ptr(item_table), V, K, _ptr(item), _ptr(seq),
          _ptr(seq_len), B, L, _ptr(W1), _ptr(b1), _ptr(W2), _ptr(b2),
          H, _ptr(attn), _ptr(gout), _ptr(gq), _ptr(gkey), _ptr(gW1),
          _ptr(gb1), _ptr(gW2), _ptr(gb2), _ptr(ws), ws.numel(), int(parts), int(bool(keep_pad_rows)),
          _ptr(_din_hid(hid, B, L, K, order is not None)), _ptr(_din_order(order, B)), _stream())
    return gq, gkey, gW1, gb1, gW2, gb2


def din_attn_dense_fwd(q, keys, seq_len, W1, b1, W2, b2):
    _req(q, torch.float32, "q", 2)
    _req(keys, torch.float32, "keys", 3)
    _req(seq_len, torch.int32, "seq_len", 1)
    B, L, K = keys.shape
    H = _din_params(W1, b1, W2, b2, K)
    _din_require(K, L, False, "din_attn_dense_fwd")
    out = torch.empty((B, K), dtype=torch.float32, device=q.device)
    attn = torch.empty((B, L), dtype=torch.float32, device=q.device)
    _call("lr_din_attn_dense_fwd_f32", _ptr(q), _ptr(keys), K, _ptr(seq_len), B, L,
                                                _ptr(W1), _ptr(b1), _ptr(W2), _ptr(b2), H,
                                                _ptr(out), _ptr(attn), _stream())
    return out, attn


def din_attn_dense_bwd(q, keys, seq_len, W1, b1, W2, b2, attn, gout):
    _req(q, torch.float32, "q", 2)
    _req(keys, torch.float32, "keys", 3)
    B, L, K = keys.shape
    H = _din_params(W1, b1, W2, b2, K)
    _din_require(K, L, True, "din_attn_dense_bwd")
    dev = q.device
    lib = _lib.load()
    ws = torch.empty(max(lib.lr_din_attn_ws_bytes(B, L, K, H), 8), dtype=torch.uint8, device=dev)
    gq = torch.empty((B, K), dtype=torch.float32, device=dev)
    gkey = torch.empty((B, L, K), dtype=torch.float32, device=dev)
    gW1, gb1 = torch.empty_like(W1), torch.empty_like(b1)
    gW2, gb2 = torch.empty_like(W2), torch.empty_like(b2)
    _call("lr_din_attn_dense_bwd_f32", _ptr(q), _ptr(keys), K, _ptr(seq_len), B, L, _ptr(W1),
                                        _ptr(b1), _ptr(W2), _ptr(b2), H, _ptr(attn), _ptr(gout),
                                        _ptr(gq), _ptr(gkey), _ptr(gW1), _ptr(gb1), _ptr(gW2),
                                        _ptr(gb2), _ptr(ws), ws.numel(), _stream())
    return gq, gkey, gW1, gb1, gW2, gb2


# --------------------------------------------------------------------------------------
# device-side negative sampling
# --------------------------------------------------------------------------------------
def sample_negatives(items_pos: torch.Tensor, num_neg: int, n_items: int, seed: int,
                     users: Optional[torch.Tensor] = None, consumed_ptr: Optional[torch.Tensor] = None,
                     consumed_idx: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 [n * num_neg] negatives, `num_neg` consecutive entries per positive (the layout the
    collators interleave, batch/collators.py:226-232).  With a consumed CSR the "unconsumed" rules
    apply, otherwise the "random" ones (see the header)."""
    _req(items_pos, torch.int32, "items_pos", 1)
    n = items_pos.numel()
    out = torch.empty(n * int(num_neg), dtype=torch.int32, device=items_pos.device)
    if consumed_ptr is not None:
        _req(consumed_ptr, torch.int64, "consumed_ptr", 1)
        _req(consumed_idx, torch.int32, "consumed_idx", 1)
        _req(users, torch.int32, "users", 1)
    _call("lr_sample_negatives_i32", _ptr(users), _ptr(items_pos), n, int(num_neg), int(n_items),
          _ptr(consumed_ptr), _ptr(consumed_idx), int(seed) & ((1 << 64) - 1), _ptr(out), _stream())
    return out


def fm_field_stats(table: torch.Tensor, seg: Segments, field_row_start: torch.Tensor, B: int,
                   chunks: int = 8):
    """(mean, biased var) [F*K] of the gathered block e[B,F,K] from the batch's segments (see the
    header): reads the distinct rows once instead of B*F rows.  fp64 combine of the partials."""
    _req(table, torch.float32, "table", 2)
    _req(field_row_start, torch.int32, "field_row_start", 1)
    K = table.shape[1]
    F = field_row_start.numel() - 1
    partial = torch.empty((F, chunks, 2, K), dtype=torch.float32, device=table.device)
    _call("lr_fm_field_stats_f32", _ptr(table), K, _ptr(seg.rows), _ptr(seg.start), _ptr(seg.n_seg),
          _ptr(field_row_start), F, chunks, _ptr(partial), _stream())
    tot = partial.double().sum(1)                                  # [F, 2, K]
    mean = tot[:, 0] / B
    var = torch.clamp(tot[:, 1] / B - mean * mean, min=0.0)
    return mean.reshape(-1).float(), var.reshape(-1).float()


# --------------------------------------------------------------------------------------
# first Dense layer over a materialised block (general feature nets) — csrc/dense_block.hip
# --------------------------------------------------------------------------------------
def table_colstats(table: torch.Tensor, idx: torch.Tensor, chunks: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """partial [F, chunks, 2, K]: per-chunk column sums / sums of squares of table[idx[b, f], :] (see the header)."""
    _req(table, torch.float32, "table", 2)
    _req(idx, torch.int32, "idx", 2)
    V, K = table.shape
    B, F = idx.shape
    if out is None:
        out = torch.empty((F, chunks, 2, K), dtype=torch.float32, device=table.device)
    elif out.shape != (F, chunks, 2, K):
        raise ValueError("out must be [F, chunks, 2, K]")
    _call("lr_table_colstats_f32", _ptr(table), V, K, _ptr(idx), B, F, int(chunks), _ptr(out), _stream())
    return out


def bn_remainder_(G: torch.Tensor, x: torch.Tensor, a: torch.Tensor, c: torch.Tensor, rows_per_plane: int,
                  period: int = 0) -> torch.Tensor:
    """In place: G[r] -= a[p] + c[p] * x[r]; p = r // rows_per_plane (planar block) or r % period (`period` > 0: row-major
    [B, period * Kp] block); G, x [rows, Kp], a, c [planes * Kp]."""
    for t_, n_ in ((G, "G"), (x, "x"), (a, "a"), (c, "c")):
        _req(t_, torch.float32, n_)
    rows, Kp = G.shape
    planes = period if period > 0 else -(-rows // rows_per_plane)
    if x.shape != G.shape or a.numel() < planes * Kp or c.numel() < planes * Kp:
        raise ValueError("shape mismatch")
    _call("lr_bn_remainder_f32", _ptr(G), _ptr(x), _ptr(a), _ptr(c), rows, int(rows_per_plane), int(period), Kp, _stream())
    return G


# --------------------------------------------------------------------------------------
# LightGCN: normalised bipartite Laplacian built on the device — csrc/laplacian.hip
# --------------------------------------------------------------------------------------
def csr_laplacian(users: torch.Tensor, items: torch.Tensor, n_users: int, n_items: int, want_tperm: bool = True):
    """(rowptr int64 [n+1], col int32 [nnz], val fp32 [nnz], tperm int32 [nnz] | None) of D^-1/2 [[0,R],[R^T,0]] D^-1/2
    from the interaction list (lightgcn_module.py:36-61).  One host read (the number of distinct pairs)."""
    _req(users, torch.int32, "users", 1)
    _req(items, torch.int32, "items", 1)
    E = users.numel()
    if items.numel() != E:
        raise ValueError("users / items must have the same length")
    dev = users.device
    lib = _lib.load()
    n = int(n_users) + int(n_items)
    rowptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
    col = torch.empty(max(2 * E, 1), dtype=torch.int32, device=dev)
    val = torch.empty(max(2 * E, 1), dtype=torch.float32, device=dev)
    tperm = torch.empty(max(2 * E, 1), dtype=torch.int32, device=dev) if want_tperm else None
    n_pairs = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.empty(max(lib.lr_csr_laplacian_ws_bytes(E), 8), dtype=torch.uint8, device=dev)
    _call("lr_csr_laplacian_build", _ptr(users), _ptr(items), E, int(n_users), int(n_items), _ptr(rowptr), _ptr(col),
          _ptr(val), _ptr(tperm), _ptr(n_pairs), _ptr(ws), ws.numel(), _stream())
    nnz = 2 * int(n_pairs.item())
    del ws
    if nnz == 2 * E:
        return rowptr, col, val, tperm
    return rowptr, col[:nnz].clone(), val[:nnz].clone(), (tperm[:nnz].clone() if want_tperm else None)


# --------------------------------------------------------------------------------------
# ALS (csrc/als.hip)
# --------------------------------------------------------------------------------------
def als_supported(K: int) -> bool:
    return bool(_lib.load().lr_als_supported(int(K)))


def _als_check_k(K: int) -> None:
    if not als_supported(K):
        raise ValueError(f"ALS supports embed_size 1..128 (the per-row K x K system is solved in LDS), got {K}")


class AlsPlan:
    """Degree plan of one CSR orientation (the rows of one half-sweep), built once per `fit`: the CSR does not change
    between epochs.  Light rows are solved one per wave from LDS, medium rows one per workgroup, heavy rows are cut into
    fixed chunks whose partial systems are reduced in chunk order (lr_als_plan_params gives the degree limits).  Owns the
    slab workspace of the heavy rows."""

    def __init__(self, rowptr: torch.Tensor, K: int):
        _req(rowptr, torch.int64, "rowptr", 1)
        _als_check_k(K)
        import ctypes as C

        lim = (C.c_int32 * 3)()
        check(_lib.load().lr_als_plan_params(int(K), lim), "lr_als_plan_params")
        self.light_cap, self.heavy_deg, self.chunk = int(lim[0]), int(lim[1]), int(lim[2])
        self.rowptr_ptr, self.rows, self.K = rowptr.data_ptr(), rowptr.numel() - 1, int(K)
        deg = rowptr[1:] - rowptr[:-1]
        light = torch.nonzero(deg <= self.light_cap).flatten()
        medium = torch.nonzero((deg > self.light_cap) & (deg <= self.heavy_deg)).flatten()
        heavy = torch.nonzero(deg > self.heavy_deg).flatten()
        n_ch = torch.div(deg[heavy] + self.chunk - 1, self.chunk, rounding_mode="floor")
        begin = torch.zeros(heavy.numel() + 1, dtype=torch.int64, device=rowptr.device)
        begin[1:] = torch.cumsum(n_ch, 0)
        chunk_row = torch.repeat_interleave(torch.arange(heavy.numel(), device=rowptr.device), n_ch)
        self.plan = torch.cat([light, medium, heavy, begin, chunk_row]).to(torch.int32).contiguous()
        self.n_light, self.n_medium, self.n_heavy = light.numel(), medium.numel(), heavy.numel()
        self.n_chunks = chunk_row.numel()
        need = _lib.load().lr_als_ws_bytes(self.n_chunks, self.K)
        self.ws = torch.empty(max(need, 256), dtype=torch.uint8, device=rowptr.device)

    def matches(self, rowptr: torch.Tensor, K: int) -> bool:
        return rowptr.data_ptr() == self.rowptr_ptr and rowptr.numel() - 1 == self.rows and int(K) == self.K


def als_plan(rowptr: torch.Tensor, K: int) -> AlsPlan:
    return AlsPlan(rowptr, K)


def als_gram(Y: torch.Tensor, reg: float, implicit: bool, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """G0 = Y^T Y + reg I (implicit) or reg I (explicit), [K, K] f32; the Gram's partials are summed in a fixed order."""
    _req(Y, torch.float32, "Y", 2)
    N, K = Y.shape
    _als_check_k(K)
    if out is None:
        out = torch.empty((K, K), dtype=torch.float32, device=Y.device)
    else:
        _req(out, torch.float32, "out", 2)
        if tuple(out.shape) != (K, K):
            raise ValueError("out must be [K, K]")
    need = _lib.load().lr_als_gram_ws_bytes(N, K) if implicit else 0
    key = (Y.device, "als_gram")
    ws = _WS_CACHE.get(key)
    if ws is None or ws.numel() < need:
        ws = _WS_CACHE[key] = torch.empty(max(need, 256), dtype=torch.uint8, device=Y.device)
    _call("lr_als_gram_f32", _ptr(Y), N, K, float(reg), 1 if implicit else 0, _ptr(out), _ptr(ws), ws.numel(), _stream())
    return out


def als_half_sweep(rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, X: torch.Tensor, Y: torch.Tensor,
                   G0: torch.Tensor, implicit: bool, use_cg: bool, plan: AlsPlan, cg_steps: int = 3,
                   fail: Optional[torch.Tensor] = None, stage_mask: int = 15) -> Optional[torch.Tensor]:
    """Update every row of X in place against Y (one ALS half-sweep, `_als.pyx:als_update`).  `val` holds the confidence
    alpha r + 1 (implicit) or the rating (explicit).  The direct solver returns the per-row failure words (int32 [rows],
    nonzero where a pivot was not positive: that row is left unchanged); `fail` may be passed in (it is zeroed here)."""
    _req(rowptr, torch.int64, "rowptr", 1)
    _req(col, torch.int32, "col", 1)
    _req(val, torch.float32, "val", 1)
    _req(X, torch.float32, "X", 2)
    _req(Y, torch.float32, "Y", 2)
    _req(G0, torch.float32, "G0", 2)
    rows, K = X.shape
    _als_check_k(K)
    if Y.shape[1] != K or tuple(G0.shape) != (K, K):
        raise ValueError("X, Y and G0 must share the embedding width K")
    if rowptr.numel() != rows + 1 or col.numel() != val.numel():
        raise ValueError("the CSR must have one row per row of X and one value per column index")
    if not plan.matches(rowptr, K):
        raise ValueError("the AlsPlan was made for another CSR (rowptr / K differ)")
    if cg_steps < 0:
        raise ValueError("cg_steps must be non-negative")
    if not use_cg:
        if fail is None:
            fail = torch.zeros(rows, dtype=torch.int32, device=X.device)
        else:
            _req(fail, torch.int32, "fail", 1)
            if fail.numel() != rows:
                raise ValueError("fail holds one word per row")
            fail.zero_()
    _call("lr_als_half_sweep_f32", _ptr(rowptr), _ptr(col), _ptr(val), rows, _ptr(X), _ptr(Y), K, _ptr(G0),
          1 if implicit else 0, 1 if use_cg else 0, int(cg_steps), _ptr(plan.plan), plan.n_light, plan.n_medium,
          plan.n_heavy, plan.n_chunks, _ptr(None if use_cg else fail), _ptr(plan.ws), plan.ws.numel(), int(stage_mask),
          _stream())
    return None if use_cg else fail


# --------------------------------------------------------------------------------------
# UserCF / ItemCF (csrc/cf_sim.hip, csrc/cf_rank.hip)
# --------------------------------------------------------------------------------------
CF_SIM_TYPES = {"cosine": 0, "pearson": 1, "jaccard": 2}
CF_SIM_MAX_BYTES = None     # cap on the similarity CSR (columns + values); None: 90 % of the free device memory


def cf_sim_tile_cols() -> int:
    return int(_lib.load().lr_cf_sim_tile_cols())


def _mem_cap(override, device) -> int:
    """`override` (CF_SIM_MAX_BYTES / SWING_MAX_BYTES as they stand at the call) or 90 % of the free device memory."""
    if override is not None:
        return int(override)
    free, _ = torch.cuda.mem_get_info(device)
    return int(free * 0.9)


def _tile_work_items(n_rows: int, work: torch.Tensor, tmin: torch.Tensor, span: torch.Tensor):
    """The (row, tile) work items of csrc/tile_csr.hpp: row r gets the span[r] tiles from tmin[r] on.  Returns (item_row
    int32, item_tile int32, order int32: the items by the work of their row, heaviest first, n_items); one host read."""
    dev = span.device
    n_items = int(span.sum())
    if n_items == 0:
        return None, None, None, 0
    item_row = torch.repeat_interleave(torch.arange(n_rows, device=dev), span, output_size=n_items)
    istart = torch.cumsum(span, 0) - span
    item_tile = tmin[item_row] + torch.arange(n_items, device=dev) - istart[item_row]
    order = torch.argsort(work[item_row], descending=True, stable=True).to(torch.int32)
    return item_row.to(torch.int32).contiguous(), item_tile.to(torch.int32).contiguous(), order, n_items


def _two_pass_csr(fn: str, lead: tuple, rowptr: torch.Tensor, items, ws_bytes: int, cap: Optional[int], max_bytes,
                  too_large: str, mark=lambda stage: None, extra=(), entry_bytes: int = 8):
    """Count, scan, cap check, allocate, fill and rowptr of a two-pass kernel of csrc/tile_csr.hpp: `fn(*lead, item_row,
    item_tile, order, n_items, pass, item_nnz, item_off, col, val, ws, ws_bytes, stream)`.  Fills `rowptr` (zeros, int64
    [n_rows + 1]) and returns (rowptr, col, val); col and val are allocated only once the count pass has given their size
    (one host read), and a result above `cap` bytes (None: `_mem_cap(max_bytes)`, taken after the count pass) raises
    MemoryError(too_large.format(total=, gib=, cap_gib=)).  `extra`: dtypes of further per-entry outputs, passed behind
    `val` and returned behind it; `entry_bytes`: what the cap check counts per entry."""
    item_row, item_tile, order, n_items = items
    dev = rowptr.device
    ws = torch.empty(int(ws_bytes), dtype=torch.uint8, device=dev)
    item_nnz = torch.zeros(n_items, dtype=torch.int64, device=dev)
    common = (*lead, _ptr(item_row), _ptr(item_tile), _ptr(order), n_items)
    mark("plan")
    _call(fn, *common, 0, _ptr(item_nnz), 0, 0, 0, *(0 for _ in extra), _ptr(ws), ws.numel(), _stream())
    mark("count")
    item_end = torch.cumsum(item_nnz, 0)
    total = int(item_end[-1])
    need = total * entry_bytes + rowptr.numel() * 8
    cap = _mem_cap(max_bytes, dev) if cap is None else int(cap)
    if need > cap:
        raise MemoryError(too_large.format(total=total, gib=need / 2**30, cap_gib=cap / 2**30))
    col = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    val = torch.empty(max(total, 1), dtype=torch.float32, device=dev)
    more = [torch.empty(max(total, 1), dtype=dt, device=dev) for dt in extra]
    item_off = (item_end - item_nnz).contiguous()
    mark("scan")
    _call(fn, *common, 1, 0, _ptr(item_off), _ptr(col), _ptr(val), *(_ptr(t) for t in more), _ptr(ws), ws.numel(), _stream())
    rowptr[1:] = torch.cumsum(torch.zeros(rowptr.numel() - 1, dtype=torch.int64, device=dev).index_add_(
        0, item_row.to(torch.int64), item_nnz), 0)
    mark("fill")
    return (rowptr, col[:total], val[:total], *(t[:total] for t in more))


def _cf_sim_items(x_ptr: torch.Tensor, x_col: torch.Tensor, y_ptr: torch.Tensor, y_col: torch.Tensor):
    """The work items of the co-occurrence kernels of csrc/cf_sim.hip: (row, tile) over the tiles between the row's smallest
    and largest co-occurring column."""
    dev = x_ptr.device
    n_x = x_ptr.numel() - 1
    T = cf_sim_tile_cols()
    nnz = x_col.numel()
    deg_y = (y_ptr[1:] - y_ptr[:-1])
    rows_x = torch.repeat_interleave(torch.arange(n_x, device=dev), x_ptr[1:] - x_ptr[:-1], output_size=nnz)
    yc = x_col.to(torch.int64)
    work = torch.zeros(n_x, dtype=torch.int64, device=dev).index_add_(0, rows_x, deg_y[yc])
    first = y_col[y_ptr[:-1].clamp(max=max(y_col.numel() - 1, 0))].to(torch.int64) if y_col.numel() else deg_y
    last = y_col[(y_ptr[1:] - 1).clamp(min=0)].to(torch.int64) if y_col.numel() else deg_y
    tmin = torch.full((n_x,), n_x, dtype=torch.int64, device=dev).scatter_reduce_(0, rows_x, first[yc], "amin")
    tmax = torch.full((n_x,), -1, dtype=torch.int64, device=dev).scatter_reduce_(0, rows_x, last[yc], "amax")
    tmin, tmax = torch.div(tmin, T, rounding_mode="floor"), torch.div(tmax, T, rounding_mode="floor")
    span = torch.where(work > 0, tmax - tmin + 1, torch.zeros_like(work))
    return _tile_work_items(n_x, work, tmin, span)


def cf_similarity(x_ptr: torch.Tensor, x_col: torch.Tensor, x_val: torch.Tensor, y_ptr: torch.Tensor,
                  y_col: torch.Tensor, y_val: torch.Tensor, sim_type: str, min_common: int,
                  norm: Optional[torch.Tensor] = None, cnt: Optional[torch.Tensor] = None, cap: Optional[int] = None):
    """The full symmetric similarity CSR (rowptr int64 [n_x + 1], col int32 ascending per row, val f32) of the forward CSR
    X (n_x rows) against its inverted index Y, in the reference's f32 order (`_similarities.pyx`).  Pearson expects the
    values of X and Y mean-centred per x row and `norm` the centred norms; jaccard needs `cnt` (int32 row degrees).  The
    nnz is counted before anything is allocated for the result: a result above the memory cap raises MemoryError."""
    _req(x_ptr, torch.int64, "x_ptr", 1)
    _req(x_col, torch.int32, "x_col", 1)
    _req(y_ptr, torch.int64, "y_ptr", 1)
    _req(y_col, torch.int32, "y_col", 1)
    if sim_type not in CF_SIM_TYPES:
        raise ValueError("sim_type must be one of (`cosine`, `pearson`, `jaccard`)")
    st = CF_SIM_TYPES[sim_type]
    jac = st == 2
    if jac:
        _req(cnt, torch.int32, "cnt", 1)
    else:
        _req(x_val, torch.float32, "x_val", 1)
        _req(y_val, torch.float32, "y_val", 1)
        _req(norm, torch.float32, "norm", 1)
    dev = x_ptr.device
    n_x = x_ptr.numel() - 1
    if n_x > 2**31 - 1:
        raise ValueError("the similarity supports up to 2**31 - 1 rows")
    items = _cf_sim_items(x_ptr, x_col, y_ptr, y_col)
    rowptr = torch.zeros(n_x + 1, dtype=torch.int64, device=dev)
    if items[3] == 0:
        return rowptr, torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.float32, device=dev)
    vals = (None, None, None) if jac else (x_val, y_val, norm)
    lead = (_ptr(x_ptr), _ptr(x_col), _ptr(vals[0]), _ptr(y_ptr), _ptr(y_col), _ptr(vals[1]), n_x, _ptr(vals[2]),
            _ptr(cnt if jac else None), st, int(min_common))
    return _two_pass_csr("lr_cf_sim_f32", lead, rowptr, items, _lib.load().lr_cf_sim_ws_bytes(), cap, CF_SIM_MAX_BYTES,
                         "the similarity matrix has {total} entries ({gib:.2f} GiB), above the {cap_gib:.2f} GiB that the "
                         "device can hold for it; raise `min_common` or use fewer rows")


def cf_topk(rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, k: int):
    """(ids int32 [n, k'], sims f32 [n, k'], len int32 [n]) with k' = min(k, longest row) (at least 1): every row's first
    min(k, len) entries by (sim descending, column ascending), `cf_base.py:get_top_k_sims`."""
    _req(rowptr, torch.int64, "rowptr", 1)
    _req(col, torch.int32, "col", 1)
    _req(val, torch.float32, "val", 1)
    if int(k) < 1:
        raise ValueError("k must be at least 1")
    n = rowptr.numel() - 1
    longest = int((rowptr[1:] - rowptr[:-1]).max()) if n > 0 else 0
    kk = max(1, min(int(k), longest))
    ids = torch.empty((n, kk), dtype=torch.int32, device=rowptr.device)
    sims = torch.empty((n, kk), dtype=torch.float32, device=rowptr.device)
    lens = torch.zeros(n, dtype=torch.int32, device=rowptr.device)
    _call("lr_cf_topk_f32", _ptr(rowptr), _ptr(col), _ptr(val), n, kk, _ptr(ids), _ptr(sims), _ptr(lens), _stream())
    return ids, sims, lens


CF_RECOMMEND_WS_BYTES = 1 << 30     # per-call scratch of the recommend kernel (scores + flags); batches are cut to fit


def cf_recommend(users: torch.Tensor, user_cf: bool, ui_ptr: torch.Tensor, ui_col: torch.Tensor, ui_val: torch.Tensor,
                 tk_ids: torch.Tensor, tk_sims: torch.Tensor, tk_len: torch.Tensor, n_items: int,
                 cons_ptr: torch.Tensor, cons_idx: torch.Tensor, filter_consumed: bool, n_rec: int):
    """ItemCF / UserCF recommendation scores of `users` (int32, inner ids) and the best n_rec candidates by (score
    descending, id ascending).  cons_ptr / cons_idx: one consumed row per user of `users`.  Returns (ids [B, n_rec],
    scores [B, n_rec], lens [B], n_candidates [B], fallback [B]: 1 nothing touched, 2 every candidate consumed)."""
    _req(users, torch.int32, "users", 1)
    _req(ui_ptr, torch.int64, "ui_ptr", 1)
    _req(ui_col, torch.int32, "ui_col", 1)
    _req(ui_val, torch.float32, "ui_val", 1)
    _req(tk_ids, torch.int32, "tk_ids", 2)
    _req(tk_sims, torch.float32, "tk_sims", 2)
    _req(tk_len, torch.int32, "tk_len", 1)
    _req(cons_ptr, torch.int64, "cons_ptr", 1)
    _req(cons_idx, torch.int32, "cons_idx", 1)
    if int(n_rec) < 1:
        raise ValueError("n_rec must be at least 1")
    B, dev = users.numel(), users.device
    if cons_ptr.numel() != B + 1:
        raise ValueError("cons_ptr must hold one consumed row per user")
    ids = torch.empty((B, n_rec), dtype=torch.int32, device=dev)
    scores = torch.empty((B, n_rec), dtype=torch.float32, device=dev)
    lens = torch.zeros(B, dtype=torch.int32, device=dev)
    ncand = torch.zeros(B, dtype=torch.int64, device=dev)
    fallback = torch.zeros(B, dtype=torch.int32, device=dev)
    lib = _lib.load()
    per_user = max(1, int(lib.lr_cf_recommend_ws_bytes(1, n_items)) - 256)
    chunk = max(1, min(B, CF_RECOMMEND_WS_BYTES // per_user))
    ws = torch.empty(int(lib.lr_cf_recommend_ws_bytes(min(chunk, max(B, 1)), n_items)), dtype=torch.uint8, device=dev)
    for b0 in range(0, B, chunk):
        b1 = min(B, b0 + chunk)
        cp = (cons_ptr[b0:b1 + 1]).contiguous()
        _call("lr_cf_recommend_f32", _ptr(users[b0:b1]), b1 - b0, 1 if user_cf else 0, _ptr(ui_ptr), _ptr(ui_col),
              _ptr(ui_val), _ptr(tk_ids), _ptr(tk_sims), _ptr(tk_len), tk_ids.shape[1], int(n_items), _ptr(cp),
              _ptr(cons_idx), 1 if filter_consumed else 0, int(n_rec), _ptr(ids[b0:b1]), _ptr(scores[b0:b1]),
              _ptr(lens[b0:b1]), _ptr(ncand[b0:b1]), _ptr(fallback[b0:b1]), _ptr(ws), ws.numel(), _stream())
    return ids, scores, lens, ncand, fallback


def cf_predict(srow: torch.Tensor, irow: torch.Tensor, s_ptr: torch.Tensor, s_col: torch.Tensor, s_val: torch.Tensor,
               i_ptr: torch.Tensor, i_col: torch.Tensor, i_val: torch.Tensor, k: int, rating: bool, lower: float,
               upper: float, default_pred: float):
    """Neighbourhood predictions of the pairs (srow[q], irow[q]) (`cf_base.py:compute_pred`): (pred f32 [n], none int32
    [n], 1 where no positive neighbour was found and pred is default_pred)."""
    for t, nm in ((srow, "srow"), (irow, "irow"), (s_col, "s_col"), (i_col, "i_col")):
        _req(t, torch.int32, nm, 1)
    for t, nm in ((s_ptr, "s_ptr"), (i_ptr, "i_ptr")):
        _req(t, torch.int64, nm, 1)
    _req(s_val, torch.float32, "s_val", 1)
    _req(i_val, torch.float32, "i_val", 1)
    n = srow.numel()
    pred = torch.empty(n, dtype=torch.float32, device=srow.device)
    none = torch.empty(n, dtype=torch.int32, device=srow.device)
    _call("lr_cf_predict_f32", _ptr(srow), _ptr(irow), n, _ptr(s_ptr), _ptr(s_col), _ptr(s_val), _ptr(i_ptr),
          _ptr(i_col), _ptr(i_val), max(0, int(k)), 1 if rating else 0, float(lower), float(upper), float(default_pred),
          _ptr(pred), _ptr(none), _stream())
    return pred, none


# --------------------------------------------------------------------------------------
# RsUserCF / RsItemCF (csrc/cf_sim.hip, csrc/cf_state.hip): the pair state and its incremental update
# --------------------------------------------------------------------------------------
CF_STATE_ENTRY_BYTES = 16    # col int32 + prod f32 + cnt int32 + sim f32: what the memory cap counts per entry of the state


class CfState(NamedTuple):
    """The state of n_x rows: a symmetric CSR without diagonal (ptr int64 [n_x + 1], col int32 ascending per row) of every
    pair with a count above 0, with the accumulated product, the count and the cosine of its last refresh."""
    ptr: torch.Tensor
    col: torch.Tensor
    prod: torch.Tensor
    cnt: torch.Tensor
    sim: torch.Tensor


def cf_state_empty(n_x: int, device) -> CfState:
    z = lambda dt: torch.zeros(0, dtype=dt, device=device)  # noqa: E731
    return CfState(torch.zeros(int(n_x) + 1, dtype=torch.int64, device=device), z(torch.int32), z(torch.float32),
                   z(torch.int32), z(torch.float32))


def cf_pair_state(x_ptr: torch.Tensor, x_col: torch.Tensor, x_val: torch.Tensor, y_ptr: torch.Tensor, y_col: torch.Tensor,
                  y_val: torch.Tensor, cap: Optional[int] = None):
    """(rowptr int64 [n_x + 1], col int32 ascending per row, prod f32, cnt int32): every pair of rows of the forward CSR X
    that shares a y of its inverted index Y, with the f32 sum of its products in ascending y (unfused multiply and add) and
    the number of shared y; a sum of exactly 0 is kept (`invert_cosine` / `update_cosine` before the normalisation).  The
    entries are counted before anything is allocated for them; above the memory cap (16 B per entry, what the state will
    hold for them) the call raises MemoryError."""
    _req(x_ptr, torch.int64, "x_ptr", 1)
    _req(x_col, torch.int32, "x_col", 1)
    _req(x_val, torch.float32, "x_val", 1)
    _req(y_ptr, torch.int64, "y_ptr", 1)
    _req(y_col, torch.int32, "y_col", 1)
    _req(y_val, torch.float32, "y_val", 1)
    if x_col.numel() != x_val.numel() or y_col.numel() != y_val.numel() or x_col.numel() != y_col.numel():
        raise ValueError("X and Y must hold the same entries: one value per column, as many in Y as in X")
    dev = x_ptr.device
    n_x = x_ptr.numel() - 1
    if n_x < 0 or y_ptr.numel() < 1:
        raise ValueError("x_ptr and y_ptr must hold at least one element")
    if n_x > 2**31 - 1:
        raise ValueError("the pair state supports up to 2**31 - 1 rows")
    items = _cf_sim_items(x_ptr, x_col, y_ptr, y_col) if n_x else (None, None, None, 0)
    rowptr = torch.zeros(n_x + 1, dtype=torch.int64, device=dev)
    if items[3] == 0:
        e = cf_state_empty(n_x, dev)
        return rowptr, e.col, e.prod, e.cnt
    lead = (_ptr(x_ptr), _ptr(x_col), _ptr(x_val), _ptr(y_ptr), _ptr(y_col), _ptr(y_val), n_x)
    return _two_pass_csr("lr_cf_pair_state_f32", lead, rowptr, items, _lib.load().lr_cf_sim_ws_bytes(), cap, CF_SIM_MAX_BYTES,
                         "the pair state has {total} entries ({gib:.2f} GiB), above the {cap_gib:.2f} GiB that the device "
                         "can hold for it; train on fewer rows", extra=(torch.int32,),
                         entry_bytes=CF_STATE_ENTRY_BYTES)


def cf_sumsq(ptr: torch.Tensor, val: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The f32 sum of squares of every CSR row as one sequential chain in stored order (`compute_sum_squares`).  With
    `out` (f32 [n_rows]) the sums are added to it in place, one f32 add per row (`update_sum_squares`)."""
    _req(ptr, torch.int64, "ptr", 1)
    _req(val, torch.float32, "val", 1)
    n = ptr.numel() - 1
    if n < 0:
        raise ValueError("ptr must hold at least one element")
    if out is None:
        res = torch.empty(n, dtype=torch.float32, device=ptr.device)
    else:
        res = _req(out, torch.float32, "out", 1)
        if res.numel() != n:
            raise ValueError(f"out must hold one sum per row ({n}), got {res.numel()}")
    _call("lr_cf_sumsq_f32", _ptr(ptr), _ptr(val), n, 0 if out is None else 1, _ptr(res), _stream())
    return res


def cf_state_update(old: CfState, delta, sumsq: torch.Tensor, cap: Optional[int] = None) -> CfState:
    """The state after adding `delta` (rowptr, col, prod, cnt of `cf_pair_state` on the new interactions, n_x rows) to
    `old` (at most n_x rows; rows beyond its own are empty): the row-wise union, where a pair of the delta gets
    prod = old + delta, cnt = old + delta and its cosine from `sumsq` (f32 [n_x], already updated), and every other pair
    keeps its values bit for bit (`accumulate_cosine`).  Counted before it is allocated: above the memory cap (16 B per
    entry) the call raises MemoryError."""
    d_ptr, d_col, d_prod, d_cnt = delta
    for t, dt, nm in ((old.ptr, torch.int64, "old.ptr"), (old.col, torch.int32, "old.col"),
                      (old.prod, torch.float32, "old.prod"), (old.cnt, torch.int32, "old.cnt"),
                      (old.sim, torch.float32, "old.sim"), (d_ptr, torch.int64, "delta rowptr"),
                      (d_col, torch.int32, "delta col"), (d_prod, torch.float32, "delta prod"),
                      (d_cnt, torch.int32, "delta cnt"), (sumsq, torch.float32, "sumsq")):
        _req(t, dt, nm, 1)
    dev = d_ptr.device
    n_x = d_ptr.numel() - 1
    o_nnz, d_nnz = old.col.numel(), d_col.numel()
    if n_x < 0 or not 1 <= old.ptr.numel() <= n_x + 1:
        raise ValueError("the old state must have at least 0 and at most as many rows as the delta")
    if sumsq.numel() != n_x:
        raise ValueError(f"sumsq must hold one sum per row ({n_x}), got {sumsq.numel()}")
    if not (old.prod.numel() == old.cnt.numel() == old.sim.numel() == o_nnz) or not (d_prod.numel() == d_cnt.numel() == d_nnz):
        raise ValueError("every value array must have one element per column")
    if n_x > 2**31 - 1:
        raise ValueError("the state supports up to 2**31 - 1 rows")
    ends = [int(old.ptr[-1]), int(d_ptr[-1])] + [int(c.max()) if c.numel() else -1 for c in (old.col, d_col)]
    if ends[0] != o_nnz or ends[1] != d_nnz or max(ends[2:]) >= n_x:
        raise ValueError("a rowptr does not end at its number of entries, or a column is not below the number of rows")
    o_ptr = old.ptr
    if o_ptr.numel() < n_x + 1:      # rows beyond the old state are empty
        o_ptr = torch.full((n_x + 1,), o_nnz, dtype=torch.int64, device=dev)
        o_ptr[: old.ptr.numel()] = old.ptr
    sides = (_ptr(o_ptr), _ptr(old.col), _ptr(old.prod), _ptr(old.cnt), _ptr(old.sim), o_nnz, _ptr(d_ptr), _ptr(d_col),
             _ptr(d_prod), _ptr(d_cnt), d_nnz, n_x, _ptr(sumsq))
    rank = torch.zeros(d_nnz + 1, dtype=torch.int64, device=dev)
    if d_nnz:
        is_new = torch.empty(d_nnz, dtype=torch.uint8, device=dev)
        _call("lr_cf_state_merge_f32", *sides, 0, _ptr(is_new), 0, 0, 0, 0, 0, _stream())
        torch.cumsum(is_new, 0, dtype=torch.int64, out=rank[1:])
        del is_new
    total = o_nnz + int(rank[-1])
    need = total * CF_STATE_ENTRY_BYTES + (n_x + 1) * 8
    cap = _mem_cap(CF_SIM_MAX_BYTES, dev) if cap is None else int(cap)
    if need > cap:
        raise MemoryError(f"the pair state has {total} entries ({need / 2**30:.2f} GiB), above the {cap / 2**30:.2f} GiB "
                          "that the device can hold for it; train on fewer rows")
    new = CfState(o_ptr + rank[d_ptr], torch.empty(total, dtype=torch.int32, device=dev),
                  torch.empty(total, dtype=torch.float32, device=dev), torch.empty(total, dtype=torch.int32, device=dev),
                  torch.empty(total, dtype=torch.float32, device=dev))
    if total:
        _call("lr_cf_state_merge_f32", *sides, 1, 0, _ptr(rank), _ptr(new.col), _ptr(new.prod), _ptr(new.cnt),
              _ptr(new.sim), _stream())
    return new


def cf_state_visible(state: CfState, min_common: int):
    """(rowptr, col, sim) of the pairs that ranking and prediction see: cnt >= min_common (`sort_by_sims` /
    `update_by_sims`: counts only grow, so a pair enters once and is replaced whenever it is touched).  Values below 2
    keep every pair and return the state's own arrays."""
    if int(min_common) <= 1:
        return state.ptr, state.col, state.sim
    keep = state.cnt >= int(min_common)
    below = torch.zeros(keep.numel() + 1, dtype=torch.int64, device=keep.device)
    torch.cumsum(keep, 0, dtype=torch.int64, out=below[1:])
    return below[state.ptr], state.col[keep].contiguous(), state.sim[keep].contiguous()


def cf_predict_topk(srow: torch.Tensor, irow: torch.Tensor, tk_ids: torch.Tensor, tk_sims: torch.Tensor,
                    tk_len: torch.Tensor, i_ptr: torch.Tensor, i_col: torch.Tensor, i_val: torch.Tensor, k: int,
                    rating: bool, default_pred: float):
    """Predictions of the pairs (srow[q], irow[q]) the way the reference's Rust models make them (`item_cf.rs:118-153`,
    `compute_pred`): the top-k list of row srow[q] (`cf_topk`) is cut to k entries BEFORE it is intersected with the
    interaction row irow[q]; every hit counts whatever its label; ranking S / n, rating sum((label * sim) / S), sequential
    f32 sums in list order, unclipped.  Returns (pred f32 [n], none int32 [n]: 1 where there is no hit and pred is
    default_pred)."""
    for t, nm in ((srow, "srow"), (irow, "irow"), (i_col, "i_col"), (tk_len, "tk_len")):
        _req(t, torch.int32, nm, 1)
    _req(tk_ids, torch.int32, "tk_ids", 2)
    _req(tk_sims, torch.float32, "tk_sims", 2)
    _req(i_ptr, torch.int64, "i_ptr", 1)
    _req(i_val, torch.float32, "i_val", 1)
    if tk_ids.shape != tk_sims.shape or tk_len.numel() != tk_ids.shape[0] or tk_ids.shape[1] < 1:
        raise ValueError("tk_ids and tk_sims must be [n_rows, k'] with k' >= 1 and tk_len [n_rows]")
    if srow.numel() != irow.numel():
        raise ValueError("srow and irow must name as many pairs")
    if int(k) < 1:
        raise ValueError("k must be at least 1")
    if i_col.numel() != i_val.numel():
        raise ValueError("i_col and i_val must have one element per entry")
    n = srow.numel()
    pred = torch.empty(n, dtype=torch.float32, device=srow.device)
    none = torch.empty(n, dtype=torch.int32, device=srow.device)
    _call("lr_cf_predict_topk_f32", _ptr(srow), _ptr(irow), n, _ptr(tk_ids), _ptr(tk_sims), _ptr(tk_len), tk_ids.shape[1],
          int(k), _ptr(i_ptr), _ptr(i_col), _ptr(i_val), 1 if rating else 0, float(default_pred), _ptr(pred), _ptr(none),
          _stream())
    return pred, none


# --------------------------------------------------------------------------------------
# Swing (csrc/swing.hip)
# --------------------------------------------------------------------------------------
SWING_MAX_BYTES = None      # cap on the pair table, the score CSR and the kernel's scratch together; None: 90 % of the free memory


class _Stages:
    """HIP-event times of the stages of one call, in ms (scripts/swing_bench.py); inactive without a dict."""

    def __init__(self, out):
        self.out, self.marks = out, []

    def mark(self, name):
        if self.out is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.marks.append((name, e))

    def close(self):
        if self.out is not None:
            torch.cuda.synchronize()
            for (_, a), (name, b) in zip(self.marks[:-1], self.marks[1:]):
                self.out[name] = self.out.get(name, 0.0) + a.elapsed_time(b)


def swing_pair_table(u_ptr: torch.Tensor, u_col: torch.Tensor, i_ptr: torch.Tensor, i_col: torch.Tensor, alpha: float,
                     cap: Optional[int] = None, stages: Optional[dict] = None):
    """The user-pair table of Swing as an upper user x user CSR (rowptr int64, col int32 ascending, val f32): for every
    u < v that share an item, w_u * w_v / (alpha + |I_u ^ I_v| - 1) (`graph.rs:185-186`).  u_*: user x item CSR, i_*: its
    transpose.  Counted before it is allocated: a table above `cap` bytes raises MemoryError."""
    _req(u_ptr, torch.int64, "u_ptr", 1)
    _req(u_col, torch.int32, "u_col", 1)
    _req(i_ptr, torch.int64, "i_ptr", 1)
    _req(i_col, torch.int32, "i_col", 1)
    dev = u_ptr.device
    n_users = u_ptr.numel() - 1
    if n_users > 2**31 - 1:
        raise ValueError("Swing supports up to 2**31 - 1 users")
    st = _Stages(stages)
    st.mark("start")
    T = int(_lib.load().lr_swing_tile_cols())
    nnz = u_col.numel()
    rowptr = torch.zeros(n_users + 1, dtype=torch.int64, device=dev)
    empty = (rowptr, torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.float32, device=dev))
    if nnz == 0:
        return empty
    # work items: (user, tile) over the tiles between u + 1 and the largest user that shares an item with u
    deg_i = i_ptr[1:] - i_ptr[:-1]
    rows_u = torch.repeat_interleave(torch.arange(n_users, device=dev), u_ptr[1:] - u_ptr[:-1], output_size=nnz)
    ic = u_col.to(torch.int64)
    work = torch.zeros(n_users, dtype=torch.int64, device=dev).index_add_(0, rows_u, deg_i[ic])
    last = i_col[(i_ptr[1:] - 1).clamp(min=0)].to(torch.int64)
    vmax = torch.full((n_users,), -1, dtype=torch.int64, device=dev).scatter_reduce_(0, rows_u, last[ic], "amax")
    me = torch.arange(n_users, device=dev)
    tmin = torch.div(me + 1, T, rounding_mode="floor")
    tmax = torch.div(vmax, T, rounding_mode="floor")
    span = torch.where(vmax > me, tmax - tmin + 1, torch.zeros_like(work))
    items = _tile_work_items(n_users, work, tmin, span)
    if items[3] == 0:
        return empty
    lead = (_ptr(u_ptr), _ptr(u_col), _ptr(i_ptr), _ptr(i_col), n_users, float(alpha))
    out = _two_pass_csr("lr_swing_pairs_f32", lead, rowptr, items, _lib.load().lr_swing_pairs_ws_bytes(), cap, SWING_MAX_BYTES,
                        "Swing: the user-pair table has {total} entries ({gib:.2f} GiB), above the {cap_gib:.2f} GiB that "
                        "the device can hold for it; train on fewer users", lambda stage: st.mark("pairs_" + stage))
    st.close()
    return out


def _csr_add(n: int, a, b):
    """a + b of two n x n device CSRs with ascending columns; every entry has at most two addends, summed without atomics."""
    dev = a[0].device

    def keys(ptr, col):
        rows = torch.repeat_interleave(torch.arange(ptr.numel() - 1, device=dev), ptr[1:] - ptr[:-1],
                                       output_size=col.numel())
        return rows * n + col.to(torch.int64)

    ka, kb = keys(a[0], a[1]), keys(b[0], b[1])
    uniq, inv = torch.unique(torch.cat([ka, kb]), return_inverse=True)
    val = torch.zeros(uniq.numel(), dtype=torch.float32, device=dev)
    ia, ib = inv[: ka.numel()], inv[ka.numel():]
    val[ia] = a[2]
    val[ib] = val[ib] + b[2]
    rows = torch.div(uniq, n, rounding_mode="floor")
    ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    ptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0)
    return ptr, (uniq - rows * n).to(torch.int32).contiguous(), val


def swing_scores(u_ptr: torch.Tensor, u_col: torch.Tensor, i_ptr: torch.Tensor, i_col: torch.Tensor, alpha: float,
                 prev=None, stages: Optional[dict] = None):
    """The Swing score CSR (rowptr int64 [n_items + 1], col int32 ascending per row, val f32; `graph.rs:143-233`) of the
    user x item pattern u_* with transpose i_*: s[i][j] = sum over the user pairs u < v of U_i ^ U_j of
    w_u w_v / (alpha + |I_u ^ I_v| - 1).  The pattern (the item pairs with at least two common users) is counted, scanned
    and filled by the co-occurrence kernel of the CF similarity, the values by csrc/swing.hip; nothing is allocated before
    its size is known, and a pair table, result or scratch above the memory cap raises MemoryError.  `prev` (rowptr, col,
    val of an earlier result, at most n_items rows) is added entry by entry: the retrain of `init_item_scores`."""
    dev = u_ptr.device
    n_items = i_ptr.numel() - 1
    cap = _mem_cap(SWING_MAX_BYTES, dev)
    st = _Stages(stages)
    p_ptr, p_col, p_val = swing_pair_table(u_ptr, u_col, i_ptr, i_col, alpha, cap=cap, stages=stages)
    used = p_col.numel() * 8 + p_ptr.numel() * 8
    st.mark("start")
    cnt = (i_ptr[1:] - i_ptr[:-1]).to(torch.int32)
    try:
        s_ptr, s_col, s_val = cf_similarity(i_ptr, i_col, None, u_ptr, u_col, None, "jaccard", 2, cnt=cnt,
                                            cap=max(cap - used, 0))
    except MemoryError as e:
        raise MemoryError(f"Swing: {e}".replace("; raise `min_common` or use fewer rows",
                                                " next to the user-pair table; train on fewer items")) from e
    st.mark("pattern")
    nnz = s_col.numel()
    if nnz:
        lib = _lib.load()
        longest = int(cnt.max())
        ws_bytes = int(lib.lr_swing_scores_ws_bytes(longest))
        used += nnz * 12 + s_ptr.numel() * 8
        if used + ws_bytes > cap:
            raise MemoryError(f"Swing: the score kernel needs {ws_bytes / 2**30:.2f} GiB of scratch for items with up to "
                              f"{longest} users, above what is left of the {cap / 2**30:.2f} GiB cap")
        s_row = torch.repeat_interleave(torch.arange(n_items, device=dev, dtype=torch.int32), s_ptr[1:] - s_ptr[:-1],
                                        output_size=nnz)
        s_val = torch.zeros(nnz, dtype=torch.float32, device=dev)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        st.mark("scores_plan")
        _call("lr_swing_scores_f32", _ptr(i_ptr), _ptr(i_col), longest, u_ptr.numel() - 1, _ptr(p_ptr), _ptr(p_col),
              _ptr(p_val), _ptr(s_ptr), _ptr(s_col), _ptr(s_row), nnz, _ptr(s_val), _ptr(ws), ws.numel(), _stream())
        st.mark("scores")
    out = (s_ptr, s_col, s_val)
    if prev is not None and prev[1].numel():
        pp = torch.full((n_items + 1,), int(prev[0][-1]), dtype=torch.int64, device=dev)
        pp[: prev[0].numel()] = prev[0]
        out = _csr_add(n_items, (pp, prev[1], prev[2]), out)
        st.mark("merge_prev")
    st.close()
    return out


# --------------------------------------------------------------------------------------
# BPR (csrc/bpr.hip): triple score + ordered row update
# --------------------------------------------------------------------------------------
BPR_MODES = {"score": 0, "stash": 1, "grad": 2}
BPR_OPTIMIZERS = {"sgd": 0, "momentum": 1, "adam": 2}


def bpr_supported(embed_size: int, with_bias_column: bool = True) -> bool:
    """Whether the BPR kernels take rows of `embed_size` (+ 1 with the bias column) floats."""
    return bool(_lib.load().lr_bpr_supported(int(embed_size) + (1 if with_bias_column else 0)))


def bpr_triple_score(U: torch.Tensor, I: torch.Tensor, users: torch.Tensor, pos: torch.Tensor, neg: torch.Tensor,
                     mode: str = "score", ibias: Optional[torch.Tensor] = None, gscale: float = 1.0, want_loss: bool = True,
                     out: Optional[dict] = None) -> dict:
    """`lr_bpr_triple_score_f32` over W samples: {"c" [W], "loss" [W] (-log sigmoid(d)), and by `mode` "gu" [W, D] (stash:
    p - q; grad: the user gradient rows), "gi" [2 W, D] and "gb" [2 W] (grad: item rows and item bias, positive then negative
    per sample)}.  `out` may carry preallocated buffers with those keys (at least as long; their leading W rows are written)."""
    _req(U, torch.float32, "U", 2)
    _req(I, torch.float32, "I", 2)
    for t_, n_ in ((users, "users"), (pos, "pos"), (neg, "neg")):
        _req(t_, torch.int32, n_, 1)
    W, D = users.numel(), U.shape[1]
    if I.shape[1] != D or pos.numel() != W or neg.numel() != W:
        raise ValueError("shape mismatch")
    if ibias is not None:
        _req(ibias, torch.float32, "ibias")
        if ibias.numel() != I.shape[0]:
            raise ValueError("ibias must hold one value per item")
    m = BPR_MODES[mode]
    out = {} if out is None else out
    dev = U.device

    def buf(key, shape, want=True):
        if not want:
            return None
        t = out.get(key)
        if t is None:
            t = out[key] = torch.empty(shape, dtype=torch.float32, device=dev)
        elif _req(t, torch.float32, key).numel() < int(torch.Size(shape).numel()):
            raise ValueError(f"out[{key!r}] is too small")
        return t

    c = buf("c", (W,))
    loss = buf("loss", (W,), want_loss)
    gu = buf("gu", (W, D), m != 0)
    gi = buf("gi", (2 * W, D), m == 2)
    gb = buf("gb", (2 * W,), m == 2 and ibias is not None)
    _call("lr_bpr_triple_score_f32", _ptr(U), U.shape[0], D, _ptr(I), I.shape[0], D, _ptr(ibias), D, _ptr(users), _ptr(pos),
          _ptr(neg), W, m, float(gscale), _ptr(c), _ptr(loss), _ptr(gu), _ptr(gi), _ptr(gb), _stream())
    return out


def bpr_row_update(optimizer: str, table: torch.Tensor, seg: Segments, c: torch.Tensor, other: torch.Tensor, lr: float,
                   reg: float, epoch: int, state1: Optional[torch.Tensor] = None, state2: Optional[torch.Tensor] = None,
                   users: Optional[torch.Tensor] = None) -> None:
    """`lr_bpr_row_update_f32`: the ordered update of one window's touched rows of `table` [V, D].  Item rows: `seg` over the
    2 W interleaved (positive, negative) ids, `users` [W] and `other` = the user table; user rows: `seg` over the W user ids,
    `users` None and `other` = the stash [W, D] (the bias column, the last one, is not written).  `c` holds at least W values."""
    _req(table, torch.float32, "table", 2)
    _req(c, torch.float32, "c", 1)
    _req(other, torch.float32, "other", 2)
    V, D = table.shape
    item = users is not None
    W = seg.n // 2 if item else seg.n
    if item:
        _req(users, torch.int32, "users", 1)
        if seg.n != 2 * users.numel():
            raise ValueError("item segments must cover two ids per sample")
    if V != seg.V or other.shape[1] != D or c.numel() < W or (not item and other.shape[0] < W):
        raise ValueError("shape mismatch")
    opt = BPR_OPTIMIZERS[optimizer]
    for t_, n_, need in ((state1, "state1", opt >= 1), (state2, "state2", opt == 2)):
        if need:
            if _req(t_, torch.float32, n_, 2).shape != table.shape:
                raise ValueError(f"{n_} must have the table's shape")
    _call("lr_bpr_row_update_f32", opt, _ptr(table), _ptr(state1) if opt >= 1 else None, _ptr(state2) if opt == 2 else None, V, D,
          D if item else D - 1, _ptr(seg.pos), _ptr(seg.rows), _ptr(seg.start), _ptr(seg.n_seg), seg.n, _ptr(c), W, _ptr(other),
          other.shape[0] if item else W, _ptr(users), float(lr), float(reg), int(epoch), _stream())


# --------------------------------------------------------------------------------------
# SVD / SVD++ (csrc/svd.hip)
# --------------------------------------------------------------------------------------
MF_LOSSES = {"mse": 0, "cross_entropy": 1, "focal": 2}


def svd_supported(embed_size: int) -> bool:
    """Whether the SVD / SVD++ kernels take rows of `embed_size` floats."""
    return bool(_lib.load().lr_svd_supported(int(embed_size)))


def svdpp_pool(P: Optional[torch.Tensor], Y: torch.Tensor, hist_ptr: torch.Tensor, hist_idx: torch.Tensor,
               rows: Optional[torch.Tensor] = None, n_rows_dev: Optional[torch.Tensor] = None, n_rows: Optional[int] = None,
               n_users: Optional[int] = None, want_scale: bool = False):
    """`lr_svdpp_pool_f32`: out[r] = P[row(r)] + |N|^-1/2 sum of the Y rows of that user's history (`hist_ptr` int64
    [n_users + 1], `hist_idx` int32).  `rows` int32 lists the users (`n_rows_dev`: a device int32 count of its valid leading
    entries, the rows beyond stay unwritten) or is None: every user.  `P` may be None (the pooled term alone).  Returns out
    [n_rows, K], and with `want_scale` also |N|^-1/2 per row."""
    _req(Y, torch.float32, "Y", 2)
    _req(hist_ptr, torch.int64, "hist_ptr", 1)
    _req(hist_idx, torch.int32, "hist_idx", 1)
    K = Y.shape[1]
    nU = hist_ptr.numel() - 1 if n_users is None else int(n_users)
    if P is not None:
        if _req(P, torch.float32, "P", 2).shape != (nU, K):
            raise ValueError("P must be [n_users, K]")
    if hist_ptr.numel() != nU + 1:
        raise ValueError("hist_ptr must hold n_users + 1 offsets")
    if rows is not None:
        _req(rows, torch.int32, "rows", 1)
        n = rows.numel() if n_rows is None else int(n_rows)
        if n > rows.numel():
            raise ValueError("n_rows exceeds the row list")
    else:
        if n_rows_dev is not None:
            raise ValueError("n_rows_dev needs a row list")
        n = nU if n_rows is None else int(n_rows)
    if n_rows_dev is not None:
        _req(n_rows_dev, torch.int32, "n_rows_dev")
    out = torch.empty((max(n, 1), K), dtype=torch.float32, device=Y.device)
    scale = torch.empty(max(n, 1), dtype=torch.float32, device=Y.device) if want_scale else None
    _call("lr_svdpp_pool_f32", _ptr(P), _ptr(Y), nU, Y.shape[0], K, _ptr(hist_ptr), _ptr(hist_idx), hist_idx.numel(), _ptr(rows),
          _ptr(n_rows_dev), n, _ptr(out), _ptr(scale), _stream())
    return (out[:n], scale[:n]) if want_scale else out[:n]


def mf_score(X: torch.Tensor, Q: torch.Tensor, bu: Optional[torch.Tensor], bi: Optional[torch.Tensor], users: torch.Tensor,
             items: torch.Tensor, labels: torch.Tensor, loss: str, xidx: Optional[torch.Tensor] = None, mode: str = "score",
             gscale: float = 1.0) -> dict:
    """`lr_mf_score_f32` over B samples: {"score", "loss", "g" [B]} and with mode="grad" also "gx" [B, K] = g Q[item] and
    "gq" [B, K] = g X[x].  `X` is the user table (x = the user) or, with `xidx`, a block of rows addressed per sample."""
    _req(X, torch.float32, "X", 2)
    _req(Q, torch.float32, "Q", 2)
    for t_, n_ in ((users, "users"), (items, "items")):
        _req(t_, torch.int32, n_, 1)
    _req(labels, torch.float32, "labels", 1)
    B, K = users.numel(), X.shape[1]
    if Q.shape[1] != K or items.numel() != B or labels.numel() != B:
        raise ValueError("shape mismatch")
    nU = X.shape[0]
    if xidx is not None:
        if _req(xidx, torch.int32, "xidx", 1).numel() != B:
            raise ValueError("xidx must hold one row per sample")
        nU = bu.numel() if bu is not None else (1 << 31) - 1
    for t_, n_, n in ((bu, "bu", nU), (bi, "bi", Q.shape[0])):
        if t_ is not None and _req(t_, torch.float32, n_).numel() != n:
            raise ValueError(f"{n_} must hold one value per row")
    if mode not in ("score", "grad"):
        raise ValueError("mode must be `score` or `grad`")
    dev = X.device
    out = {k: torch.empty(max(B, 1), dtype=torch.float32, device=dev)[:B] for k in ("score", "loss", "g")}
    if mode == "grad":
        out["gx"] = torch.empty((max(B, 1), K), dtype=torch.float32, device=dev)[:B]
        out["gq"] = torch.empty((max(B, 1), K), dtype=torch.float32, device=dev)[:B]
    _call("lr_mf_score_f32", _ptr(X), X.shape[0], _ptr(xidx), _ptr(Q), Q.shape[0], _ptr(bu), nU, _ptr(bi), K, _ptr(users),
          _ptr(items), _ptr(labels), B, MF_LOSSES[loss], 1 if mode == "grad" else 0, float(gscale), _ptr(out["score"]),
          _ptr(out["loss"]), _ptr(out["g"]), _ptr(out.get("gx")), _ptr(out.get("gq")), _stream())
    return out


def svdpp_hist_grad(G: torch.Tensor, scale: torch.Tensor, ent_slot: torch.Tensor, seg: Segments, Y: Optional[torch.Tensor] = None,
                    m: Optional[torch.Tensor] = None, v: Optional[torch.Tensor] = None, hp: Optional[AdamHP] = None,
                    ws: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """`lr_svdpp_hist_grad_f32`: every Y row touched by the entries (`seg` over their Y rows, `ent_slot` their user slots)
    takes sum_e scale[slot_e] G[slot_e] in run order.  With `Y`, `m`, `v` and `hp`: the fused Adam step on those rows
    (returns None); without: the sums per run, [min(seg.n, n_items), K] with the first n_seg rows written, for `adam_dense`.
    No [entries, K] array is allocated in either form."""
    _req(G, torch.float32, "G", 2)
    _req(scale, torch.float32, "scale", 1)
    _req(ent_slot, torch.int32, "ent_slot", 1)
    K = G.shape[1]
    if ent_slot.numel() < seg.n or scale.numel() > G.shape[0]:
        raise ValueError("shape mismatch")
    fused = Y is not None
    if fused:
        for t_, n_ in ((Y, "Y"), (m, "m"), (v, "v")):
            if _req(t_, torch.float32, n_, 2).shape != (seg.V, K):
                raise ValueError(f"{n_} must be [n_items, K]")
        if hp is None:
            raise ValueError("the fused form needs the Adam hyper-parameters")
    # one row per touched y row, never per entry: n_seg <= min(entries, n_items)
    grows = None if fused else torch.empty((max(min(seg.n, seg.V), 1), K), dtype=torch.float32, device=G.device)
    if ws is None and seg.n > 0:
        if seg.owner is not None and hasattr(seg.owner, "hist_ws"):
            ws = seg.owner.hist_ws(K)                 # kept with the builder: no allocation per step
        else:
            ws = torch.empty(max(_lib.load().lr_svdpp_hist_grad_ws_bytes(seg.n, K), 256), dtype=torch.uint8, device=G.device)
    _call("lr_svdpp_hist_grad_f32", 0 if fused else 1, _ptr(Y), _ptr(m), _ptr(v), seg.V, K, _ptr(G), _ptr(scale), scale.numel(),
          _ptr(ent_slot), _ptr(seg.pos), _ptr(seg.rows), _ptr(seg.start), _ptr(seg.n_seg), seg.n, _ptr(grows),
          hp if hp is not None else adam_hp(0.0, 1), _ptr(ws), 0 if ws is None else ws.numel(), _stream())
    return grows


# --------------------------------------------------------------------------------------
# recurrent layers (csrc/rnn.hip)
# --------------------------------------------------------------------------------------
RNN_CELLS = {"gru": 0, "lstm": 1}


def rnn_supported(cell: str, D: int, H: int) -> bool:
    """Whether the recurrent-layer kernels take `D` inputs and `H` units for this cell."""
    return cell in RNN_CELLS and bool(_lib.load().lr_rnn_supported(RNN_CELLS[cell], int(D), int(H)))


def _rnn_check(cell, W, U, lens, x, table, ids, in_mask, rec_mask):
    """-> (B, L, D, H, V) of one recurrent-layer call, its operands validated."""
    if cell not in RNN_CELLS:
        raise ValueError("cell must be `gru` or `lstm`")
    G = 3 if cell == "gru" else 4
    _req(W, torch.float32, "W", 2)
    _req(U, torch.float32, "U", 2)
    _req(lens, torch.int32, "lens", 1)
    D, H = W.shape[0], U.shape[0]
    if W.shape[1] != G * H or U.shape[1] != G * H:
        raise ValueError(f"W must be [D, {G}H] and U [H, {G}H]")
    if x is not None:
        if table is not None or ids is not None:
            raise ValueError("give either x or (table, ids)")
        if _req(x, torch.float32, "x", 3).shape[2] != D:
            raise ValueError("x must be [B, L, D]")
        B, L, V = x.shape[0], x.shape[1], 0
    else:
        if table is None or ids is None:
            raise ValueError("give either x or (table, ids)")
        if _req(table, torch.float32, "table", 2).shape[1] != D:
            raise ValueError("table must be [V, D]")
        _req(ids, torch.int32, "ids", 2)
        B, L, V = ids.shape[0], ids.shape[1], table.shape[0]
    if lens.numel() != B:
        raise ValueError("lens must hold one length per sample")
    for t_, n_, w_ in ((in_mask, "in_mask", D), (rec_mask, "rec_mask", H)):
        if t_ is not None and _req(t_, torch.float32, n_, 2).shape != (B, w_):
            raise ValueError(f"{n_} must be [B, {w_}]")
    return B, L, D, H, V


def rnn_layer_fwd(cell: str, W: torch.Tensor, U: torch.Tensor, b: torch.Tensor, lens: torch.Tensor,
                  x: Optional[torch.Tensor] = None, table: Optional[torch.Tensor] = None, ids: Optional[torch.Tensor] = None,
                  in_mask: Optional[torch.Tensor] = None, rec_mask: Optional[torch.Tensor] = None, act: bool = True):
    """`lr_rnn_layer_fwd_f32`: one GRU / LSTM layer over x [B, L, D] or over the rows table[ids] read in place.  Returns
    (hs [B, L, H], saved): every output step (a masked step repeats the carried state) and what `rnn_layer_bwd` reads."""
    B, L, D, H, V = _rnn_check(cell, W, U, lens, x, table, ids, in_mask, rec_mask)
    G = 3 if cell == "gru" else 4
    if _req(b, torch.float32, "b").numel() != (2 if cell == "gru" else 1) * G * H:
        raise ValueError("b must be [2, 3H] for the GRU and [4H] for the LSTM")
    c = RNN_CELLS[cell]
    hs = torch.empty((max(B, 1), L, H), dtype=torch.float32, device=W.device)[:B]
    nbytes = _lib.load().lr_rnn_fwd_saved_bytes(c, B, L, H)
    saved = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=W.device)
    _call("lr_rnn_layer_fwd_f32", c, 1 if act else 0, _ptr(x), _ptr(table), V, _ptr(ids), _ptr(lens), B, L, D, H, _ptr(W), _ptr(U),
          _ptr(b), _ptr(in_mask), _ptr(rec_mask), _ptr(hs), _ptr(saved), saved.numel() * 4, _stream())
    return hs, saved


def rnn_layer_bwd(cell: str, W: torch.Tensor, U: torch.Tensor, lens: torch.Tensor, hs: torch.Tensor, saved: torch.Tensor,
                  ghs: torch.Tensor, x: Optional[torch.Tensor] = None, table: Optional[torch.Tensor] = None,
                  ids: Optional[torch.Tensor] = None, in_mask: Optional[torch.Tensor] = None,
                  rec_mask: Optional[torch.Tensor] = None, act: bool = True):
    """`lr_rnn_layer_bwd_f32`: from ghs [B, L, H] (the gradient of every output step) -> (gx [B, L, D], gW, gU, gb); gx is
    exactly 0 at masked steps, the weight gradients are summed in a fixed order."""
    B, L, D, H, V = _rnn_check(cell, W, U, lens, x, table, ids, in_mask, rec_mask)
    G = 3 if cell == "gru" else 4
    _req(hs, torch.float32, "hs", 3)
    _req(saved, torch.float32, "saved", 1)
    if _req(ghs, torch.float32, "ghs", 3).shape != (B, L, H) or hs.shape != (B, L, H):
        raise ValueError("hs and ghs must be [B, L, H]")
    c = RNN_CELLS[cell]
    if saved.numel() * 4 < _lib.load().lr_rnn_fwd_saved_bytes(c, B, L, H):
        raise ValueError("saved is not the forward's buffer for this shape")
    dev = W.device
    gx = torch.empty((max(B, 1), L, D), dtype=torch.float32, device=dev)[:B]
    gW = torch.empty((D, G * H), dtype=torch.float32, device=dev)
    gU = torch.empty((H, G * H), dtype=torch.float32, device=dev)
    gb = torch.empty((2, G * H) if cell == "gru" else (G * H,), dtype=torch.float32, device=dev)
    ws = torch.empty(max(_lib.load().lr_rnn_bwd_ws_bytes(c, B, L, D, H), 256), dtype=torch.uint8, device=dev)
    _call("lr_rnn_layer_bwd_f32", c, 1 if act else 0, _ptr(x), _ptr(table), V, _ptr(ids), _ptr(lens), B, L, D, H, _ptr(W), _ptr(U),
          _ptr(in_mask), _ptr(rec_mask), _ptr(hs), _ptr(saved), _ptr(ghs), _ptr(gx), _ptr(gW), _ptr(gU), _ptr(gb), _ptr(ws),
          ws.numel(), _stream())
    return gx, gW, gU, gb


# --------------------------------------------------------------------------------------
# WaveNet stack (csrc/wavenet.hip)
# --------------------------------------------------------------------------------------
def wavenet_supported(L: int, D: int, F: int, n_blocks: int, n_per_block: int) -> bool:
    """Whether the WaveNet kernels take windows of `L` ids, a table of width `D`, `F` filters and this many layers."""
    return bool(_lib.load().lr_wavenet_supported(int(L), int(D), int(F), int(n_blocks), int(n_per_block)))


def wavenet_param_floats(D: int, F: int, n_blocks: int, n_per_block: int) -> int:
    """Length of the parameter buffer (conv1d/kernel, conv1d/bias, conv1d_1/kernel, ... then the 1x1 pair, every tensor on a
    16-byte boundary: the layout `DenseParams` gives tensors added in that order); 0 for an unsupported shape."""
    return _lib.load().lr_wavenet_params_bytes(int(D), int(F), int(n_blocks), int(n_per_block)) // 4


def _wavenet_check(table, ids, params, F, n_blocks, n_per_block):
    """-> (B, L, D, V) of one WaveNet call, its operands validated."""
    D = _req(table, torch.float32, "table", 2).shape[1]
    _req(ids, torch.int32, "ids", 2)
    _req(params, torch.float32, "params", 1)
    B, L = ids.shape
    if table.shape[0] < 1:
        raise ValueError("table must hold at least one row")
    if not wavenet_supported(L, D, F, n_blocks, n_per_block):
        raise ValueError(f"unsupported WaveNet shape: L={L}, D={D}, F={F}, {n_blocks} x {n_per_block} layers (L, D and F from 1 "
                         "to 128, at most 16 dilated layers)")
    if params.numel() != wavenet_param_floats(D, F, n_blocks, n_per_block):
        raise ValueError("params must be the flat parameter buffer of this shape (see `wavenet_param_floats`)")
    if params.data_ptr() % 16:
        raise ValueError("params must start on a 16-byte boundary")
    return B, L, D, table.shape[0]


def wavenet_fwd(table: torch.Tensor, ids: torch.Tensor, params: torch.Tensor, F: int, n_blocks: int, n_per_block: int):
    """`lr_wavenet_fwd_f32`: the dilated stack, the 1x1 layer and the pool over the rows table[ids] read in place.  Returns
    (acts [n_layers + 1, B, L, F], pooled [B, F], arg int32 [B, F])."""
    B, L, D, V = _wavenet_check(table, ids, params, F, n_blocks, n_per_block)
    nl, dev = n_blocks * n_per_block, table.device
    acts = torch.empty((nl + 1, max(B, 1), L, F), dtype=torch.float32, device=dev)[:, :B]
    pooled = torch.empty((max(B, 1), F), dtype=torch.float32, device=dev)[:B]
    arg = torch.empty((max(B, 1), F), dtype=torch.int32, device=dev)[:B]
    if B == 0:
        return acts, pooled, arg
    _call("lr_wavenet_fwd_f32", _ptr(table), V, _ptr(ids), B, L, D, F, n_blocks, n_per_block, _ptr(params), _ptr(acts),
          acts.numel() * 4, _ptr(pooled), _ptr(arg), _stream())
    return acts, pooled, arg


def wavenet_bwd(table: torch.Tensor, ids: torch.Tensor, params: torch.Tensor, F: int, n_blocks: int, n_per_block: int,
                acts: torch.Tensor, arg: torch.Tensor, gpooled: torch.Tensor, gparams: Optional[torch.Tensor] = None):
    """`lr_wavenet_bwd_f32`: from gpooled [B, F] -> (gx [B, L, D], gparams in the layout of `params`); `gparams` may be given
    (e.g. a slice of `DenseParams.grad`) and is overwritten.  Parameter gradients are summed in a fixed order."""
    B, L, D, V = _wavenet_check(table, ids, params, F, n_blocks, n_per_block)
    nl, dev = n_blocks * n_per_block, table.device
    if _req(acts, torch.float32, "acts", 4).shape != (nl + 1, B, L, F):
        raise ValueError("acts must be the forward's [n_layers + 1, B, L, F]")
    if _req(arg, torch.int32, "arg", 2).shape != (B, F) or _req(gpooled, torch.float32, "gpooled", 2).shape != (B, F):
        raise ValueError("arg and gpooled must be [B, F]")
    if gparams is None:
        gparams = torch.empty_like(params)
    elif _req(gparams, torch.float32, "gparams", 1).numel() != params.numel():
        raise ValueError("gparams must have the length of params")
    gx = torch.empty((max(B, 1), L, D), dtype=torch.float32, device=dev)[:B]
    ws = torch.empty(max(_lib.load().lr_wavenet_bwd_ws_bytes(B, L, D, F, n_blocks, n_per_block), 256), dtype=torch.uint8, device=dev)
    _call("lr_wavenet_bwd_f32", _ptr(table), V, _ptr(ids), B, L, D, F, n_blocks, n_per_block, _ptr(params), _ptr(acts),
          _ptr(gpooled), _ptr(arg), _ptr(gx), _ptr(gparams), _ptr(ws), ws.numel(), _stream())
    return gx, gparams


# --------------------------------------------------------------------------------------
# Caser convolutions (csrc/caser.hip)
# --------------------------------------------------------------------------------------
def caser_supported(L: int, K: int, nh: int, nv: int) -> bool:
    """Whether the Caser kernels take windows of `L` ids, a table of width `K`, `nh` horizontal and `nv` vertical filters."""
    return bool(_lib.load().lr_caser_supported(int(L), int(K), int(nh), int(nv)))


def caser_param_floats(L: int, K: int, nh: int, nv: int) -> int:
    """Length of the parameter buffer (conv1d/kernel [1, K, nh], conv1d/bias, ... conv1d_{L-1}/kernel [L, K, nh] and bias, then
    the vertical conv1d_{L}/kernel [1, L, nv] and bias, every tensor on a 16-byte boundary: the layout `DenseParams` gives
    tensors added in that order); 0 for an unsupported shape."""
    return _lib.load().lr_caser_params_bytes(int(L), int(K), int(nh), int(nv)) // 4


def _caser_check(table, ids, params, nh, nv):
    """-> (B, L, K, V) of one Caser call, its operands validated."""
    K = _req(table, torch.float32, "table", 2).shape[1]
    _req(ids, torch.int32, "ids", 2)
    _req(params, torch.float32, "params", 1)
    B, L = ids.shape
    if table.shape[0] < 1:
        raise ValueError("table must hold at least one row")
    if not caser_supported(L, K, nh, nv):
        raise ValueError(f"unsupported Caser shape: L={L}, K={K}, nh={nh}, nv={nv} (L from 1 to 64, K from 1 to 128, nh and nv "
                         "from 1 to 64)")
    if params.numel() != caser_param_floats(L, K, nh, nv):
        raise ValueError("params must be the flat parameter buffer of this shape (see `caser_param_floats`)")
    if params.data_ptr() % 16:
        raise ValueError("params must start on a 16-byte boundary")
    return B, L, K, table.shape[0]


def caser_fwd(table: torch.Tensor, ids: torch.Tensor, params: torch.Tensor, nh: int, nv: int, need_arg: bool = True):
    """`lr_caser_fwd_f32`: the L horizontal convolutions with their max over time and the vertical convolution over the rows
    table[ids] read in place.  Returns (feat [B, L nh + K nv], arg int32 [B, L nh]: the first position that holds each
    maximum; None unless `need_arg`, the inference mode)."""
    B, L, K, V = _caser_check(table, ids, params, nh, nv)
    dev = table.device
    feat = torch.empty((max(B, 1), L * nh + K * nv), dtype=torch.float32, device=dev)[:B]
    arg = torch.empty((max(B, 1), L * nh), dtype=torch.int32, device=dev)[:B] if need_arg else None
    if B == 0:
        return feat, arg
    _call("lr_caser_fwd_f32", _ptr(table), V, _ptr(ids), B, L, K, nh, nv, _ptr(params), _ptr(feat), _ptr(arg), _stream())
    return feat, arg


def caser_bwd(table: torch.Tensor, ids: torch.Tensor, params: torch.Tensor, nh: int, nv: int, feat: torch.Tensor,
              arg: torch.Tensor, gfeat: torch.Tensor, gparams: Optional[torch.Tensor] = None):
    """`lr_caser_bwd_f32`: from gfeat [B, L nh + K nv] -> (gx [B, L, K], gparams in the layout of `params`); `gparams` may be
    given (e.g. a slice of `DenseParams.grad`) and is overwritten.  Parameter gradients are summed in a fixed order."""
    B, L, K, V = _caser_check(table, ids, params, nh, nv)
    dev, width = table.device, L * nh + K * nv
    if _req(feat, torch.float32, "feat", 2).shape != (B, width) or _req(gfeat, torch.float32, "gfeat", 2).shape != (B, width):
        raise ValueError("feat and gfeat must be [B, L nh + K nv]")
    if _req(arg, torch.int32, "arg", 2).shape != (B, L * nh):
        raise ValueError("arg must be the forward's [B, L nh]")
    if gparams is None:
        gparams = torch.empty_like(params)
    elif _req(gparams, torch.float32, "gparams", 1).numel() != params.numel():
        raise ValueError("gparams must have the length of params")
    gx = torch.empty((max(B, 1), L, K), dtype=torch.float32, device=dev)[:B]
    if B == 0:
        gparams.zero_()
        return gx, gparams
    ws = torch.empty(max(_lib.load().lr_caser_bwd_ws_bytes(B, L, K, nh, nv), 256), dtype=torch.uint8, device=dev)
    _call("lr_caser_bwd_f32", _ptr(table), V, _ptr(ids), B, L, K, nh, nv, _ptr(params), _ptr(feat), _ptr(arg), _ptr(gfeat),
          _ptr(gx), _ptr(gparams), _ptr(ws), ws.numel(), _stream())
    return gx, gparams


# --------------------------------------------------------------------------------------
# AutoInt stack (csrc/autoint.hip)
# --------------------------------------------------------------------------------------
def _head_dims(head_dims):
    """The per-layer head dimensions as the host int array the entry points read."""
    dims = [int(h) for h in head_dims]
    return len(dims), (_lib.C.c_int * max(len(dims), 1))(*dims)


def autoint_supported(T: int, D: int, H: int, head_dims) -> bool:
    """Whether the AutoInt kernels take `T` fields of width `D`, `H` heads and these per-layer head dimensions."""
    n, hd = _head_dims(head_dims)
    return bool(_lib.load().lr_autoint_supported(int(T), int(D), int(H), n, hd))


def autoint_param_floats(T: int, D: int, H: int, head_dims) -> int:
    """Length of the parameter buffer (per layer the query, key, value [D, H hd] and attention_output [H hd, D] kernels, then
    dense/kernel [T D] and dense/bias [1], every tensor on a 16-byte boundary: the layout `DenseParams` gives tensors added in
    that order); 0 for an unsupported shape."""
    n, hd = _head_dims(head_dims)
    return _lib.load().lr_autoint_params_bytes(int(T), int(D), int(H), n, hd) // 4


def _autoint_check(x, params, H, head_dims):
    """-> (B, T, D, n_layers, host head dimensions) of one AutoInt call, its operands validated."""
    B, T, D = _req(x, torch.float32, "x", 3).shape
    _req(params, torch.float32, "params", 1)
    if not autoint_supported(T, D, H, head_dims):
        raise ValueError(f"unsupported AutoInt shape: T={T}, D={D}, H={H}, head_dims={tuple(head_dims)} (T, D and H * head_dim "
                         "from 1 to 64, 1 to 8 heads, 1 to 8 layers)")
    if params.numel() != autoint_param_floats(T, D, H, head_dims):
        raise ValueError("params must be the flat parameter buffer of this shape (see `autoint_param_floats`)")
    if params.data_ptr() % 16:
        raise ValueError("params must start on a 16-byte boundary")
    n, hd = _head_dims(head_dims)
    return B, T, D, n, hd


def autoint_fwd(x: torch.Tensor, params: torch.Tensor, H: int, head_dims, residual: bool = True, want_acts: bool = True):
    """`lr_autoint_fwd_f32`: the attention stack over x [B, T, D] and the Dense(1) read-out.  Returns (logits [B], acts
    [n_layers, B, T, D] — slab l - 1 is the output of layer l —, saved: the opaque bytes `autoint_bwd` wants next to acts);
    without `want_acts` acts and saved are None: inference, only the logits are written."""
    B, T, D, n, hd = _autoint_check(x, params, H, head_dims)
    dev = x.device
    logits = torch.empty(max(B, 1), dtype=torch.float32, device=dev)[:B]
    acts = torch.empty((n, max(B, 1), T, D), dtype=torch.float32, device=dev)[:, :B] if want_acts else None
    saved = torch.empty(_lib.load().lr_autoint_fwd_saved_bytes(B, T, D, int(H), n, hd), dtype=torch.uint8,
                        device=dev) if want_acts else None
    if B == 0:
        return logits, acts, saved
    _call("lr_autoint_fwd_f32", _ptr(x), B, T, D, int(H), n, hd, int(bool(residual)), _ptr(params), _ptr(acts),
          0 if acts is None else acts.numel() * 4, _ptr(saved), 0 if saved is None else saved.numel(), _ptr(logits), _stream())
    return logits, acts, saved


def autoint_bwd(x: torch.Tensor, params: torch.Tensor, H: int, head_dims, residual: bool, acts: torch.Tensor,
                saved: torch.Tensor, glogits: torch.Tensor, gparams: Optional[torch.Tensor] = None):
    """`lr_autoint_bwd_f32`: from glogits [B] -> (gx [B, T, D], gparams in the layout of `params`); `gparams` may be given (e.g.
    a slice of `DenseParams.grad`) and is overwritten.  Parameter gradients are summed in a fixed order."""
    B, T, D, n, hd = _autoint_check(x, params, H, head_dims)
    dev = x.device
    if _req(acts, torch.float32, "acts", 4).shape != (n, B, T, D):
        raise ValueError("acts must be the forward's [n_layers, B, T, D]")
    if _req(glogits, torch.float32, "glogits", 1).shape != (B,):
        raise ValueError("glogits must be [B]")
    if _req(saved, torch.uint8, "saved", 1).numel() != _lib.load().lr_autoint_fwd_saved_bytes(B, T, D, int(H), n, hd):
        raise ValueError("saved must be the forward's (see `autoint_fwd`)")
    if gparams is None:
        gparams = torch.empty_like(params)
    elif _req(gparams, torch.float32, "gparams", 1).numel() != params.numel():
        raise ValueError("gparams must have the length of params")
    gx = torch.empty((max(B, 1), T, D), dtype=torch.float32, device=dev)[:B]
    if B == 0:
        gparams.zero_()
        return gx, gparams
    ws = torch.empty(max(_lib.load().lr_autoint_bwd_ws_bytes(B, T, D, int(H), n, hd), 256), dtype=torch.uint8, device=dev)
    _call("lr_autoint_bwd_f32", _ptr(x), B, T, D, int(H), n, hd, int(bool(residual)), _ptr(params), _ptr(acts),
          _ptr(saved), _ptr(glogits), _ptr(gx), _ptr(gparams), _ptr(ws), ws.numel(), _stream())
    return gx, gparams


# --------------------------------------------------------------------------------------
# sequence attention core (csrc/seq_attn.hip)
# --------------------------------------------------------------------------------------
def seq_attn_supported(Tq: int, Tk: int, H: int, hd: int) -> bool:
    """Whether the sequence-attention kernels take `Tq` queries, `Tk` keys and `H` heads of width `hd`."""
    return bool(_lib.load().lr_seq_attn_supported(int(Tq), int(Tk), int(H), int(hd)))


_SEQ_ATTN_PLAN = ("TB", "nch", "CW", "CS", "ST", "G", "vec", "lds_bytes")


def seq_attn_plan(B: int, Tq: int, Tk: int, H: int, hd: int, bwd: bool, aligned: bool = True) -> dict:
    """`lr_seq_attn_plan_params`: the launch plan of a forward (`bwd` false) or backward call of this shape, as the launch
    derives it (a host query): units per workgroup `TB`, `nch` chunks of `CW` columns per head, the LDS strides `CS` and
    `ST`, `G` lanes per softmax row, `vec` (16-byte row moves; 0 with `aligned=False`: some pointer off a 16-byte boundary)
    and `lds_bytes`."""
    import ctypes as C

    out = (C.c_int32 * 8)()
    check(_lib.load().lr_seq_attn_plan_params(int(B), int(Tq), int(Tk), int(H), int(hd), int(bool(bwd)), int(bool(aligned)), out),
          "lr_seq_attn_plan_params")
    return dict(zip(_SEQ_ATTN_PLAN, (int(x) for x in out)))


def _seq_attn_check(q, k, v, num_heads, key_ok, lens):
    """-> (B, Tq, Tk, H, hd) of one sequence-attention call, its operands validated."""
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, torch.Tensor) or t.dim() != 3:
            raise ValueError(f"{name} must be a 3-d torch.Tensor")
    (B, Tq, M), Tk, H = q.shape, k.shape[1], int(num_heads)
    if k.shape != (B, Tk, M) or v.shape != (B, Tk, M):
        raise ValueError("k and v must be [B, Tk, M] with q's B and M")
    if H < 1 or M % H or not seq_attn_supported(Tq, Tk, H, M // H):          # a host query: before any device work
        raise ValueError(f"unsupported sequence-attention shape: Tq={Tq}, Tk={Tk}, H={H}, M={M} (Tq and Tk from 1 to 64, 1 to 8 "
                         "heads of width 1 to 128, M at most 256)")
    for name, t in (("q", q), ("k", k), ("v", v)):
        _req(t, torch.float32, name, 3)
    if key_ok is not None and _req(key_ok, torch.uint8, "key_ok", 2).shape != (B, Tk):
        raise ValueError("key_ok must be [B, Tk]")
    if lens is not None and _req(lens, torch.int32, "lens", 1).shape != (B,):
        raise ValueError("lens must be [B]")
    return B, Tq, Tk, H, M // H


def seq_attn_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, num_heads: int, scale: float,
                 key_ok: Optional[torch.Tensor] = None, lens: Optional[torch.Tensor] = None, causal_or: bool = False,
                 want_saved: bool = True):
    """`lr_seq_attn_fwd_f32`: softmax((q * scale) k^T + mask) v per head over q [B, Tq, M], k, v [B, Tk, M]; `v` may be `k`
    itself.  Masked scores get -1e9 added; the mask is `key_ok` uint8 [B, Tk] or `lens` int32 [B] (j < lens[b]), ORed with
    j <= i under `causal_or`.  Returns (out [B, Tq, M], saved: the opaque bytes `seq_attn_bwd` wants, None without
    `want_saved`)."""
    B, Tq, Tk, H, hd = _seq_attn_check(q, k, v, num_heads, key_ok, lens)
    out = torch.empty((max(B, 1), Tq, H * hd), dtype=torch.float32, device=q.device)[:B]
    saved = None
    if want_saved:
        n = _lib.load().lr_seq_attn_saved_bytes(B, Tq, Tk, H, hd)
        saved = torch.empty(max(n, 1), dtype=torch.uint8, device=q.device)[:n]
    _call("lr_seq_attn_fwd_f32", _ptr(q), _ptr(k), _ptr(v), B, Tq, Tk, H, hd, float(scale), _ptr(key_ok), _ptr(lens),
          int(bool(causal_or)), _ptr(out), _ptr(saved), 0 if saved is None else saved.numel(), _stream())
    return out, saved


def seq_attn_bwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, num_heads: int, scale: float, key_ok, lens, causal_or: bool,
                 saved: torch.Tensor, gout: torch.Tensor):
    """`lr_seq_attn_bwd_f32`: from gout [B, Tq, M] -> (gq [B, Tq, M], gk, gv [B, Tk, M]); with `v is k` the key gradient is
    gk + gv."""
    B, Tq, Tk, H, hd = _seq_attn_check(q, k, v, num_heads, key_ok, lens)
    if _req(gout, torch.float32, "gout", 3).shape != q.shape:
        raise ValueError("gout must have q's shape")
    if _req(saved, torch.uint8, "saved", 1).numel() != _lib.load().lr_seq_attn_saved_bytes(B, Tq, Tk, H, hd):
        raise ValueError("saved must be the forward's (see `seq_attn_fwd`)")
    gq = torch.empty((max(B, 1), Tq, H * hd), dtype=torch.float32, device=q.device)[:B]
    gk = torch.empty((max(B, 1), Tk, H * hd), dtype=torch.float32, device=q.device)[:B]
    gv = torch.empty((max(B, 1), Tk, H * hd), dtype=torch.float32, device=q.device)[:B]
    _call("lr_seq_attn_bwd_f32", _ptr(q), _ptr(k), _ptr(v), B, Tq, Tk, H, hd, float(scale), _ptr(key_ok), _ptr(lens),
          int(bool(causal_or)), _ptr(saved), _ptr(gout), _ptr(gq), _ptr(gk), _ptr(gv), _stream())
    return gq, gk, gv


class _SeqAttn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, num_heads, scale, key_ok, lens, causal_or):
        shared = v is None                       # the keys are the values
        q, k = q.contiguous(), k.contiguous()
        v = k if shared else v.contiguous()
        grad = any(ctx.needs_input_grad[:3])
        out, saved = seq_attn_fwd(q, k, v, num_heads, scale, key_ok, lens, causal_or, want_saved=grad)
        if grad:
            ctx.save_for_backward(q, k, key_ok, lens, saved, *(() if shared else (v,)))
            ctx.cfg = (int(num_heads), float(scale), bool(causal_or), shared)
        return out

    @staticmethod
    def backward(ctx, gout):
        q, k, key_ok, lens, saved, *rest = ctx.saved_tensors
        num_heads, scale, causal_or, shared = ctx.cfg
        v = k if shared else rest[0]
        gq, gk, gv = seq_attn_bwd(q, k, v, num_heads, scale, key_ok, lens, causal_or, saved, gout.contiguous())
        if shared:
            return gq, gk + gv, None, None, None, None, None, None
        return gq, gk, gv, None, None, None, None, None


def seq_attn(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, num_heads: int, scale: float,
             key_ok: Optional[torch.Tensor] = None, lens: Optional[torch.Tensor] = None, causal_or: bool = False) -> torch.Tensor:
    """The scaled-dot-product attention core under autograd: out [B, Tq, M] of `seq_attn_fwd`, gradients to q, k and v from
    `seq_attn_bwd`.  Passing the same tensor as `k` and `v` (the keys are the values) makes the kernel read the rows once; its
    gradient is then gk + gv."""
    return _SeqAttn.apply(q, k, None if v is k else v, num_heads, scale, key_ok, lens, causal_or)


# --------------------------------------------------------------------------------------
# skip-gram word2vec in windows (csrc/word2vec.hip)
# --------------------------------------------------------------------------------------
W2V_NEGATIVES = 5
_U64 = (1 << 64) - 1


def w2v_supported(embed_size: int) -> bool:
    """Whether the word2vec kernels take rows of `embed_size` floats (1 to 256)."""
    return bool(_lib.load().lr_w2v_supported(int(embed_size)))


def w2v_walks(starts: torch.Tensor, succ_ptr: torch.Tensor, succ_idx: torch.Tensor, n_items: int, walk_length: int, seed: int,
              pass_no: int):
    """`lr_w2v_walks_i32`: one random walk per entry of `starts` over the successor CSR -> (walks [n, walk_length] int32 padded
    with -1, lens [n] int32)."""
    _req(starts, torch.int32, "starts", 1)
    _req(succ_ptr, torch.int64, "succ_ptr", 1)
    _req(succ_idx, torch.int32, "succ_idx", 1)
    if succ_ptr.numel() != int(n_items) + 1:
        raise ValueError("succ_ptr must hold n_items + 1 entries")
    if walk_length < 1:
        raise ValueError("`walk_length` must be at least 1")
    n, L = starts.numel(), int(walk_length)
    walks = torch.empty((max(n, 1), L), dtype=torch.int32, device=starts.device)[:n]
    lens = torch.empty(max(n, 1), dtype=torch.int32, device=starts.device)[:n]
    _call("lr_w2v_walks_i32", _ptr(starts), n, L, _ptr(succ_ptr), _ptr(succ_idx), int(n_items), succ_idx.numel(),
          int(seed) & _U64, int(pass_no), _ptr(walks), _ptr(lens), _stream())
    return walks, lens


def w2v_keep(tokens: torch.Tensor, keep_thr: torch.Tensor, seed: int, epoch: int) -> torch.Tensor:
    """`lr_w2v_keep_u8`: the subsampling flag of every raw token (`keep_thr` [n_items] int64: 2^32 * keep probability)."""
    _req(tokens, torch.int32, "tokens", 1)
    _req(keep_thr, torch.int64, "keep_thr", 1)
    n = tokens.numel()
    keep = torch.empty(max(n, 1), dtype=torch.uint8, device=tokens.device)[:n]
    _call("lr_w2v_keep_u8", _ptr(tokens), n, _ptr(keep_thr), keep_thr.numel(), int(seed) & _U64, int(epoch), _ptr(keep),
          _stream())
    return keep


def w2v_pairs(ctok: torch.Tensor, craw: torch.Tensor, csent: torch.Tensor, cptr: torch.Tensor, window: int, seed: int,
              epoch: int):
    """`lr_w2v_pairs_count_i32` / `lr_w2v_pairs_emit_i32` over the compacted corpus -> (in_ids, pred, centre), int32 [n_pairs]
    in ascending (centre, context) order.  The scan between the two passes is a torch op; the pair count is read back once."""
    for t_, n_ in ((ctok, "ctok"), (craw, "craw"), (csent, "csent")):
        _req(t_, torch.int32, n_, 1)
    _req(cptr, torch.int64, "cptr", 1)
    nc, n_sent = ctok.numel(), cptr.numel() - 1
    if craw.numel() != nc or csent.numel() != nc or n_sent < 0:
        raise ValueError("shape mismatch")
    if window < 1:
        raise ValueError("`window_size` must be at least 1")
    dev = ctok.device
    counts = torch.empty(max(nc, 1), dtype=torch.int32, device=dev)[:nc]
    args = (_ptr(craw), _ptr(csent), _ptr(cptr), nc, n_sent, int(window), int(seed) & _U64, int(epoch))
    _call("lr_w2v_pairs_count_i32", *args, _ptr(counts), _stream())
    incl = torch.cumsum(counts, 0, dtype=torch.int64)
    n_pairs = int(incl[-1].item()) if nc else 0
    if n_pairs >= 1 << 31:
        raise ValueError("an epoch of 2^31 pairs or more is not supported")
    offs = (incl - counts).contiguous()
    out = [torch.empty(max(n_pairs, 1), dtype=torch.int32, device=dev)[:n_pairs] for _ in range(3)]
    _call("lr_w2v_pairs_emit_i32", _ptr(ctok), *args, _ptr(offs), n_pairs, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _stream())
    return tuple(out)


def w2v_targets(in_ids: torch.Tensor, pred: torch.Tensor, cum: torch.Tensor, seed: int, epoch: int, pair_base: int = 0,
                hs=None) -> dict:
    """`lr_w2v_targets_i32` (count, a torch scan, fill) for the given pairs -> {"offs" int64 [W + 1], "rows", "labels",
    "slot_in" int32 [n_slots]}.  `hs` is None (negatives only: the offsets are 6 p, nothing is read back) or the Huffman CSR
    (hs_ptr [n_items + 1], hs_nodes, hs_codes), int32; then the slot count is read back."""
    _req(in_ids, torch.int32, "in_ids", 1)
    _req(pred, torch.int32, "pred", 1)
    _req(cum, torch.int64, "cum", 1)
    W, n_items, dev = pred.numel(), cum.numel(), pred.device
    if in_ids.numel() != W:
        raise ValueError("shape mismatch")
    hp = hn = hc = None
    if hs is not None:
        hp, hn, hc = (_req(t_, torch.int32, n_, 1) for t_, n_ in zip(hs, ("hs_ptr", "hs_nodes", "hs_codes")))
        if hp.numel() != n_items + 1 or hn.numel() != hc.numel():
            raise ValueError("the Huffman CSR must hold n_items + 1 offsets and one code per node")
    head = (_ptr(in_ids), _ptr(pred), W, int(pair_base), n_items, _ptr(cum), _ptr(hp), _ptr(hn), _ptr(hc),
            0 if hn is None else hn.numel(), int(seed) & _U64, int(epoch))
    offs = torch.zeros(W + 1, dtype=torch.int64, device=dev)
    if hs is None:
        torch.arange(0, (W + 1) * (W2V_NEGATIVES + 1), W2V_NEGATIVES + 1, out=offs)
        n_slots = W * (W2V_NEGATIVES + 1)
    else:
        lens = torch.empty(max(W, 1), dtype=torch.int32, device=dev)[:W]
        _call("lr_w2v_targets_i32", *head, None, _ptr(lens), 0, None, None, None, _stream())
        torch.cumsum(lens, 0, dtype=torch.int64, out=offs[1:])
        n_slots = int(offs[-1].item())
    if n_slots >= 1 << 31:
        raise ValueError("2^31 target slots or more in one call are not supported")
    rows, labels, slot_in = (torch.empty(max(n_slots, 1), dtype=torch.int32, device=dev)[:n_slots] for _ in range(3))
    _call("lr_w2v_targets_i32", *head, _ptr(offs), None, n_slots, _ptr(rows), _ptr(labels), _ptr(slot_in), _stream())
    return {"offs": offs, "rows": rows, "labels": labels, "slot_in": slot_in}


def w2v_score(syn0: torch.Tensor, syn1: torch.Tensor, in_ids: torch.Tensor, centre: torch.Tensor, offs: torch.Tensor,
              rows: torch.Tensor, labels: torch.Tensor, pos0: float, inv_total: float, g: Optional[torch.Tensor] = None,
              stash: Optional[torch.Tensor] = None, want_loss: bool = True):
    """`lr_w2v_score_f32` over the W pairs of a window (`offs` [W + 1] indexes `rows` / `labels` / `g`, which may cover more
    than the window) -> (g [n_slots], stash [W, D], loss [W] or None).  `g` and `stash` may be preallocated."""
    _req(syn0, torch.float32, "syn0", 2)
    _req(syn1, torch.float32, "syn1", 2)
    _req(in_ids, torch.int32, "in_ids", 1)
    _req(centre, torch.int32, "centre", 1)
    _req(offs, torch.int64, "offs", 1)
    _req(rows, torch.int32, "rows", 1)
    _req(labels, torch.int32, "labels", 1)
    D, W, n_slots, dev = syn0.shape[1], in_ids.numel(), rows.numel(), syn0.device
    if not w2v_supported(D):
        raise ValueError(f"the word2vec kernels take rows of 1 to 256 floats, got {D}")
    if syn1.shape[1] != D or centre.numel() != W or offs.numel() != W + 1 or labels.numel() != n_slots:
        raise ValueError("shape mismatch")
    if g is None:
        g = torch.empty(max(n_slots, 1), dtype=torch.float32, device=dev)[:n_slots]
    elif _req(g, torch.float32, "g", 1).numel() < n_slots:
        raise ValueError("g is too small")
    if stash is None:
        stash = torch.empty((max(W, 1), D), dtype=torch.float32, device=dev)[:W]
    elif _req(stash, torch.float32, "stash", 2).shape[1] != D or stash.shape[0] < W:
        raise ValueError("stash is too small")
    loss = torch.empty(max(W, 1), dtype=torch.float32, device=dev)[:W] if want_loss else None
    _call("lr_w2v_score_f32", _ptr(syn0), syn0.shape[0], _ptr(syn1), syn1.shape[0], D, _ptr(in_ids), _ptr(centre), W, _ptr(offs),
          _ptr(rows), _ptr(labels), n_slots, float(pos0), float(inv_total), _ptr(g), _ptr(stash), _ptr(loss), _stream())
    return g, stash, loss


def w2v_out_update(table: torch.Tensor, seg: Segments, other: torch.Tensor, g: Optional[torch.Tensor] = None,
                   slot_in: Optional[torch.Tensor] = None) -> None:
    """`lr_w2v_out_update_f32`: the ordered update of one window's touched rows of `table` [V, D].  Output rows: `seg` over
    the window's flat target rows, `g` / `slot_in` the window's slices and `other` = syn0.  Input rows: `seg` over the window's
    input ids, `g` / `slot_in` None and `other` = the stash (at least `seg.n` rows)."""
    _req(table, torch.float32, "table", 2)
    _req(other, torch.float32, "other", 2)
    V, D = table.shape
    if not w2v_supported(D):
        raise ValueError(f"the word2vec kernels take rows of 1 to 256 floats, got {D}")
    if (g is None) != (slot_in is None):
        raise ValueError("`g` and `slot_in` go together")
    if g is not None:
        _req(g, torch.float32, "g", 1)
        _req(slot_in, torch.int32, "slot_in", 1)
        if g.numel() < seg.n or slot_in.numel() < seg.n:
            raise ValueError("g and slot_in must cover the segmented positions")
    elif other.shape[0] < seg.n:
        raise ValueError("the stash must hold one row per segmented position")
    if V != seg.V or other.shape[1] != D:
        raise ValueError("shape mismatch")
    _call("lr_w2v_out_update_f32", _ptr(table), V, D, _ptr(seg.pos), _ptr(seg.rows), _ptr(seg.start), _ptr(seg.n_seg), seg.n,
          _ptr(g), _ptr(slot_in), _ptr(other), other.shape[0], _stream())


# --------------------------------------------------------------------------------------
# GraphSage: neighbour sampling and the fused tower (csrc/sage.hip)
# --------------------------------------------------------------------------------------
SAGE_NEG_MODES = {"random": 0, "popular": 1, "out-batch": 2}


@dataclass
class SageGraph:
    """The two CSRs of the bipartite graph on the device (int64 pointers, int32 indices, duplicates kept)."""

    item_ptr: torch.Tensor     # [n_items + 1]: the consumers of an item
    item_idx: torch.Tensor
    user_ptr: torch.Tensor     # [n_users + 1]: the items of a user
    user_idx: torch.Tensor

    def __post_init__(self):
        _req(self.item_ptr, torch.int64, "item_ptr", 1)
        _req(self.item_idx, torch.int32, "item_idx", 1)
        _req(self.user_ptr, torch.int64, "user_ptr", 1)
        _req(self.user_idx, torch.int32, "user_idx", 1)
        if self.item_ptr.numel() < 2 or self.user_ptr.numel() < 2:
            raise ValueError("the graph needs at least one item and one user")

    def args(self):
        return (_ptr(self.item_ptr), _ptr(self.item_idx), self.item_ptr.numel() - 1, self.item_idx.numel(), _ptr(self.user_ptr),
                _ptr(self.user_idx), self.user_ptr.numel() - 1, self.user_idx.numel())


def sage_supported(K: int, T: int, num_layers: int, num_neighbors: int) -> bool:
    """`lr_sage_supported`: whether the fused tower takes this shape."""
    return bool(_lib.load().lr_sage_supported(int(K), int(T), int(num_layers), int(num_neighbors)))


def sage_param_floats(K: int, T: int, num_layers: int) -> int:
    """Length of the parameter pack: proj W^T [T K, K], proj b [K], then per layer W^T [2 K, K], b [K] (0: unsupported)."""
    return _lib.load().lr_sage_params_bytes(int(K), int(T), int(num_layers)) // 4


def sage_bwd_slabs(B: int, K: int, T: int, num_layers: int, num_neighbors: int) -> int:
    return int(_lib.load().lr_sage_bwd_slabs(int(B), int(K), int(T), int(num_layers), int(num_neighbors)))


def sage_neighbors(nodes: torch.Tensor, graph: SageGraph, num_neighbors: int, seed: int, step: int, level: int) -> torch.Tensor:
    """`lr_sage_neighbors_i32`: int32 [n_nodes, num_neighbors], the sampled neighbours of one level of nodes."""
    _req(nodes, torch.int32, "nodes", 1)
    if not 1 <= int(num_neighbors) <= 10:
        raise ValueError("`num_neighbors` must be from 1 to 10")
    n = nodes.numel()
    out = torch.empty((max(n, 1), int(num_neighbors)), dtype=torch.int32, device=nodes.device)[:n]
    _call("lr_sage_neighbors_i32", _ptr(nodes), n, int(num_neighbors), *graph.args(), int(seed) & _U64, int(step), int(level),
          _ptr(out), _stream())
    return out


def sage_pairs(starts: torch.Tensor, graph: SageGraph, num_walks: int, walk_len: int, focus_start: bool, seed: int, step: int):
    """`lr_sage_pairs_i32` (count, a torch scan, emit) -> (items, items_pos) int32 [n_pairs] in ascending (start, walk, step).
    The pair count is read back once."""
    _req(starts, torch.int32, "starts", 1)
    if num_walks < 1 or walk_len < 1:
        raise ValueError("`num_walks` and `sample_walk_len` must be at least 1")
    n, dev = starts.numel(), starts.device
    head = (_ptr(starts), n, int(num_walks), int(walk_len), 1 if focus_start else 0, *graph.args(), int(seed) & _U64, int(step))
    counts = torch.empty(max(n * num_walks, 1), dtype=torch.int32, device=dev)[:n * num_walks]
    _call("lr_sage_pairs_i32", *head, _ptr(counts), None, 0, None, None, _stream())
    incl = torch.cumsum(counts, 0, dtype=torch.int64)
    n_pairs = int(incl[-1].item()) if n else 0
    offs = (incl - counts).contiguous()
    items, items_pos = (torch.empty(max(n_pairs, 1), dtype=torch.int32, device=dev)[:n_pairs] for _ in range(2))
    _call("lr_sage_pairs_i32", *head, None, _ptr(offs), n_pairs, _ptr(items), _ptr(items_pos), _stream())
    return items, items_pos


def sage_starts(n: int, n_items: int, seed: int, step: int, device, cum: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`lr_sage_starts_i32`: n start nodes, uniform or (with `cum` int64 [n_items]) from the cumulative table."""
    if cum is not None and _req(cum, torch.int64, "cum", 1).numel() != int(n_items):
        raise ValueError("cum must hold n_items entries")
    out = torch.empty(max(int(n), 1), dtype=torch.int32, device=device)[:int(n)]
    _call("lr_sage_starts_i32", int(n), int(n_items), _ptr(cum), int(seed) & _U64, int(step), _ptr(out), _stream())
    return out


def sage_negatives(items: Optional[torch.Tensor], items_pos: torch.Tensor, num_neg: int, n_items: int, mode: str, seed: int,
                   step: int, cum: Optional[torch.Tensor] = None, in_batch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`lr_sage_negatives_i32`: int32 [n * num_neg]; `mode` is "random", "popular" (needs `cum`) or "out-batch" (needs
    `in_batch` uint8 [n_items])."""
    _req(items_pos, torch.int32, "items_pos", 1)
    n = items_pos.numel()
    if items is not None and _req(items, torch.int32, "items", 1).numel() != n:
        raise ValueError("items and items_pos must have the same length")
    if mode not in SAGE_NEG_MODES:
        raise ValueError(f"unknown negative mode: {mode}")
    if mode == "popular" and (cum is None or _req(cum, torch.int64, "cum", 1).numel() != int(n_items)):
        raise ValueError("`popular` needs cum int64 [n_items]")
    if mode == "out-batch" and (in_batch is None or _req(in_batch, torch.uint8, "in_batch", 1).numel() != int(n_items)):
        raise ValueError("`out-batch` needs in_batch uint8 [n_items]")
    if num_neg < 1:
        raise ValueError("`num_neg` must be at least 1")
    out = torch.empty(max(n * int(num_neg), 1), dtype=torch.int32, device=items_pos.device)[:n * int(num_neg)]
    _call("lr_sage_negatives_i32", _ptr(items), _ptr(items_pos), n, int(num_neg), int(n_items), SAGE_NEG_MODES[mode], _ptr(cum),
          _ptr(in_batch), int(seed) & _U64, int(step), _ptr(out), _stream())
    return out


def sage_dropout_mask(n_nodes: int, K: int, p: float, seed: int, step: int, layer: int, level: int, role: int, device):
    """`lr_sage_dropout_u8`: the keep flags uint8 [n_nodes, K] of one (layer, level, role)."""
    if not 0.0 <= float(p) < 1.0:
        raise ValueError("`dropout_rate` must be in [0, 1)")
    keep = torch.empty((max(int(n_nodes), 1), int(K)), dtype=torch.uint8, device=device)[:int(n_nodes)]
    _call("lr_sage_dropout_u8", int(n_nodes), int(K), float(p), int(seed) & _U64, int(step), int(layer), int(level), int(role),
          _ptr(keep), _stream())
    return keep


def sage_tree_nodes(num_layers: int, num_neighbors: int) -> int:
    return sum(int(num_neighbors) ** k for k in range(int(num_layers) + 1)) if num_layers > 0 else 1


def _sage_check(table, rows, scale, params, num_layers, num_neighbors, dropout):
    _req(table, torch.float32, "table", 2)
    _req(rows, torch.int32, "rows", 2)
    _req(params, torch.float32, "params", 1)
    V, K = table.shape
    T = rows.shape[1]
    N = sage_tree_nodes(num_layers, num_neighbors)
    if not sage_supported(K, T, num_layers, num_neighbors):
        raise ValueError(f"unsupported GraphSage shape: K={K} T={T} num_layers={num_layers} num_neighbors={num_neighbors} "
                         "(see `sage_supported`)")
    if rows.shape[0] % N:
        raise ValueError(f"rows must hold a whole number of trees of {N} nodes")
    if scale is not None and _req(scale, torch.float32, "scale", 2).shape != rows.shape:
        raise ValueError("scale must have the shape of rows")
    if params.numel() != sage_param_floats(K, T, num_layers):
        raise ValueError("params must be the parameter pack of this shape (see `sage_param_floats`)")
    if not 0.0 <= float(dropout) < 1.0:
        raise ValueError("`dropout_rate` must be in [0, 1)")
    return rows.shape[0] // N, K, T, V


def sage_fwd(table: torch.Tensor, rows: torch.Tensor, scale: Optional[torch.Tensor], params: torch.Tensor, num_layers: int,
             num_neighbors: int, dropout: float = 0.0, seed: int = 0, step: int = 0, train: bool = False) -> torch.Tensor:
    """`lr_sage_fwd_f32`: repr [B, K] of B trees whose slots `rows` / `scale` [B N, T] are laid out level-major (see the
    header).  `train=False` is the inference mode: no dropout is drawn."""
    B, K, T, V = _sage_check(table, rows, scale, params, num_layers, num_neighbors, dropout)
    repr_ = torch.empty((max(B, 1), K), dtype=torch.float32, device=table.device)[:B]
    _call("lr_sage_fwd_f32", _ptr(table), V, _ptr(rows), _ptr(scale), B, K, T, int(num_layers), int(num_neighbors), _ptr(params),
          float(dropout), int(seed) & _U64, int(step), 1 if train else 0, _ptr(repr_), _stream())
    return repr_


def sage_bwd(table: torch.Tensor, rows: torch.Tensor, scale: Optional[torch.Tensor], params: torch.Tensor, num_layers: int,
             num_neighbors: int, grepr: torch.Tensor, dropout: float = 0.0, seed: int = 0, step: int = 0,
             want_relu: bool = False):
    """`lr_sage_bwd_f32` -> (grow [B N, T, K], gparams in the layout of `params`, relu flags uint8 or None)."""
    B, K, T, V = _sage_check(table, rows, scale, params, num_layers, num_neighbors, dropout)
    _req(grepr, torch.float32, "grepr", 2)
    if grepr.shape != (B, K):
        raise ValueError("grepr must be [B, K]")
    dev = table.device
    n, L = int(num_neighbors), int(num_layers)
    grow = torch.empty((max(rows.shape[0], 1), T, K), dtype=torch.float32, device=dev)[:rows.shape[0]]
    gparams = torch.empty(params.numel(), dtype=torch.float32, device=dev)
    relu = None
    if want_relu:
        n_relu = sum(sage_tree_nodes(L - l - 1, n) for l in range(L - 1))
        relu = torch.empty((max(B * n_relu, 1), K), dtype=torch.uint8, device=dev)[:B * n_relu]
    ws = torch.empty(max(_lib.load().lr_sage_bwd_ws_bytes(B, K, T, L, n), 256), dtype=torch.uint8, device=dev)
    _call("lr_sage_bwd_f32", _ptr(table), V, _ptr(rows), _ptr(scale), B, K, T, L, n, _ptr(params), float(dropout),
          int(seed) & _U64, int(step), _ptr(grepr), _ptr(grow), _ptr(gparams), _ptr(relu), _ptr(ws), ws.numel(), _stream())
    return grow, gparams, relu


# --------------------------------------------------------------------------------------
# PinSage: importance-walk sampling and the fused tower (csrc/pinsage.hip)
# --------------------------------------------------------------------------------------
def pinsage_supported(K: int, T: int, num_layers: int, num_neighbors: int) -> bool:
    """`lr_pinsage_supported`: whether the fused tower takes this shape."""
    return bool(_lib.load().lr_pinsage_supported(int(K), int(T), int(num_layers), int(num_neighbors)))


def pinsage_param_floats(K: int, T: int, num_layers: int) -> int:
    """Length of the parameter pack: proj W^T [T K, K], proj b [K]; per layer Q^T [K, K], bq [K], W^T [2 K, K], bw [K]; the
    head G1^T [K, K], b1 [K], G2^T [K, K] (0: unsupported)."""
    return _lib.load().lr_pinsage_params_bytes(int(K), int(T), int(num_layers)) // 4


def pinsage_bwd_slabs(B: int, K: int, T: int, num_layers: int, num_neighbors: int) -> int:
    return int(_lib.load().lr_pinsage_bwd_slabs(int(B), int(K), int(T), int(num_layers), int(num_neighbors)))


def pinsage_neighbors(nodes: torch.Tensor, graph: SageGraph, num_neighbors: int, num_walks: int, walk_len: int,
                      termination_prob: float, seed: int, step: int, level: int, tree_target: Optional[torch.Tensor] = None,
                      tree_exclude: Optional[torch.Tensor] = None):
    """`lr_pinsage_neighbors_i32` -> (ids, counts) int32 [n_nodes, num_neighbors]: the most visited items of the node's walks in
    selection order, unused slots -1 / 0.  `tree_target` / `tree_exclude` int32 [n_trees] carry the i2i exclusion."""
    _req(nodes, torch.int32, "nodes", 1)
    nn, nw, wl = int(num_neighbors), int(num_walks), int(walk_len)
    if not 1 <= nn <= 10:
        raise ValueError("`num_neighbors` must be from 1 to 10")
    if nw < 1 or wl < 1 or nw * wl > 64:
        raise ValueError("`num_walks` and `neighbor_walk_len` must be at least 1 and their product at most 64")
    if not float(termination_prob) == float(termination_prob):
        raise ValueError("`termination_prob` must be a number")
    n, n_trees = nodes.numel(), 0
    if tree_exclude is not None:
        _req(tree_exclude, torch.int32, "tree_exclude", 1)
        if tree_target is None or _req(tree_target, torch.int32, "tree_target", 1).numel() != tree_exclude.numel():
            raise ValueError("tree_target and tree_exclude must have the same length")
        n_trees = tree_exclude.numel()
        if n != n_trees * nn ** int(level):
            raise ValueError("nodes must hold one level of every tree")
    else:
        tree_target = None
    ids, counts = (torch.empty((max(n, 1), nn), dtype=torch.int32, device=nodes.device)[:n] for _ in range(2))
    _call("lr_pinsage_neighbors_i32", _ptr(nodes), n, nn, nw, wl, float(termination_prob), _ptr(tree_target), _ptr(tree_exclude),
          n_trees, *graph.args(), int(seed) & _U64, int(step), int(level), _ptr(ids), _ptr(counts), _stream())
    return ids, counts


def pinsage_weights(counts: torch.Tensor) -> torch.Tensor:
    """The importance weights f32 of visit counts [n_nodes, num_neighbors]: count / row total, exactly 0 in an unused slot."""
    c = counts.to(torch.float32)
    return (c / c.sum(dim=1, keepdim=True).clamp(min=1.0)).contiguous()


def _pinsage_check(table, rows, scale, weights, params, num_layers, num_neighbors, dropout):
    _req(table, torch.float32, "table", 2)
    _req(rows, torch.int32, "rows", 2)
    _req(params, torch.float32, "params", 1)
    V, K = table.shape
    T = rows.shape[1]
    N = sage_tree_nodes(num_layers, num_neighbors)
    if not pinsage_supported(K, T, num_layers, num_neighbors):
        raise ValueError(f"unsupported PinSage shape: K={K} T={T} num_layers={num_layers} num_neighbors={num_neighbors} "
                         "(see `pinsage_supported`)")
    if rows.shape[0] % N:
        raise ValueError(f"rows must hold a whole number of trees of {N} nodes")
    B = rows.shape[0] // N
    if scale is not None and _req(scale, torch.float32, "scale", 2).shape != rows.shape:
        raise ValueError("scale must have the shape of rows")
    if N > 1 and (weights is None or _req(weights, torch.float32, "weights", 1).numel() != B * (N - 1)):
        raise ValueError("weights must hold one value per node of the levels 1 .. num_layers")
    if params.numel() != pinsage_param_floats(K, T, num_layers):
        raise ValueError("params must be the parameter pack of this shape (see `pinsage_param_floats`)")
    if not 0.0 <= float(dropout) < 1.0:
        raise ValueError("`dropout_rate` must be in [0, 1)")
    return B, K, T, V


def pinsage_fwd(table: torch.Tensor, rows: torch.Tensor, scale: Optional[torch.Tensor], weights: Optional[torch.Tensor],
                params: torch.Tensor, num_layers: int, num_neighbors: int, dropout: float = 0.0, seed: int = 0, step: int = 0,
                train: bool = False) -> torch.Tensor:
    """`lr_pinsage_fwd_f32`: repr [B, K] of B trees laid out as for `sage_fwd`, `weights` f32 [B (N - 1)] aligned with the nodes
    of the levels 1 .. num_layers.  `train=False` is the inference mode: no dropout is drawn."""
    B, K, T, V = _pinsage_check(table, rows, scale, weights, params, num_layers, num_neighbors, dropout)
    repr_ = torch.empty((max(B, 1), K), dtype=torch.float32, device=table.device)[:B]
    _call("lr_pinsage_fwd_f32", _ptr(table), V, _ptr(rows), _ptr(scale), _ptr(weights), B, K, T, int(num_layers),
          int(num_neighbors), _ptr(params), float(dropout), int(seed) & _U64, int(step), 1 if train else 0, _ptr(repr_), _stream())
    return repr_


def pinsage_relu_rows(num_layers: int, num_neighbors: int) -> int:
    """Rows of `relu_out` per tree: per layer the q flags and the w flags, then the head's row."""
    L, n = int(num_layers), int(num_neighbors)
    return sum(sage_tree_nodes(L - l, n) - 1 + sage_tree_nodes(L - l - 1, n) for l in range(L)) + 1


def pinsage_bwd(table: torch.Tensor, rows: torch.Tensor, scale: Optional[torch.Tensor], weights: Optional[torch.Tensor],
                params: torch.Tensor, num_layers: int, num_neighbors: int, grepr: torch.Tensor, dropout: float = 0.0,
                seed: int = 0, step: int = 0, want_relu: bool = False):
    """`lr_pinsage_bwd_f32` -> (grow [B N, T, K], gparams in the layout of `params`, relu flags uint8 or None)."""
    B, K, T, V = _pinsage_check(table, rows, scale, weights, params, num_layers, num_neighbors, dropout)
    _req(grepr, torch.float32, "grepr", 2)
    if grepr.shape != (B, K):
        raise ValueError("grepr must be [B, K]")
    dev = table.device
    n, L = int(num_neighbors), int(num_layers)
    grow = torch.empty((max(rows.shape[0], 1), T, K), dtype=torch.float32, device=dev)[:rows.shape[0]]
    gparams = torch.empty(params.numel(), dtype=torch.float32, device=dev)
    relu = None
    if want_relu:
        n_relu = B * pinsage_relu_rows(L, n)
        relu = torch.empty((max(n_relu, 1), K), dtype=torch.uint8, device=dev)[:n_relu]
    ws = torch.empty(max(_lib.load().lr_pinsage_bwd_ws_bytes(B, K, T, L, n), 256), dtype=torch.uint8, device=dev)
    _call("lr_pinsage_bwd_f32", _ptr(table), V, _ptr(rows), _ptr(scale), _ptr(weights), B, K, T, L, n, _ptr(params),
          float(dropout), int(seed) & _U64, int(step), _ptr(grepr), _ptr(grow), _ptr(gparams), _ptr(relu), _ptr(ws), ws.numel(),
          _stream())
    return grow, gparams, relu
