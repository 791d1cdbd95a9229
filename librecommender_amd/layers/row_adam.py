"""What every model with `[V, K]` row tables and TF1 Adam moments shares: the segment builders of its id spaces, the update
of a table from one (index, gradient) stream, and the named tables with their checkpoint arrays (BPR, SVD / SVD++, the
retrieval and tower nets, the feature embedding layer, the owner side of the row-sharded tables).

Three rules live here instead of at every call site:
  * a `Segments` is a view of its builder's buffers: it dies with the next build in the same id space, so streams that must
    be alive together within a step (SVD++: users, items, history entries) are built in different spaces;
  * the `row_slot` scratch of the dense update is all -1 on entry and the kernel restores it before it returns, so tables
    of the same height share one;
  * a table with a `[V, 1]` twin on the same stream is ONE `embed_scatter_adam_lin` launch, without the long-run workspace
    that `embed_scatter_adam` takes: a caller that wants two `embed_scatter_adam` launches makes two `update` calls.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops

REG_NEEDS_DENSE = ("`reg` regularises every embedding row each step (tf.keras.regularizers.l2 on the variables): "
                   "use `dense_adam=True` with it; the row-wise Adam on touched rows cannot represent that term")


def row_slot_of(cache: dict, table):
    """The int32 [V] scratch of `ops.adam_dense` for tables of this height on this device, kept in `cache`: all -1 between calls."""
    key = (table.shape[0], table.device)
    if key not in cache:
        cache[key] = torch.full(key[:1], -1, dtype=torch.int32, device=table.device)
    return cache[key]


class SegmentSpaces:
    """One `ops.SegmentBuilder` per id space, grown when a stream outgrows it."""

    def __init__(self, device):
        self.device, self._builders = device, {}

    def segments(self, space, ids, V, want_slots=False):
        """The `Segments` of `ids` (int32, -1 = no row) over `V` rows.  It is a view of the space's builder (its `owner`,
        which keeps `seg.long_ws(K)` and `owner.hist_ws(K)` persistent): the next build in `space` overwrites it."""
        b = self._builders.get(space)
        if b is None or b.n_max < ids.numel():
            b = self._builders[space] = ops.SegmentBuilder(max(ids.numel(), 1), V, self.device)
        return b.build(ids.reshape(-1), want_slots=want_slots)


class RowAdam(SegmentSpaces):
    """TF1 Adam on row tables: `dense=False` moves the rows a stream touches, `dense=True` is the reference's semantics
    (every row decays and moves every step), the only form that can carry the l2 term `l2` of a regulariser."""

    def __init__(self, device, dense: bool, l2: float):
        super().__init__(device)
        self.dense, self.l2, self._row_slots = bool(dense), float(l2 or 0.0), {}
        if self.l2 and not self.dense:
            raise ValueError(REG_NEEDS_DENSE)

    def row_slot(self, table):
        """The `row_slot` scratch that `update` hands to `ops.adam_dense` for `table`."""
        return row_slot_of(self._row_slots, table)

    def update(self, hp, seg, table, m, v, grad, lin=None):
        """One Adam step of `table` from the per-position gradients `grad` [seg.n, K]; `lin` = (lin, lin_m, lin_v, glin): the
        table's `[V, 1]` twin and its per-position gradient [seg.n], updated from the same segments."""
        if not self.dense:
            if lin is None:
                ops.embed_scatter_adam(table, m, v, grad, seg, hp)
            else:
                ops.embed_scatter_adam_lin(table, m, v, grad, *lin, seg, hp)
            return
        ops.adam_dense(table, m, v, hp, grows=ops.embed_segment_sum(grad, seg), seg=seg, row_slot=self.row_slot(table), l2=self.l2)
        if lin is not None:
            self.update(hp, seg, *lin[:3], lin[3].view(-1, 1))

    def update_all_rows(self, hp, table, m, v):
        """The dense step of a table that no row of the batch touches (zero gradient: decay and the l2 term alone)."""
        ops.adam_dense(table, m, v, hp, l2=self.l2)


class NamedTables:
    """`vars`, `m`, `v`: {name: tensor [rows, width]} of variables and their Adam moments, and the step count."""

    def __init__(self, vars, m=None, v=None):
        self.vars, self.step = vars, 0
        self.m = {k: torch.zeros_like(t) for k, t in vars.items()} if m is None else m
        self.v = {k: torch.zeros_like(t) for k, t in vars.items()} if v is None else v

    def optimizer_arrays(self):
        out = {"opt::step": np.asarray(self.step, dtype=np.int64)}
        for k in self.m:
            out[f"opt::m_{k}"], out[f"opt::v_{k}"] = self.m[k].cpu().numpy(), self.v[k].cpu().numpy()
        return out

    @torch.no_grad()
    def take_over(self, arrays, saved_name_of, n_old_of, full_assign):
        """Retraining on merged data: the first `n_old_of(k)` rows of every variable come from `arrays[saved_name_of(k)]`
        (ids keep their place, new ones are appended) and, with `full_assign`, so do their moments and the step count; later
        rows keep their fresh draws and zero moments.  A name that `arrays` lacks is skipped."""
        def put(dst, key, n):
            if key in arrays:
                dst[:n] = torch.from_numpy(arrays[key][:n]).to(dst.device).view(n, -1)

        for k, var in self.vars.items():
            put(var, saved_name_of(k), n_old_of(k))
            if full_assign and k in self.m:
                put(self.m[k], f"opt::m_{k}", n_old_of(k))
                put(self.v[k], f"opt::v_{k}", n_old_of(k))
        if full_assign and "opt::step" in arrays:
            self.step = int(arrays["opt::step"])
