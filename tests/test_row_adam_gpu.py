"""`layers.RowAdam` against the op sequences its call sites issued before it existed, written out here on cloned tensors:
bit for bit, in the row-wise and the dense (TF1) form, with and without a `[V, 1]` twin on the same stream; the builders of
its id spaces (growth, two spaces alive in one step, the persistent long-run workspace) and its `row_slot` scratch."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import librecommender_amd
from librecommender_amd import ops
from librecommender_amd.layers import RowAdam

pytestmark = pytest.mark.gpu

V, K = 7, 3
IDS9 = (3, 0, 3, -1, 6, 0, 3, 5, 0)             # duplicates, one dropped position; rows 1, 2, 4 untouched
LONG_RUN = int(re.search(r"constexpr int kLongRun = (\d+);",
                         (Path(librecommender_amd.__file__).parent / "csrc" / "embed_scatter.hip").read_text()).group(1))
FORMS = {"rows": (False, 0.0, False), "rows_lin": (False, 0.0, True), "dense_l2": (True, 0.01, False),
         "dense_lin": (True, 0.0, True), "dense_lin_l2": (True, 0.01, True)}         # (dense, l2, with the [V, 1] twin)


def hp(step):
    return ops.adam_hp(1e-2, step, eps=1e-5, tf_style=True)


def make_state(rng, dev, n_rows=V, width=K):
    """[table, m, v, lin, lin_m, lin_v] in mid-training (non-zero moments)."""
    out = []
    for w in (width, 1):
        out += [rng.standard_normal((n_rows, w)), rng.standard_normal((n_rows, w)) * 0.01, rng.random((n_rows, w)) * 0.01]
    return [torch.from_numpy(x.astype(np.float32)).to(dev) for x in out]


def make_stream(rng, dev, ids, width=K):
    ids = np.asarray(ids, dtype=np.int32)
    return (torch.from_numpy(ids).to(dev), torch.from_numpy(rng.standard_normal((len(ids), width)).astype(np.float32)).to(dev),
            torch.from_numpy(rng.standard_normal(len(ids)).astype(np.float32)).to(dev))


def parent_update(dense, l2, with_lin, h, seg, st, grad, glin, row_slot):
    """What `BprNet`, `SvdNet`, the retrieval and tower nets and `FeatEmbedding` did with one stream."""
    t, m, v, lin, lin_m, lin_v = st
    if not dense:
        if with_lin:
            ops.embed_scatter_adam_lin(t, m, v, grad, lin, lin_m, lin_v, glin, seg, h)
        else:
            ops.embed_scatter_adam(t, m, v, grad, seg, h)
        return
    ops.adam_dense(t, m, v, h, grows=ops.embed_segment_sum(grad, seg), seg=seg, row_slot=row_slot, l2=l2)
    if with_lin:
        ops.adam_dense(lin, lin_m, lin_v, h, grows=ops.embed_segment_sum(glin.view(-1, 1), seg), seg=seg, row_slot=row_slot, l2=l2)


def helper_update(adam, with_lin, h, seg, st, grad, glin):
    adam.update(h, seg, *st[:3], grad, lin=(*st[3:], glin) if with_lin else None)


def assert_same(got, ref, what):
    for name, a, b in zip(("table", "m", "v", "lin", "lin_m", "lin_v"), got, ref):
        assert torch.equal(a, b), (what, name)


def valid_part(seg):
    n = seg.count()
    start = seg.start[:n + 1].cpu()
    return seg.rows[:n].cpu(), start, seg.pos[:int(start[-1])].cpu()


@pytest.mark.parametrize("form", list(FORMS))
def test_update_matches_the_parents_sequence_and_regrows(dev, form):
    dense, l2, with_lin = FORMS[form]
    rng = np.random.default_rng(sorted(FORMS).index(form))
    got = make_state(rng, dev)
    ref = [x.clone() for x in got]
    start = [x.clone() for x in got]
    adam = RowAdam(dev, dense, l2)
    ref_slot = torch.full((V,), -1, dtype=torch.int32, device=dev)
    owners, touched = [], set()
    for step, ids in ((1, IDS9), (2, rng.integers(-1, V, 20))):          # the second stream outgrows the first builder
        touched |= {int(r) for r in ids}
        ids, grad, glin = make_stream(rng, dev, ids)
        seg = adam.segments("a", ids, V)
        owners.append(seg.owner)
        assert seg.owner.n_max == ids.numel() and seg.n == ids.numel() and seg.V == V
        helper_update(adam, with_lin, hp(step), seg, got, grad, glin)
        parent_update(dense, l2, with_lin, hp(step), ops.build_segments(ids, V), ref, grad, glin, ref_slot)
        assert_same(got, ref, (form, step))
        if dense:
            assert bool((adam.row_slot(got[0]) == -1).all()) and adam.row_slot(got[0]).shape == (V,)
            assert adam.row_slot(got[0]) is adam.row_slot(got[3])                   # one scratch per table height
    assert owners[0] is not owners[1]
    assert adam.segments("a", make_stream(rng, dev, IDS9)[0], V).owner is owners[1]     # a shorter stream keeps the builder
    moved = (got[0] != start[0]).any(dim=1).cpu().tolist()
    assert moved == [dense or r in touched for r in range(V)]           # TF1: every row; else the touched ones
    if not with_lin:
        assert_same(got[3:], start[3:], form)


def test_update_all_rows(dev):
    rng = np.random.default_rng(7)
    got = make_state(rng, dev)[:3]
    ref = [x.clone() for x in got]
    before = got[0].clone()
    RowAdam(dev, True, 0.01).update_all_rows(hp(3), *got)
    ops.adam_dense(*ref, hp(3), l2=0.01)
    assert_same(got, ref, "all rows")
    assert bool((got[0] != before).any(dim=1).all())


def test_two_spaces_in_one_step(dev):
    rng = np.random.default_rng(8)
    adam = RowAdam(dev, True, 0.01)
    ids_a, grad_a, glin_a = make_stream(rng, dev, IDS9)
    ids_b, grad_b, glin_b = make_stream(rng, dev, (4, 4, -1, 0, 2, 4))
    seg_a = adam.segments("a", ids_a, V, want_slots=True)
    seg_b = adam.segments("b", ids_b, 5)
    assert seg_a.owner is not seg_b.owner and seg_b.V == 5 and seg_b.slots is None
    ref_a = ops.SegmentBuilder(9, V, dev).build(ids_a, want_slots=True)
    for x, y in zip(valid_part(seg_a), valid_part(ref_a)):                 # the build in "b" left "a" as it was
        assert torch.equal(x, y)
    keep = (ids_a >= 0).cpu()
    assert torch.equal(seg_a.slots.cpu()[keep], ref_a.slots.cpu()[keep])
    for x, y in zip(valid_part(seg_b), valid_part(ops.build_segments(ids_b, 5))):
        assert torch.equal(x, y)
    # both streams applied after both builds, as SVD++ applies its user stream after the history and item builds
    got_a, got_b = make_state(rng, dev), make_state(rng, dev, n_rows=5)
    ref_a_st, ref_b_st = [x.clone() for x in got_a], [x.clone() for x in got_b]
    helper_update(adam, True, hp(1), seg_b, got_b, grad_b, glin_b)
    helper_update(adam, True, hp(1), seg_a, got_a, grad_a, glin_a)
    parent_update(True, 0.01, True, hp(1), ops.build_segments(ids_b, 5), ref_b_st, grad_b, glin_b, None)
    parent_update(True, 0.01, True, hp(1), ops.build_segments(ids_a, V), ref_a_st, grad_a, glin_a, None)
    assert_same(got_a, ref_a_st, "a")
    assert_same(got_b, ref_b_st, "b")
    assert adam.row_slot(got_a[0]) is not adam.row_slot(got_b[0]) and adam.row_slot(got_b[0]).shape == (5,)
    assert bool((adam.row_slot(got_a[0]) == -1).all()) and bool((adam.row_slot(got_b[0]) == -1).all())


@pytest.mark.parametrize("width", [K, 16])      # 16: a width whose long runs the whole-workgroup kernels sum
@pytest.mark.parametrize("dense", [False, True])
def test_long_run_keeps_the_builders_workspace(dev, dense, width):
    rng = np.random.default_rng(9 + width + dense)
    ids = np.concatenate([np.full(LONG_RUN + 4, 2), [5, 0, 5, -1]]).astype(np.int32)
    rng.shuffle(ids)
    got = make_state(rng, dev, width=width)
    ref = [x.clone() for x in got]
    adam, parent = RowAdam(dev, dense, 0.0), ops.SegmentBuilder(len(ids), V, dev)
    ws = []
    for step in (1, 2):
        idt, grad, glin = make_stream(rng, dev, ids, width=width)
        seg = adam.segments("a", idt, V)
        assert int((seg.start[1:seg.count() + 1] - seg.start[:seg.count()]).max()) > LONG_RUN
        helper_update(adam, False, hp(step), seg, got, grad, glin)
        parent_update(dense, 0.0, False, hp(step), parent.build(idt), ref, grad, glin, None)
        assert_same(got, ref, (dense, width, step))
        ws.append((seg.owner, seg.long_ws(width).data_ptr()))
    assert ws[0][0] is ws[1][0] and ws[0][1] == ws[1][1] and ws[0][1] != 0


def test_lin_on_a_long_run_is_the_one_pass_kernel(dev):
    """`lin=` is `embed_scatter_adam_lin`, never two `embed_scatter_adam` launches: on a run past the threshold it matches
    that kernel bit for bit and, unlike the plain kernel, never asks the builder for a long-run workspace."""
    rng = np.random.default_rng(21)
    ids = np.concatenate([np.full(LONG_RUN + 4, 2), [5, 0, 5, -1]]).astype(np.int32)
    rng.shuffle(ids)
    got = make_state(rng, dev, width=16)
    ref = [x.clone() for x in got]
    adam = RowAdam(dev, False, 0.0)
    idt, grad, glin = make_stream(rng, dev, ids, width=16)
    seg = adam.segments("a", idt, V)
    helper_update(adam, True, hp(1), seg, got, grad, glin)
    assert seg.owner._long_ws == {}                                        # the plain kernel would have made [16] and [1]
    parent_update(False, 0.0, True, hp(1), ops.build_segments(idt, V), ref, grad, glin, None)
    assert_same(got, ref, "lin, long run")
    helper_update(adam, False, hp(2), seg, got, grad, glin)                # without `lin=`: the plain kernel, with workspace
    assert set(seg.owner._long_ws) == {16}


def test_l2_needs_the_dense_form(dev):
    with pytest.raises(ValueError, match="use `dense_adam=True` with it"):
        RowAdam(dev, False, 0.01)
    assert RowAdam(dev, False, 0.0).l2 == 0.0 and RowAdam(dev, False, None).l2 == 0.0 and RowAdam(dev, True, 0.01).dense
