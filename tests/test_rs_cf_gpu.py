"""RsUserCF / RsItemCF on the device against the numpy restatement (tests/rs_cf_oracle.py), bit for bit: every order is
fixed (ascending y for a pair's products, ascending column for a row's squares, list order for a prediction), so no
comparison here has a tolerance.  The kernel-level cases (pair state, merge and refresh, sums of squares, predict, same bits
on two runs, argument errors) run again on guarded allocations in tests/test_guarded_rs_cf_gpu.py."""
import json
import os
from functools import lru_cache

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from librecommender_amd import ops
from librecommender_amd.algorithms import ItemCF, RsItemCF, RsUserCF
from librecommender_amd.bases.cf_base import _DeviceCsr
from librecommender_amd.data import DataInfo, DatasetPure, split_by_ratio_chrono

from . import rs_cf_oracle as O
from .test_api_gpu import check_preds, check_recommends

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DATA = os.path.join(GOLDEN, "sample_movielens_rating.dat")
CASES = json.load(open(os.path.join(GOLDEN, "rs_cf_rust_cases.json")))
DEV = "cuda"


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def same_preds(a, b):
    """Bit for bit, except that a NaN (a rating over hits whose sims sum to 0) only has to be a NaN."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a[~nan]), bits(b[~nan]))


def to_dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def to_np(ts):
    return tuple(t.cpu().numpy() for t in ts)


def random_x(n_x, n_y, nnz, seed, integer=False):
    """An x-major interaction CSR with arbitrary float labels (negatives included) or integer labels 1-5."""
    rng = np.random.default_rng(seed)
    key = np.unique(rng.integers(0, n_x, nnz).astype(np.int64) * n_y + rng.integers(0, n_y, nnz))
    v = rng.integers(1, 6, key.size).astype(np.float32) if integer else rng.standard_normal(key.size).astype(np.float32)
    m = sp.csr_matrix((v, (key // n_y, key % n_y)), shape=(n_x, n_y), dtype=np.float32)
    m.sort_indices()
    return m


def with_entries(m, rows, cols, seed):
    """m with the entries (rows[i], cols[i]) set to random floats."""
    rng = np.random.default_rng(seed)
    m = m.tolil()
    m[rows, cols] = rng.standard_normal(len(rows)).astype(np.float32)
    m = m.tocsr().astype(np.float32)
    m.sort_indices()
    return m


# ---- pair state ------------------------------------------------------------------------------------------------------
def device_pair_state(x):
    X = _DeviceCsr.from_scipy(x, torch.device(DEV))
    Y = X.transpose()
    return to_np(ops.cf_pair_state(X.ptr, X.col, X.val, Y.ptr, Y.col, Y.val))


def oracle_pair_state(x):
    x1, x2, prod, cnt = O.delta_pairs(x.T.tocsr())
    return O.symmetric_csr(x.shape[0], x1, x2, prod, cnt.astype(np.int32))


def _tiles(extra):
    return lambda: random_x(extra[0] * ops.cf_sim_tile_cols() + extra[1], 300, extra[2], seed=11)


def _long_x_rows():
    rng = np.random.default_rng(12)
    m = random_x(40, 1200, 1500, seed=12)
    for r, n in ((0, 513), (1, 1100)):                 # more than one and more than two metadata batches of 512 y
        c = rng.choice(1200, n, replace=False)
        m = with_entries(m[:, :], np.full(n, r), c, seed=r)
        assert m.indptr[r + 1] - m.indptr[r] >= n
    return m


def _long_y_lists():
    rng = np.random.default_rng(13)
    m = random_x(1600, 30, 3000, seed=13)
    for y, n in ((0, 513), (1, 1500)):                 # longer than one workgroup pass of 512 entries
        m = with_entries(m, rng.choice(1600, n, replace=False), np.full(n, y), seed=y)
    return m


def _cancelling():
    # rows 0 / 1 share y 0 and 1 with products +6 and -6: prod is exactly 0 with count 2, and the pair must be present
    return sp.csr_matrix(np.array([[2, 3, 0, 0], [3, -2, 0, 1], [0, 0, 5, 1]], dtype=np.float32))


def _empty_trailing():
    m = random_x(90, 60, 900, seed=14).tolil()
    m[70:] = 0
    m = m.tocsr().astype(np.float32)
    m.eliminate_zeros()
    m.sort_indices()
    return m


PAIR_CASES = {
    "two_tiles": _tiles((1, 1, 20000)),                # n_x 8,193 at the library's tile of 8,192 columns
    "three_tiles": _tiles((2, 116, 30000)),            # n_x 16,500
    "x_rows_513_1100": _long_x_rows,
    "y_lists_513_1500": _long_y_lists,
    "cancelling_pair": _cancelling,
    "empty": lambda: sp.csr_matrix((5, 4), dtype=np.float32),
    "empty_trailing_rows": _empty_trailing,
}


@lru_cache(maxsize=None)
def pair_reference(case):
    """(x, the oracle's pair state) of a case: computed once, shared and left unchanged."""
    x = PAIR_CASES[case]()
    return x, oracle_pair_state(x)


@pytest.mark.parametrize("case", sorted(PAIR_CASES))
def test_pair_state(dev, case):
    x, ref = pair_reference(case)
    if case == "two_tiles":
        assert x.shape[0] == ops.cf_sim_tile_cols() + 1 == 8193
    if case == "three_tiles":
        assert x.shape[0] == 2 * ops.cf_sim_tile_cols() + 116 == 16500
    got = device_pair_state(x)
    for g, r, name in zip(got, ref, ("rowptr", "col", "prod", "cnt")):
        assert same(g, r), (case, name)
    ptr, col, prod, cnt = got
    S = sp.csr_matrix((np.arange(1, len(col) + 1), col, ptr), shape=(x.shape[0],) * 2)
    T = S.T.tocsr()
    T.sort_indices()
    assert np.array_equal(T.indices, col) and np.array_equal(T.indptr, ptr)                      # symmetric pattern
    assert same(prod[T.data - 1], prod) and same(cnt[T.data - 1], cnt)                           # and bits
    assert not np.any(col == np.repeat(np.arange(x.shape[0]), np.diff(ptr)))                     # no diagonal
    if case == "cancelling_pair":
        assert col[ptr[0]:ptr[1]].tolist() == [1] and prod[ptr[0]] == 0.0 and cnt[ptr[0]] == 2
    if case == "empty":
        assert len(col) == 0 and not ptr.any()


# ---- sums of squares -------------------------------------------------------------------------------------------------
def test_sumsq(dev):
    rng = np.random.default_rng(21)
    lens = [0, 1, 65, 3000, 0, 64, 130]
    rows = [np.sort(rng.choice(4000, n, replace=False)) for n in lens]
    x = sp.csr_matrix((rng.standard_normal(sum(lens)).astype(np.float32), np.concatenate(rows),
                       np.concatenate([[0], np.cumsum(lens)])), shape=(len(lens), 4000))
    X = _DeviceCsr.from_scipy(x, torch.device(DEV))
    ref = O.row_sumsq(x, len(lens))
    fresh = ops.cf_sumsq(X.ptr, X.val)
    assert same(fresh.cpu().numpy(), ref)
    start = rng.standard_normal(len(lens)).astype(np.float32) ** 2
    acc = to_dev(start, np.float32)
    assert ops.cf_sumsq(X.ptr, X.val, out=acc) is acc
    assert same(acc.cpu().numpy(), (start + ref).astype(np.float32))
    assert acc.cpu().numpy()[0] == start[0] and acc.cpu().numpy()[4] == start[4]                 # empty rows: unchanged


# ---- merge and refresh -----------------------------------------------------------------------------------------------
N_MERGE = 6000
# (old length, delta length, how the delta's columns relate to the old row's)
MERGE_ROWS = [(0, 0, "disjoint"), (0, 7, "disjoint"), (7, 0, "disjoint"), (40, 9, "subset"), (9, 40, "superset"),
              (30, 30, "disjoint"), (50, 50, "interleaved"), (63, 64, "interleaved"), (64, 65, "disjoint"),
              (65, 63, "subset"), (64, 64, "same"), (1025, 65, "interleaved"), (65, 1025, "superset"),
              (4100, 1025, "subset"), (1025, 4100, "interleaved"), (4100, 1500, "disjoint"), (0, 0, "disjoint")]
N_OLD_ROWS = len(MERGE_ROWS)          # the rows behind these exist in the delta only: beyond the old n_x


def _merge_inputs(seed=31):
    rng = np.random.default_rng(seed)
    o_cols, d_cols = [], []
    for lo, ld, how in MERGE_ROWS:
        pool = rng.permutation(N_MERGE)
        if how == "subset":
            oc = pool[:lo]
            dc = rng.choice(oc, ld, replace=False)
        elif how == "superset":
            dc = pool[:ld]
            oc = rng.choice(dc, lo, replace=False)
        elif how == "same":
            oc = dc = pool[:lo]
        elif how == "interleaved":
            both = min(lo, ld) // 2
            oc = pool[:lo]
            dc = np.concatenate([oc[:both], pool[lo:lo + ld - both]])
        else:
            oc, dc = pool[:lo], pool[lo:lo + ld]
        o_cols.append(np.sort(oc))
        d_cols.append(np.sort(dc))
    for n in (3, 70, 0, 1500):                          # rows beyond the old n_x
        d_cols.append(np.sort(rng.choice(N_MERGE, n, replace=False)))
    n_x = N_MERGE
    d_cols += [np.zeros(0, dtype=np.int64)] * (n_x - len(d_cols))

    def csr(cols):
        ptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
        return ptr, (np.concatenate(cols) if len(cols) else np.zeros(0)).astype(np.int32)

    o_ptr, o_col = csr(o_cols)
    d_ptr, d_col = csr(d_cols)
    f = lambda n: rng.standard_normal(n).astype(np.float32)  # noqa: E731
    old = (o_ptr, o_col, f(len(o_col)), rng.integers(1, 3, len(o_col)).astype(np.int32), f(len(o_col)))
    d_prod = f(len(d_col))
    d_prod[::11] = 0.0                                  # a product sum of 0
    delta = (d_ptr, d_col, d_prod, rng.integers(1, 3, len(d_col)).astype(np.int32))
    sumsq = (rng.standard_normal(n_x).astype(np.float32) ** 2 + np.float32(0.5)).astype(np.float32)
    sumsq[rng.choice(n_x, 40, replace=False)] = 0.0     # zero sums on the column side ...
    sumsq[5] = 0.0                                      # ... and on the row side (row 5: 30 delta columns)
    return old, delta, sumsq


@lru_cache(maxsize=None)
def merge_reference():
    """The inputs of the merge cases, the oracle's result and the oracle's result of a second update on top of it."""
    old, delta, sumsq = _merge_inputs()
    first = O.merge_rows(old, delta, sumsq)
    rng = np.random.default_rng(32)
    _, delta2, sumsq2 = _merge_inputs(seed=33)
    sumsq2 = (sumsq + rng.random(len(sumsq)).astype(np.float32)).astype(np.float32)
    second = O.merge_rows(first, delta2, sumsq2)
    return old, delta, sumsq, first, delta2, sumsq2, second


def device_merge(old, delta, sumsq):
    dts = (np.int64, np.int32, np.float32, np.int32, np.float32)
    o = ops.CfState(*(to_dev(a, dt) for a, dt in zip(old, dts)))
    d = tuple(to_dev(a, dt) for a, dt in zip(delta, dts))
    return ops.cf_state_update(o, d, to_dev(sumsq, np.float32))


NAMES = ("rowptr", "col", "prod", "cnt", "sim")


def test_merge_and_refresh(dev):
    old, delta, sumsq, first, delta2, sumsq2, second = merge_reference()
    assert len(old[0]) - 1 == N_OLD_ROWS < len(delta[0]) - 1
    got = device_merge(old, delta, sumsq)
    for g, r, name in zip(to_np(got), first, NAMES):
        assert same(g, r), name
    # an untouched pair keeps its old sim bits although the sums of squares are not what they were computed from
    o_ptr, o_col, _, _, o_sim = old
    ptr, col, _, _, sim = to_np(got)
    r = 3                                              # 40 old columns, 9 of them in the delta
    oc = o_col[o_ptr[r]:o_ptr[r + 1]]
    untouched = ~np.isin(oc, delta[1][delta[0][r]:delta[0][r + 1]])
    assert untouched.sum() == 31 and np.array_equal(col[ptr[r]:ptr[r + 1]], oc)
    assert same(sim[ptr[r]:ptr[r + 1]][untouched], o_sim[o_ptr[r]:o_ptr[r + 1]][untouched])
    assert not same(sim[ptr[r]:ptr[r + 1]][~untouched], o_sim[o_ptr[r]:o_ptr[r + 1]][~untouched])
    assert np.all(sim[ptr[5]:ptr[6]][np.isin(col[ptr[5]:ptr[6]], delta[1][delta[0][5]:delta[0][6]])] == 0)   # sumsq[5] = 0
    # a second update on top of the first
    got2 = ops.cf_state_update(got, tuple(to_dev(a, dt) for a, dt in zip(delta2, (np.int64, np.int32, np.float32, np.int32))),
                               to_dev(sumsq2, np.float32))
    for g, r_, name in zip(to_np(got2), second, NAMES):
        assert same(g, r_), name


@pytest.mark.parametrize("min_common", [0, 1, 2, 3])
def test_visible_pairs(dev, min_common):
    old, delta, sumsq, first, *_ = merge_reference()
    state = device_merge(old, delta, sumsq)
    got = to_np(ops.cf_state_visible(state, min_common))
    ref = O.visible(first, min_common)
    for g, r, name in zip(got, ref, ("rowptr", "col", "sim")):
        assert same(g, r), name
    # counts are 1 or 2 on either side: pairs of count 1 + 1 and 1 + 2 cross the thresholds 2 and 3 only at the update
    o_vis = O.visible((old[0], old[1], old[2], old[3], old[4]), min_common)
    if min_common >= 2:
        r = 6                                          # interleaved: 25 shared columns
        was = set(o_vis[1][o_vis[0][r]:o_vis[0][r + 1]].tolist())
        now = set(got[1][got[0][r]:got[0][r + 1]].tolist())
        shared = set(old[1][old[0][r]:old[0][r + 1]].tolist()) & set(delta[1][delta[0][r]:delta[0][r + 1]].tolist())
        assert (now - was) & shared
    if min_common <= 1:
        assert got[1].size == first[1].size


def test_update_of_the_empty_state_and_empty_delta(dev):
    old, delta, sumsq, *_ = merge_reference()
    n_x = len(delta[0]) - 1
    empty_old = tuple(t.cpu().numpy() for t in ops.cf_state_empty(3, DEV))
    got = to_np(device_merge(empty_old, delta, sumsq))
    ref = O.merge_rows(empty_old, delta, sumsq)
    assert all(same(g, r) for g, r in zip(got, ref)) and same(got[2], delta[2]) and same(got[3], delta[3])
    none = (np.zeros(n_x + 1, dtype=np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, np.int32))
    kept = to_np(device_merge(old, none, sumsq))
    assert same(kept[0][: len(old[0])], old[0]) and np.all(kept[0][len(old[0]):] == old[0][-1])
    assert all(same(g, r) for g, r in zip(kept[1:], old[1:]))
    nothing = to_np(device_merge(empty_old, none, sumsq))
    assert not nothing[0].any() and all(a.size == 0 for a in nothing[1:])


# ---- predict ---------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def predict_reference():
    rng = np.random.default_rng(41)
    n, n_other, k = 60, 50, 8
    sim = random_x(n, n, 1400, seed=41)
    sim.data = np.round(sim.data, 1)                   # tied sims, and visible neighbours with sim 0 (stored zeros)
    assert (sim.data == 0).sum() > 20
    sim.data[::9] = rng.standard_normal(len(sim.data[::9])).astype(np.float32)
    inter = random_x(n_other, n, 900, seed=42)         # rows: the other side; columns: the neighbours' ids
    lists = O.top_lists(sim.indptr, sim.indices, sim.data, k)
    srow, irow = rng.integers(0, n, 700), rng.integers(0, n_other, 700)
    irow[:20] = n_other - 1
    inter = inter.tolil()
    inter[n_other - 1] = 0                             # an empty interaction row: no hit
    inter = inter.tocsr().astype(np.float32)
    inter.eliminate_zeros()
    inter.sort_indices()
    ref = {}
    for task in ("ranking", "rating"):
        ref[task] = [O.predict_list(lists[s], inter.indices[inter.indptr[i]:inter.indptr[i + 1]],
                                    inter.data[inter.indptr[i]:inter.indptr[i + 1]], k, task, 2.5)
                     for s, i in zip(srow, irow)]
    full = O.top_lists(sim.indptr, sim.indices, sim.data, 10 ** 9)
    uncut = [O.predict_list(full[s], inter.indices[inter.indptr[i]:inter.indptr[i + 1]],
                            inter.data[inter.indptr[i]:inter.indptr[i + 1]], 10 ** 9, "ranking", 2.5)
             for s, i in zip(srow, irow)]
    return sim, inter, srow, irow, k, ref, uncut, lists


def device_predict(task, k_list=None):
    sim, inter, srow, irow, k, *_ = predict_reference()
    S = _DeviceCsr.from_scipy(sim, torch.device(DEV))
    # explicit zeros must survive: from_scipy keeps stored entries as they are
    I = _DeviceCsr.from_scipy(inter, torch.device(DEV))
    ids, sims, lens = ops.cf_topk(S.ptr, S.col, S.val, k_list or k)
    p, none = ops.cf_predict_topk(to_dev(srow, np.int32), to_dev(irow, np.int32), ids, sims, lens, I.ptr, I.col, I.val, k,
                                  task == "rating", 2.5)
    return p.cpu().numpy(), none.cpu().numpy()


@pytest.mark.parametrize("task", ["ranking", "rating"])
def test_predict(dev, task):
    *_, k, ref, uncut, lists = predict_reference()
    p, none = device_predict(task)
    want = np.array([r[0] for r in ref[task]], dtype=np.float32)
    want_none = np.array([r[1] for r in ref[task]], dtype=np.int32)
    assert np.array_equal(none, want_none) and 20 <= want_none.sum() < len(want_none)
    assert same_preds(p, want)
    assert np.all(p[none == 1] == np.float32(2.5))
    if task == "ranking":
        # the cut comes before the intersection: with the whole row many of these would differ
        assert sum(u[0] != w for u, w in zip(uncut, want)) > 50
        assert any(len({s for _, s in row}) < len(row) for row in lists)                         # tied sims in a list
        assert any(s == 0 for row in lists for _, s in row)                                      # a neighbour with sim 0
    # the same from longer lists cut by k in the kernel
    p2, none2 = device_predict(task, k_list=30)
    assert same_preds(p2, p) and np.array_equal(none2, none)


# ---- same bits on two runs -------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(dev):
    x, _ = pair_reference("three_tiles")
    a, b = device_pair_state(x), device_pair_state(x)
    assert all(same(p, q) for p, q in zip(a, b))
    old, delta, sumsq, *_ = merge_reference()
    a, b = to_np(device_merge(old, delta, sumsq)), to_np(device_merge(old, delta, sumsq))
    assert all(same(p, q) for p, q in zip(a, b))
    X = _DeviceCsr.from_scipy(x, torch.device(DEV))
    assert same(ops.cf_sumsq(X.ptr, X.val).cpu().numpy(), ops.cf_sumsq(X.ptr, X.val).cpu().numpy())
    for task in ("ranking", "rating"):
        (p, n), (q, m) = device_predict(task), device_predict(task)
        assert same_preds(p, q) and np.array_equal(n, m)


# ---- argument errors -------------------------------------------------------------------------------------------------
def test_argument_errors(dev):
    x = PAIR_CASES["cancelling_pair"]()
    X = _DeviceCsr.from_scipy(x, torch.device(DEV))
    Y = X.transpose()
    with pytest.raises(ValueError):
        ops.cf_pair_state(X.ptr, X.col, X.val[:-1].contiguous(), Y.ptr, Y.col, Y.val)
    with pytest.raises(ValueError):
        ops.cf_pair_state(X.ptr, X.col, X.val, Y.ptr, Y.col[:-1].contiguous(), Y.val[:-1].contiguous())
    with pytest.raises(ValueError):
        ops.cf_pair_state(X.ptr, X.col[::2], X.val[::2], Y.ptr, Y.col, Y.val)                    # not contiguous
    with pytest.raises(TypeError):
        ops.cf_pair_state(X.ptr, X.col, X.val.double(), Y.ptr, Y.col, Y.val)
    with pytest.raises(ValueError):
        ops.cf_sumsq(X.ptr, X.val, out=torch.zeros(2, device=DEV))
    delta = ops.cf_pair_state(X.ptr, X.col, X.val, Y.ptr, Y.col, Y.val)
    sumsq = ops.cf_sumsq(X.ptr, X.val)
    empty = ops.cf_state_empty(3, DEV)
    with pytest.raises(ValueError):
        ops.cf_state_update(empty, delta, sumsq[:2].contiguous())
    with pytest.raises(ValueError):
        ops.cf_state_update(ops.cf_state_empty(4, DEV), delta, sumsq)                            # more old rows than new
    with pytest.raises(ValueError):
        ops.cf_state_update(empty, (delta[0], delta[1], delta[2][:-1].contiguous(), delta[3]), sumsq)
    with pytest.raises(ValueError):
        ops.cf_state_update(empty, (delta[0], delta[1] + 3, delta[2], delta[3]), sumsq)          # a column beyond n_x
    with pytest.raises(ValueError):
        ops.cf_state_update(empty, (delta[0] + 1, delta[1], delta[2], delta[3]), sumsq)          # rowptr past the entries
    state = ops.cf_state_update(empty, delta, sumsq)
    ids, sims, lens = ops.cf_topk(state.ptr, state.col, state.sim, 2)
    q = to_dev([0], np.int32)
    with pytest.raises(ValueError):
        ops.cf_predict_topk(q, q, ids, sims, lens, Y.ptr, Y.col, Y.val, 0, False, 0.0)
    with pytest.raises(ValueError):
        ops.cf_predict_topk(q, to_dev([0, 1], np.int32), ids, sims, lens, Y.ptr, Y.col, Y.val, 2, False, 0.0)
    with pytest.raises(ValueError):
        ops.cf_predict_topk(q, q, ids, sims[:, :1].contiguous(), lens, Y.ptr, Y.col, Y.val, 2, False, 0.0)
    lib = ops._lib.load()
    assert lib.lr_cf_sumsq_f32(0, 0, -1, 0, 0, 0) == ops._lib.LR_EINVAL
    assert lib.lr_cf_state_merge_f32(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4, 0, 2, 0, 0, 0, 0, 0, 0, 0) == ops._lib.LR_EINVAL
    assert lib.lr_cf_predict_topk_f32(0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0.0, 0, 0, 0) == ops._lib.LR_EINVAL


def test_oversize_raises_before_allocating(dev, monkeypatch):
    x, ref = pair_reference("three_tiles")
    entries = len(ref[1])
    monkeypatch.setattr(ops, "CF_SIM_MAX_BYTES", entries * 16 - 1)        # 16 B per entry of the state, plus the rowptr
    with pytest.raises(MemoryError, match="pair state"):
        device_pair_state(x)
    old, delta, sumsq, first, *_ = merge_reference()
    monkeypatch.setattr(ops, "CF_SIM_MAX_BYTES", len(first[1]) * 16)
    with pytest.raises(MemoryError, match="pair state"):
        device_merge(old, delta, sumsq)
    monkeypatch.setattr(ops, "CF_SIM_MAX_BYTES", len(first[1]) * 16 + len(first[0]) * 8)
    assert device_merge(old, delta, sumsq).col.numel() == len(first[1])


# ---- property check, independent of the oracle -----------------------------------------------------------------------
def engine_update(state, sumsq, x, n_x):
    """One update the way `RsCfBase.fit` does it, on an x-major host CSR."""
    dev = torch.device(DEV)
    x = sp.csr_matrix(x)
    x.resize((n_x, x.shape[1]))
    X = _DeviceCsr.from_scipy(x, dev)
    Y = X.transpose()
    new_sumsq = torch.zeros(n_x, dtype=torch.float32, device=dev)
    if state is None:
        state = ops.cf_state_empty(n_x, dev)
    else:
        new_sumsq[: sumsq.numel()] = sumsq
    ops.cf_sumsq(X.ptr, X.val, out=new_sumsq)
    delta = ops.cf_pair_state(X.ptr, X.col, X.val, Y.ptr, Y.col, Y.val)
    return ops.cf_state_update(state, delta, new_sumsq), new_sumsq, delta


@pytest.mark.parametrize("side", ["item_cf", "user_cf"])
def test_update_equals_a_fit_on_the_union(dev, side):
    # integer labels 1-5 and disjoint y between the two batches: every sum is an exact integer below 2^24, so the order
    # of the additions cannot matter and the incremental state must equal the from-scratch one bit for bit
    ui = random_x(300, 220, 9000, seed=51, integer=True)
    zeros = lambda r, c: sp.csr_matrix((r, c), dtype=np.float32)  # noqa: E731
    if side == "item_cf":                              # x = items, y = users: the second batch's users are new
        first = ui[:170, :180].T.tocsr()               # 180 items are known at the first fit, 220 at the update
        second = sp.hstack([zeros(220, 170), ui[170:].T]).tocsr()
        n1, n2 = 180, 220
    else:                                              # x = users, y = items: the second batch's items are new
        first = ui[:250, :120].tocsr()                 # 250 users are known at the first fit, 300 at the update
        second = sp.hstack([zeros(300, 120), ui[:, 120:]]).tocsr()
        n1, n2 = 250, 300
    grown = first.copy()
    grown.resize(second.shape)
    union = (grown + second).tocsr()
    assert union.nnz == first.nnz + second.nnz
    for m in (first, second, union):
        m.eliminate_zeros()
        m.sort_indices()
    s1, q1, _ = engine_update(None, None, first, n1)
    s2, q2, delta = engine_update(s1, q1, second, n2)
    scratch, qs, _ = engine_update(None, None, union, n2)
    a, b = to_np(s2), to_np(scratch)
    for g, r, name in zip(a[:4], b[:4], NAMES):
        assert same(g, r), name
    assert same(q2.cpu().numpy(), qs.cpu().numpy())
    assert float(np.abs(a[2]).max()) < 2 ** 24 and float(q2.max()) < 2 ** 24
    # sim: the from-scratch value on every touched pair, the pre-update value on every untouched one
    ptr, col = a[0], a[1]
    rows = np.repeat(np.arange(n2), np.diff(ptr))
    d_ptr, d_col = delta[0].cpu().numpy(), delta[1].cpu().numpy()
    touched = np.isin(rows * n2 + col, np.repeat(np.arange(n2), np.diff(d_ptr)) * n2 + d_col)
    assert 0 < touched.sum() < len(col)
    assert same(a[4][touched], b[4][touched])
    o = to_np(s1)
    before = dict(zip((np.repeat(np.arange(n1), np.diff(o[0])) * n2 + o[1]).tolist(), bits(o[4]).tolist()))
    keys = (rows * n2 + col)[~touched].tolist()
    assert [before[k_] for k_ in keys] == bits(a[4][~touched]).tolist()
    assert not same(a[4][~touched], b[4][~touched])    # stale on purpose: their rows' sums of squares have grown


# ---- model level: the Rust cases -------------------------------------------------------------------------------------
def step_frame(step, side):
    m = step["x_major"]
    x = sp.csr_matrix((np.array(m["data"], dtype=np.float32), m["indices"], m["indptr"]),
                      shape=(len(m["indptr"]) - 1, step["n_y"])).tocoo()
    xs, ys = ("item", "user") if side == "item_cf" else ("user", "item")
    return pd.DataFrame({xs: x.row, ys: x.col, "label": x.data})[["user", "item", "label"]]


def model_lists(model, n_x):
    return {str(r): [i for i, _ in model.get_top_k_sims(r)] for r in range(n_x) if model.get_top_k_sims(r)}


@pytest.mark.parametrize("side", ["item_cf", "user_cf"])
def test_model_on_the_rust_cases(dev, side, tmp_path):
    cls = RsItemCF if side == "item_cf" else RsUserCF
    steps, k_sim = CASES["steps"], CASES["k_sim"]
    engine = O.Engine(CASES["min_common"], alias_keys=False)
    train, info = DatasetPure.build_trainset(step_frame(steps[0], side))
    assert all(info.user2id[u] == u for u in info.user2id) and all(info.item2id[i] == i for i in info.item2id)
    model = cls("ranking", info, k_sim=k_sim, min_common=CASES["min_common"])
    model.fit(train, neg_sampling=True, verbose=1)
    assert model_lists(model, steps[0]["n_x"]) == steps[0]["neighbours"]          # test_*_cf_training
    engine.update(step_matrix_x(steps[0]), steps[0]["n_x"])
    for n, step in enumerate(steps[1:]):
        info.save(str(tmp_path), "m")
        model.save(str(tmp_path), "m")
        info = DataInfo.load(str(tmp_path), "m")
        train, info = DatasetPure.merge_trainset(step_frame(step, side), info, merge_behavior=True)
        assert all(info.user2id[u] == u for u in info.user2id) and all(info.item2id[i] == i for i in info.item2id)
        model = cls("ranking", info, k_sim=k_sim, min_common=CASES["min_common"])
        model.rebuild_model(str(tmp_path), "m")
        assert model.incremental and model.n_x == step["n_x"]
        model.fit(train, neg_sampling=True, verbose=1)
        engine.update(step_matrix_x(step), step["n_x"])
        want = {str(r): engine.neighbour_ids(r, k_sim) for r in range(step["n_x"]) if engine.neighbour_ids(r)}
        assert model_lists(model, step["n_x"]) == want                            # the pair-identity lists
        if n == 0:
            assert {r: want[r] for r in CASES["pair_identity_first_update"]} == CASES["pair_identity_first_update"]
        st = model.pair_state()
        for g, r, name in zip([st[k_] for k_ in ("ptr", "col", "prod", "cnt", "sim")], engine.state(), NAMES):
            assert same(g, r), (step["name"], name)
        assert same(st["sumsq"], engine.sumsq)
        recs = model.recommend_user([5, 1], 10, inner_id=True)
        assert len(recs) == 2
        popular = {info.item2id[i] for i in info.popular_items}       # the fallback draws ten of these with replacement
        ui = model.user_interaction
        for u in (5, 1):
            rec = np.asarray(recs[u]).tolist()
            if u >= info.n_users:                      # unknown to this side's test: the popular items
                assert len(rec) == 10 and set(rec) <= popular
                continue
            mine = ui.indices[ui.indptr[u]:ui.indptr[u + 1]].tolist()
            if side == "item_cf":
                cand = {j for i in mine for j in engine.neighbour_ids(i, k_sim)}
            else:
                cand = {j for v in engine.neighbour_ids(u, k_sim) for j in ui.indices[ui.indptr[v]:ui.indptr[v + 1]].tolist()}
            cand -= set(info.user_consumed[u])
            if cand:                                   # ranked candidates: none of them consumed, short lists not padded
                assert set(rec) == cand and len(rec) == len(cand) <= 10
            else:                                      # every candidate consumed: the popular items, as the reference
                assert len(rec) == 10 and set(rec) <= popular


def step_matrix_x(step):
    m = step["x_major"]
    return sp.csr_matrix((np.array(m["data"], dtype=np.float32), m["indices"], m["indptr"]),
                         shape=(len(m["indptr"]) - 1, step["n_y"]))


# ---- model level: the reference's retrain flow on the sample file -----------------------------------------------------
def model_predict_oracle(model, engine, users, items):
    ui = model.user_interaction if model.cf_type == "item_cf" else model.item_interaction
    out = []
    for u, i in zip(users, items):
        s, o = (i, u) if model.cf_type == "item_cf" else (u, i)
        sl = slice(ui.indptr[o], ui.indptr[o + 1])
        out.append(O.predict_list(engine.neighbours(s, model.k_sim), ui.indices[sl], ui.data[sl], model.k_sim, model.task,
                                  model.default_pred)[0])
    return np.array(out, dtype=np.float32)


@pytest.mark.parametrize("side", ["item_cf", "user_cf"])
def test_retrain_on_the_sample_file(dev, side, tmp_path):
    cls = RsItemCF if side == "item_cf" else RsUserCF
    all_data = pd.read_csv(DATA, sep="::", engine="python", names=["user", "item", "label", "time"])
    n = len(all_data)
    parts = [all_data[: n // 2], all_data[n // 2: n * 3 // 4], all_data[n * 3 // 4:]]
    engine = O.ArrayEngine(1)
    path, name = str(tmp_path), side + "_model"
    info = model = None
    metrics = ["loss", "balanced_accuracy", "roc_auc", "pr_auc", "precision", "recall", "map", "ndcg"]
    for step, part in enumerate(parts):
        tr, ev = split_by_ratio_chrono(part, test_size=0.2)
        if step == 0:
            train_data, info = DatasetPure.build_trainset(tr)
            eval_data = DatasetPure.build_evalset(ev)
        else:
            info = DataInfo.load(path, name)
            train_data, info = DatasetPure.merge_trainset(tr, info, merge_behavior=True)
            eval_data = DatasetPure.merge_evalset(ev, info)
        model = cls(task="ranking", data_info=info, k_sim=20, mode="invert", num_threads=1, min_common=1, seed=42)
        if step:
            model.rebuild_model(path=path, model_name=name)
            assert model.incremental
        model.fit(train_data, neg_sampling=True, verbose=2, eval_data=eval_data, metrics=metrics, eval_user_num=100)
        check_preds(model, part)
        model.default_recs = np.array([info.item2id[i] for i in info.popular_items])       # what the checker compares with
        check_recommends(model, info, part)
        # the state, the neighbour lists and the predictions against the oracle
        new = sp.csr_matrix(train_data.sparse_interaction)
        new.resize((info.n_users, info.n_items))
        x = new if side == "user_cf" else new.T.tocsr()
        engine.update(x, x.shape[0])
        st = model.pair_state()
        for g, r, nm in zip([st[k_] for k_ in ("ptr", "col", "prod", "cnt", "sim")], engine.state(), NAMES):
            assert same(g, r), (step, nm)
        assert same(st["sumsq"], engine.sumsq)
        assert model.sim_matrix.nnz == engine.num_sim_elements()
        for r in range(0, x.shape[0], 37):
            got = model.get_top_k_sims(r) or []
            assert [(i, np.float32(s)) for i, s in got] == engine.neighbours(r, 20), (step, r)
        rng = np.random.default_rng(step)
        us, its = rng.integers(0, info.n_users, 400), rng.integers(0, info.n_items, 400)
        got = model.predict(us, its, inner_id=True)
        assert same_preds(got, model_predict_oracle(model, engine, us, its)), step
        info.save(path=path, model_name=name)
        model.save(path=path, model_name=name)
    # save -> load: identical predict and recommend_user; a loaded model refuses `fit`
    loaded = cls.load(path, name, info)
    assert (loaded.k_sim, loaded.min_common, loaded.mode, loaded.loaded) == (20, 1, "invert", True)
    users = list(range(0, info.n_users, 5))
    a = model.recommend_user(users, 10, inner_id=True)
    b = loaded.recommend_user(users, 10, inner_id=True)
    assert all(np.array_equal(a[u], b[u]) for u in users)
    us, its = np.arange(1000) % info.n_users, (np.arange(1000) * 7) % info.n_items
    assert same_preds(model.predict(us, its, inner_id=True), loaded.predict(us, its, inner_id=True))
    assert (loaded.sim_matrix != model.sim_matrix).nnz == 0
    with pytest.raises(RuntimeError, match="rebuild_model"):
        loaded.fit(train_data, neg_sampling=True, verbose=0)
    with pytest.raises(NotImplementedError):
        ItemCF("ranking", info).rebuild_model(path, name)


def test_multi_rank_fit_raises(dev, monkeypatch):
    train, info = DatasetPure.build_trainset(step_frame(CASES["steps"][0], "item_cf"))
    from librecommender_amd import distributed as D

    monkeypatch.setattr(D, "active", lambda group=None: (0, 2))
    with pytest.raises(RuntimeError, match="single process"):
        RsItemCF("ranking", info).fit(train, neg_sampling=True, verbose=0)
