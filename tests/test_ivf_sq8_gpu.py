"""The IVF-SQ8 kernels (csrc/ivf_sq8.hip), `IVFSQ8Index` and its three seams against the numpy oracle (tests/ivf_sq8_oracle.py).

Kernel-level inputs lie on the grid of tests/ivf_oracle.py (multiples of 1/4 in [-2, 2]).  There every code dot is exact in f32
in any order (|dot| <= 256 * 2 * 127 at resolution 1/4: tests/test_ivf_sq8_cpu.py), the approximate score is that dot times the
scale, one rounded multiply, and exact scores are exact: every grid comparison is BIT FOR BIT on ids and on uint32 views of
scores.  Encoding is bit for bit off the grid too: both sides round the division correctly and rint to even."""
import os

import numpy as np
import pytest
import torch

from librecommender_amd import _lib, ops
from librecommender_amd.recommendation.ivf import IVFFlatIndex
from librecommender_amd.recommendation.ivf_sq8 import IVFSQ8Index

from . import ivf_oracle as O
from . import ivf_sq8_oracle as Q
from .test_ivf_gpu import SEARCH_CASES, _consumed, _csr, _dev, _index, _same, model  # noqa: F401  (model: the fixture)

pytestmark = pytest.mark.gpu


# ---- encode -----------------------------------------------------------------------------------------------------------
def _check_encode(dev, rows, ids=None):
    exp_c, exp_s = Q.encode(rows, ids)
    codes, scales = ops.ivf_sq8_encode(_dev(rows, dev), None if ids is None else _dev(ids, dev))
    assert codes.dtype == torch.int8 and tuple(codes.shape) == (exp_c.shape[0], Q.stride(rows.shape[1]))
    assert np.array_equal(codes.cpu().numpy(), exp_c)                                   # the padding codes (0) included
    assert np.array_equal(scales.cpu().numpy().view(np.uint32), exp_s.view(np.uint32))


@pytest.mark.parametrize("D", [4, 6, 16, 20, 128, 256])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 5000])
def test_encode(dev, D, n):
    rng = np.random.default_rng(1000 * D + n)
    perm = rng.permutation(n).astype(np.int32)
    for rows in (O.grid(rng, (n, D)), (rng.standard_normal((n, D)) * 0.3).astype(np.float32)):
        rows[n // 2] = 0                                                                # a zero row: scale 0, codes 0
        _check_encode(dev, rows)
        _check_encode(dev, rows, perm)
        _check_encode(dev, rows, perm[: max(1, n // 3)])                                # fewer codes than rows


def test_encode_hand_made_rows(dev):
    _check_encode(dev, Q.HAND_MADE)
    codes, scales = ops.ivf_sq8_encode(_dev(Q.HAND_MADE, dev))
    assert np.array_equal(codes.cpu().numpy()[:, :4], Q.HAND_MADE_CODES)
    assert scales.cpu().numpy().tolist() == [0.0, float(np.float32(2) / np.float32(127)), 1.0, float(np.float32(0.3) / np.float32(127)),
                                             float(np.float32(1.5) / np.float32(127))]
    _check_encode(dev, np.array([[0.3]], np.float32))                                   # a row of one element (padded by the host)


# ---- search -----------------------------------------------------------------------------------------------------------
def _sq8(dev, rows, cent, ptr, ids, queries, k, nprobe, refine, lists=None, flags=None, out=None):
    """Stage 1 (+ stage 2) through the ops, on codes the device encoded; returns numpy (scores, ids)."""
    d_rows, d_ids, q = _dev(rows, dev), _dev(ids, dev), _dev(queries, dev)
    codes, scales = ops.ivf_sq8_encode(d_rows, d_ids)
    args = [q, _dev(cent, dev), _dev(ptr, dev), d_ids, codes, scales, Q.kk_of(k, refine), nprobe]
    if lists is not None:
        cp, ci = _csr(lists)
        args += [_dev(cp, dev), _dev(ci, dev), None if flags is None else _dev(flags, dev)]
    s, i = ops.ivf_sq8_search(*args, out=out) if out is not None else ops.ivf_sq8_search(*args)
    if refine:
        s, i = ops.ivf_rerank(q, d_rows, i, k)
    return s.cpu().numpy(), i.cpu().numpy()


@pytest.mark.parametrize("refine", [0, 1, 4])
@pytest.mark.parametrize("N,nlist,D,B,k,nprobe,kind", SEARCH_CASES + [(5000, 80, 128, 3, 300, 10, "assign")])      # kk clipped: 300 * 4
def test_search(dev, N, nlist, D, B, k, nprobe, kind, refine):
    rng = np.random.default_rng(N + 31 * nlist + D + B + k + nprobe)
    rows, cent, ptr, ids = _index(rng, N, nlist, D, kind)
    queries = O.grid(rng, (B, D))
    lists, flags = _consumed(rng, B, N)
    for ls, fl in ((None, None), (lists, flags), (lists, None)):
        _same(_sq8(dev, rows, cent, ptr, ids, queries, k, nprobe, refine, ls, fl),
              Q.search(queries, cent, ptr, ids, rows, k, nprobe, refine, ls, fl))


@pytest.mark.parametrize("refine", [0, 4])
@pytest.mark.parametrize("nprobe", [1, 2])
def test_search_consumed_list_empties_a_probed_list(dev, nprobe, refine):
    rng = np.random.default_rng(5)
    N, nlist, D, k = 1000, 7, 16, 10
    rows, cent, ptr, ids = _index(rng, N, nlist, D, "assign")
    queries = O.grid(rng, (3, D))
    best = O.rank(O.scores64(queries, cent)[0], np.arange(nlist))[0]
    assert ptr[best + 1] > ptr[best]
    lists = [np.sort(ids[ptr[best]:ptr[best + 1]]).astype(np.int32), np.zeros(0, np.int32), np.arange(N, dtype=np.int32)]
    got = _sq8(dev, rows, cent, ptr, ids, queries, k, nprobe, refine, lists, None)
    _same(got, Q.search(queries, cent, ptr, ids, rows, k, nprobe, refine, lists, None))
    if nprobe == 1:
        assert (got[1][0] == -1).all() and np.isneginf(got[0][0]).all()
    assert (got[1][2] == -1).all() and np.isneginf(got[0][2]).all()                     # everything consumed


@pytest.mark.parametrize("refine", [0, 4])
def test_search_a_list_of_all_zero_rows(dev, refine):
    """Scale 0: every row of list 0 scores +0 at stage 1 and ranks by id among the zeros."""
    rng = np.random.default_rng(9)
    N, nlist, D, k = 1000, 7, 20, 1000                                                  # k = N: every row comes back
    rows, cent, ptr, ids = _index(rng, N, nlist, D, "assign")
    rows[ids[ptr[0]:ptr[1]]] = 0
    assert ptr[1] - ptr[0] > 10
    queries = O.grid(rng, (5, D))
    got = _sq8(dev, rows, cent, ptr, ids, queries, k, nlist, refine)
    _same(got, Q.search(queries, cent, ptr, ids, rows, k, nlist, refine))
    zero = np.isin(got[1], ids[ptr[0]:ptr[1]])
    assert (zero.sum(axis=1) == ptr[1] - ptr[0]).all() and (got[0][zero] == 0).all()


@pytest.mark.parametrize("N,nlist,D,B,k,nprobe", [(1000, 7, 16, 3, 10, 3), (900, 80, 6, 3, 100, 80), (1000, 7, 128, 65, 5, 7)])
def test_full_refine_equals_flat(dev, N, nlist, D, B, k, nprobe):
    """With kk >= the number of probed rows stage 1 drops nothing, so the re-rank sees what the Flat scan sees."""
    rng = np.random.default_rng(N + D)
    rows, cent, ptr, ids = _index(rng, N, nlist, D, "assign")
    queries = O.grid(rng, (B, D))
    lists, flags = _consumed(rng, B, N)
    cp, ci = _csr(lists)
    d = [_dev(x, dev) for x in (queries, cent, ptr, ids, rows)]
    codes, scales = ops.ivf_sq8_encode(d[4], d[3])
    filt = (_dev(cp, dev), _dev(ci, dev), _dev(flags, dev))
    _, cand = ops.ivf_sq8_search(d[0], d[1], d[2], d[3], codes, scales, 1024, nprobe, *filt)
    assert (cand >= 0).sum(dim=1).max() < 1024                                      # kk exceeded the probed rows of every query
    s, i = ops.ivf_rerank(d[0], d[4], cand, k)
    es, ei = ops.ivf_search(d[0], d[1], d[2], d[3], _dev(rows[ids], dev), k, nprobe, *filt)
    _same((s.cpu().numpy(), i.cpu().numpy()), (es.cpu().numpy(), ei.cpu().numpy()))


@pytest.mark.parametrize("N,D,B,kk,k", [(500, 16, 3, 40, 10), (50, 6, 2, 64, 64), (3000, 128, 65, 1024, 100), (7, 256, 1, 1, 1),
                                        (500, 20, 4, 100, 1024)])
def test_rerank(dev, N, D, B, kk, k):
    """Alone, on candidate lists with -1 holes (no duplicate ids), k above the number of valid ids among the cases."""
    rng = np.random.default_rng(N + kk)
    rows, queries = O.grid(rng, (N, D)), O.grid(rng, (B, D))
    cand = np.full((B, kk), -1, dtype=np.int64)
    for b in range(B):
        n_valid = int(rng.integers(0, min(N, kk) + 1)) if b else min(N, kk)
        slots = rng.choice(kk, size=n_valid, replace=False)
        cand[b, slots] = rng.choice(N, size=n_valid, replace=False)
    if B > 1:
        cand[1] = -1                                                                    # nothing valid at all
    s, i = ops.ivf_rerank(_dev(queries, dev), _dev(rows, dev), _dev(cand, dev), k)
    _same((s.cpu().numpy(), i.cpu().numpy()), Q.rerank(queries, rows, cand, k))


def test_two_runs_give_the_same_bits(dev):
    rng = np.random.default_rng(11)
    N, nlist, D = 5000, 64, 128
    rows = (rng.standard_normal((N, D)) * 0.3).astype(np.float32)       # off the grid: rounding takes part
    queries = rng.standard_normal((65, D)).astype(np.float32)
    runs = []
    for _ in range(2):
        idx = IVFSQ8Index.train_add(_dev(rows, dev), nlist, niter=3)
        s, i = idx.search(_dev(queries, dev), 100, nprobe=8)
        s0, i0 = idx.search(_dev(queries, dev), 100, nprobe=8, refine=0)
        runs.append((idx.centroids.clone(), idx.list_ptr.clone(), idx.list_ids.clone(), idx.codes.clone(), idx.scales.clone(), s, i, s0, i0))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    flat = IVFFlatIndex.train_add(_dev(rows, dev), nlist, niter=3)      # the same training and lists, bit for bit
    for a, b in zip(runs[0][:3], (flat.centroids, flat.list_ptr, flat.list_ids)):
        assert torch.equal(a, b)


@pytest.fixture(scope="module")
def off_grid():
    return Q.off_grid_case()


@pytest.mark.parametrize("refine", [0, 4])
def test_off_grid_within_the_bound(dev, off_grid, refine):
    """Against the fp64 oracle with the derived tolerance of `ivf_sq8_oracle.off_grid_case` (tol_j = 2 D 2^-24 scale_j sum_d |q_d
    c_jd| at stage 1, the same form over the f32 rows at stage 2): every returned score is within tol_j of the oracle's value for
    that id, and every returned id's oracle score is >= the oracle's k-th score - tol (the query's largest).  At refine 4 the
    queries whose fp64 stage-1 gap at the kk cut is below tol are left out of the stage-2 check (1 of 65 for this seed; at most
    5 % is asserted in tests/test_ivf_sq8_cpu.py); for the others the device's candidate set must be the oracle's."""
    c = off_grid
    D = c["rows"].shape[1]
    k, kk = c["k"], (c["kk"] if refine else c["k"])
    d = [_dev(c[n], dev) for n in ("queries", "cent", "ptr", "ids", "rows")]
    codes, scales = ops.ivf_sq8_encode(d[4], d[3])
    assert np.array_equal(codes.cpu().numpy(), c["codes"]) and np.array_equal(scales.cpu().numpy(), c["scales"])
    s1, i1 = (t.cpu().numpy() for t in ops.ivf_sq8_search(d[0], d[1], d[2], d[3], codes, scales, kk, c["nprobe"]))
    for b, (gid, s64, tol) in enumerate(c["ref"]):
        n1 = min(kk, gid.size)
        assert (i1[b, :n1] >= 0).all() and (i1[b, n1:] == -1).all() and len(set(i1[b, :n1].tolist())) == n1
        at = {int(g): p for p, g in enumerate(gid)}
        pos = np.array([at[int(g)] for g in i1[b, :n1]])                                # a KeyError: an id outside the probed lists
        assert (np.abs(s1[b, :n1].astype(np.float64) - s64[pos]) <= tol[pos]).all()
        assert (s64[pos] >= -np.sort(-s64)[n1 - 1] - tol.max()).all()
    if not refine:
        return
    s2, i2 = (t.cpu().numpy() for t in ops.ivf_rerank(d[0], d[4], _dev(i1, dev), k))
    u = 2.0 ** -24
    checked = 0
    for b, (gid, s64, tol) in enumerate(c["ref"]):
        if c["left_out"][b]:
            continue
        checked += 1
        cand = gid[O.rank(s64, gid)[:kk]]
        assert set(cand.tolist()) == set(i1[b][i1[b] >= 0].tolist())
        q, x = c["queries"][b].astype(np.float64), c["rows"][cand].astype(np.float64)
        e64, tol2 = x @ q, 2 * D * u * (np.abs(x) @ np.abs(q))
        at = {int(g): p for p, g in enumerate(cand)}
        n2 = min(k, cand.size)
        pos = np.array([at[int(g)] for g in i2[b, :n2]])
        assert len(set(i2[b, :n2].tolist())) == n2 and (i2[b, n2:] == -1).all()
        assert (np.abs(s2[b, :n2].astype(np.float64) - e64[pos]) <= tol2[pos]).all()
        assert (e64[pos] >= -np.sort(-e64)[n2 - 1] - tol2.max()).all()
    assert checked >= 0.95 * len(c["ref"])


def test_unsupported_shapes_raise_and_write_nothing(dev):
    rng = np.random.default_rng(3)
    N, nlist, D, B = 1000, 7, 16, 3
    rows, cent, ptr, ids = _index(rng, N, nlist, D, "assign")
    queries = O.grid(rng, (B, D))
    idx = IVFSQ8Index.train_add(_dev(rows, dev), nlist, niter=1)
    with pytest.raises(ValueError, match="shape not supported"):
        idx.search(_dev(queries, dev), 10, refine=65)
    with pytest.raises(ValueError, match="shape not supported"):
        idx.search(_dev(queries, dev), 1025)
    assert _lib.load().lr_ivf_sq8_supported(B, N, D, 10, 2, nlist, 65) == 0
    t = [_dev(x, dev) for x in (queries, cent, ptr, ids, rows)]
    codes, scales = ops.ivf_sq8_encode(t[4], t[3])
    for k, D_bad in ((1025, None), (10, 6), (10, 260)):
        out_s = torch.full((B, k), 1234.5, dtype=torch.float32, device=dev)
        out_i = torch.full((B, k), 777, dtype=torch.int64, device=dev)
        if D_bad is None:
            with pytest.raises(ValueError, match="shape not supported"):
                ops.ivf_sq8_search(t[0], t[1], t[2], t[3], codes, scales, k, 2, out=(out_s, out_i))
            with pytest.raises(ValueError, match="shape not supported"):
                ops.ivf_rerank(t[0], t[4], torch.zeros((B, 4), dtype=torch.int64, device=dev), k, out=(out_s, out_i))
        else:                                    # the C entry points themselves: a width they do not take (the wrappers would pad 6)
            ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
            with pytest.raises(ValueError):
                ops._call("lr_ivf_sq8_search_f32", t[0].data_ptr(), B, t[1].data_ptr(), nlist, t[2].data_ptr(), t[3].data_ptr(),
                          codes.data_ptr(), codes.shape[1], scales.data_ptr(), N, D_bad, 0, 0, 0, k, 2, out_s.data_ptr(), out_i.data_ptr(),
                          ws.data_ptr(), ws.numel(), ops._stream())
            with pytest.raises(ValueError):
                ops._call("lr_ivf_rerank_f32", t[0].data_ptr(), B, t[4].data_ptr(), N, D_bad, out_i.data_ptr(), k, k, out_s.data_ptr(),
                          out_i.data_ptr(), ops._stream())
            oc = torch.full((N, 272), 55, dtype=torch.int8, device=dev)
            osc = torch.full((N,), 1234.5, dtype=torch.float32, device=dev)
            with pytest.raises(ValueError):
                ops._call("lr_ivf_sq8_encode_f32", t[4].data_ptr(), N, D_bad, 0, N, oc.data_ptr(), 272 if D_bad > 256 else 16,
                          osc.data_ptr(), ops._stream())
            torch.cuda.synchronize()
            assert (oc == 55).all() and (osc == 1234.5).all()
            assert _lib.load().lr_ivf_sq8_supported(B, N, D_bad, k, 2, nlist, 4) == 0
        torch.cuda.synchronize()
        assert (out_s == 1234.5).all() and (out_i == 777).all()
    with pytest.raises(ValueError, match="shape not supported"):
        ops.ivf_sq8_encode(torch.zeros((4, 260), device=dev))


# ---- model level ------------------------------------------------------------------------------------------------------
def test_init_knn_sq8_neighbours_are_within_the_bound(model):  # noqa: F811
    """`init_knn(codes="sq8", nprobe=2)`: with refine 4 and k = 10 the scan keeps 40 candidates.  Every returned neighbour's exact
    fp64 score is >= the k-th exact score among the oracle's own 40 candidates minus the stage-2 bound, for the queries whose
    fp64 stage-1 gap at the cut of 40 exceeds the stage-1 bound (the bounds of `ivf_sq8_oracle.off_grid_case`)."""
    m, info = model
    with pytest.raises(ValueError, match="unknown codes"):
        m.init_knn(False, "cosine", nlist=8, nprobe=2, codes="pq")
    m.init_knn(False, "cosine", nlist=8, nprobe=2, codes="sq8")
    assert set(m._knn_index) == {"user", "item"} and all(isinstance(i, IVFSQ8Index) for i in m._knn_index.values())
    u, k, kk, checked = 2.0 ** -24, 10, 40, 0
    for side, names, fn in (("user", list(info.user2id)[:8], m.search_knn_users), ("item", list(info.item2id)[:8], m.search_knn_items)):
        idx, rows = m._knn_index[side], m._knn_rows[side].cpu().numpy()
        assert idx.nprobe == 2 and idx.refine == 4 and idx.rows.data_ptr() == m._knn_rows[side].data_ptr()      # no copy of the rows
        D = rows.shape[1]
        cent, ptr, ids = idx.centroids.cpu().numpy(), idx.list_ptr.cpu().numpy(), idx.list_ids.cpu().numpy()
        codes, scales = Q.encode(rows, ids)
        assert np.array_equal(idx.codes.cpu().numpy(), codes) and np.array_equal(idx.scales.cpu().numpy(), scales)
        name2id = info.user2id if side == "user" else info.item2id
        for name in names:
            q = rows[name2id[name]]
            got = [name2id[n] for n in fn(name, k)]
            s64, i64 = Q.stage1(q[None], cent, ptr, ids, codes, scales, kk + 1, 2, as_f64=True)
            valid = i64[0] >= 0
            cand, sc = i64[0][valid][:kk], s64[0][valid]
            pos = np.array([int(np.nonzero(ids == g)[0][0]) for g in i64[0][valid]])
            tol = (2 * D * u * scales[pos].astype(np.float64) * (np.abs(codes[pos, :D].astype(np.float64)) @ np.abs(q.astype(np.float64)))).max()
            if sc.size > kk and sc[kk - 1] - sc[kk] < tol:
                continue
            checked += 1
            x = rows[cand].astype(np.float64)
            e64, tol2 = x @ q.astype(np.float64), (2 * D * u * (np.abs(x) @ np.abs(q.astype(np.float64)))).max()
            assert len(got) == min(k, cand.size) and len(set(got)) == len(got) and set(got) <= set(cand.tolist())
            kth = -np.sort(-e64)[len(got) - 1]
            assert all(e64[np.nonzero(cand == g)[0][0]] >= kth - tol2 for g in got)
    assert checked >= 12
    m.init_knn(False, "cosine", nlist=8, nprobe=2)                     # codes=None: today's path
    assert all(isinstance(i, IVFFlatIndex) for i in m._knn_index.values())


def test_embed_server_through_the_sq8_index(model, tmp_path):  # noqa: F811
    from librecommender_amd import serving

    m, info = model
    path = str(tmp_path / "serve")
    serving.save_embed(path, m)
    file = serving.save_ivf_sq8_index(path, m, nlist=8, nprobe=8)
    assert os.path.basename(file) == "ivf_sq8_index.npz"
    assert sorted(np.load(file).files) == ["centroids", "d", "list_ids", "list_ptr", "nprobe", "refine"]      # no codes on disk
    exact = serving.EmbedServer(path, "cuda", use_index=False)
    served = serving.EmbedServer(path, "cuda", use_index=True)
    assert exact.index is None and isinstance(served.index, IVFSQ8Index) and served.index.nprobe == 8 and served.index.refine == 4
    d = served.item_embeds.shape[1]
    if d % 4 == 0:
        assert served.index.rows.data_ptr() == served.item_embeds.data_ptr()            # the table is held once
    else:                                            # a width that is no multiple of 4 (a bias column) is zero-padded once
        assert tuple(served.index.rows.shape) == (served.n_items, (d + 3) // 4 * 4)
        assert torch.equal(served.index.rows[:, :d], served.item_embeds) and not served.index.rows[:, d:].any()
    users = list(info.user2id)[:50]
    for nprobe in (1, 2, 8):
        served.index.nprobe = nprobe
        for usr, recs in served.recommend(users, 10).items():
            seen = {info.id2item[i] for i in info.user_consumed[info.user2id[usr]]}
            assert len(recs) == len(set(recs)) and not seen & set(recs)
    # every list probed: with E the largest |approximate - exact| score of the user (fp64 oracle) and t the 10th best exact score
    # among the unseen items, every recommendation scores >= t - 2 E.  (If the 40 candidates hold the true top 10 the re-rank
    # returns it; if one of them, x, is missing, all 40 have approximate scores >= approx(x) >= t - E, hence exact ones >= t - 2 E.)
    served.index.nprobe = 8
    items, raw2id = served.item_embeds.cpu().numpy().astype(np.float64), {v: int(i) for i, v in served.id2item.items()}
    codes, scales = Q.encode(served.item_embeds.cpu().numpy())
    approx = (codes[:, : items.shape[1]] * scales[:, None].astype(np.float64))
    for usr, recs in served.recommend(users, 10).items():
        q = served.user_embeds[info.user2id[usr]].cpu().numpy().astype(np.float64)
        unseen = np.setdiff1d(np.arange(len(items)), np.asarray(info.user_consumed[info.user2id[usr]]))
        ex = items @ q
        E = np.abs(approx @ q - ex).max() + 1e-5 * np.abs(ex).max()                    # f32 rounding of both stages rides along
        t = -np.sort(-ex[unseen])[min(10, unseen.size) - 1]
        assert len(recs) == min(10, unseen.size) and all(ex[raw2id[r]] >= t - 2 * E for r in recs)
    serving.save_ivf_index(path, m, nlist=8, nprobe=8)
    both = serving.EmbedServer(path, "cuda", use_index=True)
    assert isinstance(both.index, IVFFlatIndex)                                         # the Flat file wins when both exist


def test_index_save_load_round_trip_and_bytes(model, dev, tmp_path):  # noqa: F811
    m, _ = model
    rows = m.item_embeds[: m.n_items].contiguous()
    idx = IVFSQ8Index.train_add(rows, 8, nprobe=3, refine=2)
    idx.save(str(tmp_path))
    back = IVFSQ8Index.load(str(tmp_path), dev, rows)
    assert (back.nprobe, back.refine, back.d, back.nlist) == (3, 2, idx.d, 8)
    assert torch.equal(idx.codes, back.codes) and torch.equal(idx.scales, back.scales)
    q = m.user_embeds[:33].contiguous()
    for refine in (None, 0):
        for a, b in zip(idx.search(q, 20, refine=refine), back.search(q, 20, refine=refine)):
            assert torch.equal(a, b)
    flat = IVFFlatIndex.train_add(rows, 8, nprobe=3)
    assert torch.equal(flat.list_ids, idx.list_ids) and torch.equal(flat.centroids, idx.centroids)
    assert idx.nbytes == sum(t.numel() * t.element_size() for t in (idx.codes, idx.scales, idx.list_ids, idx.list_ptr, idx.centroids))
    assert idx.nbytes < flat.list_rows.numel() * 4
