"""numpy restatement of the IVF-SQ8 semantics on top of tests/ivf_oracle.py: training and lists are the Flat
index's; encoding is per-row symmetric int8; stage 1 ranks `scale * dot(q, codes)`; stage 2 re-scores the kk survivors exactly.

`encode` is bit-exact by construction (f32 division and rint are correctly rounded in numpy as on the device).  Stage-1 scores are
computed in fp64 and rounded: `dot` exactly (an integer-valued sum far below 2^53 ulps), then ONE f32 multiply by the scale, which
is what the device computes whenever its f32 dot is exact (the test grid); off the grid the tests bound the difference.
A plain helper module (no test in it), shared by tests/test_ivf_sq8_cpu.py and tests/test_ivf_sq8_gpu.py."""
from __future__ import annotations

import functools

import numpy as np

from . import ivf_oracle as O

MAX_K = 1024


def stride(D: int) -> int:
    return (D + 15) // 16 * 16


def kk_of(k: int, refine: int) -> int:
    return k if refine == 0 else min(max(k, k * refine), MAX_K)


def encode(rows: np.ndarray, list_ids=None):
    """(codes int8 [n, stride(D)], scales f32 [n]) of rows[list_ids] (identity without list_ids); padding columns are code 0."""
    x = np.asarray(rows, dtype=np.float32)
    if list_ids is not None:
        x = x[np.asarray(list_ids, dtype=np.int64)]
    n, D = x.shape
    a = np.abs(x).max(axis=1) if D else np.zeros(n, np.float32)
    scales = (a / np.float32(127)).astype(np.float32)
    codes = np.zeros((n, stride(D)), dtype=np.int8)
    live = scales > 0
    q = np.rint((x[live] / scales[live, None]).astype(np.float32))
    codes[live, :D] = np.clip(q, -127, 127).astype(np.int8)
    return codes, scales


def approx_scores(q: np.ndarray, codes: np.ndarray, scales: np.ndarray, as_f64: bool = False):
    """scale_j * dot(q, codes_j) for one query against code rows: the dot in fp64; `as_f64` keeps the product in fp64 too (the
    reference of the off-grid bound), otherwise dot is rounded to f32 and multiplied once in f32 (the device's value whenever its
    dot is exact)."""
    D = q.shape[0]
    dot = codes[:, :D].astype(np.float64) @ q.astype(np.float64)
    if as_f64:
        return scales.astype(np.float64) * dot
    return (scales.astype(np.float32) * dot.astype(np.float32) + np.float32(0)).astype(np.float32)      # + 0: -0 reads as +0


def _probed(q, cs_q, list_ptr, nprobe, nlist):
    probe = O.rank(cs_q, np.arange(nlist))[:nprobe]
    return np.concatenate([np.arange(list_ptr[l], list_ptr[l + 1]) for l in probe] + [np.zeros(0, np.int64)]).astype(np.int64)


def stage1(queries, centroids, list_ptr, list_ids, codes, scales, kk, nprobe, consumed=None, flags=None, as_f64=False):
    """([B, kk] scores, [B, kk] int64 ids) by (approximate score desc, global id asc) over the probed lists; -inf / -1 fill.
    `codes` / `scales` are in list order.  Scores are f32 (or fp64 with `as_f64`)."""
    B, nlist = queries.shape[0], centroids.shape[0]
    out_s = np.full((B, kk), -np.inf, dtype=np.float64 if as_f64 else np.float32)
    out_i = np.full((B, kk), -1, dtype=np.int64)
    cs = O.scores64(queries, centroids)
    for b in range(B):
        pos = _probed(queries[b], cs[b], list_ptr, nprobe, nlist)
        gid = list_ids[pos].astype(np.int64)
        if consumed is not None and consumed[b] is not None and (flags is None or flags[b]):
            keep = ~np.isin(gid, np.asarray(consumed[b]))
            pos, gid = pos[keep], gid[keep]
        if pos.size == 0:
            continue
        s = approx_scores(queries[b], codes[pos], scales[pos], as_f64)
        order = O.rank(s, gid)[:kk]
        out_s[b, :order.size] = s[order]
        out_i[b, :order.size] = gid[order]
    return out_s, out_i


def rerank(queries, rows, cand_ids, k):
    """Stage 2: exact fp64 inner products of the candidates (ids of -1 skipped), the k best by (score desc, id asc) as f32."""
    B = queries.shape[0]
    out_s = np.full((B, k), -np.inf, dtype=np.float32)
    out_i = np.full((B, k), -1, dtype=np.int64)
    for b in range(B):
        cand = cand_ids[b][cand_ids[b] >= 0]
        if cand.size == 0:
            continue
        s = O.scores64(queries[b:b + 1], rows[cand])[0]
        order = O.rank(s, cand)[:k]
        out_s[b, :order.size] = s[order].astype(np.float32)
        out_i[b, :order.size] = cand[order]
    return out_s, out_i


def search(queries, centroids, list_ptr, list_ids, rows, k, nprobe, refine, consumed=None, flags=None):
    """The whole SQ8 search over the catalogue `rows` (original order): encode in list order, stage 1 at kk, stage 2 if refine."""
    codes, scales = encode(rows, list_ids)
    s, i = stage1(queries, centroids, list_ptr, list_ids, codes, scales, kk_of(k, refine), nprobe, consumed, flags)
    if refine == 0:
        return s, i
    return rerank(queries, rows, i, k)


# a zero row; a row whose maximum is negative; a = 127 with halves (2.5 -> 2, 3.5 -> 4, -0.5 -> -0); one element; all at the maximum
HAND_MADE = np.array([[0.0, 0.0, 0.0, 0.0], [0.5, -2.0, 1.5, 0.0], [127.0, 2.5, 3.5, -0.5], [0.3, 0.0, 0.0, 0.0],
                      [-1.5, 1.5, -1.5, 1.5]], dtype=np.float32)
HAND_MADE_CODES = np.array([[0, 0, 0, 0], [32, -127, 95, 0], [127, 2, 4, 0], [127, 0, 0, 0], [-127, 127, -127, 127]], dtype=np.int8)


def mixture(rng: np.random.Generator, N: int, D: int, B: int, centres: int = 32, sigma: float = 0.3):
    """(rows [N, D], queries [B, D]) f32 from one Gaussian mixture: standard-normal centres, noise of scale sigma."""
    c = rng.standard_normal((centres, D))
    rows = c[rng.integers(0, centres, size=N)] + sigma * rng.standard_normal((N, D))
    queries = c[rng.integers(0, centres, size=B)] + sigma * rng.standard_normal((B, D))
    return rows.astype(np.float32), queries.astype(np.float32)


OFF_GRID_SEED = 33      # chosen on the oracle alone: 1 of 65 queries left out, coarse gap 0.016 against a bound of 0.0024


@functools.lru_cache(maxsize=2)      # computed once per process, shared by the tests that need it and left unchanged
def off_grid_case(seed: int = OFF_GRID_SEED, N: int = 5000, D: int = 128, nlist: int = 64, nprobe: int = 8, k: int = 100, B: int = 65,
                  refine: int = 4):
    """The inputs and fp64 references of the off-grid test.  Rounding bound of a device score, u = 2^-24: the f32 dot is a sum of D
    products in some order, each partial sum rounded once and bounded by S_j = sum_d |q_d c_jd|, so it errs by at most D u S_j (the
    device takes far fewer than D roundings on any path: 16 fmas and log2(lanes) pair sums); the multiply by the scale adds one
    rounding.  tol_j = 2 D u scale_j S_j doubles that, so that two scores that each err by tol_j / 2 still compare within tol_j.
    The same form with the f32 rows in place of scale * codes bounds the exact re-rank score: tol2_j = 2 D u sum_d |q_d x_jd|.

    Per query b: ref[b] = (global ids, fp64 stage-1 scores, tol) over the rows of the probed lists; `left_out[b]`: the fp64
    stage-1 gap at the kk cut is below the largest tol of the query, so the device's candidate set may differ from the oracle's;
    `coarse_gap`: the smallest gap of the centroid scores at the nprobe cut, and `coarse_tol` the same bound for those scores
    (the probe sets must not depend on rounding either)."""
    rows, queries = mixture(np.random.default_rng(seed), N, D, B)
    cent, _, ptr, ids = O.train_add(rows, nlist, 5)
    codes, scales = encode(rows, ids)
    kk = kk_of(k, refine)
    u = 2.0 ** -24
    cs = O.scores64(queries, cent)
    top = -np.sort(-cs, axis=1)
    coarse_gap = float((top[:, nprobe - 1] - top[:, nprobe]).min())
    coarse_tol = float(2 * D * u * (np.abs(queries).astype(np.float64) @ np.abs(cent).astype(np.float64).T).max())
    ref, left_out, tol_max = [], np.zeros(B, dtype=bool), 0.0
    for b in range(B):
        pos = _probed(queries[b], cs[b], ptr, nprobe, nlist)
        c = codes[pos, :D].astype(np.float64)
        q = queries[b].astype(np.float64)
        s64 = scales[pos].astype(np.float64) * (c @ q)
        tol = 2 * D * u * scales[pos].astype(np.float64) * (np.abs(c) @ np.abs(q))
        ref.append((ids[pos].astype(np.int64), s64, tol))
        tol_max = max(tol_max, float(tol.max()))
        if pos.size > kk:
            srt = -np.sort(-s64)
            left_out[b] = (srt[kk - 1] - srt[kk]) < tol.max()
    return dict(rows=rows, queries=queries, cent=cent, ptr=ptr, ids=ids, codes=codes, scales=scales, k=k, kk=kk, nprobe=nprobe,
                ref=ref, left_out=left_out, tol_max=tol_max, coarse_gap=coarse_gap, coarse_tol=coarse_tol,
                score_scale=float(max(np.abs(r[1]).max() for r in ref)))


def recall(got_ids: np.ndarray, ref_ids: np.ndarray) -> float:
    """Mean over queries of |got ∩ ref| / |ref| (ids >= 0 only)."""
    vals = []
    for g, r in zip(got_ids, ref_ids):
        r = r[r >= 0]
        if r.size:
            vals.append(np.isin(r, g[g >= 0]).mean())
    return float(np.mean(vals))
