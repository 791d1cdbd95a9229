"""numpy restatement of the IVF-Flat semantics: deterministic k-means, list build and search.

Scores are fp64 inner products; every sort is stable; the search is a brute-force ranking by (score desc, global id asc) over the
union of the probed lists.  A plain helper module (no test in it), shared by tests/test_ivf_cpu.py and tests/test_ivf_gpu.py."""
from __future__ import annotations

import numpy as np

TRAIN_CAP = 256          # training rows per list at most (faiss's cap)


def train_ids(N: int, nlist: int) -> np.ndarray:
    n_train = min(N, TRAIN_CAP * nlist)
    return (np.arange(n_train, dtype=np.int64) * N) // n_train


def init_ids(n_train: int, nlist: int) -> np.ndarray:
    return (np.arange(nlist, dtype=np.int64) * n_train) // nlist


def scores64(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return a.astype(np.float64) @ b.astype(np.float64).T


def assign(rows: np.ndarray, centroids: np.ndarray, want_scores: bool = False):
    """The centroid of largest inner product per row, ties to the lowest list id (argmax returns the first maximum)."""
    s = scores64(rows, centroids)
    a = np.argmax(s, axis=1).astype(np.int32)
    return (a, s) if want_scores else a


def build_lists(list_of: np.ndarray, nlist: int):
    """CSR of the lists (int64 [nlist + 1]) and the row ids in list order, ascending within a list (stable sort)."""
    ids = np.argsort(list_of, kind="stable").astype(np.int32)
    ptr = np.zeros(nlist + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(np.bincount(list_of, minlength=nlist))
    return ptr, ids


def centroid_means(rows: np.ndarray, list_ptr: np.ndarray, list_ids: np.ndarray, centroids: np.ndarray) -> np.ndarray:
    """f32 mean per list: the sum (fp64 here; exact in f32 on the test grid) rounded to f32 and divided ONCE by f32(count); an empty
    list keeps its previous centroid."""
    out = centroids.astype(np.float32).copy()
    for l in range(len(list_ptr) - 1):
        a, b = int(list_ptr[l]), int(list_ptr[l + 1])
        if b > a:
            s = rows[list_ids[a:b]].astype(np.float64).sum(axis=0)
            out[l] = s.astype(np.float32) / np.float32(b - a)
    return out


def train(rows: np.ndarray, nlist: int, niter: int = 20, want_gaps: bool = False):
    """Centroids after `niter` rounds on the deterministic training sample.  `want_gaps`: also the smallest gap between a training
    row's best and second-best centroid score relative to the score scale (largest |score|) over all rounds."""
    N = rows.shape[0]
    tr = rows[train_ids(N, nlist)]
    cent = tr[init_ids(tr.shape[0], nlist)].astype(np.float32).copy()
    min_gap = np.inf
    for _ in range(niter):
        a, s = assign(tr, cent, want_scores=True)
        if want_gaps and nlist > 1:
            top2 = np.partition(s, nlist - 2, axis=1)[:, -2:]
            min_gap = min(min_gap, float(((top2[:, 1] - top2[:, 0]) / np.abs(s).max()).min()))
        ptr, ids = build_lists(a, nlist)
        cent = centroid_means(tr, ptr, ids, cent)
    return (cent, min_gap) if want_gaps else cent


def train_add(rows: np.ndarray, nlist: int, niter: int = 20):
    cent = train(rows, nlist, niter)
    list_of = assign(rows, cent)
    ptr, ids = build_lists(list_of, nlist)
    return cent, list_of, ptr, ids


def rank(scores: np.ndarray, ids: np.ndarray) -> np.ndarray:
    """Positions ordered by (score desc, id asc)."""
    return np.lexsort((ids, -scores))


def search(queries: np.ndarray, centroids: np.ndarray, list_ptr: np.ndarray, list_ids: np.ndarray, rows: np.ndarray, k: int,
           nprobe: int, consumed=None, flags=None):
    """([B, k] f32 scores, [B, k] int64 ids): id -1 / score -inf beyond the surviving candidates.  `rows` are the catalogue in its
    ORIGINAL order; `consumed`: one ascending id array per query (or None); `flags`: filter on / off per query (default on)."""
    B = queries.shape[0]
    nlist = centroids.shape[0]
    out_s = np.full((B, k), -np.inf, dtype=np.float32)
    out_i = np.full((B, k), -1, dtype=np.int64)
    cs = scores64(queries, centroids)
    for q in range(B):
        probe = rank(cs[q], np.arange(nlist))[:nprobe]
        cand = np.concatenate([list_ids[list_ptr[l]:list_ptr[l + 1]] for l in probe] + [np.zeros(0, np.int32)]).astype(np.int64)
        if consumed is not None and consumed[q] is not None and (flags is None or flags[q]):
            cand = cand[~np.isin(cand, np.asarray(consumed[q]))]
        if cand.size == 0:
            continue
        s = scores64(queries[q:q + 1], rows[cand])[0]
        order = rank(s, cand)[:k]
        out_s[q, :order.size] = s[order].astype(np.float32)
        out_i[q, :order.size] = cand[order]
    return out_s, out_i


def brute_force(queries: np.ndarray, rows: np.ndarray, k: int):
    s = scores64(queries, rows)
    ids = np.arange(rows.shape[0])
    idx = np.stack([rank(s[q], ids)[:k] for q in range(queries.shape[0])])
    return np.take_along_axis(s, idx, axis=1).astype(np.float32), idx.astype(np.int64)


def grid(rng: np.random.Generator, shape) -> np.ndarray:
    """Multiples of 1/4 in [-2, 2]: every product and every partial sum of up to 256 of them is exact in f32."""
    return (rng.integers(-8, 9, size=shape) / 4.0).astype(np.float32)
