"""A numpy restatement of the reference's UserCF / ItemCF semantics, the yardstick of tests/test_cf_*.py.

* statistics: `libreco/utils/similarities.py:206-240`;
* similarity: `utils/_similarities.pyx:73-143` (compute_cosine; pearson :177-250, jaccard :284-343) with the symmetric sum
  of `similarities.py:96-99` (scipy drops the entries that are exactly 0): a dense f32 accumulator per row x1, updated
  once per y in ascending y with separate f32 multiply and add;
* top-k: `bases/cf_base.py:340-355`; recommend: `algorithms/item_cf.py:117-149`, `user_cf.py:117-147`,
  `cf_base.py:310-338`; predict: `item_cf.py:70-115`, `user_cf.py:70-115`, `cf_base.py:212-250`;
* serving: `libserving/serialization/knn.py:36-46`.
"""
from collections import defaultdict
from operator import itemgetter

import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.linalg import norm as spnorm


def stat_norm(x):
    return spnorm(x, axis=1).astype(np.float32)


def stat_mean(x):
    s = np.asarray(x.sum(axis=1)).flatten()
    with np.errstate(divide="ignore", invalid="ignore"):
        return (s / np.diff(x.indptr)).astype(np.float32)


def stat_centred_norm(x):
    data = x.data.copy()
    for r in range(x.shape[0]):
        sl = slice(x.indptr[r], x.indptr[r + 1])
        if sl.stop > sl.start:
            data[sl] -= np.mean(data[sl])
    return stat_norm(csr_matrix((data, x.indices.copy(), x.indptr.copy()), shape=x.shape))


def stat_count(x):
    return np.diff(x.indptr)


def similarity_rows(x, sim_type, min_common=1, rows=None):
    """row -> (cols ascending, f32 values) of the full symmetric similarity of the rows of the CSR x (f32, sorted)."""
    x = x.tocsr().astype(np.float32)
    x.sort_indices()
    y = x.T.tocsr()
    y.sort_indices()
    n_x = x.shape[0]
    if sim_type == "cosine":
        norm = stat_norm(x)
    elif sim_type == "pearson":
        mean = stat_mean(x)
        norm = stat_centred_norm(x)
    else:
        cnt = stat_count(x).astype(np.int64)
    yval = y.data
    if sim_type == "pearson":
        yval = (y.data - mean[y.indices]).astype(np.float32)
    mc = max(int(min_common), 1)
    out = {}
    for x1 in (range(n_x) if rows is None else rows):
        prods = np.zeros(n_x, dtype=np.float32)
        freq = np.zeros(n_x, dtype=np.int64)
        for k in range(x.indptr[x1], x.indptr[x1 + 1]):
            yy = x.indices[k]
            a = x.data[k] if sim_type != "pearson" else np.float32(x.data[k] - mean[x1])
            sl = slice(y.indptr[yy], y.indptr[yy + 1])
            cols = y.indices[sl]
            keep = cols != x1
            cols = cols[keep]
            freq[cols] += 1
            if sim_type != "jaccard":
                prods[cols] = prods[cols] + np.float32(a) * yval[sl][keep]
        cand = np.flatnonzero(freq >= mc)
        if sim_type == "jaccard":
            inter = freq[cand].astype(np.float32)
            val = inter / ((cnt[x1] + cnt[cand]).astype(np.float32) - inter)
        else:
            p = prods[cand]
            n1, n2 = norm[x1], norm[cand]
            with np.errstate(divide="ignore", invalid="ignore"):
                val = np.where((p == 0) | (n1 == 0) | (n2 == 0), np.float32(0), p / (n1 * n2)).astype(np.float32)
        nz = val != 0
        out[x1] = (cand[nz].astype(np.int32), val[nz].astype(np.float32))
    return out


def similarity(x, sim_type, min_common=1):
    """The similarity as a scipy CSR (int32 columns ascending, f32 values)."""
    rows = similarity_rows(x, sim_type, min_common)
    n = x.shape[0]
    ptr = np.zeros(n + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(rows[r][0]) for r in range(n)])
    col = np.concatenate([rows[r][0] for r in range(n)]) if n else np.zeros(0, np.int32)
    val = np.concatenate([rows[r][1] for r in range(n)]) if n else np.zeros(0, np.float32)
    return csr_matrix((val, col, ptr), shape=(n, n))


def topk(sim, k):
    """`get_top_k_sims` of every row: None for an empty row, else [(id, sim)] by sim descending, stable."""
    out = {}
    for r in range(sim.shape[0]):
        sl = slice(sim.indptr[r], sim.indptr[r + 1])
        if sl.stop == sl.start:
            out[r] = None
            continue
        pairs = sorted(zip(sim.indices[sl].tolist(), sim.data[sl].tolist()), key=itemgetter(1), reverse=True)
        out[r] = pairs[:k]
    return out


def recommend_scores(cf_type, user_inter, tk, u):
    """item -> f32 score of user u in the reference's accumulation order, or None when nothing is touched."""
    scores = defaultdict(lambda: 0.0)
    sl = slice(user_inter.indptr[u], user_inter.indptr[u + 1])
    if cf_type == "item_cf":
        for i, lab in zip(user_inter.indices[sl], user_inter.data[sl]):
            for j, s in tk[i] or []:
                scores[j] += s * lab
    else:
        for v, s in tk[u] or []:
            vs = slice(user_inter.indptr[v], user_inter.indptr[v + 1])
            for i, lab in zip(user_inter.indices[vs], user_inter.data[vs]):
                scores[i] += s * lab
    return dict(scores) if scores else None


def recommend(cf_type, user_inter, tk, u, n_rec, consumed, filter_consumed):
    """(kind, ids, scores): kind 0 ranked by (score descending, id ascending), 1 nothing touched, 2 all consumed."""
    sc = recommend_scores(cf_type, user_inter, tk, u)
    if sc is None:
        return 1, None, None
    items = [i for i in sc if not (filter_consumed and i in set(consumed))]
    if not items:
        return 2, None, None
    items.sort(key=lambda i: (-float(sc[i]), i))
    items = items[:n_rec]
    return 0, np.array(items), np.array([sc[i] for i in items], dtype=np.float32)


def predict(sim, inter, srow, irow, k_sim, task, lower, upper, default_pred):
    """`compute_pred` on the first k_sim entries of sim row srow intersected with interaction row irow."""
    sl = slice(sim.indptr[srow], sim.indptr[srow + 1])
    sims_i, sims_v = sim.indices[sl][:k_sim], sim.data[sl][:k_sim]
    il = slice(inter.indptr[irow], inter.indptr[irow + 1])
    common, a, b = np.intersect1d(sims_i, inter.indices[il], assume_unique=True, return_indices=True)
    cs, cl = sims_v[a], inter.data[il][b]
    if common.size == 0 or np.all(cs <= 0.0):
        return default_pred, True
    pairs = sorted(zip(cl, cs), key=itemgetter(1), reverse=True)      # cf_base.py:228-238: by sim descending, stable
    pairs = [p for p in pairs if p[1] > 0][:k_sim]
    lab, s = np.array([p[0] for p in pairs], dtype=np.float32), np.array([p[1] for p in pairs], dtype=np.float32)
    if task == "rating":
        w = s / np.sum(s)
        return np.float32(np.clip(np.average(lab, weights=w), lower, upper)), False
    return np.float32(np.mean(s)), False


def save_sim_matrix(sim, k):
    """The content of `sim.json` (`knn.py:36-46`) with string keys, as json reads it back."""
    out = {}
    for i in range(sim.shape[0]):
        sl = slice(sim.indptr[i], sim.indptr[i + 1])
        pairs = sorted(zip(sim.indices[sl].tolist(), sim.data[sl].tolist()), key=lambda t: -t[1])[:k]
        out[str(i)] = [[a, b] for a, b in pairs]
    return out
