"""A numpy restatement of the reference's Swing semantics, the yardstick of tests/test_swing_*.py.

* weights and pair term: `rust/src/graph.rs:210-213` (w_u = 1 / sqrt(|I_u|)) and `:185-186`
  (w_u * w_v * (alpha + |I_u ^ I_v| - 1).recip());
* scores: `graph.rs:143-198` (compute_single_swing: per target item every pair u < v of its users in ascending order, the
  term added to every common item but the target; rows start from the previous scores, `:124-136` init_item_scores; rows
  of items without users keep their previous scores, `:161-167`; zeros are dropped, `:138-141`);
* predict: `rust/src/swing.rs:153-185` (the first min(top_k, len) entries of the row, those in the user's items, the mean
  of their scores, `inference.rs:62-65`); recommend: `swing.rs:187-240` with `inference.rs:72-97`;
* merge of the interactions after a retrain: `rust/src/sparse.rs` CsrMatrix::merge (union, new labels win).
Ties are ordered by ascending item id here (the reference's unstable sorts leave them arbitrary).
"""
import numpy as np
import scipy.sparse as sp


def _pattern(A):
    A = sp.csr_matrix(A)
    B = sp.csr_matrix((np.ones(A.nnz), A.indices.copy(), A.indptr.copy()), shape=A.shape)
    B.sort_indices()
    return B


def pair_weights64(A, alpha):
    """F[u][v] = w_u w_v / (alpha + c_uv - 1) for u != v that share an item, fp64, as a CSR."""
    B = _pattern(A)
    C = (B @ B.T).tocoo()
    deg = np.diff(B.indptr).astype(np.float64)
    with np.errstate(divide="ignore"):
        w = 1.0 / np.sqrt(deg)
    keep = C.row != C.col
    r, c, n = C.row[keep], C.col[keep], C.data[keep]
    return sp.csr_matrix((w[r] * w[c] / (alpha + n - 1.0), (r, c)), shape=C.shape)


def scores64(A, alpha, prev=None):
    """The Swing scores in fp64 as a CSR with ascending columns and no stored zeros:
    S[i] = 1/2 colsum(B_i o (F[U_i, U_i] B_i)) with B_i the rows U_i of the pattern, plus `prev`."""
    B = _pattern(A)
    Bt = B.T.tocsr()
    Bt.sort_indices()
    F = pair_weights64(A, alpha)
    n_items = B.shape[1]
    rows, cols, vals = [], [], []
    for i in range(n_items):
        U = Bt.indices[Bt.indptr[i]: Bt.indptr[i + 1]]
        if len(U) < 2:
            continue
        Bi = B[U]
        s = 0.5 * np.asarray(Bi.multiply(F[U][:, U] @ Bi).sum(axis=0)).ravel()
        s[i] = 0.0
        nz = np.flatnonzero(s)
        rows.append(np.full(len(nz), i))
        cols.append(nz)
        vals.append(s[nz])
    cat = lambda x, dt: np.concatenate(x).astype(dt) if x else np.zeros(0, dtype=dt)  # noqa: E731
    S = sp.csr_matrix((cat(vals, np.float64), (cat(rows, np.int64), cat(cols, np.int64))), shape=(n_items, n_items))
    if prev is not None:
        P = sp.csr_matrix(prev, dtype=np.float64)
        P.resize((n_items, n_items))
        S = (S + P).tocsr()
    S.eliminate_zeros()
    S.sort_indices()
    return S


def pairs(A):
    """P[i][j]: the number of user pairs that contribute to entry (i, j), C(|U_i ^ U_j|, 2), as a CSR."""
    B = _pattern(A)
    T = (B.T @ B).tocoo()
    keep = T.row != T.col
    t = T.data[keep]
    P = sp.csr_matrix((t * (t - 1.0) / 2.0, (T.row[keep], T.col[keep])), shape=T.shape)
    P.eliminate_zeros()
    P.sort_indices()
    return P


def scores32_ref(A, alpha, prev=None):
    """The reference's own order in f32, with loops (small inputs): a dense [n_items, n_items] f32 array."""
    B = _pattern(A)
    Bt = B.T.tocsr()
    Bt.sort_indices()
    n_users, n_items = B.shape
    f = np.float32
    items = [B.indices[B.indptr[u]: B.indptr[u + 1]] for u in range(n_users)]
    w = [f(1.0) / np.sqrt(f(len(it))) if len(it) else f(0) for it in items]
    S = np.zeros((n_items, n_items), dtype=f)
    if prev is not None:
        P = np.asarray(sp.csr_matrix(prev).todense(), dtype=f)
        S[: P.shape[0], : P.shape[1]] = P
    for i in range(n_items):
        U = Bt.indices[Bt.indptr[i]: Bt.indptr[i + 1]]
        for a in range(len(U)):
            for b in range(a + 1, len(U)):
                u, v = U[a], U[b]
                common = np.intersect1d(items[u], items[v])
                score = f(f(w[u] * w[v]) * (f(1.0) / f(f(alpha) + f(len(common) - 1))))
                for c in common:
                    if c != i:
                        S[i, c] = f(S[i, c] + score)
    return S


def topk(S, k):
    """row -> [(item, score)] of the first min(k, len) entries by (score descending, id ascending)."""
    S = sp.csr_matrix(S)
    out = {}
    for i in range(S.shape[0]):
        c, v = S.indices[S.indptr[i]: S.indptr[i + 1]], S.data[S.indptr[i]: S.indptr[i + 1]]
        order = np.lexsort((c, -v))[:k]
        out[i] = [(int(c[o]), v[o]) for o in order]
    return out


def predict(S, A, u, i, top_k, default_pred=0.0):
    """The mean (f32) of the scores of row i's top_k entries whose item is one of u's; default_pred when there is none or
    an id is the out-of-range one."""
    A, S = sp.csr_matrix(A), sp.csr_matrix(S)
    if u >= A.shape[0] or i >= S.shape[0]:
        return np.float32(default_pred)
    mine = set(A.indices[A.indptr[u]: A.indptr[u + 1]].tolist())
    s = [np.float64(v) for j, v in topk(S[i], top_k)[0] if j in mine]
    if not s:
        return np.float32(default_pred)
    return np.float32(sum(s) / len(s))


def recommend(S, A, consumed, u, n_rec, top_k, filter_consumed=True, tk=None):
    """(ids by (score descending, id ascending) cut to n_rec, shortfall to pad with popular items, all candidates).
    Scores are f32 products summed sequentially in f32 over u's items in ascending id and each row's top-k in order."""
    A = sp.csr_matrix(A)
    tk = topk(S, top_k) if tk is None else tk
    f = np.float32
    acc = {}
    seen = set(consumed) if filter_consumed else set()
    for i, label in zip(A.indices[A.indptr[u]: A.indptr[u + 1]], A.data[A.indptr[u]: A.indptr[u + 1]]):
        for j, s in tk.get(int(i), []):
            if j in seen:
                continue
            acc[j] = f(acc.get(j, f(0)) + f(f(s) * f(label)))
    ranked = sorted(acc, key=lambda j: (-acc[j], j))
    return ranked[:n_rec], n_rec - min(n_rec, len(ranked)), ranked


def merge(old, new):
    """The union of two interaction CSRs, the labels of `new` winning, shaped to hold both."""
    old, new = sp.csr_matrix(old), sp.csr_matrix(new)
    shape = (max(old.shape[0], new.shape[0]), max(old.shape[1], new.shape[1]))
    d = {}
    for m in (old, new):
        c = m.tocoo()
        for r, k, v in zip(c.row.tolist(), c.col.tolist(), c.data.tolist()):
            d[(r, k)] = v
    keys = sorted(d)
    out = sp.csr_matrix(([d[k] for k in keys], ([k[0] for k in keys], [k[1] for k in keys])), shape=shape,
                        dtype=np.float32)
    out.sort_indices()
    return out
