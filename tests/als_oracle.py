"""fp64 numpy restatement of one ALS half-sweep as `libreco/algorithms/_als.pyx` writes it (test oracle, no GPU):
`_least_squares` (per-row Cholesky `posv`, failure on a non-positive pivot) and `_least_squares_cg` (cg_steps CG iterations
from the current row, `continue` when r.r < 1e-10, `break` when the new r.r < 1e-10; the explicit branch on
A = reg I + sum y y^T).  `val` is the confidence alpha r + 1 (implicit) or the rating (explicit)."""
import numpy as np


def gram0(Y, reg, implicit):
    K = Y.shape[1]
    Y = np.asarray(Y, dtype=np.float64)
    return (Y.T @ Y if implicit else np.zeros((K, K))) + reg * np.eye(K)


def row_system(indptr, indices, val, Y, G0, m, implicit):
    s, e = int(indptr[m]), int(indptr[m + 1])
    Ym = np.asarray(Y, dtype=np.float64)[indices[s:e]]
    v = np.asarray(val[s:e], dtype=np.float64)
    w = v - 1.0 if implicit else np.ones_like(v)
    return G0 + (Ym * w[:, None]).T @ Ym, Ym.T @ v


def half_sweep(indptr, indices, val, X, Y, reg, implicit, use_cg, cg_steps=3, rows=None):
    """Returns the updated rows (all, or `rows`) as fp64; raises ValueError like the reference's posv failure."""
    X = np.array(X, dtype=np.float64)
    G0 = gram0(Y, reg, implicit)
    for m in (range(X.shape[0]) if rows is None else rows):
        A, b = row_system(indptr, indices, val, Y, G0, m, implicit)
        if not use_cg:
            try:
                L = np.linalg.cholesky(A)
            except np.linalg.LinAlgError:
                raise ValueError(f"posv failed on row {m}. Try increasing the regularization parameter.") from None
            X[m] = np.linalg.solve(L.T, np.linalg.solve(L, b))
            continue
        x = X[m].copy()
        r = b - A @ x
        p = r.copy()
        rsold = r @ r
        if rsold < 1e-10:
            continue
        for _ in range(cg_steps):
            Ap = A @ p
            ak = rsold / (p @ Ap)
            x += ak * p
            r -= ak * Ap
            rsnew = r @ r
            if rsnew < 1e-10:
                break
            p = r + (rsnew / rsold) * p
            rsold = rsnew
        X[m] = x
    return X if rows is None else X[list(rows)]


def objective(indptr, indices, val, X, Y, reg, implicit):
    """The loss one exact half-sweep minimises over X (and the next over Y): sum_(m,i) w (p - x.y)^2 + reg (|X|^2 + |Y|^2),
    over all pairs with confidence c (p = 1) for implicit, the observed ratings for explicit."""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    tot = reg * ((X * X).sum() + (Y * Y).sum())
    if implicit:
        tot += ((X @ Y.T) ** 2).sum()          # every pair at confidence 1, preference 0
    for m in range(X.shape[0]):
        s, e = int(indptr[m]), int(indptr[m + 1])
        pred = Y[indices[s:e]] @ X[m]
        v = np.asarray(val[s:e], dtype=np.float64)
        if implicit:
            tot += (v * (1 - pred) ** 2 - pred ** 2).sum()
        else:
            tot += ((v - pred) ** 2).sum()
    return tot


def random_csr(rng, rows, cols, degrees, values=(1.0, 5.0)):
    """CSR with the given row degrees (distinct columns per row), values uniform in `values`."""
    indptr = np.zeros(rows + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(degrees)
    indices = np.concatenate([rng.choice(cols, d, replace=False) if d else np.zeros(0, np.int64) for d in degrees])
    val = rng.uniform(values[0], values[1], int(indptr[-1])).astype(np.float32)
    return indptr, indices.astype(np.int32), val
