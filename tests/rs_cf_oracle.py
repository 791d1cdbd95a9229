"""A plain numpy f32 restatement of the reference's incremental neighbourhood engine (`rust/src/similarities.rs`,
`incremental.rs`, `item_cf.rs`, `user_cf.rs`, `inference.rs`), dictionary-based like the Rust: checker only.

`x` is the side that gets similarities (items for RsItemCF, users for RsUserCF) and `y` the other side.  The engine keeps
`sumsq` (f32 per x), `cum` (key -> [x1, x2, prod, cnt] for every pair with a common y) and `sim` (x -> {neighbour: cosine},
the pairs whose cumulative count has reached `min_common`).  `fit` is `update` on the empty engine.

`alias_keys=True` keys `cum` the way the reference does, by `x1 * n_x + x2` with the n_x of the call: after the id space has
grown, a pair's key can name another pair's entry, and the sums are taken from and added to that entry.  `False` keys by the
pair itself, which is what the package does.  `last` holds the cosine of every pair's last touch whatever its count (the
package's state carries it for pairs below `min_common` too); it is meaningful with pair keys only.

Every sum is a sequential f32 chain in the reference's order: ascending y for a pair's products, ascending column for a
row's squares, list order for a prediction.  Ties in a neighbour list are broken by ascending id (the reference's unstable
sort leaves them arbitrary)."""
import numpy as np
import scipy.sparse as sp

F = np.float32


def _csr(m):
    m = sp.csr_matrix(m, dtype=np.float32)
    m.sort_indices()
    return m


def row_sumsq(x, n):
    """`compute_sum_squares`: fold(0.0, |ss, d| ss + d * d) over every row in ascending column order."""
    x = _csr(x)
    out = np.zeros(n, dtype=np.float32)
    for r in range(min(n, x.shape[0])):
        s = F(0.0)
        for d in x.data[x.indptr[r]:x.indptr[r + 1]]:
            s = F(s + F(d * d))
        out[r] = s
    return out


def delta_pairs(y_major):
    """(x1, x2, prod, cnt) arrays, x1 < x2, of every pair that shares a row of the y-major CSR: prod the f32 sum over
    ascending y of the f32 products (from 0), cnt the number of shared y.  `update_cosine` / `invert_cosine` without the
    normalisation, vectorised: the triples are grouped by pair in y order and every group is folded one term at a time."""
    y = _csr(y_major)
    a, b, p = [], [], []
    for r in range(y.shape[0]):
        sl = slice(y.indptr[r], y.indptr[r + 1])
        c, d = y.indices[sl], y.data[sl]
        if len(c) < 2:
            continue
        i, j = np.triu_indices(len(c), 1)
        a.append(c[i].astype(np.int64))
        b.append(c[j].astype(np.int64))
        p.append((d[i] * d[j]).astype(np.float32))
    if not a:
        z = np.zeros(0, dtype=np.int64)
        return z, z, np.zeros(0, dtype=np.float32), z
    a, b, p = np.concatenate(a), np.concatenate(b), np.concatenate(p)
    n = int(max(a.max(), b.max())) + 1
    order = np.argsort(a * n + b, kind="stable")           # stable: the y order inside a pair is kept
    key = (a * n + b)[order]
    p = p[order]
    start = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    cnt = np.diff(np.r_[start, len(key)])
    acc = np.zeros(len(start), dtype=np.float32)
    for t in range(int(cnt.max())):
        live = cnt > t
        acc[live] = (acc[live] + p[start[live] + t]).astype(np.float32)
    return key[start] // n, key[start] % n, acc, cnt


def cosine(prod, s1, s2):
    """`compute_cosine` / `accumulate_cosine`."""
    if prod == 0.0 or s1 == 0.0 or s2 == 0.0:
        return F(0.0)
    return F(F(prod) / F(np.sqrt(F(s1)) * np.sqrt(F(s2))))


class Engine:
    def __init__(self, min_common=1, alias_keys=False):
        self.min_common = max(int(min_common), 1)
        self.alias_keys = alias_keys
        self.n_x = 0
        self.sumsq = np.zeros(0, dtype=np.float32)
        self.cum = {}
        self.sim = {}
        self.last = {}
        self.touched = set()      # the pairs of the latest update

    def update(self, x_major, n_x):
        """`update_similarities` with the new interactions (x-major CSR; rows beyond its own are empty) and the new n_x."""
        x = _csr(x_major)
        assert x.shape[0] <= n_x and n_x >= self.n_x
        add = row_sumsq(x, n_x)
        old = np.zeros(n_x, dtype=np.float32)
        old[: self.n_x] = self.sumsq
        rows = np.flatnonzero(np.diff(x.indptr) > 0)       # `get_row` is None for an empty row: it is left alone
        old[rows] = (old[rows] + add[rows]).astype(np.float32)
        self.sumsq, self.n_x = old, n_x
        self.touched = set()
        x1s, x2s, prods, cnts = delta_pairs(x.T.tocsr())
        for x1, x2, prod, cnt in zip(x1s.tolist(), x2s.tolist(), prods, cnts.tolist()):
            key = x1 * n_x + x2 if self.alias_keys else (x1, x2)
            e = self.cum.get(key)
            if e is None:
                e = self.cum[key] = [x1, x2, F(prod), cnt]
            else:
                e[2] = F(e[2] + prod)
                e[3] += cnt
            c = cosine(e[2], self.sumsq[x1], self.sumsq[x2])
            self.last[(x1, x2)] = c
            self.touched.add((x1, x2))
            if e[3] >= self.min_common:
                self.sim.setdefault(x1, {})[x2] = c
                self.sim.setdefault(x2, {})[x1] = c
        return self

    fit = update

    # ---- views ---------------------------------------------------------------------------------------------------------
    def neighbours(self, x, k=None):
        """[(id, sim)] of row x by (sim descending, id ascending), cut to k."""
        row = sorted(self.sim.get(x, {}).items(), key=lambda t: (-float(t[1]), t[0]))
        return row if k is None else row[:k]

    def neighbour_ids(self, x, k=None):
        return [i for i, _ in self.neighbours(x, k)]

    def state(self):
        """(rowptr int64, col int32, prod f32, cnt int32, sim f32) of the symmetric state CSR (pair keys only)."""
        assert not self.alias_keys
        rows = [[] for _ in range(self.n_x)]
        for (x1, x2), (_, _, prod, cnt) in self.cum.items():
            c = self.last[(x1, x2)]
            rows[x1].append((x2, prod, cnt, c))
            rows[x2].append((x1, prod, cnt, c))
        ptr = np.zeros(self.n_x + 1, dtype=np.int64)
        flat = []
        for r, row in enumerate(rows):
            row.sort(key=lambda t: t[0])
            flat.extend(row)
            ptr[r + 1] = len(flat)
        col = np.array([t[0] for t in flat], dtype=np.int32)
        prod = np.array([t[1] for t in flat], dtype=np.float32)
        cnt = np.array([t[2] for t in flat], dtype=np.int32)
        sim = np.array([t[3] for t in flat], dtype=np.float32)
        return ptr, col, prod, cnt, sim

    def num_sim_elements(self):
        return sum(len(v) for v in self.sim.values())


def symmetric_csr(n_x, x1, x2, *values):
    """The symmetric CSR (rowptr int64, col int32 ascending, one array per value) of the pairs (x1, x2) and (x2, x1)."""
    rows, cols = np.concatenate([x1, x2]).astype(np.int64), np.concatenate([x2, x1]).astype(np.int64)
    order = np.argsort(rows * max(n_x, 1) + cols, kind="stable")
    ptr = np.zeros(n_x + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(np.bincount(rows, minlength=n_x))
    return (ptr, cols[order].astype(np.int32), *(np.concatenate([v, v])[order] for v in values))


def cosines(prod, s1, s2):
    """`cosine` on arrays."""
    prod, s1, s2 = (np.asarray(a, dtype=np.float32) for a in (prod, s1, s2))
    with np.errstate(divide="ignore", invalid="ignore"):
        c = (prod / (np.sqrt(s1) * np.sqrt(s2)).astype(np.float32)).astype(np.float32)
    return np.where((prod == 0) | (s1 == 0) | (s2 == 0), np.float32(0.0), c).astype(np.float32)


class ArrayEngine:
    """`Engine` with pair keys, on sorted arrays instead of dictionaries: the same values (tests/test_rs_cf_cpu.py compares
    the two), fast enough for the sample file.  A pair is the int64 key x1 << 32 | x2 with x1 < x2."""

    def __init__(self, min_common=1):
        self.min_common = max(int(min_common), 1)
        self.n_x = 0
        self.sumsq = np.zeros(0, dtype=np.float32)
        self.key = np.zeros(0, dtype=np.int64)
        self.prod = np.zeros(0, dtype=np.float32)
        self.cnt = np.zeros(0, dtype=np.int64)
        self.last = np.zeros(0, dtype=np.float32)
        self.touched = np.zeros(0, dtype=bool)
        self._vis = None

    def update(self, x_major, n_x):
        x = _csr(x_major)
        assert x.shape[0] <= n_x and n_x >= self.n_x
        add = row_sumsq(x, n_x)
        old = np.zeros(n_x, dtype=np.float32)
        old[: self.n_x] = self.sumsq
        self.sumsq, self.n_x = (old + add).astype(np.float32), n_x      # adding 0 leaves an untouched row's bits alone
        x1, x2, dprod, dcnt = delta_pairs(x.T.tocsr())
        dkey = (x1 << 32) | x2
        pos = np.searchsorted(self.key, dkey)
        found = np.zeros(len(dkey), dtype=bool)
        inside = pos < len(self.key)
        found[inside] = self.key[pos[inside]] == dkey[inside]
        self.prod[pos[found]] = (self.prod[pos[found]] + dprod[found]).astype(np.float32)
        self.cnt[pos[found]] += dcnt[found]
        touched = np.zeros(len(self.key), dtype=bool)
        touched[pos[found]] = True
        key = np.concatenate([self.key, dkey[~found]])
        order = np.argsort(key, kind="stable")
        self.key = key[order]
        self.prod = np.concatenate([self.prod, dprod[~found]])[order]
        self.cnt = np.concatenate([self.cnt, dcnt[~found]])[order]
        self.last = np.concatenate([self.last, np.zeros((~found).sum(), dtype=np.float32)])[order]
        self.touched = np.concatenate([touched, np.ones((~found).sum(), dtype=bool)])[order]
        a, b = self.key[self.touched] >> 32, self.key[self.touched] & 0xFFFFFFFF
        self.last[self.touched] = cosines(self.prod[self.touched], self.sumsq[a], self.sumsq[b])
        self._vis = None
        return self

    def state(self):
        return symmetric_csr(self.n_x, self.key >> 32, self.key & 0xFFFFFFFF, self.prod, self.cnt.astype(np.int32), self.last)

    def neighbours(self, x, k=None):
        if self._vis is None:
            self._vis = visible(self.state(), self.min_common)
        ptr, col, sim = self._vis
        row = sorted(zip(col[ptr[x]:ptr[x + 1]].tolist(), sim[ptr[x]:ptr[x + 1]]), key=lambda t: (-float(t[1]), t[0]))
        return row if k is None else row[:k]

    def neighbour_ids(self, x, k=None):
        return [i for i, _ in self.neighbours(x, k)]

    def num_sim_elements(self):
        return 2 * int((self.cnt >= self.min_common).sum())


def merge_rows(old, delta, sumsq):
    """The merge-and-refresh of the package's state on arbitrary CSRs, row by row with dictionaries: `old` = (ptr, col,
    prod, cnt, sim) with at most as many rows as `delta` = (ptr, col, prod, cnt).  A column of the delta gets
    prod = old + delta (the delta alone if new), cnt = old + delta and a fresh cosine; every other column is copied."""
    o_ptr, o_col, o_prod, o_cnt, o_sim = old
    d_ptr, d_col, d_prod, d_cnt = delta
    n_x = len(d_ptr) - 1
    ptr = np.zeros(n_x + 1, dtype=np.int64)
    col, prod, cnt, sim = [], [], [], []
    for r in range(n_x):
        row = {}
        if r < len(o_ptr) - 1:
            for e in range(o_ptr[r], o_ptr[r + 1]):
                row[int(o_col[e])] = (F(o_prod[e]), int(o_cnt[e]), F(o_sim[e]))
        for j in range(d_ptr[r], d_ptr[r + 1]):
            c = int(d_col[j])
            p, n = F(d_prod[j]), int(d_cnt[j])
            if c in row:
                p, n = F(row[c][0] + p), row[c][1] + n
            row[c] = (p, n, cosine(p, sumsq[r], sumsq[c]))
        for c in sorted(row):
            col.append(c)
            prod.append(row[c][0])
            cnt.append(row[c][1])
            sim.append(row[c][2])
        ptr[r + 1] = len(col)
    return (ptr, np.array(col, dtype=np.int32), np.array(prod, dtype=np.float32), np.array(cnt, dtype=np.int32),
            np.array(sim, dtype=np.float32))


def visible(state, min_common):
    """(rowptr, col, sim) of the entries with cnt >= min_common."""
    ptr, col, _, cnt, sim = state
    keep = cnt >= max(int(min_common), 1)
    below = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    return below[ptr], col[keep], sim[keep]


def top_lists(ptr, col, sim, k):
    """Every row's first k entries by (sim descending with -0 == +0, id ascending), as [(id, sim)]."""
    out = []
    for r in range(len(ptr) - 1):
        row = list(zip(col[ptr[r]:ptr[r + 1]].tolist(), sim[ptr[r]:ptr[r + 1]]))
        row.sort(key=lambda t: (-float(t[1]), t[0]))
        out.append(row[:k])
    return out


def predict_list(nbs, other_cols, other_vals, k_sim, task, default_pred):
    """`predict` of item_cf.rs / user_cf.rs on one pair: `nbs` the row's neighbour list [(id, sim)] in list order, cut to
    k_sim BEFORE it is intersected with the other side's interaction row; every hit is used, in list order (the reference
    pops a max-heap by sim).  Returns (pred f32, none)."""
    labels = dict(zip(np.asarray(other_cols).tolist(), np.asarray(other_vals, dtype=np.float32)))
    hits = [(F(s), labels[i]) for i, s in nbs[:k_sim] if i in labels]
    if not hits:
        return F(default_pred), True
    S = F(0.0)
    for s, _ in hits:
        S = F(S + s)
    if task == "ranking":
        return F(S / F(len(hits))), False
    out = F(0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        for s, l in hits:
            out = F(out + F(F(l * s) / S))
    return out, False
