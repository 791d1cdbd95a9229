"""A numpy restatement of GraphSage's device sampling and tower (csrc/sage.hip).

The integer parts (neighbours, pairs, start nodes, negatives, dropout flags) are exact integer arithmetic over uint64: the device
must give the same integers.  The tower's forward and backward exist in an f32 and an f64 variant; tests/test_graphsage_cpu.py
shows that the f64 variant equals the reference module's arithmetic restated with torch under autograd."""
import numpy as np

from .wavenet_oracle import delta_bound, max_diff

F32 = np.float32
U64 = np.uint64
GOLD = U64(0x9E3779B97F4A7C15)
NEIGHBOR, WALK, START, NEGATIVE, DROPOUT = 16, 17, 18, 19, 20
TOLERANCE, NEG_TRIES = 5, 10


def mix64(z):
    z = np.asarray(z, dtype=U64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def H(seed, stream, a, b):
    """H(seed, stream, a, b) of DESIGN §7.9, elementwise over uint64 arrays."""
    with np.errstate(over="ignore"):
        z = mix64(np.asarray(seed, dtype=U64) + GOLD * U64(stream))
        z = mix64(z + GOLD * (np.asarray(a, dtype=U64) + U64(1)))
        return mix64(z + GOLD * (np.asarray(b, dtype=U64) + U64(1)))


def below(h, length):
    return (((np.asarray(h, dtype=U64) >> U64(32)) * np.asarray(length, dtype=U64)) >> U64(32)).astype(np.int64)


class Graph:
    def __init__(self, user_lists, n_items):
        """`user_lists`: the item list of every user, duplicates kept; an item's consumers are listed in (user, position) order."""
        self.n_users, self.n_items = len(user_lists), n_items
        self.user_lists = [list(map(int, x)) for x in user_lists]
        self.item_lists = [[] for _ in range(n_items)]
        for u, lst in enumerate(self.user_lists):
            for i in lst:
                self.item_lists[i].append(u)
        self.user_ptr, self.user_idx = self._csr(self.user_lists)
        self.item_ptr, self.item_idx = self._csr(self.item_lists)

    @staticmethod
    def _csr(lists):
        ptr = np.zeros(len(lists) + 1, dtype=np.int64)
        ptr[1:] = np.cumsum([len(x) for x in lists])
        idx = np.asarray([i for x in lists for i in x], dtype=np.int32)
        return ptr, idx

    def one_walk(self, items, seed, stream, a, b2):
        """item -> uniform consumer -> uniform item of the consumer, elementwise; an item nobody consumed returns itself."""
        items = np.asarray(items, dtype=np.int64)
        b2 = np.asarray(b2, dtype=U64)
        ok = (items >= 0) & (items < self.n_items)
        it = np.where(ok, items, 0)
        lo, hi = self.item_ptr[it], self.item_ptr[it + 1]
        ok &= hi > lo
        pick = lo + below(H(seed, stream, a, b2), np.maximum(hi - lo, 1))
        u = self.item_idx[np.where(ok, pick, 0)].astype(np.int64) if len(self.item_idx) else np.zeros_like(items)
        ulo, uhi = self.user_ptr[u], self.user_ptr[u + 1]
        ok &= uhi > ulo
        pick = ulo + below(H(seed, stream, a, b2 + U64(1)), np.maximum(uhi - ulo, 1))
        nxt = self.user_idx[np.where(ok, pick, 0)].astype(np.int64) if len(self.user_idx) else np.zeros_like(items)
        return np.where(ok, nxt, items).astype(np.int32)

    def no_neighbor(self, item):
        return all(len(self.user_lists[u]) <= 1 for u in self.item_lists[item]) if 0 <= item < self.n_items else True


def neighbors(g, nodes, nn, seed, step, level, first_only=False):
    """[n_nodes, nn] by the retry ladder of `bipartite_neighbors` (`first_only`: the attempt-0 draws alone)."""
    nodes = np.asarray(nodes, dtype=np.int32)
    n = len(nodes)
    idx = np.arange(n, dtype=U64)
    a = U64(step * 8 + level)
    out = np.zeros((n, nn), dtype=np.int32)
    for j in range(nn):
        def draw(attempt):
            return g.one_walk(nodes, seed, NEIGHBOR, a, ((idx * U64(16) + U64(j)) * U64(16) + U64(attempt)) * U64(2))

        def taken(x):
            return (out[:, :j] == x[:, None]).any(axis=1) if j else np.zeros(n, dtype=bool)

        x = draw(0)
        if not first_only:
            need = (x == nodes) | taken(x)
            success = ~need
            for t in range(1, TOLERANCE + 1):
                act = ~success
                d = draw(t)
                x = np.where(act, d, x)
                success = np.where(act, (d != nodes) & ~taken(d), success)
            for t in range(1, TOLERANCE + 1):
                act = ~success
                d = draw(TOLERANCE + t)
                x = np.where(act, d, x)
                success = np.where(act, d != nodes, success)
            x = np.where(~success, draw(2 * TOLERANCE + 1), x)
        out[:, j] = x
    return out


def pairs(g, starts, num_walks, walk_len, focus_start, seed, step):
    """(items, items_pos) of `pairs_from_random_walk`, in ascending (start, walk, step)."""
    starts = np.asarray(starts, dtype=np.int32)
    W = len(starts) * num_walks
    node = np.repeat(starts, num_walks)
    w = np.arange(W, dtype=U64)
    src = np.zeros((W, walk_len + 1), dtype=np.int32)
    dst = np.zeros((W, walk_len + 1), dtype=np.int32)
    on = np.zeros((W, walk_len + 1), dtype=bool)
    lone = np.asarray([g.no_neighbor(int(x)) for x in starts], dtype=bool)
    on[::num_walks, 0] = lone
    src[:, 0] = dst[:, 0] = node
    cur = node.copy()
    for s in range(walk_len):
        nxt = g.one_walk(cur, seed, WALK, U64(step), (w * U64(walk_len) + U64(s)) * U64(2))
        if focus_start:
            on[:, s + 1], src[:, s + 1] = nxt != node, node
        else:
            on[:, s + 1], src[:, s + 1] = nxt != cur, cur
        dst[:, s + 1] = nxt
        cur = nxt
    return src[on], dst[on]


def table_pick(cum, r):
    return np.minimum(np.searchsorted(cum, r, side="right"), len(cum) - 1).astype(np.int64)


def start_nodes(n, n_items, seed, step, cum=None):
    h = H(seed, START, U64(step), np.arange(n, dtype=U64))
    return (table_pick(cum, (h >> U64(32)).astype(np.int64)) if cum is not None else below(h, n_items)).astype(np.int32)


def negatives(items, items_pos, num_neg, n_items, mode, seed, step, cum=None, in_batch=None):
    pos = np.repeat(np.asarray(items_pos, dtype=np.int64), num_neg)
    it = np.repeat(np.asarray(items, dtype=np.int64), num_neg) if items is not None else np.full(len(pos), -1, dtype=np.int64)
    q = np.arange(len(pos), dtype=U64)
    tries = 1 if mode == "popular" else NEG_TRIES
    d = np.zeros(len(pos), dtype=np.int64)
    live = np.ones(len(pos), dtype=bool)
    for t in range(tries + 1):
        h = H(seed, NEGATIVE, U64(step), q * U64(16) + U64(t))
        x = table_pick(cum, (h >> U64(32)).astype(np.int64)) if mode == "popular" else below(h, n_items)
        d = np.where(live, x, d)
        invalid = in_batch[d] != 0 if mode == "out-batch" else (d == pos) | (d == it)
        live = live & invalid
    return d.astype(np.int32)


def dropout_keep(n_nodes, K, p, seed, step, layer, level, role):
    node = np.repeat(np.arange(n_nodes, dtype=U64), K)
    col = np.tile(np.arange(K, dtype=U64), n_nodes)
    b = (((node * U64(128) + col) * U64(2) + U64(role)) * U64(4) + U64(level)) * U64(4) + U64(layer)
    thr = U64(int(p * 4294967296.0))
    return ((H(seed, DROPOUT, U64(step), b) >> U64(32)) >= thr).reshape(n_nodes, K)


def unpopular_table(g):
    """The cumulative table (int64 [n_items], scaled to 2^32) of `pos_probs_from_frequency` (alpha 1e-3), an item nobody
    consumed weighing nothing."""
    w = np.zeros(g.n_items)
    for i in range(g.n_items):
        prob = len(set(g.item_lists[i])) / g.n_users
        if prob > 0:
            w[i] = (np.sqrt(prob / 1e-3) + 1) * (1e-3 / prob)
    cs = np.cumsum(w)
    cum = np.floor(cs / cs[-1] * 4294967296.0).astype(np.int64)
    cum[np.flatnonzero(w > 0)[-1]:] = 1 << 32
    return cum


# ---- the tower -------------------------------------------------------------------------------------------------------
def tree_nodes(L, n):
    return sum(n ** k for k in range(L + 1)) if L > 0 else 1


def level_slices(B, L, n):
    """Slice of level k inside the level-major node arrays."""
    out, off = [], 0
    for k in range(L + 1):
        cnt = B * (n ** k if L > 0 else 1)
        out.append(slice(off, off + cnt))
        off += cnt
    return out


def pack_params(p):
    parts = [p["proj_W"].T.reshape(-1), p["proj_b"]]
    for W, b in p["layers"]:
        parts += [W.T.reshape(-1), b]
    return np.concatenate(parts).astype(F32)


def unpack_params(flat, K, T, L):
    flat = np.asarray(flat)
    o = T * K * K
    out = {"proj_W": flat[:o].reshape(T * K, K).T, "proj_b": flat[o:o + K], "layers": []}
    o += K
    for _ in range(L):
        out["layers"].append((flat[o:o + 2 * K * K].reshape(2 * K, K).T, flat[o + 2 * K * K:o + 2 * K * K + K]))
        o += 2 * K * K + K
    assert o == len(flat)
    return out


def make_case(B, K, T, L, n, seed=0, V=53, p=0.0, dense_slots=()):
    """A seeded tower case: Zipf row ids, the scale of `dense_slots` random and 1 elsewhere."""
    rng = np.random.default_rng([seed, B, K, T, L, n])
    N = tree_nodes(L, n)
    rows = (rng.zipf(1.3, (B * N, T)) % V).astype(np.int32)
    scale = np.ones((B * N, T), dtype=F32)
    for t in dense_slots:
        scale[:, t] = rng.standard_normal(B * N).astype(F32)
    xav = lambda fo, fi, gain=1.0: (rng.uniform(-1, 1, (fo, fi)) * gain * np.sqrt(6.0 / (fi + fo))).astype(F32)  # noqa: E731
    params = {"proj_W": xav(K, T * K), "proj_b": (0.1 * rng.standard_normal(K)).astype(F32), "layers": []}
    for l in range(L):
        params["layers"].append((xav(K, 2 * K, 1.0 if l == L - 1 else np.sqrt(2.0)), (0.1 * rng.standard_normal(K)).astype(F32)))
    return dict(shape=(B, K, T, L, n), V=V, table=rng.standard_normal((V, K)).astype(F32), rows=rows, scale=scale, params=params,
                grepr=rng.standard_normal((B, K)).astype(F32), p=p, seed=1234 + seed, step=7)


def case_masks(c):
    """{(layer, level, role): keep [B n^level, K]} of a case's dropout (empty at p = 0)."""
    B, K, T, L, n = c["shape"]
    if not c["p"]:
        return {}
    out = {}
    for l in range(L):
        for k in range(L - l + 1):
            for role in (0, 1):
                out[(l, k, role)] = dropout_keep(B * n ** k, K, c["p"], c["seed"], c["step"], l, k, role)
    return out


def _drop(h, keep, inv_keep):
    return h if keep is None else np.where(keep, h * inv_keep, 0).astype(h.dtype)


def tower(c, variant, rows=None, relu=None, masks=None):
    """Forward and backward of a case in one arithmetic -> dict(repr, grow [B N, T, K], gparams (packed), relu (one flag array
    [B n^k, K] per (ReLU layer, level)), pre (the smallest |pre-activation| of a ReLU unit)).  `relu` forces the pattern."""
    dt = np.float64 if variant == "f64" else F32
    B, K, T, L, n = c["shape"]
    rows = c["rows"] if rows is None else rows
    masks = case_masks(c) if masks is None else masks
    inv_keep = dt(F32(1.0 / (1.0 - c["p"]))) if c["p"] else dt(1)
    inside = (rows >= 0) & (rows < c["V"])
    x = (c["table"].astype(dt)[np.where(inside, rows, 0)] * c["scale"].astype(dt)[:, :, None] * inside[:, :, None]).astype(dt)
    P = c["params"]
    Wp, bp = P["proj_W"].astype(dt), P["proj_b"].astype(dt)
    h0 = (x.reshape(len(rows), T * K) @ Wp.T + bp).astype(dt)
    sl = level_slices(B, L, n)
    h = [h0[s] for s in sl]
    saved, pattern, pre_min = [], {}, np.inf
    for l in range(L):
        W, b = P["layers"][l][0].astype(dt), P["layers"][l][1].astype(dt)
        nxt, zs_all = [], []
        for k in range(L - l):
            zs = _drop(h[k], masks.get((l, k, 0)), inv_keep)
            dn = _drop(h[k + 1], masks.get((l, k + 1, 1)), inv_keep)
            zn = (dn.reshape(len(zs), n, K).sum(axis=1, dtype=dt) / dt(n)).astype(dt)
            z = np.concatenate([zs, zn], axis=1)
            out = (z @ W.T + b).astype(dt)
            if l < L - 1:
                pre_min = min(pre_min, float(np.abs(out).min()))
                on = out > 0 if relu is None else relu[(l, k)]
                pattern[(l, k)] = on
                out = np.where(on, out, 0).astype(dt)
            nxt.append(out)
            zs_all.append(z)
        saved.append(zs_all)
        h = nxt
    rep = h[0]
    # backward
    g = [c["grepr"].astype(dt)]
    gparams = {"layers": [None] * L}
    for l in range(L - 1, -1, -1):
        W = P["layers"][l][0].astype(dt)
        gW, gb = np.zeros_like(W), np.zeros(K, dtype=dt)
        gin = [np.zeros((B * n ** k, K), dtype=dt) for k in range(L - l + 1)]
        for k in range(L - l):
            go = g[k]
            if l < L - 1:
                go = np.where(pattern[(l, k)], go, 0).astype(dt)
            gW += go.T @ saved[l][k]
            gb += go.sum(axis=0)
            gz = (go @ W).astype(dt)
            m0, m1 = masks.get((l, k, 0)), masks.get((l, k + 1, 1))
            own = gz[:, :K] * inv_keep if c["p"] else gz[:, :K]
            gin[k] = gin[k] + (own if m0 is None else np.where(m0, own, 0))
            nb = np.repeat(gz[:, K:] / dt(n), n, axis=0)
            nb = nb * inv_keep if c["p"] else nb
            gin[k + 1] = gin[k + 1] + (nb if m1 is None else np.where(m1, nb, 0))
        gparams["layers"][l] = (gW, gb)
        g = [a.astype(dt) for a in gin]
    g0 = np.zeros((len(rows), K), dtype=dt)
    for k, s in enumerate(sl):
        g0[s] = g[k]
    gparams["proj_W"] = g0.T @ x.reshape(len(rows), T * K)
    gparams["proj_b"] = g0.sum(axis=0)
    grow = ((g0 @ Wp).reshape(len(rows), T, K) * c["scale"].astype(dt)[:, :, None] * inside[:, :, None]).astype(dt)
    return dict(repr=rep, grow=grow, gparams=pack_params(gparams) if variant == "f32" else _pack64(gparams), relu=pattern,
                pre=pre_min)


def _pack64(p):
    parts = [p["proj_W"].T.reshape(-1), p["proj_b"]]
    for W, b in p["layers"]:
        parts += [W.T.reshape(-1), b]
    return np.concatenate(parts)


def device_relu(flags, c):
    """The device's relu_out (per ReLU layer a block [B, nodes with an output, K]) as {(layer, level): [B n^level, K]}."""
    B, K, T, L, n = c["shape"]
    flags = np.asarray(flags).astype(bool)
    out, at = {}, 0
    for l in range(L - 1):
        nout = tree_nodes(L - l - 1, n)
        blk = flags[at:at + B * nout].reshape(B, nout, K)
        at += B * nout
        off = 0
        for k in range(L - l):
            out[(l, k)] = blk[:, off:off + n ** k].reshape(B * n ** k, K)
            off += n ** k
    assert at == len(flags)
    return out


def delta_rule(got, want64, want32, layers, what):
    bound = delta_bound(want64, want32, layers)
    gap = max_diff(got, want64)
    print(f"SAGE-FIGURE {what} delta={max_diff(want32, want64):.3e} got={gap:.3e} bound={bound:.3e}")
    assert np.isfinite(np.asarray(got)).all() and gap <= bound, what
    return bound


def check_tower(got, c, what, rows=None):
    """`got` = dict(repr, grow, gparams, relu (the device's flags or None)).  repr against f64 by the delta rule; grow and every
    parameter gradient against the f64 backward run with the result's own ReLU pattern; grow at rows outside the table is 0."""
    B, K, T, L, n = c["shape"]
    rows = c["rows"] if rows is None else rows
    f64, f32 = tower(c, "f64", rows), tower(c, "f32", rows)
    delta_rule(got["repr"], f64["repr"], f32["repr"], L + 1, f"{what} repr")
    relu = device_relu(got["relu"], c) if got.get("relu") is not None and L > 1 else None
    b64, b32 = tower(c, "f64", rows, relu=relu), tower(c, "f32", rows, relu=relu)
    delta_rule(got["grow"], b64["grow"], b32["grow"], L + 1, f"{what} grow")
    inside = (rows >= 0) & (rows < c["V"])
    assert not np.asarray(got["grow"])[~inside].any(), f"{what} grow at rows outside the table"
    gp, g64, g32 = (unpack_params(x, K, T, L) for x in (got["gparams"], b64["gparams"], b32["gparams"]))
    delta_rule(gp["proj_W"], g64["proj_W"], g32["proj_W"], L + 1, f"{what} g proj_W")
    delta_rule(gp["proj_b"], g64["proj_b"], g32["proj_b"], L + 1, f"{what} g proj_b")
    for l in range(L):
        delta_rule(gp["layers"][l][0], g64["layers"][l][0], g32["layers"][l][0], L + 1, f"{what} gW[{l}]")
        delta_rule(gp["layers"][l][1], g64["layers"][l][1], g32["layers"][l][1], L + 1, f"{what} gb[{l}]")


def oracle_result(c, variant, rows=None):
    r = tower(c, variant, rows)
    return dict(repr=r["repr"].astype(F32), grow=r["grow"].astype(F32), gparams=r["gparams"].astype(F32), relu=None)


# ---- graphs ----------------------------------------------------------------------------------------------------------
def forced_graph():
    """Items: 0 only consumed by user 0, who holds nothing else; 1 and 2 share user 1 alone; 3 is a hub consumed by users 2 .. 5,
    who hold 3 and two of the items 4 .. 9 each; item 10 is consumed by nobody."""
    users = [[0], [1, 2], [3, 4, 5], [3, 6, 7], [3, 8, 9], [3, 4, 9]]
    return Graph(users, 11)


def zipf_graph(n_users=23, n_items=37, seed=5):
    rng = np.random.default_rng(seed)
    users = [list((rng.zipf(1.4, int(rng.integers(1, 9))) - 1) % n_items) for _ in range(n_users)]
    return Graph(users, n_items)


TOWER_SHAPES = [  # (B, K, T, L, n)
    (1, 16, 1, 2, 3), (37, 16, 3, 2, 3), (37, 1, 1, 1, 1), (37, 17, 3, 2, 3), (37, 33, 1, 3, 4), (5, 64, 16, 2, 10), (37, 16, 3, 0, 1),
    (37, 64, 1, 1, 1), (3, 16, 16, 3, 4),
]
WIDE_SHAPE = (1100, 16, 3, 2, 3)


def shape_case(shape, p=0.0, seed=0):
    B, K, T, L, n = shape
    return make_case(B, K, T, L, n, seed=seed, p=p, dense_slots=(1,) if T >= 3 else ())
