"""A numpy restatement of PinSage's device sampling and tower (csrc/pinsage.hip).

The sampler is exact integer arithmetic over uint64: the device must give the same integers.  The tower's forward and backward
exist in an f32 and an f64 variant; tests/test_pinsage_cpu.py shows that the f64 variant equals the reference module's
arithmetic restated with torch under autograd."""
import numpy as np

from .sage_oracle import (F32, U64, H, Graph, delta_rule, dropout_keep, forced_graph, level_slices, tree_nodes,  # noqa: F401
                          zipf_graph)

PIN_WALK = 21
MAX_VISITS = 64


# ---- sampling --------------------------------------------------------------------------------------------------------
def threshold(termination_prob):
    """floor(termination_prob * 2^32) in 64 bits: >= 1 never continues, <= 0 always does."""
    if termination_prob >= 1.0:
        return 1 << 32
    return 0 if termination_prob <= 0.0 else int(termination_prob * 4294967296.0)


def coord(i, w, s, walk_len):
    """b of the consumer draw of step s of walk w of node i; + 1 the item draw, + 2 the continue draw."""
    return (np.asarray(i, dtype=U64) * U64(64) + U64(w * walk_len + s)) * U64(4)


def visits(g, nodes, num_walks, walk_len, termination_prob, seed, step, level):
    """int64 [n_nodes, num_walks * walk_len]: the visited items in (walk, step) order, -2 where the walk had ended."""
    nodes = np.asarray(nodes, dtype=np.int32)
    n = len(nodes)
    idx, a, thr = np.arange(n, dtype=U64), U64(step * 8 + level), U64(threshold(termination_prob))
    out = np.full((n, num_walks * walk_len), -2, dtype=np.int64)
    for w in range(num_walks):
        cur, alive = nodes.copy(), np.ones(n, dtype=bool)
        for s in range(walk_len):
            b = coord(idx, w, s, walk_len)
            if s > 0:
                alive &= (H(seed, PIN_WALK, a, b + U64(2)) >> U64(32)) >= thr
            nxt = g.one_walk(cur, seed, PIN_WALK, a, b)
            cur = np.where(alive, nxt, cur).astype(np.int32)
            out[:, w * walk_len + s] = np.where(alive, nxt, -2)
    return out


def remove_target(lst, x):
    cnt = lst.count(x)
    if cnt == 0:
        return lst
    return [x] if cnt == len(lst) else [y for y in lst if y != x]


def select(lst, nn):
    """The nn most frequent entries, ties by first occurrence -> (items, counts)."""
    order, count = [], {}
    for x in lst:
        if x not in count:
            count[x] = 0
            order.append(x)
        count[x] += 1
    best = sorted(range(len(order)), key=lambda e: (-count[order[e]], e))[:nn]
    return [order[e] for e in best], [count[order[e]] for e in best]


def neighbors(g, nodes, nn, num_walks, walk_len, termination_prob, seed, step, level, tree_target=None, tree_exclude=None):
    """(ids, counts) int32 [n_nodes, nn] of `bipartite_neighbors_with_weights`; unused slots -1 / 0."""
    assert 1 <= nn <= 10 and num_walks >= 1 and walk_len >= 1 and num_walks * walk_len <= MAX_VISITS
    nodes = np.asarray(nodes, dtype=np.int32)
    vis = visits(g, nodes, num_walks, walk_len, termination_prob, seed, step, level)
    ids = np.full((len(nodes), nn), -1, dtype=np.int32)
    counts = np.zeros((len(nodes), nn), dtype=np.int32)
    lone = {}
    per_tree = nn ** level
    for i, node in enumerate(nodes.tolist()):
        if node not in lone:
            lone[node] = g.no_neighbor(node)
        if lone[node]:
            ids[i, 0], counts[i, 0] = node, 1
            continue
        lst = remove_target([x for x in vis[i].tolist() if x != -2], node)
        if tree_exclude is not None:
            t = i // per_tree
            if tree_exclude[t] >= 0 and tree_target[t] == node:
                lst = remove_target(lst, int(tree_exclude[t]))
        it, cn = select(lst, nn)
        ids[i, :len(it)], counts[i, :len(it)] = it, cn
    return ids, counts


def weights_of(counts):
    c = np.asarray(counts).astype(F32)
    return (c / np.maximum(c.sum(axis=1, keepdims=True, dtype=F32), F32(1))).astype(F32)


# ---- the tower -------------------------------------------------------------------------------------------------------
def param_floats(K, T, L):
    return T * K * K + K + L * (3 * K * K + 2 * K) + 2 * K * K + K


def pack_params(p, dtype=F32):
    parts = [p["proj_W"].T.reshape(-1), p["proj_b"]]
    for Q, bq, W, bw in p["layers"]:
        parts += [Q.T.reshape(-1), bq, W.T.reshape(-1), bw]
    parts += [p["G1"].T.reshape(-1), p["b1"], p["G2"].T.reshape(-1)]
    return np.concatenate(parts).astype(dtype)


def unpack_params(flat, K, T, L):
    flat = np.asarray(flat)
    o = T * K * K
    out = {"proj_W": flat[:o].reshape(T * K, K).T, "proj_b": flat[o:o + K], "layers": []}
    o += K
    for _ in range(L):
        Q, bq = flat[o:o + K * K].reshape(K, K).T, flat[o + K * K:o + K * K + K]
        o += K * K + K
        W, bw = flat[o:o + 2 * K * K].reshape(2 * K, K).T, flat[o + 2 * K * K:o + 2 * K * K + K]
        o += 2 * K * K + K
        out["layers"].append((Q, bq, W, bw))
    out["G1"], out["b1"] = flat[o:o + K * K].reshape(K, K).T, flat[o + K * K:o + K * K + K]
    o += K * K + K
    out["G2"] = flat[o:o + K * K].reshape(K, K).T
    assert o + K * K == len(flat)
    return out


def make_case(B, K, T, L, n, seed=0, V=53, p=0.0, dense_slots=(), ragged=True):
    """A seeded tower case: Zipf row ids, the scale of `dense_slots` random and 1 elsewhere, importance weights from random visit
    counts; with `ragged` a parent uses 1 .. n of its child slots, the others having rows of -1 and weight 0."""
    rng = np.random.default_rng([seed, B, K, T, L, n, 77])
    N = tree_nodes(L, n)
    rows = (rng.zipf(1.3, (B * N, T)) % V).astype(np.int32)
    scale = np.ones((B * N, T), dtype=F32)
    for t in dense_slots:
        scale[:, t] = rng.standard_normal(B * N).astype(F32)
    counts = rng.integers(1, 9, (B * (N - 1) // max(n, 1), n)).astype(np.int32) if N > 1 else np.zeros((0, 1), dtype=np.int32)
    if ragged and N > 1:
        used = rng.integers(1, n + 1, len(counts))
        counts[np.arange(n)[None, :] >= used[:, None]] = 0
    weights = weights_of(counts).reshape(-1) if N > 1 else np.zeros(0, dtype=F32)
    rows[B:][weights == 0] = -1
    xav = lambda fo, fi, gain=1.0: (rng.uniform(-1, 1, (fo, fi)) * gain * np.sqrt(6.0 / (fi + fo))).astype(F32)  # noqa: E731
    bias = lambda: (0.1 * rng.standard_normal(K)).astype(F32)  # noqa: E731
    r2 = np.sqrt(2.0)
    params = {"proj_W": xav(K, T * K, r2), "proj_b": bias(), "layers": [], "G1": None}
    for _ in range(L):
        params["layers"].append((xav(K, K, r2), bias(), xav(K, 2 * K, r2), bias()))
    params["G1"], params["b1"], params["G2"] = xav(K, K, r2), bias(), xav(K, K)
    return dict(shape=(B, K, T, L, n), V=V, table=rng.standard_normal((V, K)).astype(F32), rows=rows, scale=scale, weights=weights,
                params=params, grepr=rng.standard_normal((B, K)).astype(F32), p=p, seed=1234 + seed, step=7)


def case_masks(c):
    """{(layer, level): keep [B n^level, K]} of the neighbour branch's dropout (role 1; empty at p = 0)."""
    B, K, T, L, n = c["shape"]
    if not c["p"]:
        return {}
    return {(l, k): dropout_keep(B * n ** k, K, c["p"], c["seed"], c["step"], l, k, 1) for l in range(L) for k in range(1, L - l + 1)}


def tower(c, variant, rows=None, relu=None, masks=None):
    """Forward and backward of a case in one arithmetic -> dict(repr, grow [B N, T, K], gparams (packed), relu {("q", l, k),
    ("w", l, k), ("head",)}: flags [B n^k, K]).  `relu` forces the patterns."""
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
    wts = [None] + [c["weights"].astype(dt)[s.start - B:s.stop - B] for s in sl[1:]]
    pattern, saved = {}, []
    for l in range(L):
        Q, bq, W, bw = (a.astype(dt) for a in P["layers"][l])
        nxt, keep = [], []
        for k in range(L - l):
            q = (h[k + 1] @ Q.T + bq).astype(dt)
            qon = q > 0 if relu is None else relu[("q", l, k + 1)]
            nb = np.where(qon, q, 0).astype(dt)
            m = masks.get((l, k + 1))
            if c["p"]:
                nb = np.where(m, nb * inv_keep, 0).astype(dt)
            wk = wts[k + 1]
            agg = np.zeros((len(h[k]), K), dtype=dt)
            for j in range(n):
                agg = (agg + wk.reshape(-1, n)[:, j:j + 1] * nb.reshape(-1, n, K)[:, j]).astype(dt)
            zin = np.concatenate([h[k], agg], axis=1)
            zp = (zin @ W.T + bw).astype(dt)
            won = zp > 0 if relu is None else relu[("w", l, k)]
            z = np.where(won, zp, 0).astype(dt)
            nrm = np.sqrt((z * z).sum(axis=1, keepdims=True, dtype=dt)).astype(dt)
            nrm = np.where(nrm == 0, dt(1), nrm)
            y = (z / nrm).astype(dt)
            pattern[("q", l, k + 1)], pattern[("w", l, k)] = qon, won
            keep.append((qon, m, zin, won, nrm, y))
            nxt.append(y)
        saved.append((h, keep))
        h = nxt
    top = h[0]
    G1, b1, G2 = P["G1"].astype(dt), P["b1"].astype(dt), P["G2"].astype(dt)
    tp = (top @ G1.T + b1).astype(dt)
    hon = tp > 0 if relu is None else relu[("head",)]
    pattern[("head",)] = hon
    t = np.where(hon, tp, 0).astype(dt)
    rep = (t @ G2.T).astype(dt)
    # backward
    go = c["grepr"].astype(dt)
    gp = {"layers": [None] * L, "G2": go.T @ t}
    gpre = np.where(hon, go @ G2, 0).astype(dt)
    gp["G1"], gp["b1"] = gpre.T @ top, gpre.sum(axis=0)
    g = [(gpre @ G1).astype(dt)]
    for l in range(L - 1, -1, -1):
        Q, bq, W, bw = (a.astype(dt) for a in P["layers"][l])
        hl, keep = saved[l]
        gQ, gbq, gW, gbw = np.zeros_like(Q), np.zeros(K, dtype=dt), np.zeros_like(W), np.zeros(K, dtype=dt)
        gin = [np.zeros((B * n ** k, K), dtype=dt) for k in range(L - l + 1)]
        for k in range(L - l):
            qon, m, zin, won, nrm, y = keep[k]
            d = (y * g[k]).sum(axis=1, keepdims=True, dtype=dt)
            gz = np.where(won, (g[k] - y * d) / nrm, 0).astype(dt)
            gW += gz.T @ zin
            gbw += gz.sum(axis=0)
            gzin = (gz @ W).astype(dt)
            gin[k] = gin[k] + gzin[:, :K]
            gnb = np.repeat(gzin[:, K:], n, axis=0) * wts[k + 1][:, None]
            if c["p"]:
                gnb = np.where(m, gnb * inv_keep, 0)
            gq = np.where(qon, gnb, 0).astype(dt)
            gQ += gq.T @ hl[k + 1]
            gbq += gq.sum(axis=0)
            gin[k + 1] = gin[k + 1] + gq @ Q
        gp["layers"][l] = (gQ, gbq, gW, gbw)
        g = [a.astype(dt) for a in gin]
    g0 = np.zeros((len(rows), K), dtype=dt)
    for k, s in enumerate(sl):
        g0[s] = g[k]
    gp["proj_W"] = g0.T @ x.reshape(len(rows), T * K)
    gp["proj_b"] = g0.sum(axis=0)
    grow = ((g0 @ Wp).reshape(len(rows), T, K) * c["scale"].astype(dt)[:, :, None] * inside[:, :, None]).astype(dt)
    return dict(repr=rep, grow=grow, gparams=pack_params(gp, dt), relu=pattern)


def device_relu(flags, c):
    """The device's relu_out (per layer a q block [B, n_l - 1, K] and a w block [B, m_l, K], then the head's [B, K]) as the
    oracle's {key: [B n^level, K]}."""
    B, K, T, L, n = c["shape"]
    flags = np.asarray(flags).astype(bool)
    out, at = {}, 0
    for l in range(L):
        nin, nout = tree_nodes(L - l, n), tree_nodes(L - l - 1, n)
        blk = flags[at:at + B * (nin - 1)].reshape(B, nin - 1, K)
        at += B * (nin - 1)
        off = 0
        for k in range(1, L - l + 1):
            out[("q", l, k)] = blk[:, off:off + n ** k].reshape(B * n ** k, K)
            off += n ** k
        blk = flags[at:at + B * nout].reshape(B, nout, K)
        at += B * nout
        off = 0
        for k in range(L - l):
            out[("w", l, k)] = blk[:, off:off + n ** k].reshape(B * n ** k, K)
            off += n ** k
    out[("head",)] = flags[at:at + B]
    assert at + B == len(flags)
    return out


def check_tower(got, c, what, rows=None):
    """`got` = dict(repr, grow, gparams, relu (the device's flags or None)).  repr against f64 by the delta rule; grow and every
    parameter gradient against the f64 backward run with the result's own ReLU patterns; grow at rows outside the table is 0."""
    B, K, T, L, n = c["shape"]
    rows = c["rows"] if rows is None else rows
    f64, f32 = tower(c, "f64", rows), tower(c, "f32", rows)
    delta_rule(got["repr"], f64["repr"], f32["repr"], L + 2, f"{what} repr")
    relu = device_relu(got["relu"], c) if got.get("relu") is not None else None
    b64, b32 = tower(c, "f64", rows, relu=relu), tower(c, "f32", rows, relu=relu)
    delta_rule(got["grow"], b64["grow"], b32["grow"], L + 2, f"{what} grow")
    inside = (rows >= 0) & (rows < c["V"])
    assert not np.asarray(got["grow"])[~inside].any(), f"{what} grow at rows outside the table"
    gp, g64, g32 = (unpack_params(x, K, T, L) for x in (got["gparams"], b64["gparams"], b32["gparams"]))
    for name in ("proj_W", "proj_b", "G1", "b1", "G2"):
        delta_rule(gp[name], g64[name], g32[name], L + 2, f"{what} g {name}")
    for l in range(L):
        for j, name in enumerate(("Q", "bq", "W", "bw")):
            delta_rule(gp["layers"][l][j], g64["layers"][l][j], g32["layers"][l][j], L + 2, f"{what} g {name}[{l}]")


def oracle_result(c, variant, rows=None):
    r = tower(c, variant, rows)
    return dict(repr=r["repr"].astype(F32), grow=r["grow"].astype(F32), gparams=r["gparams"].astype(F32), relu=None)


TOWER_SHAPES = [  # (B, K, T, L, n)
    (1, 16, 1, 2, 3), (37, 16, 3, 2, 3), (37, 1, 1, 1, 1), (37, 17, 3, 2, 3), (37, 33, 1, 3, 4), (5, 64, 16, 2, 10), (37, 16, 3, 0, 1),
]
WIDE_SHAPE = (1100, 16, 3, 2, 3)


def shape_case(shape, p=0.0, seed=0):
    B, K, T, L, n = shape
    return make_case(B, K, T, L, n, seed=seed, p=p, dense_slots=(1,) if T >= 3 else ())
