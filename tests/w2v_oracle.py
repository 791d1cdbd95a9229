"""A numpy restatement of DESIGN §7.9 (skip-gram word2vec in windows): the generator, walks, keep flags, pairs, the
negative table, the Huffman tree, targets and one window in f64 or f32.  A plain helper, not a test module.

Integers are meant to be bit-exact against csrc/word2vec.hip.  The window is held on the CPU to torch autograd of the same
summed loss and, at window 1, to a per-pair Python loop (tests/test_word2vec_cpu.py)."""
from __future__ import annotations

import heapq

import numpy as np

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
WALK, KEEP, SHRINK, NEG = 1, 2, 3, 4
NEGATIVES = 5
SAMPLE = 1e-3
ALPHA0, ALPHA_MIN = 0.025, 1e-4
MAX_EXP = 6.0


def mix64(z):
    """The splitmix64 finaliser on a uint64 array (wrapping arithmetic)."""
    z = np.atleast_1d(np.asarray(z, dtype=np.uint64))
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def w2v_hash(seed, stream, a, b):
    """H(seed, stream, a, b) of include/libreco_hip.h; `a` and `b` broadcast."""
    a = np.atleast_1d(np.asarray(a)).astype(np.uint64)
    b = np.atleast_1d(np.asarray(b)).astype(np.uint64)
    g = np.uint64(GOLD)
    z0 = mix64(np.uint64((int(seed) + GOLD * int(stream)) & M64))
    z = mix64(z0 + g * (a + np.uint64(1)))
    return mix64(z + g * (b + np.uint64(1)))


def hi32(h):
    return (h >> np.uint64(32)).astype(np.int64)


# ---- corpus ---------------------------------------------------------------------------------------------------------
def successor_csr(user_lists, n_items):
    """The reference's graph: items[i] -> items[i + 1] of every user list, duplicates kept, in list order per node."""
    succ = [[] for _ in range(n_items)]
    for items in user_lists:
        for x, y in zip(items[:-1], items[1:]):
            succ[int(x)].append(int(y))
    ptr = np.zeros(n_items + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(s) for s in succ])
    idx = np.asarray([y for s in succ for y in s], dtype=np.int32)
    return ptr, idx


def walks(starts, sptr, sidx, n_items, L, seed, pass_no):
    """Walk w starts at starts[w]; step s picks successor (hi32(H(seed, WALK, pass, w L + s)) * degree) >> 32; a node
    without successors (or an id outside the items) ends the walk.  -> (walks [n, L] padded with -1, lens [n])."""
    n = len(starts)
    out = np.full((n, L), -1, dtype=np.int32)
    lens = np.zeros(n, dtype=np.int32)
    node = np.asarray(starts, dtype=np.int64).copy()
    alive = (node >= 0) & (node < n_items)
    for s in range(L):
        out[alive, s] = node[alive]
        lens += alive
        if s + 1 == L or not alive.any():
            break
        nc = np.where(alive, node, 0)
        lo, deg = sptr[nc], sptr[nc + 1] - sptr[nc]
        alive &= deg > 0
        h = hi32(w2v_hash(seed, WALK, pass_no, np.arange(n) * L + s))
        pick = np.where(alive, lo + ((h * deg) >> 32), 0)
        node = np.where(alive, sidx[pick] if len(sidx) else 0, node)
        alive &= (node >= 0) & (node < n_items)
    return out, lens


def deepwalk_corpus(user_lists, n_items, n_walks, L, seed):
    """`corpus_of(pass)` of DeepWalk: per pass `n_walks` permutations of the items from one default_rng(seed), consumed pass
    after pass, and the walks from them."""
    sptr, sidx = successor_csr(user_lists, n_items)
    rng, memo = np.random.default_rng(seed), {}

    def corpus_of(pass_no):
        while len(memo) <= pass_no:
            p = len(memo)
            starts = np.concatenate([rng.permutation(n_items) for _ in range(n_walks)]).astype(np.int32)
            w, lens = walks(starts, sptr, sidx, n_items, L, seed, p)
            ptr = np.zeros(len(lens) + 1, dtype=np.int64)
            ptr[1:] = np.cumsum(lens)
            memo[p] = (w[w >= 0].astype(np.int32), ptr)
        return memo[pass_no]

    return corpus_of


def flatten_sentences(sentences):
    """-> (tokens int32 [T], sptr int64 [S + 1])."""
    sptr = np.zeros(len(sentences) + 1, dtype=np.int64)
    sptr[1:] = np.cumsum([len(s) for s in sentences])
    tokens = np.asarray([t for s in sentences for t in s], dtype=np.int32)
    return tokens, sptr


def word_counts(tokens, n_items):
    t = tokens[(tokens >= 0) & (tokens < n_items)]
    return np.bincount(t, minlength=n_items).astype(np.int64)


def keep_thresholds(counts, sample=SAMPLE):
    """floor(2^32 * min(1, (sqrt(c / (sample T)) + 1) * sample T / c)) per word, 0 for a word that never occurs."""
    c = counts.astype(np.float64)
    thr = sample * float(counts.sum())
    out = np.zeros(len(counts), dtype=np.int64)
    nz = counts > 0
    p = np.minimum(1.0, (np.sqrt(c[nz] / thr) + 1.0) * thr / c[nz])
    out[nz] = np.floor(p * 4294967296.0).astype(np.int64)
    return out


def keep_flags(tokens, thr, seed, epoch):
    n_items = len(thr)
    ok = (tokens >= 0) & (tokens < n_items)
    h = hi32(w2v_hash(seed, KEEP, epoch, np.arange(len(tokens))))
    return (ok & (h < thr[np.where(ok, tokens, 0)])).astype(np.uint8)


def compact(tokens, sptr, keep):
    """-> (ctok, craw, csent int32 [nc], cptr int64 [S + 1]): the kept tokens, their raw positions, sentences, and the
    compacted sentence starts."""
    craw = np.flatnonzero(keep).astype(np.int32)
    sent = np.repeat(np.arange(len(sptr) - 1), np.diff(sptr)).astype(np.int32)
    pre = np.concatenate([[0], np.cumsum(keep.astype(np.int64))])
    return tokens[craw].astype(np.int32), craw, sent[craw], pre[sptr].astype(np.int64)


def pairs(ctok, craw, csent, cptr, window, seed, epoch):
    """-> (in_ids, pred, centre) int32, in ascending (i, j)."""
    b = (w2v_hash(seed, SHRINK, epoch, craw) % np.uint64(window)).astype(np.int64) if len(craw) else np.zeros(0, np.int64)
    ins, pred, centre = [], [], []
    for i in range(len(ctok)):
        r = window - int(b[i])
        sb, se = int(cptr[csent[i]]), int(cptr[csent[i] + 1])
        for j in range(max(i - r, sb), min(i + r, se - 1) + 1):
            if j != i:
                ins.append(ctok[j])
                pred.append(ctok[i])
                centre.append(craw[i])
    return tuple(np.asarray(x, dtype=np.int32) for x in (ins, pred, centre))


# ---- targets --------------------------------------------------------------------------------------------------------
def negative_table(counts):
    """The cumulative count^0.75 table scaled to 2^32 (int64 [n_items]); a draw r picks the first word with cum > r."""
    w = counts.astype(np.float64) ** 0.75
    w[counts <= 0] = 0.0
    cs = np.cumsum(w)
    if cs[-1] <= 0:
        return np.zeros(len(counts), dtype=np.int64)
    cum = np.floor(cs / cs[-1] * 4294967296.0).astype(np.int64)
    cum[np.flatnonzero(counts > 0)[-1]:] = 1 << 32
    return cum


def huffman(counts):
    """heapq over (count, index) of the words that occur; the k-th merge gets index n_items + k, its first-popped child code
    0 and the other code 1.  -> CSR (ptr int32 [n_items + 1], nodes int32, codes int32), the path from the root down."""
    n = len(counts)
    heap = [(int(c), i) for i, c in enumerate(counts) if c > 0]
    heapq.heapify(heap)
    parent, code, k = {}, {}, 0
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        node = n + k
        k += 1
        parent[a[1]], code[a[1]] = node, 0
        parent[b[1]], code[b[1]] = node, 1
        heapq.heappush(heap, (a[0] + b[0], node))
    ptr, nodes, codes = np.zeros(n + 1, dtype=np.int32), [], []
    for w in range(n):
        path = []
        x = w
        while x in parent:
            path.append((parent[x], code[x]))
            x = parent[x]
        for nd, cd in reversed(path):
            nodes.append(nd)
            codes.append(cd)
        ptr[w + 1] = len(nodes)
    return ptr, np.asarray(nodes, dtype=np.int32), np.asarray(codes, dtype=np.int32)


def targets(in_ids, pred, cum, seed, epoch, pair_base=0, hs=None):
    """-> (offs int64 [W + 1], rows, labels, slot_in int32 [n_slots])."""
    n_items, W = len(cum), len(pred)
    valid = (pred >= 0) & (pred < n_items)
    plen = np.zeros(W, dtype=np.int64)
    if hs is not None:
        pc = np.where(valid, pred, 0)
        plen = np.where(valid, hs[0][pc + 1] - hs[0][pc], 0).astype(np.int64)
    offs = np.zeros(W + 1, dtype=np.int64)
    offs[1:] = np.cumsum(1 + NEGATIVES + plen)
    rows = np.full(offs[-1], -1, dtype=np.int32)
    labels = np.zeros(offs[-1], dtype=np.int32)
    slot_in = np.repeat(in_ids.astype(np.int32), np.diff(offs))
    idx = (pair_base + np.arange(W))[:, None] * NEGATIVES + np.arange(NEGATIVES)[None, :]
    r = hi32(w2v_hash(seed, NEG, epoch, idx.reshape(-1))).reshape(W, NEGATIVES) if W else np.zeros((0, NEGATIVES), np.int64)
    draw = np.searchsorted(cum, r, side="right")
    for p in range(W):
        o = offs[p]
        labels[o] = 1
        if valid[p]:
            rows[o] = pred[p]
            for k in range(NEGATIVES):
                d = int(draw[p, k])
                rows[o + 1 + k] = d if d < n_items and d != pred[p] else -1
            if plen[p]:
                hb = hs[0][pred[p]]
                rows[o + 1 + NEGATIVES:o + 1 + NEGATIVES + plen[p]] = hs[1][hb:hb + plen[p]]
                labels[o + 1 + NEGATIVES:o + 1 + NEGATIVES + plen[p]] = 1 - hs[2][hb:hb + plen[p]]
    return offs, rows, labels, slot_in


# ---- one window -----------------------------------------------------------------------------------------------------
def alphas(centre, pos0, inv_total):
    progress = (pos0 + centre.astype(np.float64)) * inv_total
    return np.maximum(ALPHA_MIN, ALPHA0 - (ALPHA0 - ALPHA_MIN) * progress)


def window(syn0, syn1, in_ids, centre, offs, rows, labels, pos0, inv_total, dtype=np.float64):
    """One window from the tables as they stand -> (g [n_slots], stash [W, D], loss [W], new syn0, new syn1) in `dtype`
    arithmetic.  Row sums are added one occurrence after the other in ascending position (np.add.at)."""
    s0, s1 = syn0.astype(dtype), syn1.astype(dtype)
    W, n_slots = len(in_ids), int(offs[-1]) if len(offs) else 0
    pair_of = np.repeat(np.arange(W), np.diff(offs))
    ins = in_ids[pair_of]
    live = (ins >= 0) & (ins < len(s0)) & (rows >= 0) & (rows < len(s1))
    a = alphas(centre, pos0, inv_total).astype(dtype)[pair_of]
    g = np.zeros(n_slots, dtype=dtype)
    lossv = np.zeros(n_slots, dtype=dtype)
    li = np.flatnonzero(live)
    v, w = s0[ins[li]], s1[rows[li]]
    f = (v * w).sum(1, dtype=dtype)
    lab = labels[li].astype(dtype)
    one = dtype(1)
    with np.errstate(over="ignore"):                 # exp(-f) = inf at a very negative f: the sigmoid is 0, as on the device
        gl = (lab - one / (one + np.exp(-f))) * a[li]
    gl[np.abs(f) >= MAX_EXP] = 0
    g[li] = gl
    x = np.where(labels[li] == 1, f, -f)
    lossv[li] = np.maximum(-x, 0) + np.log1p(np.exp(-np.abs(x)))
    stash = np.zeros((W, s0.shape[1]), dtype=dtype)
    np.add.at(stash, pair_of[li], gl[:, None] * w)
    loss = np.zeros(W, dtype=dtype)
    np.add.at(loss, pair_of, lossv)
    n1 = s1.copy()
    np.add.at(n1, rows[li], gl[:, None] * v)
    n0 = s0.copy()
    pv = np.flatnonzero((in_ids >= 0) & (in_ids < len(s0)))
    np.add.at(n0, in_ids[pv], stash[pv])
    return g, stash, loss, n0, n1


# ---- whole runs -----------------------------------------------------------------------------------------------------
def initial_tables(n_items, D, seed, hs):
    rng = np.random.default_rng(seed)
    syn0 = ((rng.random((n_items, D), dtype=np.float32) - 0.5) / D).astype(np.float32)
    syn1 = np.zeros((n_items + (max(n_items - 1, 0) if hs else 0), D), dtype=np.float32)
    return syn0, syn1


def epoch_pairs(tokens, sptr, thr, window_size, seed, epoch):
    keep = keep_flags(tokens, thr, seed, epoch)
    return pairs(*compact(tokens, sptr, keep), window_size, seed, epoch)


def train(corpus_of, n_items, D, window_size, n_epochs, seed, batch_size, hs=False, dtype=np.float64):
    """`corpus_of(pass)` -> (tokens, sptr); pass 0 gives the counts, passes 1 .. n_epochs are trained.  -> (syn0, syn1, the
    mean loss per pair of every epoch)."""
    tokens, sptr = corpus_of(0)
    counts = word_counts(tokens, n_items)
    T = int(counts.sum())
    thr, cum = keep_thresholds(counts), negative_table(counts)
    tree = huffman(counts) if hs else None
    syn0, syn1 = initial_tables(n_items, D, seed, hs)
    syn0, syn1 = syn0.astype(dtype), syn1.astype(dtype)
    losses = []
    for epoch in range(1, n_epochs + 1):
        tokens, sptr = corpus_of(epoch)
        ins, pred, centre = epoch_pairs(tokens, sptr, thr, window_size, seed, epoch)
        offs, rows, labels, _ = targets(ins, pred, cum, seed, epoch, 0, tree)
        total = 0.0
        for a in range(0, len(ins), batch_size):
            e = min(a + batch_size, len(ins))
            o = offs[a:e + 1]
            _, _, loss, syn0, syn1 = window(syn0, syn1, ins[a:e], centre[a:e], o - o[0], rows[o[0]:o[-1]], labels[o[0]:o[-1]],
                                            float((epoch - 1) * T), 1.0 / (n_epochs * T), dtype)
            total += float(loss.sum())
        losses.append(total / max(len(ins), 1))
    return syn0, syn1, losses


def cluster_cosines(emb, cluster_of):
    """(mean within-cluster cosine, mean across-cluster cosine) over the rows whose cluster is >= 0."""
    sel = np.flatnonzero(cluster_of >= 0)
    e = emb[sel].astype(np.float64)
    e = e / np.maximum(np.linalg.norm(e, axis=1, keepdims=True), 1e-30)
    c = e @ e.T
    same = cluster_of[sel][:, None] == cluster_of[sel][None, :]
    off = ~np.eye(len(sel), dtype=bool)
    return float(c[same & off].mean()), float(c[~same].mean())


def planted_clusters(n_users, n_clusters, per_cluster, list_len, seed):
    """Users who each consume `list_len` distinct items of one of `n_clusters` disjoint clusters -> (user lists, the
    cluster of every item)."""
    rng = np.random.default_rng(seed)
    lists = []
    for u in range(n_users):
        c = u % n_clusters
        lists.append([int(x) for x in c * per_cluster + rng.permutation(per_cluster)[:list_len]])
    return lists, np.repeat(np.arange(n_clusters), per_cluster)
