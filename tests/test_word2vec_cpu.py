"""Item2Vec / DeepWalk without a device: the numpy oracle of DESIGN §7.9 (tests/w2v_oracle.py) held to two independent
checks (torch autograd of the same summed loss; a plain per-pair loop at window 1), the Huffman tree, the negative table, the
host helpers of bases/word2vec_base.py, the constructors against tests/golden/word2vec_signatures.json (written by hand from
the reference's two constructors and `GensimBase`), the assertion texts, and the planted-cluster property on the oracle."""
import heapq
import json
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

from librecommender_amd.algorithms import DeepWalk, Item2Vec
from librecommender_amd.bases import GensimBase, Word2VecBase
from librecommender_amd.bases import word2vec_base as B
from librecommender_amd.data import DatasetPure

from . import w2v_oracle as O
from .test_api_signatures_cpu import accepts, resolve

GOLDEN = json.loads((Path(__file__).parent / "golden" / "word2vec_signatures.json").read_text())

# The planted-cluster margins (mean within-cluster cosine minus mean across-cluster cosine of syn0), from the oracle over
# seeds 1 .. 5 on `planted()` below at window 64, D = 16, window_size 5.  Each margin is the worst seed minus the spread
# over the seeds, rounded down.
#   Item2Vec, 40 epochs:                      gaps 0.6593 0.6559 0.6568 0.6579 0.6569 (f64 and f32 alike): 0.6559 - 0.0034
#   DeepWalk, n_walks 5, walk_length 10, 20 epochs: gaps 0.7852 0.7556 0.7756 0.7697 0.7553:                0.7553 - 0.0299
ITEM2VEC_MARGIN, ITEM2VEC_EPOCHS = 0.65, 40
DEEPWALK_MARGIN, DEEPWALK_EPOCHS, DEEPWALK_WALKS, DEEPWALK_LENGTH = 0.72, 20, 5, 10
CLUSTER_WINDOW = 64


def planted():
    """200 users, each consuming all 10 items of one of four disjoint clusters in a random order."""
    return O.planted_clusters(200, 4, 10, 10, 0)


def random_window(rng, n_items, n1, D, W, hs_len, scale=0.5):
    """A window with every special case: ids outside the tables, masked slots, repeated rows, variable-length lists."""
    syn0 = rng.standard_normal((n_items, D)) * scale
    syn1 = rng.standard_normal((n1, D)) * scale
    in_ids = rng.integers(0, n_items, W).astype(np.int32)
    lens = 6 + rng.integers(0, hs_len + 1, W)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = rng.integers(0, n1, offs[-1]).astype(np.int32)
    labels = rng.integers(0, 2, offs[-1]).astype(np.int32)
    rows[rng.random(offs[-1]) < 0.1] = -1
    if W > 3:
        in_ids[1], in_ids[2] = -1, n_items
        rows[offs[3]] = n1
    centre = rng.integers(0, 1000, W).astype(np.int32)
    return syn0, syn1, in_ids, centre, offs, rows, labels


# ---- the oracle against autograd ------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [0.3, 1.5])
def test_window_is_one_gradient_step_of_the_summed_loss(scale):
    """new table = old table - d/dtable sum_slots alpha * (-log sigmoid(+-f)) over the live slots with |f| < 6 (word2vec
    skips the others): the window's update is the gradient of that sum at the window-start tables.  At scale 1.5 some
    |f| >= 6 occur."""
    rng = np.random.default_rng(5)
    syn0, syn1, in_ids, centre, offs, rows, labels = random_window(rng, 11, 17, 8, 40, 4, scale)
    pos0, inv_total = 2000.0, 1.0 / 9000.0
    g, stash, loss, n0, n1 = O.window(syn0, syn1, in_ids, centre, offs, rows, labels, pos0, inv_total)
    t0 = torch.tensor(syn0, requires_grad=True)
    t1 = torch.tensor(syn1, requires_grad=True)
    pair_of = np.repeat(np.arange(len(in_ids)), np.diff(offs))
    ins = in_ids[pair_of]
    live = (ins >= 0) & (ins < 11) & (rows >= 0) & (rows < 17)
    li = torch.tensor(np.flatnonzero(live))
    f = (t0[torch.tensor(ins[live]).long()] * t1[torch.tensor(rows[live]).long()]).sum(1)
    x = torch.where(torch.tensor(labels[live]) == 1, f, -f)
    alpha = torch.tensor(O.alphas(centre, pos0, inv_total)[pair_of][live])
    keep = (f.abs() < 6).detach()
    if scale > 1:
        assert bool((~keep).any()) and bool(keep.any())
    per_slot = -torch.nn.functional.logsigmoid(x)
    (alpha * per_slot)[keep].sum().backward()
    np.testing.assert_allclose(n0, syn0 - t0.grad.numpy(), rtol=0, atol=1e-13)
    np.testing.assert_allclose(n1, syn1 - t1.grad.numpy(), rtol=0, atol=1e-13)
    # the reported loss counts the skipped slots too
    want = np.zeros(len(in_ids))
    np.add.at(want, pair_of[li.numpy()], per_slot.detach().numpy())
    np.testing.assert_allclose(loss, want, rtol=0, atol=1e-12)
    assert np.all(g[~live] == 0) and np.all(stash[[1, 2]] == 0)


def per_pair_loop(syn0, syn1, ins, centre, offs, rows, labels, pos0, inv_total):
    """An epoch at window 1 written as word2vec's loop: pair after pair, target after target, every f of a pair from the
    tables as the pair found them."""
    syn0, syn1 = syn0.copy(), syn1.copy()
    for p in range(len(ins)):
        i = int(ins[p])
        if not 0 <= i < len(syn0):
            continue
        progress = (pos0 + float(centre[p])) * inv_total
        alpha = max(1e-4, 0.025 - (0.025 - 1e-4) * progress)
        v = syn0[i].copy()
        old1 = syn1.copy()
        neu = np.zeros_like(v)
        for s in range(int(offs[p]), int(offs[p + 1])):
            r = int(rows[s])
            if not 0 <= r < len(syn1):
                continue
            f = float(v @ old1[r])
            if abs(f) >= 6:
                continue
            g = (float(labels[s]) - 1.0 / (1.0 + np.exp(-f))) * alpha
            neu += g * old1[r]
            syn1[r] += g * v
        syn0[i] += neu
    return syn0, syn1


@pytest.mark.parametrize("hs", [False, True])
def test_window_one_epoch_is_the_per_pair_loop(hs):
    lists, _ = O.planted_clusters(12, 3, 6, 6, 1)
    lists[3] = lists[3] + [99]                        # an id outside the vocabulary: dropped by the keep flags
    tokens, sptr = O.flatten_sentences(lists)
    n_items, D, seed = 18, 5, 9
    counts = O.word_counts(tokens, n_items)
    # (every word kept: at 73 tokens the subsampling of DESIGN §7.9 would leave a handful of pairs)
    ins, pred, centre = O.epoch_pairs(tokens, sptr, np.full(n_items, 1 << 32, dtype=np.int64), 3, seed, 1)
    assert len(ins) > 100 and ins.max() < n_items
    tree = O.huffman(counts) if hs else None
    offs, rows, labels, _ = O.targets(ins, pred, O.negative_table(counts), seed, 1, 0, tree)
    rng = np.random.default_rng(0)
    syn0 = rng.standard_normal((n_items, D)) * 0.4
    syn1 = rng.standard_normal((n_items + (n_items - 1 if hs else 0), D)) * 0.4
    T = int(counts.sum())
    a0, a1 = syn0.copy(), syn1.copy()
    for p in range(len(ins)):
        o = offs[p:p + 2]
        _, _, _, a0, a1 = O.window(a0, a1, ins[p:p + 1], centre[p:p + 1], o - o[0], rows[o[0]:o[1]], labels[o[0]:o[1]], 0.0,
                                   1.0 / (2 * T))
    b0, b1 = per_pair_loop(syn0, syn1, ins, centre, offs, rows, labels, 0.0, 1.0 / (2 * T))
    np.testing.assert_allclose(a0, b0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(a1, b1, rtol=0, atol=1e-12)
    assert np.abs(a0 - syn0).max() > 1e-3


def test_f32_window_is_close_to_f64():
    rng = np.random.default_rng(2)
    args = random_window(rng, 37, 73, 33, 255, 5)
    w64 = O.window(*args, 0.0, 1e-4)
    w32 = O.window(*args, 0.0, 1e-4, dtype=np.float32)
    for a, b in zip(w64, w32):
        assert b.dtype == np.float32
        np.testing.assert_allclose(b, a, rtol=1e-4, atol=1e-5)


# ---- corpus, pairs ----------------------------------------------------------------------------------------------------
def test_pairs_follow_the_shrunk_window_inside_sentences():
    sentences = [[], [3], [1, 2], list(range(12)), [5, 5, 5, 5]]
    tokens, sptr = O.flatten_sentences(sentences)
    keep = np.ones(len(tokens), dtype=np.uint8)
    keep[4] = 0
    ctok, craw, csent, cptr = O.compact(tokens, sptr, keep)
    assert len(ctok) == len(tokens) - 1 and list(cptr) == [0, 0, 1, 3, 14, 18]
    for window in (1, 2, 5):
        ins, pred, centre = O.pairs(ctok, craw, csent, cptr, window, 3, 1)
        b = (O.w2v_hash(3, O.SHRINK, 1, craw) % np.uint64(window)).astype(np.int64)
        raw_to_c = {int(r): i for i, r in enumerate(craw)}
        seen = set()
        for x, y, c in zip(ins, pred, centre):
            i = raw_to_c[int(c)]
            assert ctok[i] == y
            seen.add(i)
        assert 1 not in {int(csent[i]) for i in seen}                         # a sentence of one token has no pair
        n_expect = sum(min(i + window - b[i], cptr[csent[i] + 1] - 1) - max(i - (window - b[i]), cptr[csent[i]])
                       for i in range(len(ctok)))
        assert len(ins) == n_expect
        assert np.all(np.diff(centre.astype(np.int64)) >= 0)
    assert window == 5 and len(set(b.tolist())) > 1


def test_walks_stop_at_dead_ends():
    lists = [[0, 1, 2], [0, 2], [3]]
    sptr, sidx = O.successor_csr(lists, 5)
    assert list(sptr) == [0, 2, 3, 3, 3, 3] and list(sidx) == [1, 2, 2]
    w, lens = O.walks(np.array([0, 1, 2, 3, 4, 7], dtype=np.int32), sptr, sidx, 5, 4, 11, 0)
    assert list(lens[2:]) == [1, 1, 1, 0] and list(w[5]) == [-1] * 4 and list(w[2]) == [2, -1, -1, -1]
    assert w[1, 1] == 2 and lens[1] == 2 and lens[0] in (2, 3) and w[0, lens[0] - 1] == 2
    w1, l1 = O.walks(np.array([0, 3], dtype=np.int32), sptr, sidx, 5, 1, 11, 0)
    assert w1.tolist() == [[0], [3]] and l1.tolist() == [1, 1]


# ---- Huffman tree -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_huffman_tree_is_prefix_free_and_optimal(seed):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 50, 41).astype(np.int64) * (rng.random(41) < 0.8)
    counts[:3] = [0, 7, 7]
    ptr, nodes, codes = O.huffman(counts)
    words = np.flatnonzero(counts > 0)
    assert all(ptr[w + 1] == ptr[w] for w in np.flatnonzero(counts == 0))
    paths = {int(w): tuple(codes[ptr[w]:ptr[w + 1]].tolist()) for w in words}
    for a in paths:
        for b in paths:
            if a != b:
                assert paths[a] != paths[b][: len(paths[a])], "a code is a prefix of another"
    # inner nodes: rows n .. n + (#words - 2); every path starts at the root, the last merge
    assert nodes.min() == len(counts) and nodes.max() == len(counts) + len(words) - 2
    assert all(nodes[ptr[w]] == nodes.max() for w in words)
    # the same words reach the same inner node by the same code prefix
    by_prefix = {}
    for w in words:
        for d in range(ptr[w + 1] - ptr[w]):
            assert by_prefix.setdefault(paths[int(w)][:d], nodes[ptr[w] + d]) == nodes[ptr[w] + d]
    heap = [int(c) for c in counts[words]]
    heapq.heapify(heap)
    best = 0
    while len(heap) > 1:
        s = heapq.heappop(heap) + heapq.heappop(heap)
        best += s
        heapq.heappush(heap, s)
    assert sum(int(counts[w]) * len(paths[int(w)]) for w in words) == best
    mine = B.huffman_csr(counts)
    assert all(np.array_equal(a, b) for a, b in zip(mine, (ptr, nodes, codes)))


def test_one_word_has_no_path():
    ptr, nodes, codes = O.huffman(np.array([0, 5, 0]))
    assert ptr.tolist() == [0, 0, 0, 0] and len(nodes) == 0


# ---- negative table -----------------------------------------------------------------------------------------------------
def test_negative_draws_follow_count_to_the_three_quarters():
    """10^5 draws: every word's frequency within 5 binomial standard deviations of n p (p = count^0.75 / sum).  With 37 words
    a correct table fails this with probability below 37 * 5.8e-7."""
    rng = np.random.default_rng(0)
    counts = np.floor(1000.0 / np.arange(1, 38)).astype(np.int64)
    counts[[4, 20]] = 0
    rng.shuffle(counts)
    cum = O.negative_table(counts)
    assert np.array_equal(cum, B.negative_table(counts)) and cum[-1] == 1 << 32
    n = 100_000
    r = O.hi32(O.w2v_hash(42, O.NEG, 1, np.arange(n)))
    draw = np.searchsorted(cum, r, side="right")
    freq = np.bincount(draw, minlength=len(counts))
    p = counts.astype(np.float64) ** 0.75
    p[counts == 0] = 0
    p /= p.sum()
    assert np.all(freq[counts == 0] == 0)
    sd = np.sqrt(n * p * (1 - p))
    assert np.all(np.abs(freq - n * p) <= 5 * sd + 1e-9), (freq - n * p) / np.maximum(sd, 1)


def test_keep_thresholds():
    counts = np.array([0, 1, 10, 1000, 100000], dtype=np.int64)
    thr = O.keep_thresholds(counts)
    assert np.array_equal(thr, B.keep_thresholds(counts))
    T = counts.sum()
    assert thr[0] == 0 and thr[1] == 1 << 32 and thr[2] == 1 << 32           # rare words are always kept
    p = (np.sqrt(100000 / (1e-3 * T)) + 1) * (1e-3 * T) / 100000
    assert abs(thr[4] / 2.0 ** 32 - p) < 1e-9 and 0 < p < 0.2
    tokens = np.array([4] * 20000 + [9, -1], dtype=np.int32)
    keep = O.keep_flags(tokens, thr, 1, 1)
    assert keep[-1] == 0 and keep[-2] == 0
    assert abs(keep[:20000].mean() - p) <= 5 * np.sqrt(p * (1 - p) / 20000)       # 5 binomial standard deviations


def test_targets_mask_a_draw_of_the_predicted_word():
    counts = np.array([5, 1000, 3], dtype=np.int64)
    cum, tree = O.negative_table(counts), O.huffman(counts)
    pred = np.array([1] * 50 + [-1, 3], dtype=np.int32)
    ins = np.arange(52, dtype=np.int32)
    offs, rows, labels, slot_in = O.targets(ins, pred, cum, 1, 1, 7, tree)
    assert np.array_equal(np.diff(offs)[:50], np.full(50, 6 + tree[0][2] - tree[0][1])) and list(np.diff(offs)[50:]) == [6, 6]
    first = rows[offs[:-1]]
    assert np.array_equal(first[:50], pred[:50]) and list(first[50:]) == [-1, -1]
    negs = np.stack([rows[offs[:50] + 1 + k] for k in range(5)], 1)
    assert (negs == -1).sum() > 100 and not (negs == 1).any() and set(np.unique(negs)) <= {-1, 0, 2}
    assert np.all(rows[offs[50]:offs[52]] == -1)
    assert np.array_equal(slot_in, np.repeat(ins, np.diff(offs)))


# ---- constructors -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(GOLDEN))
def test_reference_signature_is_accepted(key):
    problem = accepts(GOLDEN[key], resolve(key))
    assert problem is None, f"{key}: {problem}"


def test_added_options_come_behind_the_reference_parameters():
    import inspect

    for cls, key in ((Item2Vec, "algorithms.Item2Vec.__init__"), (DeepWalk, "algorithms.DeepWalk.__init__")):
        names = list(inspect.signature(cls.__init__).parameters)
        assert names == [s[0] for s in GOLDEN[key]] + ["batch_size", "device"]
    assert GensimBase is Word2VecBase


@pytest.fixture(scope="module")
def data():
    lists, _ = planted()
    df = pd.DataFrame({"user": np.repeat(np.arange(len(lists)), 10), "item": np.concatenate(lists), "label": 1})
    return DatasetPure.build_trainset(df)


@pytest.fixture(scope="module")
def info(data):
    return data[1]


def test_assertion_texts_and_value_errors(info):
    with pytest.raises(AssertionError, match="Item2Vec is only suitable for ranking"):
        Item2Vec("rating", info)
    with pytest.raises(AssertionError, match="DeepWalk is only suitable for ranking"):
        DeepWalk("rating", info)
    for cls in (Item2Vec, DeepWalk):
        for bad in (0, 257, 16.0):
            with pytest.raises(ValueError, match="embed_size"):
                cls("ranking", info, embed_size=bad)
        with pytest.raises(ValueError, match="batch_size"):
            cls("ranking", info, batch_size=0)
        m = cls("ranking", info, embed_size=256, n_threads=3)
        assert m.n_threads == 3 and m.window_size == 5 and cls("ranking", info, window_size=0).window_size == 5
    with pytest.raises(ValueError, match="walk_length"):
        DeepWalk("ranking", info, walk_length=0)
    assert Item2Vec("ranking", info).n_epochs == 10 and DeepWalk("ranking", info).n_walks == 10


def test_window_is_capped_against_the_vocabulary(info):
    """profiles/word2vec.md: 8 pairs per item, and 1,024 pairs with hierarchical softmax."""
    assert Item2Vec("ranking", info).window_pairs() == 256 == DeepWalk("ranking", info).window_pairs()
    assert Item2Vec("ranking", info, batch_size=10 ** 6).window_pairs() == 8 * 40
    assert DeepWalk("ranking", info, batch_size=10 ** 6).window_pairs() == 8 * 40
    m = DeepWalk("ranking", info, batch_size=10 ** 6)
    m.n_items = 1000
    assert m.window_pairs() == 1024


def test_fit_raises_under_a_process_group(data, monkeypatch):
    from librecommender_amd import distributed

    monkeypatch.setattr(distributed, "active", lambda: object())
    for cls in (Item2Vec, DeepWalk):
        with pytest.raises(RuntimeError, match="single process"):
            cls("ranking", data[1]).fit(data[0], neg_sampling=True, verbose=0)


def test_models_have_no_cpu_engine(info):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Item2Vec("ranking", info, device="cpu").build_model()
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            DeepWalk("ranking", info).build_model()


def test_successor_csr_of_the_model_is_the_oracles(info):
    m = DeepWalk("ranking", info)
    lists = [list(v) for v in info.user_consumed.values()]
    ptr, idx = O.successor_csr(lists, info.n_items)
    got = m.successor_csr()
    assert np.array_equal(got[0], ptr) and np.array_equal(got[1], idx)


# ---- the planted-cluster property on the oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_planted_clusters_separate_item2vec(seed):
    lists, cluster_of = planted()
    tokens, sptr = O.flatten_sentences(lists)
    syn0, _, losses = O.train(lambda p: (tokens, sptr), 40, 16, 5, ITEM2VEC_EPOCHS, seed, CLUSTER_WINDOW, dtype=np.float32)
    within, across = O.cluster_cosines(syn0, cluster_of)
    assert within - across >= ITEM2VEC_MARGIN and losses[-1] < 0.5 * losses[0]


def test_planted_clusters_separate_deepwalk():
    lists, cluster_of = planted()
    corpus_of = O.deepwalk_corpus(lists, 40, DEEPWALK_WALKS, DEEPWALK_LENGTH, 1)
    syn0, _, losses = O.train(corpus_of, 40, 16, 5, DEEPWALK_EPOCHS, 1, CLUSTER_WINDOW, hs=True, dtype=np.float32)
    within, across = O.cluster_cosines(syn0, cluster_of)
    assert within - across >= DEEPWALK_MARGIN and losses[-1] < 0.6 * losses[0]
