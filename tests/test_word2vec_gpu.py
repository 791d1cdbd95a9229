"""Item2Vec / DeepWalk on the device (csrc/word2vec.hip, bases/word2vec_base.py) against the numpy oracle of DESIGN §7.9
(tests/w2v_oracle.py): integers bit for bit, floats within 10 x the oracle's own f32 / f64 gap (the rule of §7.4), two runs
the same bits, and the two models through fit / predict / recommend / kNN / save / load / rebuild_model."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

from librecommender_amd import ops
from librecommender_amd.algorithms import DeepWalk, Item2Vec
from librecommender_amd.data import DatasetPure

from . import w2v_oracle as O
from .test_word2vec_cpu import (CLUSTER_WINDOW, DEEPWALK_EPOCHS, DEEPWALK_LENGTH, DEEPWALK_MARGIN, DEEPWALK_WALKS,
                                ITEM2VEC_EPOCHS, ITEM2VEC_MARGIN, planted)

pytestmark = pytest.mark.gpu


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.cpu().numpy()


# ---- integers: walks, keep flags, pairs, targets ------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 7])
def test_walks(dev, L):
    """A graph with dead ends (items 30 .. 36 have no successor), multiplicities, starts outside the items and walk_length 1."""
    rng = np.random.default_rng(L)
    n_items = 37
    lists = [[int(x) for x in rng.integers(0, 30, rng.integers(1, 9))] + [int(rng.integers(30, 37))] for _ in range(60)]
    sptr, sidx = O.successor_csr(lists, n_items)
    assert (np.diff(sptr)[30:] == 0).all() and np.diff(sptr).max() > 3
    starts = np.concatenate([rng.permutation(n_items) for _ in range(9)] + [[-1, n_items]]).astype(np.int32)
    for pass_no in (0, 3):
        want, want_len = O.walks(starts, sptr, sidx, n_items, L, 42, pass_no)
        got, got_len = ops.w2v_walks(_dev(starts, dev), _dev(sptr, dev), _dev(sidx, dev), n_items, L, 42, pass_no)
        assert np.array_equal(_np(got), want) and np.array_equal(_np(got_len), want_len)
    if L == 7:
        assert want_len.min(initial=9, where=want_len > 0) == 1 and want_len.max() == 7 and (want_len < 7).sum() > 50
        assert (want_len[-2:] == 0).all()


def _corpus(seed):
    """Sentences of length 0, 1, 2, and longer than 2 * 5 + 1, over 37 items with a Zipf head, and ids outside the items."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, 38)
    p /= p.sum()
    sentences = [[], [3], [1, 2], []] + [[int(x) for x in rng.choice(37, size=n, p=p)] for n in (2, 13, 30, 1, 64, 12, 500)]
    sentences[6][4], sentences[8][0] = 37, -1
    return O.flatten_sentences(sentences)


def test_keep_flags(dev):
    tokens, _ = _corpus(0)
    counts = O.word_counts(tokens, 37)
    thr = O.keep_thresholds(counts)
    assert (thr < 1 << 32).sum() > 3                                   # the head is subsampled, the tail always kept
    for epoch in (1, 4):
        want = O.keep_flags(tokens, thr, 7, epoch)
        got = ops.w2v_keep(_dev(tokens, dev), _dev(thr, dev), 7, epoch)
        assert np.array_equal(_np(got), want)
    assert 0 < want.sum() < len(tokens) - 2


@pytest.mark.parametrize("window", [1, 2, 5])
def test_pairs(dev, window):
    tokens, sptr = _corpus(1)
    counts = O.word_counts(tokens, 37)
    keep = O.keep_flags(tokens, O.keep_thresholds(counts * 4), 3, 2)  # (a milder subsampling: sentences stay long)
    keep[:3] = 1                                                      # kept sentences of exactly one and two tokens
    c = O.compact(tokens, sptr, keep)
    lens = np.diff(c[3])
    assert {0, 1, 2} <= set(lens.tolist()) and lens.max() > 2 * window + 1
    want = O.pairs(*c, window, 3, 2)
    got = ops.w2v_pairs(*(_dev(x, dev) for x in c), window, 3, 2)
    assert len(want[0]) > 100
    for g, w in zip(got, want):
        assert np.array_equal(_np(g), w)
    empty = ops.w2v_pairs(*(_dev(x[:0], dev) for x in c[:3]), _dev(np.zeros(1, dtype=np.int64), dev), window, 3, 2)
    assert all(t.numel() == 0 for t in empty)


@pytest.mark.parametrize("hs", [False, True])
def test_targets(dev, hs):
    """Item 1 holds most of the mass, so many draws hit the predicted word and are masked; ids outside the items."""
    rng = np.random.default_rng(3)
    counts = rng.integers(1, 20, 37).astype(np.int64)
    counts[1], counts[5] = 2000, 0
    cum, tree = O.negative_table(counts), O.huffman(counts)
    W = 700
    pred = rng.integers(0, 37, W).astype(np.int32)
    pred[:200] = 1
    pred[[300, 301, 302]] = (-1, 37, 5)
    ins = rng.integers(-1, 38, W).astype(np.int32)
    want = O.targets(ins, pred, cum, 11, 2, 12345, tree if hs else None)
    got = ops.w2v_targets(_dev(ins, dev), _dev(pred, dev), _dev(cum, dev), 11, 2, pair_base=12345,
                          hs=tuple(_dev(a, dev) for a in tree) if hs else None)
    for k, w in zip(("offs", "rows", "labels", "slot_in"), want):
        assert np.array_equal(_np(got[k]), w), k
    rows, offs = want[1], want[0]
    assert (rows[offs[:200, None] + np.arange(1, 6)] == -1).sum() > 300
    assert hs == (np.diff(offs).max() > 6)


# ---- floats: one window ---------------------------------------------------------------------------------------------------
def _window_case(D, W, hs, seed=0):
    """37 items (every row has long runs at W = 4096), targets from the oracle, a few rows scaled so that some |f| >= 6,
    ids outside both tables."""
    rng = np.random.default_rng(seed + 1000 * D + W)
    n_items = 37
    counts = np.floor(400.0 / np.arange(1, n_items + 1)).astype(np.int64)
    cum, tree = O.negative_table(counts), O.huffman(counts)
    V1 = n_items + (n_items - 1 if hs else 0)
    syn0 = (rng.standard_normal((n_items, D)) * 0.5 / np.sqrt(D)).astype(np.float32)
    syn1 = (rng.standard_normal((V1, D)) * 0.5 / np.sqrt(D)).astype(np.float32)
    syn0[1:3] *= 8
    syn1[[1, 2, V1 - 1]] *= 8
    syn0[0] = syn1[0] = 3.0 / np.sqrt(D)                         # f = 9 for the pair of the two most frequent rows
    pcount = counts / counts.sum()
    ins = rng.choice(n_items, size=W, p=pcount).astype(np.int32)
    pred = rng.choice(n_items, size=W, p=pcount).astype(np.int32)
    if W > 3:
        ins[1], ins[2], pred[3] = -1, n_items, n_items
    centre = rng.integers(0, 5000, W).astype(np.int32)
    offs, rows, labels, slot_in = O.targets(ins, pred, cum, seed, 1, 0, tree if hs else None)
    if W > 3:
        rows[offs[4] + 1] = V1                                   # a target row outside the output table
    return syn0, syn1, ins, centre, offs, rows, labels, slot_in


def _device_window(dev, case):
    syn0, syn1, ins, centre, offs, rows, labels, slot_in = (_dev(x, dev) for x in case)
    g, stash, loss = ops.w2v_score(syn0, syn1, ins, centre, offs, rows, labels, 1000.0, 1.0 / 20000.0)
    seg_o = ops.build_segments(rows, syn1.shape[0])
    seg_i = ops.build_segments(ins, syn0.shape[0])
    ops.w2v_out_update(syn1, seg_o, syn0, g, slot_in)
    ops.w2v_out_update(syn0, seg_i, stash)
    return g, stash, loss, syn0, syn1


@pytest.mark.parametrize("hs", [False, True])
@pytest.mark.parametrize("W", [1, 255, 4096])
@pytest.mark.parametrize("D", [1, 16, 17, 33, 100, 129, 256])
def test_one_window(dev, D, W, hs):
    """g, the stash and both tables after the update against the f64 oracle, each within 10 x the oracle's own f32 / f64 gap
    on this very case.  The per-pair loss is held to the same rule with a floor: it is an f32 sum of up to `n` softplus terms,
    each a few ulp off (expf, log1pf) and each addition half an ulp of the running sum, so 4 n eps32 max|loss| is what f32
    can promise; at W = 1 the oracle's own gap is one sample of that rounding and can be ten times smaller by luck
    (measured: D = 16, W = 1, negatives only: oracle 1.0e-7, device 8.5e-7, floor 1.2e-5)."""
    case = _window_case(D, W, hs)
    w64 = O.window(*case[:7], 1000.0, 1.0 / 20000.0)
    w32 = O.window(*case[:7], 1000.0, 1.0 / 20000.0, dtype=np.float32)
    got = [_np(t) for t in _device_window(dev, case)]
    if W > 3:
        f = np.abs((case[0][np.clip(case[7], 0, 36)] * case[1][np.clip(case[5], 0, len(case[1]) - 1)]).sum(1))
        assert (f >= 6).sum() > 0 and (f < 6).sum() > (f >= 6).sum()
        assert (w64[0] == 0).sum() > (case[5] < 0).sum() and np.abs(w64[0]).max() > 1e-3
    for name, dv, a64, a32 in zip(("g", "stash", "loss", "syn0", "syn1"), got, w64, w32):
        delta = float(np.abs(a32.astype(np.float64) - a64).max())
        gap = float(np.abs(dv.astype(np.float64) - a64).max())
        print(f"W2V-FIGURE one-window D={D} W={W} hs={int(hs)} {name}: delta={delta:.3e} device={gap:.3e} bound={10 * delta:.3e}")
        assert np.isfinite(dv).all()
        floor = 4 * int(np.diff(case[4]).max()) * np.finfo(np.float32).eps * float(np.abs(a64).max()) if name == "loss" else 0.0
        assert gap <= max(10 * delta, floor), name
    if W > 3:                                                    # a pair whose input id is outside the table takes no part
        o = case[4]
        assert (got[0][o[1]:o[3]] == 0).all() and (got[1][1:3] == 0).all() and (got[2][1:3] == 0).all()


@pytest.mark.parametrize("D", [16, 100])
def test_two_runs_give_the_same_bits(dev, D):
    case = _window_case(D, 4096, True, seed=5)
    a = _device_window(dev, case)
    b = _device_window(dev, case)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[3], _dev(case[0], dev)) and not torch.equal(a[4], _dev(case[1], dev))


def test_wrappers_check_their_arguments(dev):
    case = [_dev(x, dev) for x in _window_case(16, 8, False)]
    syn0, syn1, ins, centre, offs, rows, labels, slot_in = case
    with pytest.raises(TypeError):
        ops.w2v_score(syn0.double(), syn1, ins, centre, offs, rows, labels, 0.0, 1.0)
    with pytest.raises(ValueError):
        ops.w2v_score(syn0, syn1[:, :8], ins, centre, offs, rows, labels, 0.0, 1.0)
    with pytest.raises(ValueError):
        ops.w2v_score(syn0.t().contiguous().t(), syn1, ins, centre, offs, rows, labels, 0.0, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.w2v_score(syn0.cpu(), syn1, ins, centre, offs, rows, labels, 0.0, 1.0)
    wide = torch.zeros((4, 257), device=dev)
    with pytest.raises(ValueError, match="1 to 256"):
        ops.w2v_score(wide, wide, ins, centre, offs, rows, labels, 0.0, 1.0)
    seg = ops.build_segments(rows, syn1.shape[0])
    with pytest.raises(ValueError):
        ops.w2v_out_update(syn1, seg, syn0, g=torch.zeros(rows.numel(), device=dev))
    with pytest.raises(ValueError):
        ops.w2v_out_update(syn0, seg, syn0)                     # segments of another table
    assert ops.w2v_supported(256) and not ops.w2v_supported(257) and not ops.w2v_supported(0)


# ---- the models -------------------------------------------------------------------------------------------------------------
def _frame(lists, user0=0):
    return pd.DataFrame({"user": np.repeat(np.arange(len(lists)) + user0, [len(x) for x in lists]),
                         "item": np.concatenate(lists), "label": 1})


@pytest.fixture(scope="module")
def cluster_data():
    lists, cluster_of = planted()
    train, info = DatasetPure.build_trainset(_frame(lists))
    assert all(list(info.user_consumed[info.user2id[u]]) == [info.item2id[i] for i in lists[u]] for u in range(len(lists)))
    by_inner = np.empty(40, dtype=np.int64)
    by_inner[[info.item2id[i] for i in range(40)]] = cluster_of
    # the corpus in inner ids, in `user_consumed` order
    return train, info, [list(v) for v in info.user_consumed.values()], by_inner


MODELS = {"item2vec": (Item2Vec, {}), "deepwalk": (DeepWalk, {"n_walks": DEEPWALK_WALKS, "walk_length": DEEPWALK_LENGTH})}


@pytest.mark.parametrize("name", sorted(MODELS))
def test_model_surface(dev, cluster_data, tmp_path, name):
    train, info, lists, _ = cluster_data
    cls, kw = MODELS[name]
    kw = dict(kw, embed_size=16, n_epochs=2, batch_size=64, seed=3)
    model = cls("ranking", info, **kw)
    model.fit(train, neg_sampling=True, verbose=0)
    assert model.item_embeds.shape == (41, 16) and model.user_embeds.shape == (201, 16) and model.item_embeds.is_cuda
    assert torch.equal(model.item_embeds[:40], model.syn0) and model.syn1.shape[0] == (79 if name == "deepwalk" else 40)
    # the epoch's corpus and pair list are the oracle's, bit for bit
    if name == "item2vec":
        tokens, sptr = O.flatten_sentences(lists)
        corpus_of = lambda p: (tokens, sptr)                                             # noqa: E731
    else:
        corpus_of = O.deepwalk_corpus(lists, 40, DEEPWALK_WALKS, DEEPWALK_LENGTH, 3)
    counts = O.word_counts(corpus_of(0)[0], 40)
    assert np.array_equal(model.counts, counts)
    t2, s2 = model.corpus(2)
    assert np.array_equal(_np(t2), corpus_of(2)[0]) and np.array_equal(_np(s2), corpus_of(2)[1])
    want = O.epoch_pairs(*corpus_of(2), O.keep_thresholds(counts), 5, 3, 2)
    assert len(want[0]) > 500 and all(np.array_equal(_np(g), w) for g, w in zip(model.last_epoch_pairs, want))
    # the whole fit against the f32 oracle from the same draws: same pairs, same targets, so only rounding differs
    s0, s1, _ = O.train(corpus_of, 40, 16, 5, 2, 3, 64, hs=name == "deepwalk", dtype=np.float32)
    np.testing.assert_allclose(_np(model.syn0), s0, rtol=1e-3, atol=1e-6)
    np.testing.assert_allclose(_np(model.syn1), s1, rtol=1e-3, atol=1e-6)
    users = np.asarray(info.user_consumed[0])
    np.testing.assert_allclose(_np(model.user_embeds[0]), _np(model.syn0)[users].mean(0), rtol=1e-5, atol=1e-7)
    # predict / recommend / kNN
    preds = model.predict(user=[0, 1, 2], item=[0, 11, 25])
    assert len(preds) == 3 and np.isfinite(preds).all()
    recs = model.recommend_user(user=5, n_rec=7)[5]
    assert len(recs) == 7 and not set(recs.tolist()) & {info.id2item[i] for i in info.user_consumed[info.user2id[5]]}
    assert len(model.recommend_user(user=-7, n_rec=5)[-7]) == 5 and len(model.default_recs) == 40
    model.init_knn(approximate=False, sim_type="cosine")
    assert len(model.search_knn_items(3, 5)) == 5
    # checkpoints: full, and the reference's inference layout
    model.save(str(tmp_path), name)
    full = cls.load(str(tmp_path), name, info)
    assert torch.equal(full.syn0, model.syn0) and torch.equal(full.syn1, model.syn1) and np.array_equal(full.counts, counts)
    assert torch.equal(full.item_embeds, model.item_embeds) and torch.equal(full.user_embeds, model.user_embeds)
    with np.load(os.path.join(tmp_path, name + "_variables.npz")) as z:
        assert {"w2v/syn0", "w2v/syn1", "w2v/counts", "opt::epochs", "user_embed", "item_embed"} <= set(z.files)
        assert int(z["opt::epochs"]) == 2
    model.save(str(tmp_path), name + "_inf", inference_only=True)
    assert not os.path.exists(os.path.join(tmp_path, name + "_inf_variables.npz"))
    with np.load(os.path.join(tmp_path, name + "_inf.npz")) as z:
        assert set(z.files) == {"user_embed", "item_embed"} and z["item_embed"].shape == (41, 16)
    inf = cls.load(str(tmp_path), name + "_inf", info)
    a, b = model.recommend_user(user=[1, 2, 3], n_rec=6), inf.recommend_user(user=[1, 2, 3], n_rec=6)
    assert all(np.array_equal(a[u], b[u]) for u in (1, 2, 3))
    np.testing.assert_array_equal(full.predict(user=[0, 1], item=[3, 4]), model.predict(user=[0, 1], item=[3, 4]))
    # retraining on merged data with more items: saved rows by id, inner nodes by index, fresh draws for the new items
    new_lists = [[100 + (u + j) % 6 for j in range(4)] + [u % 40] for u in range(30)]
    train2, info2 = DatasetPure.merge_trainset(_frame(new_lists, user0=1000), info)
    assert info2.n_items == 46
    m2 = cls("ranking", info2, **dict(kw, n_epochs=1))
    m2.rebuild_model(str(tmp_path), name)
    fresh = cls("ranking", info2, **kw).initial_tables()[0]
    assert torch.equal(m2.syn0[:40], model.syn0) and np.array_equal(_np(m2.syn0[40:]), fresh[40:])
    assert torch.equal(m2.syn1[:40], model.syn1[:40]) and not bool(m2.syn1[40:46].any())
    if name == "deepwalk":
        assert m2.syn1.shape[0] == 91 and torch.equal(m2.syn1[46:46 + 39], model.syn1[40:]) and not bool(m2.syn1[85:].any())
    assert len(m2.counts) == 46 and m2.counts[40:].min() > 0
    m2.fit(train2, neg_sampling=True, verbose=0)
    assert m2.item_embeds.shape == (47, 16) and not torch.equal(m2.syn0[:40], model.syn0)
    assert bool(torch.isfinite(m2.item_embeds).all())


def test_verbose_fit_reports_the_loss_and_two_fits_agree(dev, cluster_data, capsys):
    train, info, _, _ = cluster_data
    tables = []
    for _ in range(2):
        m = DeepWalk("ranking", info, embed_size=8, n_walks=2, walk_length=6, n_epochs=2, batch_size=128, seed=1, norm_embed=True)
        m.fit(train, neg_sampling=True, verbose=1)
        tables.append((m.syn0.clone(), m.syn1.clone()))
    assert torch.equal(tables[0][0], tables[1][0]) and torch.equal(tables[0][1], tables[1][1])
    assert "train_loss" in capsys.readouterr().out and 0 < m.last_epoch_loss < 12 * np.log(2) + 1
    np.testing.assert_allclose(_np(torch.linalg.vector_norm(m.item_embeds[:40], dim=1)), 1.0, rtol=1e-5)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_planted_clusters_separate(dev, cluster_data, name):
    """The property of tests/test_word2vec_cpu.py on the device, with the margins found there on the oracle."""
    train, info, _, cluster_of = cluster_data
    cls, kw = MODELS[name]
    epochs, margin = (ITEM2VEC_EPOCHS, ITEM2VEC_MARGIN) if name == "item2vec" else (DEEPWALK_EPOCHS, DEEPWALK_MARGIN)
    model = cls("ranking", info, embed_size=16, n_epochs=epochs, batch_size=CLUSTER_WINDOW, seed=1, **kw)
    model.fit(train, neg_sampling=True, verbose=0)
    within, across = O.cluster_cosines(_np(model.syn0), cluster_of)
    print(f"W2V-FIGURE planted-clusters model={name} within={within:.4f} across={across:.4f} margin={margin}")
    assert within - across >= margin
