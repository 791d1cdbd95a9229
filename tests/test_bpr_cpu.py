"""BPR without a device: the oracle (tests/bpr_oracle.py) against recorded outputs of the compiled reference engine, the
oracle's power to tell the readings of the window semantics apart, and the constructor's contract."""
import inspect
import os

import numpy as np
import pytest

from librecommender_amd.algorithms import BPR

from . import bpr_oracle as O

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "bpr_engine.npz")

# `libreco/algorithms/bpr.py:93-114`, position by position
REFERENCE_SIGNATURE = [
    ("task", "ranking"), ("data_info", None), ("loss_type", "bpr"), ("embed_size", 16), ("norm_embed", False), ("n_epochs", 20),
    ("lr", 0.001), ("lr_decay", False), ("epsilon", 1e-5), ("reg", None), ("batch_size", 256), ("sampler", "random"),
    ("num_neg", 1), ("use_tf", True), ("seed", 42), ("lower_upper_bound", None), ("tf_sess_config", None), ("optimizer", "adam"),
    ("num_threads", 1)]


@pytest.mark.parametrize("optimizer", O.OPTIMIZERS)
@pytest.mark.parametrize("reg_index", [0, 1])
def test_oracle_matches_compiled_reference(optimizer, reg_index):
    """The fixture holds inputs and outputs of the reference's compiled `bpr_update` at `num_threads=1` (40 users x 12
    items, 3,000 samples, K = 16, two epochs; the consumed CSR lists all items but one per user, so the reference's
    rejection loop can only end on that item).  The oracle at window 1 must match it to 2e-6 absolute."""
    z = np.load(GOLDEN)
    reg = float(z["regs"][reg_index])
    lr = float(z["lrs"][list(z["optimizers"]).index(optimizer)])
    users, pos, neg = z["users"], z["pos"], z["neg"]
    # the negatives are what the CSR forces
    for u in range(int(z["n_users"])):
        row = z["indices"][z["indptr"][u]:z["indptr"][u + 1]]
        assert np.array_equal(np.setdiff1d(np.arange(int(z["n_items"])), row), np.unique(neg[users == u])) or not (users == u).any()
    U, I = z["U0"].copy(), z["I0"].copy()
    state = O.new_state(optimizer, U, I)
    for epoch in (1, 2):
        O.engine_epoch(optimizer, users, pos, neg, U, I, state, lr, reg, epoch, 1, "f64")
        tag = f"{optimizer}_r{reg_index}_e{epoch}"
        want = [z[tag + "_U"], z[tag + "_I"]] + [z[f"{tag}_{side}s{k}"] for side in "ui" for k in range(len(state[side]))]
        dev = O.max_diff(O.case_arrays(U, I, state), want)
        print(tag, "max |oracle - compiled reference| =", dev)
        assert dev <= 2e-6
    assert np.abs(U - z["U0"]).max() > 0.2            # the values moved: the comparison is not vacuous


def test_initial_draws_are_the_references():
    z = np.load(GOLDEN)
    U, I = O.truncated_normal_tables(int(z["n_users"]), int(z["n_items"]), int(z["embed_size"]), int(z["seed"]))
    assert np.array_equal(U, z["U0"]) and np.array_equal(I, z["I0"])

    class Info:
        n_users, n_items, user_consumed, global_mean, min_max_rating = int(z["n_users"]), int(z["n_items"]), {}, 0.0, (0, 1)

    u, i = BPR("ranking", Info(), use_tf=False, seed=int(z["seed"])).initial_tables()
    assert np.array_equal(u, z["U0"]) and np.array_equal(i, z["I0"])


def test_signature_is_the_references():
    params = list(inspect.signature(BPR.__init__).parameters.values())[1:]
    got = [(p.name, p.default) for p in params[: len(REFERENCE_SIGNATURE)]]
    assert got == REFERENCE_SIGNATURE
    assert [p.name for p in params[len(REFERENCE_SIGNATURE):]] == ["device", "dense_adam"]    # package-only keywords behind them
    fit = list(inspect.signature(BPR.fit).parameters)
    assert fit == ["self", "train_data", "neg_sampling", "verbose", "shuffle", "eval_data", "metrics", "k", "eval_batch_size",
                   "eval_user_num", "num_workers"]                                          # bpr.py:206-218


def test_constructor_checks():
    class Info:
        n_users, n_items, user_consumed, global_mean, min_max_rating = 5, 7, {}, 0.0, (0, 1)

    with pytest.raises(AssertionError, match="only suitable for ranking"):
        BPR("rating", Info())
    with pytest.raises(AssertionError, match="bpr loss"):
        BPR("ranking", Info(), loss_type="cross_entropy")
    with pytest.raises(ValueError, match="optimizer must be one of these"):
        BPR("ranking", Info(), use_tf=False, optimizer="adagrad")
    for bad in (0, 256, 1000):
        with pytest.raises(ValueError, match="embed_size"):
            BPR("ranking", Info(), embed_size=bad)
    with pytest.raises(ValueError, match="dense_adam=True"):
        BPR("ranking", Info(), reg=0.01)                    # the mini-batch mode's l2 moves every row: dense update only
    BPR("ranking", Info(), reg=0.01, dense_adam=True)
    m = BPR("ranking", Info(), reg=0.01, use_tf=False, tf_sess_config={"x": 1}, num_threads=8)
    assert m.reg == 0.01 and m.batch_size == 256 and m.optimizer == "adam"


@pytest.mark.parametrize("optimizer", O.OPTIMIZERS)
def test_oracle_discriminates(optimizer):
    """On the window case of the device test the other readings of the semantics — the plain sequence (window 1), the
    chain walked backwards, a `reg` term taken from the row as it stands instead of from the window's start — each move
    the result by more than the bound the device is held to (10 x the f32 / f64 gap of the oracle itself)."""
    K, reg, epoch = 16, 0.01, 3
    lr = O.WINDOW_LR[optimizer]
    users, pos, neg, U0, I0, s0 = O.window_case(K, optimizer)
    W = len(users)

    def run(window=W, variant="f64", **kw):
        U, I, st = O.copy_case(U0, I0, s0)
        O.engine_epoch(optimizer, users, pos, neg, U, I, st, lr, reg, epoch, window, variant, **kw)
        return O.case_arrays(U, I, st)

    ref = run()
    bound = 10 * O.max_diff(run(variant="f32"), ref)
    gaps = {"window 1": O.max_diff(run(window=1), ref), "fresh reg term": O.max_diff(run(reg_term="fresh"), ref)}
    if optimizer != "sgd":      # reversing an sgd chain of window-start gradients only reorders a sum: rounding, not semantics
        gaps["descending chain"] = O.max_diff(run(chain="descending"), ref)
    print(optimizer, "bound", bound, gaps)
    assert bound < 1e-3
    for name, gap in gaps.items():
        assert gap > bound, (name, gap, bound)
