"""RsUserCF / RsItemCF without a device: the numpy restatement (tests/rs_cf_oracle.py) against the neighbour lists that the
reference's Rust unit tests assert (tests/golden/rs_cf_rust_cases.json), with the reference's aliasing pair keys and with
the package's pair-identity keys; the constructors against the reference's signature; the argument checks that come before
any device work."""
import inspect
import json
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from librecommender_amd import algorithms, bases
from librecommender_amd.algorithms import ItemCF, RsItemCF, RsUserCF, UserCF

from . import rs_cf_oracle as O
from .test_api_signatures_cpu import accepts

GOLDEN = Path(__file__).resolve().parent / "golden"
CASES = json.loads((GOLDEN / "rs_cf_rust_cases.json").read_text())


def step_matrix(step):
    m = step["x_major"]
    return sp.csr_matrix((np.array(m["data"], dtype=np.float32), m["indices"], m["indptr"]),
                         shape=(len(m["indptr"]) - 1, step["n_y"]))


def run_engine(alias_keys):
    """The neighbour lists (row -> ids) after each step of the Rust cases."""
    e = O.Engine(CASES["min_common"], alias_keys=alias_keys)
    out = []
    for step in CASES["steps"]:
        e.update(step_matrix(step), step["n_x"])
        out.append({str(r): e.neighbour_ids(r, CASES["k_sim"]) for r in range(step["n_x"]) if e.neighbour_ids(r)})
    return out


def test_the_golden_matrices_are_consistent():
    for step in CASES["steps"]:
        x, m = step_matrix(step), step["y_major"]
        y = sp.csr_matrix((np.array(m["data"], dtype=np.float32), m["indices"], m["indptr"]),
                          shape=(len(m["indptr"]) - 1, step["n_x"]))
        a = np.zeros((step["n_x"], step["n_y"]), dtype=np.float32)
        a[: x.shape[0]] = x.toarray()
        b = np.zeros((step["n_y"], step["n_x"]), dtype=np.float32)
        b[: y.shape[0]] = y.toarray()
        assert np.array_equal(a.T, b), step["name"]


def test_oracle_with_aliasing_keys_reproduces_every_rust_list():
    got = run_engine(alias_keys=True)
    for step, lists in zip(CASES["steps"], got):
        assert lists == step["neighbours"], step["name"]


def test_oracle_with_pair_keys_differs_in_two_rows_only():
    got = run_engine(alias_keys=False)
    quoted = CASES["pair_identity_first_update"]
    assert quoted == {"1": [0, 3, 2, 5, 4], "2": [4, 1, 3, 5, 0]}
    assert got[0] == CASES["steps"][0]["neighbours"]                 # the non-incremental lists agree either way
    for step, lists in zip(CASES["steps"][1:], got[1:]):
        assert set(lists) == set(step["neighbours"])
        differ = {r for r in lists if lists[r] != step["neighbours"][r]}
        assert differ == set(quoted), step["name"]
    assert {r: got[1][r] for r in quoted} == quoted
    # the second update touches neither row: both keep their lists
    assert {r: got[2][r] for r in quoted} == quoted


def test_oracle_staleness_and_threshold():
    # pair (0, 1) shares y 0; a later update touches row 0 through pair (0, 2) only: (0, 1) keeps its cosine although
    # sumsq[0] has grown, and with min_common 2 the pair (0, 2) becomes visible only once its count reaches 2
    first = sp.csr_matrix(np.array([[1, 0, 0], [2, 0, 0], [0, 3, 0]], dtype=np.float32))
    second = sp.csr_matrix(np.array([[0, 1, 2], [0, 0, 0], [0, 0, 5]], dtype=np.float32))
    e = O.Engine(1).update(first, 3)
    before = e.sim[0][1]
    assert before == np.float32(1.0) and 2 not in e.sim[0]
    e.update(second, 3)
    assert e.sim[0][1] == before and e.sumsq[0] == np.float32(6.0) and (0, 1) not in e.touched
    assert e.cum[(0, 2)][2:] == [np.float32(10.0), 1]
    e2 = O.Engine(2).update(first, 3)
    assert e2.num_sim_elements() == 0
    e2.update(second, 3)
    assert e2.num_sim_elements() == 0                    # (0, 2) has count 1 so far
    e2.update(second, 3)                                 # the same interactions again: counted again
    assert e2.cum[(0, 2)][3] == 2 and e2.neighbour_ids(0) == [2] and e2.neighbour_ids(1) == []


@pytest.mark.parametrize("min_common", [1, 2])
def test_array_engine_equals_the_dictionary_engine(min_common):
    # the array form that the device tests use on the sample file, against the dictionary form that the Rust lists pin
    rng = np.random.default_rng(7)
    d, a = O.Engine(min_common), O.ArrayEngine(min_common)
    for n_x, n_y, nnz in ((40, 30, 300), (55, 30, 200), (55, 42, 350)):
        key = np.unique(rng.integers(0, n_x, nnz) * n_y + rng.integers(0, n_y, nnz))
        x = sp.csr_matrix((rng.standard_normal(len(key)).astype(np.float32), (key // n_y, key % n_y)), shape=(n_x, n_y))
        d.update(x, n_x)
        a.update(x, n_x)
        for p, q in zip(d.state(), a.state()):
            assert p.dtype == q.dtype and p.tobytes() == q.tobytes()
        assert d.sumsq.tobytes() == a.sumsq.tobytes() and d.num_sim_elements() == a.num_sim_elements()
        assert all(d.neighbours(r, 8) == a.neighbours(r, 8) for r in range(n_x))
        touched = {(int(k) >> 32, int(k) & 0xFFFFFFFF) for k in a.key[a.touched]}
        assert touched == d.touched
    e = O.ArrayEngine(CASES["min_common"])               # and on the Rust cases
    for step, lists in zip(CASES["steps"], run_engine(alias_keys=False)):
        e.update(step_matrix(step), step["n_x"])
        assert {str(r): e.neighbour_ids(r, CASES["k_sim"]) for r in range(step["n_x"]) if e.neighbour_ids(r)} == lists


def test_oracle_predict_cuts_before_it_intersects():
    nbs = [(7, np.float32(0.9)), (3, np.float32(0.5)), (5, np.float32(0.5)), (1, np.float32(0.25))]
    cols, vals = [1, 3, 5], [4.0, 2.0, -1.0]
    p, none = O.predict_list(nbs, cols, vals, 2, "ranking", 0.0)
    assert (p, none) == (np.float32(0.5), False)                      # 1 is ranked beyond k_sim: only 3 counts
    p, none = O.predict_list(nbs, cols, vals, 4, "ranking", 0.0)
    assert p == np.float32((0.5 + 0.5 + 0.25) / 3)
    p, _ = O.predict_list(nbs, cols, vals, 4, "rating", 3.0)
    assert p == np.float32(np.float32(1.0 / 1.25) + np.float32(-0.5 / 1.25) + np.float32(1.0 / 1.25))
    assert O.predict_list(nbs, [2, 4], [1.0, 1.0], 4, "rating", 3.0) == (np.float32(3.0), True)


def test_constructors_accept_the_reference_signature():
    golden = json.loads((GOLDEN / "rs_cf_signature.json").read_text())
    for cls in (RsItemCF, RsUserCF):
        ref = golden[f"algorithms.{cls.__name__}.__init__"]
        assert accepts(ref, cls.__init__) is None
        mine = inspect.signature(cls.__init__).parameters
        assert [p[0] for p in ref] == list(mine)                       # nothing added either
        assert list(inspect.signature(cls.fit).parameters) == [
            "self", "train_data", "neg_sampling", "verbose", "eval_data", "metrics", "k", "eval_batch_size", "eval_user_num"]
        assert list(inspect.signature(cls.rebuild_model).parameters) == ["self", "path", "model_name"]
        assert cls.__name__ in algorithms.__all__
    assert "RsCfBase" in bases.__all__ and issubclass(RsItemCF, bases.RsCfBase) and issubclass(RsUserCF, bases.CfBase)
    from librecommender_amd.algorithms import swing

    assert callable(swing.merge_interactions) and callable(swing._resized)


def _info():
    from librecommender_amd.data import DatasetPure

    df = pd.DataFrame({"user": [1, 1, 2, 2, 3], "item": [10, 11, 10, 11, 12], "label": [1, 1, 1, 1, 1]})
    return DatasetPure.build_trainset(df)


@pytest.mark.parametrize("cls", [RsItemCF, RsUserCF])
def test_bad_arguments_raise_before_any_device_work(cls):
    _, info = _info()
    with pytest.raises(ValueError, match="mode"):
        cls("ranking", info, mode="sideways")
    with pytest.raises(ValueError, match="task"):
        cls("classification", info)
    m = cls("ranking", info, k_sim=7, min_common=2, mode="forward", num_threads=3)
    assert (m.k_sim, m.min_common, m.mode, m.num_threads, m.incremental, m.default_pred) == (7, 2, "forward", 3, False, 0.0)
    assert m.sim_type == "cosine" and m.cf_type == ("item_cf" if cls is RsItemCF else "user_cf")
    assert m._hparams() == {"task": "ranking", "k_sim": 7, "num_threads": 3, "min_common": 2, "mode": "forward", "seed": 42,
                            "lower_upper_bound": None}
    assert m.sim_matrix is None
    with pytest.raises(RuntimeError, match="call `fit` or `load` first"):
        m.pair_state()
    with pytest.raises(OSError):
        cls.load("/nonexistent-folder", "m", info)
    with pytest.raises(OSError):
        m.rebuild_model("/nonexistent-folder", "m")


@pytest.mark.parametrize("cls", [ItemCF, UserCF])
def test_the_cython_models_still_refuse_retraining(cls):
    _, info = _info()
    with pytest.raises(NotImplementedError, match="doesn't support model retraining"):
        cls("ranking", info).rebuild_model("anywhere", "m")
