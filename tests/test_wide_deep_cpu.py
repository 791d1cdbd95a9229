"""Wide & Deep without a device: the constructor against the reference's recorded signature, the `lr` checks, the FTRL oracle
(tests/wide_deep_oracle.py) against a known answer and against itself, and the host-side queries of csrc/ftrl.hip."""
import json
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from librecommender_amd import _lib, algorithms, ops
from librecommender_amd.algorithms import WideDeep

from . import wide_deep_oracle as O
from .test_api_signatures_cpu import accepts

ROOT = Path(__file__).resolve().parent.parent


def _info():
    col = lambda: SimpleNamespace(name=[], index=[])
    return SimpleNamespace(n_users=5, n_items=7, user_consumed={}, sparse_col=col(), dense_col=col(), data_size=100)


def test_constructor_accepts_the_reference_signature():
    golden = json.loads((ROOT / "tests" / "golden" / "wide_deep_signature.json").read_text())
    problem = accepts(golden["algorithms.WideDeep.__init__"], WideDeep.__init__)
    assert problem is None, problem
    assert "WideDeep" in algorithms.__all__


def test_lr_default_and_checks():
    assert WideDeep("ranking", _info()).lr == {"wide": 0.01, "deep": 1e-4}
    assert WideDeep("ranking", _info(), lr={"wide": 0.1, "deep": 0.2}).lr == {"wide": 0.1, "deep": 0.2}
    for bad in (0.01, {"wide": 0.01}, {"deep": 0.01}, [0.01, 0.01]):
        with pytest.raises(AssertionError, match="wide and deep"):
            WideDeep("ranking", _info(), lr=bad)
    with pytest.raises(ValueError, match="loss_type"):
        WideDeep("ranking", _info(), loss_type="bpr")
    assert WideDeep("ranking", _info(), reg=0.01).dense_adam                    # `reg` selects the dense forms


def test_lr_decay_moves_both_rates_on_the_staircase():
    m = WideDeep("ranking", _info(), lr_decay=True, batch_size=10)              # 10 steps per stair
    m.net = SimpleNamespace(step=0, lr=None)
    assert m.current_lr() == {"wide": 0.01, "deep": 1e-4}
    m.net.step = 25
    m.apply_lr_schedule()
    assert m.net.lr == {"wide": 0.01 * 0.96 ** 2, "deep": 1e-4 * 0.96 ** 2}
    still = WideDeep("ranking", _info(), batch_size=10)
    still.net = SimpleNamespace(step=25, lr="untouched")
    still.apply_lr_schedule()
    assert still.net.lr == "untouched"


def test_tf_variable_io_is_refused():
    m = WideDeep("ranking", _info())
    with pytest.raises(NotImplementedError):
        m.save_tf_variables("x", "y")
    with pytest.raises(NotImplementedError):
        m.load_tf_variables("x", "y")


def test_ftrl_known_answer():
    """lr 0.01, l1 1e-3, l2 0, var 0.5, accum 0.1, linear 0, g 0.2, recomputed in f64 here."""
    accum = 0.1 + 0.2 * 0.2
    linear = 0.2 - (np.sqrt(accum) - np.sqrt(0.1)) / 0.01 * 0.5
    var = (np.sign(linear) * 1e-3 - linear) / (np.sqrt(accum) / 0.01)
    got = O.ftrl_elem(0.5, 0.1, 0.0, 0.2, 0.01, 1e-3, 0.0)
    assert np.allclose(got, (var, accum, linear), rtol=1e-14, atol=0)
    # the figures quoted with the case (var 0.072051, accum 0.14, linear -2.696897): f64 gives linear = -2.6968986, so the quoted
    # linear is good to 2e-6, the other two to the last digit
    assert abs(got[0] - 0.072051) < 5e-7 and abs(got[1] - 0.14) < 1e-15 and abs(got[2] + 2.696897) < 2e-6


def test_rows_equal_dense_on_the_scattered_sum():
    """A stream with duplicates: the row form equals the dense form on the scattered sum at the touched rows, and leaves the
    other rows' three values alone."""
    rng = np.random.default_rng(0)
    V, n = 50, 400
    ids = rng.integers(-3, 40, n)                                               # duplicates, dropped ids, rows 40.. untouched
    grad, var = rng.standard_normal(n), rng.uniform(-0.5, 0.5, V)
    accum, linear = 0.1 + rng.random(V), rng.standard_normal(V)
    rv, ra, rl, rows = O.ftrl_rows(var, accum, linear, ids, grad, 0.01)
    gsum, rows2 = O.scatter_sum(V, ids, grad)
    dv, da, dl = O.ftrl_dense(var, accum, linear, gsum, 0.01)
    assert np.array_equal(rows, rows2) and np.array_equal(rows, np.arange(40))
    assert np.array_equal(rv[rows], dv[rows]) and np.array_equal(ra[rows], da[rows]) and np.array_equal(rl[rows], dl[rows])
    rest = np.setdiff1d(np.arange(V), rows)
    assert len(rest) == 10
    assert np.array_equal(rv[rest], var[rest]) and np.array_equal(ra[rest], accum[rest]) and np.array_equal(rl[rest], linear[rest])


def test_first_dense_step_zeroes_what_the_row_form_leaves_alone():
    """Fresh slots and a zero gradient: |linear| = 0 <= l1, so the dense form sets var to exactly 0; the row form does not
    touch a row outside its stream."""
    rng = np.random.default_rng(1)
    var = rng.uniform(-0.5, 0.5, 20)
    accum, linear = np.full(20, O.INIT_ACCUM), np.zeros(20)
    dv, da, dl = O.ftrl_dense(var, accum, linear, np.zeros(20), 0.01)
    assert not dv.any() and np.array_equal(da, accum) and not dl.any()
    rv, _, _, rows = O.ftrl_rows(var, accum, linear, np.array([3, 3, 7]), np.array([0.5, -0.5, 0.25]), 0.01)
    assert list(rows) == [3, 7] and rv[3] == 0.0 and rv[7] != 0.0               # a touched row whose gradients cancel: 0.0 too
    keep = np.setdiff1d(np.arange(20), rows)
    assert np.array_equal(rv[keep], var[keep]) and var[keep].all()


def test_workspace_query_and_constants():
    lib = _lib.load()
    sizes = [lib.lr_ftrl_rows_ws_bytes(n) for n in (0, 1, 33, 256, 8192, 8192 * 39, 1 << 24)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert lib.lr_ftrl_rows_ws_bytes(-1) == 0
    # the two constants the kernel commits to are those `ops` publishes
    src = (ROOT / "librecommender_amd" / "csrc" / "ftrl.hip").read_text()
    const = lambda name: int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))
    assert const("kFtrlLongRun") == ops.FTRL_LONG_RUN and const("kFtrlChunk") == ops.FTRL_CHUNK
    assert ops.FTRL_INIT_ACCUM == O.INIT_ACCUM == 0.1


def test_kernel_cases_hold_what_they_are_named_for():
    T, C = ops.FTRL_LONG_RUN, ops.FTRL_CHUNK
    _, _, runs = O.oracle_rows("collide", T, C)
    assert runs.sum() == 64 and 0 < runs.max() <= T
    _, _, runs = O.oracle_rows("boundaries", T, C)
    assert sorted(runs[runs > 0]) == sorted([T, T + 1, C, C + 1, 3 * C + 5, 1, 2])
    _, _, runs = O.oracle_rows("two_valued", T, C)
    assert runs[2] == 0 and runs[:2].sum() == 8192 and runs[:2].min() > 3900
    c, (var, _, linear, rows), _ = O.oracle_rows("threshold", T, C)
    inside = np.abs(linear[rows]) <= c["l1"]
    assert 0.2 < inside.mean() < 0.8 and not var[rows][inside].any() and var[rows][~inside].all()
    assert c["var"][:5].all() and not var[:5].any()                              # zero gradient at fresh slots: exactly 0.0
    c, (_, accum, _, rows), _ = O.oracle_rows("dropped", T, C)
    assert (c["ids"] < 0).any() and (c["ids"] >= c["V"]).any() and rows.max() < c["V"]
