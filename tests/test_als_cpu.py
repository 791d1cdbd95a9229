"""ALS without a GPU: constructor checks, the reference's signatures and initial draws, the fp64 restatement of the
half-sweep (tests/als_oracle.py) against the reference's own numpy showcases, and the C-ABI's host-side queries."""
import inspect
import sys

import numpy as np
import pandas as pd
import pytest

from librecommender_amd import _lib
from librecommender_amd.algorithms import ALS
from librecommender_amd.data import DatasetPure
from librecommender_amd.utils.initializers import truncated_normal
from oracle import ref_loader

from . import als_oracle as O

needs_ref = pytest.mark.skipif(not ref_loader.available(), reason="reference checkout absent")


@pytest.fixture
def ref():
    """The reference importable for one test; sys.path is restored afterwards (the reference checkout has a `tests`
    package of its own, which would shadow this one for processes spawned by later tests)."""
    saved = list(sys.path)
    ref_loader.load()
    yield
    sys.path[:] = saved


def small_info(n=400, seed=0):
    rng = np.random.default_rng(seed)
    df = pd.DataFrame({"user": rng.integers(0, 40, n), "item": rng.integers(0, 60, n),
                       "label": rng.integers(1, 6, n).astype(np.float32)})
    return DatasetPure.build_trainset(df)


@pytest.mark.parametrize("task", ["rating", "ranking"])
@pytest.mark.parametrize("reg", [None, 0, -1.0, 1, 0.0])
def test_reg_must_be_positive_float(task, reg):
    _, info = small_info()
    with pytest.raises(ValueError):
        ALS(task, info, reg=reg)


def test_embed_size_limit():
    _, info = small_info()
    ALS("ranking", info, embed_size=128, reg=0.1)
    with pytest.raises(ValueError, match="128"):
        ALS("ranking", info, embed_size=129, reg=0.1)


def test_bad_task():
    _, info = small_info()
    with pytest.raises(ValueError):
        ALS("ctr", info, reg=0.1)


@needs_ref
def test_signatures_match_reference(ref):
    from libreco.algorithms.als import ALS as RefALS

    assert inspect.signature(ALS.__init__) == inspect.signature(RefALS.__init__)
    assert inspect.signature(ALS.fit) == inspect.signature(RefALS.fit)


@needs_ref
@pytest.mark.parametrize("seed", [0, 42, 7])
def test_initial_tables_are_the_reference_draws(ref, seed):
    from libreco.utils.initializers import truncated_normal as ref_tn

    _, info = small_info()
    model = ALS("ranking", info, embed_size=24, reg=0.1, seed=seed)
    u, i = model.initial_tables()
    rng = np.random.default_rng(seed)
    ru = ref_tn(rng, shape=[info.n_users, 24], mean=0.0, scale=0.03)
    ri = ref_tn(rng, shape=[info.n_items, 24], mean=0.0, scale=0.03)
    assert u.dtype == ru.dtype == np.float32
    np.testing.assert_array_equal(u, ru)
    np.testing.assert_array_equal(i, ri)


@needs_ref
@pytest.mark.parametrize("shape,scale,tol", [([1000], 0.05, 5), ([300, 7], 1.0, 0), ([50, 64], 0.03, 2)])
def test_truncated_normal_bit_for_bit(ref, shape, scale, tol):
    from libreco.utils.initializers import truncated_normal as ref_tn

    a = truncated_normal(np.random.default_rng(3), shape, mean=0.1, scale=scale, tolerance=tol)
    b = ref_tn(np.random.default_rng(3), shape, mean=0.1, scale=scale, tolerance=tol)
    np.testing.assert_array_equal(a, b)


def _case(seed, rows=30, cols=50, K=6):
    rng = np.random.default_rng(seed)
    deg = rng.integers(1, 12, rows)
    indptr, indices, val = O.random_csr(rng, rows, cols, deg)
    X = rng.normal(0, 0.3, (rows, K)).astype(np.float32)
    Y = rng.normal(0, 0.3, (cols, K)).astype(np.float32)
    return indptr, indices, val, X, Y


@needs_ref
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("mode", ["explicit", "implicit"])
def test_restatement_matches_reference_least_squares(ref, seed, mode):
    from scipy.sparse import csr_matrix

    from libreco.algorithms.als import least_squares

    indptr, indices, val, X, Y = _case(seed)
    implicit = mode == "implicit"
    if implicit:
        val = val * 10 + 1
    ref = X.astype(np.float64).copy()
    csr = csr_matrix((val.astype(np.float64), indices, indptr), shape=(X.shape[0], Y.shape[0]))
    least_squares(csr, ref, Y.astype(np.float64), 0.1, X.shape[1], X.shape[0], mode)
    ours = O.half_sweep(indptr, indices, val, X, Y, 0.1, implicit, use_cg=False)
    # the reference's implicit showcase keeps A and b in float32
    np.testing.assert_allclose(ours, ref, rtol=1e-4 if implicit else 1e-6, atol=1e-6 if implicit else 1e-9)


@needs_ref
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_matches_reference_least_squares_cg(ref, seed):
    from scipy.sparse import csr_matrix

    from libreco.algorithms.als import least_squares_cg

    indptr, indices, val, X, Y = _case(seed)
    val = val * 10 + 1
    ref = X.astype(np.float64).copy()
    csr = csr_matrix((val.astype(np.float64), indices, indptr), shape=(X.shape[0], Y.shape[0]))
    least_squares_cg(csr, ref, Y.astype(np.float64), 0.1, X.shape[1], X.shape[0], "implicit", cg_steps=3)
    ours = O.half_sweep(indptr, indices, val, X, Y, 0.1, True, use_cg=True)
    np.testing.assert_allclose(ours, ref, rtol=1e-6, atol=1e-9)


def test_restatement_posv_failure_and_exact_minimum():
    indptr, indices, val, X, Y = _case(4)
    ours = O.half_sweep(indptr, indices, val, X, Y, 0.1, False, use_cg=False)
    # the exact solve is the minimiser of the objective over X
    f0 = O.objective(indptr, indices, val, ours, Y, 0.1, False)
    rng = np.random.default_rng(0)
    for _ in range(3):
        assert O.objective(indptr, indices, val, ours + rng.normal(0, 1e-3, ours.shape), Y, 0.1, False) > f0
    with pytest.raises(ValueError, match="row 0"):
        O.half_sweep(indptr, indices, -np.abs(val) - 5, X, Y, 1e-3, True, use_cg=False)   # w = c - 1 < 0


def test_cabi_size_and_support_queries():
    lib = _lib.load()
    assert [lib.lr_als_supported(k) for k in (0, 1, 20, 64, 128, 129)] == [0, 1, 1, 1, 1, 0]
    import ctypes as C

    lim = (C.c_int32 * 3)()
    assert lib.lr_als_plan_params(64, lim) == 0
    light, heavy, chunk = list(lim)
    assert 1 <= light < heavy and chunk >= 1
    assert lib.lr_als_plan_params(129, lim) == _lib.LR_EINVAL
    assert lib.lr_als_ws_bytes(10, 64) == 10 * (64 * 64 + 64) * 4
    assert lib.lr_als_ws_bytes(10, 20) == 10 * (20 * 20 + 20) * 4
    assert lib.lr_als_ws_bytes(0, 64) > 0 and lib.lr_als_ws_bytes(1, 200) == 0
    assert lib.lr_als_gram_ws_bytes(10_000_000, 64) >= 64 * 64 * 4
    assert lib.lr_als_gram_ws_bytes(5, 129) == 0
    # argument checks before any launch: a plan that does not cover the rows is refused
    assert lib.lr_als_half_sweep_f32(None, None, None, 5, None, None, 8, None, 1, 1, 3, None, 1, 1, 1, 0,
                                     None, None, 0, 15, None) == _lib.LR_EINVAL
    assert lib.lr_als_half_sweep_f32(None, None, None, 0, None, None, 8, None, 1, 1, 3, None, 0, 0, 0, 0,
                                     None, None, 0, 15, None) == 0
