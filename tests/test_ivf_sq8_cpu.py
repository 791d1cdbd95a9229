"""The IVF-SQ8 index without a device: the numpy oracle itself (encoding of hand-made rows, recall against the Flat oracle at the
same probe, the off-grid case of the GPU test), the C ABI table, the seams' signatures and the argument errors that come before
any device work."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from librecommender_amd import _lib, ops, serving
from librecommender_amd.recommendation.ivf_sq8 import IVFSQ8Index

from . import ivf_oracle as O
from . import ivf_sq8_oracle as Q

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ["lr_ivf_sq8_supported", "lr_ivf_sq8_search_ws_bytes", "lr_ivf_sq8_encode_f32", "lr_ivf_sq8_search_f32", "lr_ivf_rerank_f32"]


def test_encoding_of_hand_made_rows():
    codes, scales = Q.encode(Q.HAND_MADE)
    assert codes.shape == (5, 16) and codes.dtype == np.int8 and scales.dtype == np.float32
    assert scales[0] == 0 and not codes[0].any()                                    # a zero row
    assert np.array_equal(codes[:, :4], Q.HAND_MADE_CODES)
    assert codes[1, :4].tolist() == [32, -127, 95, 0] and scales[1] == np.float32(2.0) / np.float32(127)    # the maximum is negative
    assert scales[2] == 1 and codes[2, :4].tolist() == [127, 2, 4, 0]               # halves go to even: 2.5 -> 2, 3.5 -> 4, -0.5 -> -0
    assert codes[3, 0] == 127 and scales[3] == np.float32(0.3) / np.float32(127)    # one element (the others are the pad)
    assert codes[4, :4].tolist() == [-127, 127, -127, 127]                          # every element at the maximum
    assert not codes[:, 4:].any()                                                   # padding columns are code 0
    one = Q.encode(np.array([[0.3]], np.float32))
    assert one[0].shape == (1, 16) and one[0][0, 0] == 127 and not one[0][0, 1:].any()
    # list order: row j encodes rows[list_ids[j]]
    perm = np.array([4, 2, 0, 1, 3], np.int32)
    c2, s2 = Q.encode(Q.HAND_MADE, perm)
    assert np.array_equal(c2, codes[perm]) and np.array_equal(s2, scales[perm])
    # decoding errs by at most half a step per element
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((50, 20)) * 0.3).astype(np.float32)
    c, s = Q.encode(x)
    assert c.shape == (50, 32) and np.abs(c).max() == 127
    assert (np.abs(c[:, :20] * s[:, None].astype(np.float64) - x) <= 0.5 * s[:, None] * (1 + 1e-6)).all()


@pytest.mark.parametrize("N,D,nlist,k,nprobe", [(5000, 128, 64, 100, 8), (2000, 16, 8, 10, 2), (5000, 20, 64, 10, 8)])
def test_oracle_recall_against_the_flat_oracle(N, D, nlist, k, nprobe):
    """Recall@k of the SQ8 oracle against the Flat oracle at the same probe, on a Gaussian mixture (32 centres, sigma 0.3, 65
    queries from the same mixture).  Values of this oracle, (refine 0, 1, 2, 4):
      (5000, 128, 64, 100, 8): 0.9931, 0.9931, 1.0000, 1.0000
      (2000,  16,  8,  10, 2): 0.9846, 0.9846, 1.0000, 1.0000
      (5000,  20, 64,  10, 8): 0.9800, 0.9800, 1.0000, 1.0000
    (refine 1 re-scores the same k candidates, so its recall is refine 0's.)"""
    rows, queries = Q.mixture(np.random.default_rng(N + D), N, D, 65)
    cent, _, ptr, ids = O.train_add(rows, nlist, 5)
    _, flat = O.search(queries, cent, ptr, ids, rows, k, nprobe)
    got = {r: Q.recall(Q.search(queries, cent, ptr, ids, rows, k, nprobe, r)[1], flat) for r in (0, 1, 2, 4)}
    print(f"recall@{k} at refine 0/1/2/4:", [round(got[r], 4) for r in (0, 1, 2, 4)])
    assert got[4] >= 0.99
    assert got[1] == got[0] and got[0] > 0.95 and got[2] >= got[0]


def test_the_off_grid_case_is_well_posed():
    """The case of test_off_grid_within_the_bound (tests/test_ivf_sq8_gpu.py): the derived tolerance is far below the score scale,
    and at most 5 % of the queries have a stage-1 gap at the kk cut below it (they are left out of the stage-2 check)."""
    case = Q.off_grid_case()
    assert case["left_out"].mean() <= 0.05
    assert case["tol_max"] < 1e-4 * case["score_scale"]
    assert case["coarse_gap"] > case["coarse_tol"]   # the probe sets do not hang on f32 rounding
    print("coarse gap", case["coarse_gap"], "tol", case["coarse_tol"])
    print("left out:", int(case["left_out"].sum()), "of", case["left_out"].size, "tol_max", case["tol_max"], "scale", case["score_scale"])


def test_grid_dots_are_exact_in_f32():
    """|dot| <= 256 * 2 * 127 at resolution 1/4: 2^18 quarter steps, well inside f32's 24 bits, in any summation order."""
    assert 256 * 2 * 127 * 4 < 2 ** 24
    rng = np.random.default_rng(1)
    rows, q = O.grid(rng, (300, 256)), O.grid(rng, (256,))
    codes, scales = Q.encode(rows)
    dot = codes[:, :256].astype(np.float64) @ q.astype(np.float64)
    assert np.array_equal(dot, dot.astype(np.float32).astype(np.float64)) and np.array_equal(dot * 4, np.rint(dot * 4))
    f32 = np.zeros(300, np.float32)
    for d in range(256):                                    # an f32 chain in column order
        f32 = f32 + codes[:, d].astype(np.float32) * q[d]
    assert np.array_equal(f32.astype(np.float64), dot)


def test_kk_and_stride():
    assert [Q.kk_of(k, r) for k, r in ((10, 0), (10, 1), (10, 4), (300, 4), (1024, 4), (1, 64))] == [10, 10, 40, 1024, 1024, 64]
    assert [ops.ivf_sq8_kk(k, r) for k, r in ((10, 0), (10, 1), (10, 4), (300, 4), (1024, 4), (1, 64))] == [10, 10, 40, 1024, 1024, 64]
    assert [ops.ivf_sq8_stride(D) for D in (1, 4, 6, 16, 20, 128, 250, 256)] == [Q.stride(D) for D in (1, 4, 6, 16, 20, 128, 250, 256)]
    assert ops.ivf_sq8_stride(20) == 32 and ops.ivf_sq8_stride(256) == 256


def test_symbols_are_bound_and_declared():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "libreco_hip.h").read_text(), flags=re.S)
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and re.search(rf"\b{name}\s*\(", header) and hasattr(lib, name)
    # host-only entry points: the envelope and the workspace size
    assert lib.lr_ivf_sq8_supported(1, 10_000_000, 128, 100, 32, 12649, 4) == 1
    assert lib.lr_ivf_sq8_supported(1024, 100_000_000, 128, 100, 128, 40000, 4) == 1
    assert lib.lr_ivf_sq8_supported(3, 1000, 16, 10, 2, 7, 0) == 1 and lib.lr_ivf_sq8_supported(3, 1000, 16, 10, 2, 7, 64) == 1
    assert lib.lr_ivf_sq8_supported(3, 1000, 16, 10, 2, 7, 65) == 0         # refine > 64
    assert lib.lr_ivf_sq8_supported(3, 1000, 16, 10, 2, 7, -1) == 0
    assert lib.lr_ivf_sq8_supported(3, 1000, 6, 10, 2, 7, 4) == 0           # D % 4 != 0: the host pads
    assert lib.lr_ivf_sq8_supported(3, 1000, 16, 1025, 2, 7, 0) == 0        # k > 1024
    assert lib.lr_ivf_sq8_supported(3, 1000, 16, 1024, 2, 7, 4) == 1        # kk clipped at 1024
    assert lib.lr_ivf_sq8_supported(3, 1000, 16, 10, 8, 7, 4) == 0          # nprobe > nlist
    assert lib.lr_ivf_sq8_supported(3, 5, 16, 10, 2, 7, 4) == 0             # nlist > N
    assert lib.lr_ivf_sq8_search_ws_bytes(3, 1000, 16, 1025, 2, 7) == 0 < lib.lr_ivf_sq8_search_ws_bytes(3, 1000, 16, 40, 2, 7)
    assert lib.lr_ivf_sq8_search_ws_bytes(3, 1000, 16, 40, 2, 7) == lib.lr_ivf_search_ws_bytes(3, 1000, 16, 40, 2, 7)


def test_seams_are_additive():
    sig = inspect.signature(serving.save_ivf_sq8_index).parameters
    assert list(sig) == ["path", "model", "nlist", "nprobe", "refine"]
    assert [sig[n].default for n in ("nlist", "nprobe", "refine")] == [80, 10, 4]
    assert "save_ivf_sq8_index" in serving.__all__ and "save_ivf_index" in serving.__all__
    knn = inspect.signature(__import__("librecommender_amd.bases", fromlist=["EmbedBase"]).EmbedBase.init_knn).parameters
    assert [knn[n].kind.name for n in ("nlist", "nprobe", "codes", "refine")] == ["KEYWORD_ONLY"] * 4
    assert knn["codes"].default is None and knn["refine"].default == 4
    ta = inspect.signature(IVFSQ8Index.train_add).parameters
    assert list(ta) == ["rows", "nlist", "niter", "nprobe", "refine", "timings"]
    assert [ta[n].default for n in ("niter", "nprobe", "refine", "timings")] == [20, 1, 4, False]
    se = inspect.signature(IVFSQ8Index.search).parameters
    assert list(se) == ["self", "queries", "k", "nprobe", "consumed_ptr", "consumed_idx", "filter_flag", "refine"]


def test_argument_errors_come_before_any_device_work():
    """All on CPU tensors: a call that got as far as the device check would raise RuntimeError ("no CPU fallback") instead."""
    rows = torch.zeros((10, 8))
    with pytest.raises(ValueError, match="nlist 11 exceeds"):
        IVFSQ8Index.train_add(rows, 11)
    with pytest.raises(ValueError, match="shape not supported"):
        IVFSQ8Index.train_add(torch.zeros((10, 300)), 2)
    with pytest.raises(ValueError, match="refine must be in 0..64"):
        IVFSQ8Index.train_add(rows, 2, refine=65)
    with pytest.raises(ValueError, match="refine must be in 0..64"):
        IVFSQ8Index.train_add(rows, 2, refine=-1)
    idx = IVFSQ8Index(torch.zeros((4, 8)), torch.tensor([0, 3, 5, 5, 10]), torch.arange(10, dtype=torch.int32),
                      torch.zeros((10, 16), dtype=torch.int8), torch.zeros(10), rows, nprobe=2, refine=4, d=8)
    assert (idx.nlist, idx.ntotal, idx.nprobe, idx.refine) == (4, 10, 2, 4)
    assert idx.nbytes == 10 * 16 + 10 * 4 + 10 * 4 + 5 * 8 + 4 * 8 * 4
    q = torch.zeros((2, 8))
    with pytest.raises(ValueError, match="nprobe must be in 1..nlist"):
        idx.search(q, 3, nprobe=5)
    with pytest.raises(ValueError, match="k must be >= 1"):
        idx.search(q, 0)
    with pytest.raises(ValueError, match="width"):
        idx.search(torch.zeros((2, 12)), 3)
    with pytest.raises(ValueError, match="shape not supported"):
        idx.search(q, 1025)
    with pytest.raises(ValueError, match="shape not supported"):
        idx.search(q, 3, refine=65)
    with pytest.raises(ValueError, match="refine must be >= 0"):
        idx.search(q, 3, refine=-1)
    with pytest.raises(ValueError, match="shape not supported"):
        ops.ivf_sq8_encode(torch.zeros((4, 260)))
    with pytest.raises(ValueError, match="shape not supported"):
        ops.ivf_rerank(q, rows, torch.zeros((2, 1025), dtype=torch.int64), 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):       # well-formed arguments: only the device is missing
        idx.search(q, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IVFSQ8Index.train_add(rows, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ivf_sq8_encode(rows)
