"""The IVF-Flat index without a device: the numpy oracle against brute force, its training on a separated mixture, the C ABI
table, the reference's `save_faiss_index` signature and the argument errors that come before any device work."""
import inspect
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from librecommender_amd import _lib, ops, serving
from librecommender_amd.recommendation.ivf import IVFFlatIndex

from . import ivf_oracle as O

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ["lr_ivf_supported", "lr_ivf_search_ws_bytes", "lr_ivf_build_ws_bytes", "lr_ivf_centroids_ws_bytes", "lr_ivf_assign_f32",
           "lr_ivf_build_lists", "lr_ivf_centroids_f32", "lr_ivf_search_f32"]


@pytest.mark.parametrize("N,nlist,D,B,k", [(500, 7, 16, 5, 10), (63, 2, 4, 3, 100), (300, 80, 20, 2, 1)])
def test_oracle_with_every_list_probed_is_brute_force(N, nlist, D, B, k):
    rng = np.random.default_rng(N)
    rows, cent, queries = O.grid(rng, (N, D)), O.grid(rng, (nlist, D)), O.grid(rng, (B, D))
    ptr, ids = O.build_lists(O.assign(rows, cent), nlist)
    assert ptr[-1] == N and sorted(ids.tolist()) == list(range(N))
    assert all((np.diff(ids[ptr[l]:ptr[l + 1]]) > 0).all() for l in range(nlist))
    s, i = O.search(queries, cent, ptr, ids, rows, k, nlist)
    bs, bi = O.brute_force(queries, rows, min(k, N))
    assert np.array_equal(i[:, :min(k, N)], bi) and np.array_equal(s[:, :min(k, N)], bs)
    assert (i[:, N:] == -1).all() and np.isneginf(s[:, N:]).all()
    # fewer lists: a subset of the catalogue, ranked the same way, and nothing consumed comes back
    consumed = [np.arange(0, N, 2, dtype=np.int32)] * B
    s1, i1 = O.search(queries, cent, ptr, ids, rows, k, 1, consumed, np.array([1] * (B - 1) + [0], np.uint8))
    assert (i1[:-1][i1[:-1] >= 0] % 2 == 1).all()
    assert (np.diff(s1, axis=1) <= 0).all() or np.isneginf(s1).any()


def test_oracle_training_reaches_a_fixed_point_on_a_separated_mixture():
    N, nlist, D = 1200, 6, 12
    rng = np.random.default_rng(0)
    centre = (np.arange(N) * nlist) // N
    rows = (0.1 * rng.standard_normal((N, D))).astype(np.float32)
    rows[np.arange(N), centre] += 10.0
    c20, gap = O.train(rows, nlist, 20, want_gaps=True)
    assert gap > 1e-3
    assert np.array_equal(O.train(rows, nlist, 21), c20)            # one more round changes nothing
    assert np.array_equal(O.assign(rows, c20), centre)
    assert np.array_equal(O.train_ids(1100, 4), (np.arange(1024) * 1100) // 1024) and len(O.train_ids(100, 4)) == 100
    assert O.init_ids(1024, 4).tolist() == [0, 256, 512, 768]
    # an empty list keeps its previous centroid
    prev = np.full((3, D), 7.0, np.float32)
    ptr, ids = O.build_lists(np.zeros(5, np.int32), 3)
    out = O.centroid_means(rows[:5], ptr, ids, prev)
    assert np.array_equal(out[1:], prev[1:]) and not np.array_equal(out[0], prev[0])


def test_symbols_are_bound_and_declared():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "libreco_hip.h").read_text(), flags=re.S)
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and re.search(rf"\b{name}\s*\(", header) and hasattr(lib, name)
    assert _lib.ABI_VERSION == 26
    # host-only entry points: the envelope and the workspace sizes
    assert lib.lr_ivf_supported(1, 10_000_000, 128, 100, 32, 12649) == 1
    assert lib.lr_ivf_supported(1024, 100_000_000, 128, 100, 128, 40000) == 1
    assert lib.lr_ivf_supported(3, 1000, 6, 10, 2, 7) == 0          # D % 4 != 0: the host pads
    assert lib.lr_ivf_supported(3, 1000, 16, 1025, 2, 7) == 0       # k > 1024
    assert lib.lr_ivf_supported(3, 1000, 16, 10, 8, 7) == 0         # nprobe > nlist
    assert lib.lr_ivf_supported(3, 5, 16, 10, 2, 7) == 0            # nlist > N
    assert lib.lr_ivf_supported(3, 100000, 16, 10, 2, 65537) == 0
    assert lib.lr_ivf_search_ws_bytes(3, 1000, 16, 1025, 2, 7) == 0 < lib.lr_ivf_search_ws_bytes(3, 1000, 16, 10, 2, 7)
    assert lib.lr_ivf_build_ws_bytes(1000, 7) >= 1000 * 4 and lib.lr_ivf_centroids_ws_bytes(5000, 128) >= 5 * 2 * 128 * 4


def test_save_ivf_index_has_the_references_signature():
    ref = json.loads((ROOT / "tests" / "golden" / "ivf_signature.json").read_text())["libserving.serialization.embed.save_faiss_index"]
    mine = inspect.signature(serving.save_ivf_index).parameters
    assert [p[0] for p in ref] == list(mine)
    for name, kind, default in ref:
        assert mine[name].kind.name == kind
        assert (None if mine[name].default is inspect.Parameter.empty else repr(mine[name].default)) == default
    assert "save_ivf_index" in serving.__all__
    params = inspect.signature(serving.EmbedServer.__init__).parameters
    assert list(params) == ["self", "path", "device", "use_index"] and params["use_index"].default is True
    knn = inspect.signature(__import__("librecommender_amd.bases", fromlist=["EmbedBase"]).EmbedBase.init_knn).parameters
    assert [knn[n].kind.name for n in ("nlist", "nprobe")] == ["KEYWORD_ONLY"] * 2 and knn["nlist"].default is None


def test_argument_errors_come_before_any_device_work():
    """All on CPU tensors: a call that got as far as the device check would raise RuntimeError ("no CPU fallback") instead."""
    rows = torch.zeros((10, 8))
    with pytest.raises(ValueError, match="nlist 11 exceeds"):
        IVFFlatIndex.train_add(rows, 11)
    with pytest.raises(ValueError, match="nlist must be >= 1"):
        IVFFlatIndex.train_add(rows, 0)
    with pytest.raises(ValueError, match="shape not supported"):
        IVFFlatIndex.train_add(torch.zeros((10, 300)), 2)
    idx = IVFFlatIndex(torch.zeros((4, 8)), torch.tensor([0, 3, 5, 5, 10]), torch.arange(10, dtype=torch.int32), rows, nprobe=2, d=8)
    assert (idx.nlist, idx.ntotal, idx.nprobe) == (4, 10, 2)
    q = torch.zeros((2, 8))
    with pytest.raises(ValueError, match="nprobe must be in 1..nlist"):
        idx.search(q, 3, nprobe=5)
    with pytest.raises(ValueError, match="nprobe must be in 1..nlist"):
        idx.search(q, 3, nprobe=0)
    with pytest.raises(ValueError, match="k must be >= 1"):
        idx.search(q, 0)
    with pytest.raises(ValueError, match="width"):
        idx.search(torch.zeros((2, 12)), 3)
    with pytest.raises(ValueError, match="shape not supported"):
        idx.search(q, 1025)
    with pytest.raises(ValueError, match="nlist 4 exceeds"):
        ops.ivf_search(q, torch.zeros((4, 8)), torch.zeros(5, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), torch.zeros((3, 8)), 1, 1)
    with pytest.raises(ValueError, match="share the embedding width"):
        ops.ivf_assign(rows, torch.zeros((2, 12)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):       # well-formed arguments: only the device is missing
        idx.search(q, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IVFFlatIndex.train_add(rows, 2)
