"""The kernel parity cases of the suite, run again on poisoned, guarded device allocations (tests/guarded_alloc.py).

Every case below calls an EXISTING test function of the kernel-level modules inside `guarded(fill)`: each `torch.empty`
of the package then holds 0xFF or 0x5A bytes instead of zero pages or the last call's result, and sits between two guard
zones of 0xA5 bytes.  A case asserts

* the existing function's own assertions, unchanged (oracle parity at its own tolerances: no number is new here);
* that every guard zone is intact afterwards (no store before or after any output or workspace);
* that no device allocation of the package escaped the guard (`unguarded == 0`).

So a kernel that leaves part of an output unwritten, relies on a workspace being zero where include/libreco_hip.h does not
promise it, or stores outside its buffers fails here, where it passes on ordinary allocations.  Out-of-bounds READS are not
detectable this way (that takes a device address sanitizer or page-fault runs, which shared machines do not allow) and are
not covered.  Nothing in this module makes a kernel write out of bounds.

Which fill a case gets: `fill` alternates with the case's index within its function, and the first and the last case of
every function run under the other fill as well: every function sees both patterns, every shape sees one.

Fixtures: `dev`, `golden_dir` and `tmp_path` are passed through.  The arithmetic fixtures (`f32_chain`, `l1_arith`,
`sce_arith`, `topk_arith`) and the `tile` / `override` fixtures of the two first-layer modules only set a library mode; a
case sets the same mode in try / finally, and runs every mode of a parametrized one.  Functions that need `monkeypatch`, a
module-scoped fitted model, hipGraph capture (a guard's fills would be captured with the step) or child processes are
not re-run: `NOT_RERUN` gives the reason for each.

The last test is the coverage condition: every entry point of `_lib.SIGNATURES` that launches a kernel was called under a
guard in this session; `NO_DEVICE_WRITES` lists the ones that launch nothing or exist for measurement."""
import importlib
import inspect
import re

import numpy as np
import pytest
import torch

from librecommender_amd import _lib, ops
from oracle import ops_np
from tests import guarded_alloc as ga

pytestmark = pytest.mark.gpu

MODULES = ["test_ops_gpu", "test_edge_cases_gpu", "test_deepfm_fused_gpu", "test_dense_adam_fused_gpu", "test_din_gpu",
           "test_din_fused_gpu", "test_softmax_ce_gpu", "test_score_topk_gpu", "test_sampling_gpu", "test_als_gpu", "test_cf_gpu",
           "test_swing_gpu", "test_bpr_gpu", "test_owner_partition_gpu", "test_l1_wide_gpu", "test_l1_split_bf16_gpu",
           "test_tail_fused_gpu", "test_tail_dropout_gpu", "test_feat_block_gpu", "test_rank_seam_gpu", "test_lightgcn_gpu",
           "test_zz_ngcf_gpu", "test_graph_nodes_gpu"]

MONKEYPATCH = "needs the monkeypatch fixture"
FITTED = "needs a module-scoped fitted model or dataset fixture"
CAPTURE = "captures a hipGraph: the guard's fill kernels would be recorded into the step"
NOT_RERUN = {
    ("test_deepfm_fused_gpu", "test_merged_fold_chain_equals_the_four_launch_chain"): MONKEYPATCH,
    ("test_deepfm_fused_gpu", "test_graph_replayed_steps_equal_eager_steps"): CAPTURE,
    ("test_deepfm_fused_gpu", "test_graph_replays_with_alternating_batch_shapes"): CAPTURE,
    ("test_din_fused_gpu", "test_graph_replays_bit_identical_to_eager_and_alternating_shapes"): CAPTURE,
    ("test_graph_nodes_gpu", "test_capture_refuses_memset_nodes_and_accepts_kernel_steps"): CAPTURE,
    ("test_graph_nodes_gpu", "test_fused_steps_hold_kernel_nodes_only"): CAPTURE,
    ("test_tail_fused_gpu", "test_chain_form_under_more_than_one_rank"): MONKEYPATCH,
    ("test_als_gpu", "test_model_surface"): FITTED,
    ("test_als_gpu", "test_fit_is_deterministic_and_continues"): FITTED,
    ("test_als_gpu", "test_rebuild_model_keeps_old_rows"): FITTED,
    ("test_als_gpu", "test_multi_rank_fit_raises"): FITTED,
    ("test_als_gpu", "test_embed_size_over_limit"): FITTED,
    ("test_cf_gpu", "test_recommend_and_predict"): FITTED,
    ("test_cf_gpu", "test_model_surface"): FITTED,
    ("test_cf_gpu", "test_fit_twice_identical_bytes"): FITTED,
    ("test_cf_gpu", "test_multi_rank_fit_raises"): FITTED,
    ("test_cf_gpu", "test_oversize_result_raises_before_allocating"): FITTED,
    ("test_swing_gpu", "test_model_scores"): FITTED,
    ("test_swing_gpu", "test_topk_on_device_scores"): FITTED,
    ("test_swing_gpu", "test_recommend_on_device_scores"): FITTED,
    ("test_swing_gpu", "test_predict_on_device_scores"): FITTED,
    ("test_swing_gpu", "test_model_surface"): FITTED,
    ("test_swing_gpu", "test_all_consumed_and_cold_start"): FITTED,
    ("test_swing_gpu", "test_multi_rank_fit_raises"): FITTED,
    ("test_swing_gpu", "test_oversize_raises_before_allocating"): FITTED,
    ("test_bpr_gpu", "test_two_runs_give_the_same_bits"): FITTED,
    ("test_bpr_gpu", "test_epoch_through_fit"): FITTED,
    ("test_bpr_gpu", "test_model_surface_and_quality"): FITTED,
    ("test_bpr_gpu", "test_multi_rank_fit_raises"): FITTED,
    ("test_zz_ngcf_gpu", "test_reference_module_fixture"): FITTED,
    ("test_zz_ngcf_gpu", "test_full_fit_matches_reference_fit"): FITTED,
}
# single cases of a re-run function that capture: (module, function) -> (the kwargs that select them, reason)
NOT_RERUN_CASES = {
    ("test_dense_adam_fused_gpu", "test_fused_dense_adam_trajectory_vs_fp64_oracle"): ({"graph": True}, CAPTURE),
}

PASS_THROUGH = {"dev", "golden_dir", "tmp_path"}
# fixture name -> the modes a case runs (None: one run); what each does is in `_with_mode`
MODES = {"f32_chain": ["f32_chain"], "l1_arith": ["split_bf16", "f32_chain"], "sce_arith": ["split_bf16", "f32_chain"],
         "topk_arith": ["f32_chain", "split_bf16", "filter"], "tile": ["f32_chain"], "override": [None]}
AUTOUSE = {"test_softmax_ce_gpu": "sce_arith", "test_score_topk_gpu": "topk_arith"}


def _build_cases():
    cases, ids, n_fn = [], [], 0
    seen = set()
    for mname in MODULES:
        mod = importlib.import_module("tests." + mname)
        for fname, fn in vars(mod).items():
            if not (fname.startswith("test_") and inspect.isfunction(fn) and fn.__module__ == mod.__name__):
                continue
            seen.add((mname, fname))
            kws = ga.expand(fn)
            fixtures = [a for a in inspect.signature(fn).parameters if a not in (kws[0] if kws else {})]
            if (mname, fname) in NOT_RERUN:
                continue
            unknown = [f for f in fixtures if f not in PASS_THROUGH and f not in MODES]
            assert not unknown, f"{mname}::{fname} needs {unknown}: handle the fixture here or give NOT_RERUN a reason"
            if (mname, fname) in NOT_RERUN_CASES:
                sel, _ = NOT_RERUN_CASES[(mname, fname)]
                kws = [kw for kw in kws if any(kw.get(k) != v for k, v in sel.items())]
            n_fn += 1
            runs = [(i, ga.FILLS[i % 2]) for i in range(len(kws))]
            for i in sorted({0, len(kws) - 1}):
                runs.append((i, ga.FILLS[(i + 1) % 2]))
            for i, fill in sorted(runs):
                cases.append((mname, fname, kws[i], fill, tuple(fixtures)))
                cid = ga.case_id(kws[i])
                ids.append(f"{mname[5:-4]}.{fname[5:]}" + (f"[{cid}]" if cid else "") + f"-{fill:02X}")
    stale = [k for k in list(NOT_RERUN) + list(NOT_RERUN_CASES) if k not in seen]
    assert not stale, f"NOT_RERUN names functions that do not exist: {stale}"
    assert len(set(ids)) == len(ids)
    return cases, ids, n_fn


CASES, IDS, N_FUNCTIONS = _build_cases()
ATTEMPTED = {"rerun": 0, "direct": 0, "unguarded": 0}
DIRECT = []          # the direct cases below register themselves here


class _Mode:
    """What the fixture of that name does, in try / finally; `value` is what the test function receives for it."""

    def __init__(self, fixture, mode):
        self.fixture, self.mode, self.value = fixture, mode, mode
        self._undo = []

    def __enter__(self):
        lib = _lib.load()
        f, m = self.fixture, self.mode
        if f in ("f32_chain", "l1_arith", "tile"):
            prev = ops.set_l1_arith(m)
            self._undo.append(lambda: ops.set_l1_arith(prev))
        if f == "f32_chain":
            self.value = None
        elif f == "tile":
            self.value = lambda ts: lib.lr_deepfm_l1_tile_override(int(ts))
            self._undo.append(lambda: lib.lr_deepfm_l1_tile_override(0))
        elif f == "override":
            self.value = lambda fwd_tile=0, ksplit=0, wgrad_cw=0, wgrad_fg=0: lib.lr_deepfm_l1_sb_override(
                int(fwd_tile), int(ksplit), int(wgrad_cw), int(wgrad_fg))
            self._undo.append(lambda: lib.lr_deepfm_l1_sb_override(0, 0, 0, 0))
        elif f == "sce_arith":
            prev = ops.set_sce_arith(m)
            self._undo.append(lambda: ops.set_sce_arith(prev))
        elif f == "topk_arith":
            prev = (ops.TOPK_ARITH, ops.TOPK_FILTER_FORCE)
            ops.TOPK_ARITH, ops.TOPK_FILTER_FORCE = m, True
            self._undo.append(lambda: (setattr(ops, "TOPK_ARITH", prev[0]), setattr(ops, "TOPK_FILTER_FORCE", prev[1])))
        return self

    def __exit__(self, *exc):
        for u in reversed(self._undo):
            u()
        return False


def run_guarded(fn, kwargs, fill):
    """`fn(**kwargs)` on guarded allocations, then the two conditions of this module."""
    with ga.guarded(fill) as g:
        try:
            fn(**kwargs)
        finally:
            ATTEMPTED["unguarded"] += g.unguarded
        g.check()
        assert g.unguarded == 0, "device allocations that escaped the guard:\n" + "\n".join(g.unguarded_sites)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_parity_case_on_guarded_allocations(case, request, dev):
    mname, fname, kwargs, fill, fixtures = case
    ATTEMPTED["rerun"] += 1
    mod = importlib.import_module("tests." + mname)
    fn = getattr(mod, fname)
    kw = dict(kwargs)
    moded = [f for f in fixtures if f in MODES]
    auto = AUTOUSE.get(mname)
    if auto and auto not in moded:
        moded.append(auto)
    assert len(moded) <= 1, moded
    for f in fixtures:
        if f in PASS_THROUGH:
            kw[f] = dev if f == "dev" else request.getfixturevalue(f)
    if not moded:
        run_guarded(fn, kw, fill)
        return
    f = moded[0]
    skipped = []
    for mode in MODES[f]:
        with _Mode(f, mode) as m:
            if f in fixtures:
                kw[f] = m.value
            try:
                run_guarded(fn, kw, fill)
            except pytest.skip.Exception as e:      # the function has nothing to run in this mode (it says so itself)
                skipped.append(e)
    if len(skipped) == len(MODES[f]):
        raise skipped[0]


# ---- direct cases: writing entry points that no re-run function reaches, against the existing oracles -----------------
def direct(fn):
    DIRECT.append(fn.__name__)
    return pytest.mark.parametrize("fill", ga.FILLS, ids=["FF", "5A"])(fn)


def t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


from tests import test_deepfm_fused_gpu as deepfm_cases  # noqa: E402  (module objects only: nothing is collected twice)
from tests import test_dense_adam_fused_gpu as dense_adam_cases  # noqa: E402
from tests import test_din_gpu as din_cases  # noqa: E402
from tests import test_ops_gpu as ops_cases  # noqa: E402


def gt(x, dev):
    """A GUARDED device copy of a host array: operands a kernel updates in place get guard zones too."""
    x = np.ascontiguousarray(x)
    out = ga.PROXY.empty(x.shape, dtype=torch.from_numpy(x).dtype, device=dev)
    out.copy_(torch.from_numpy(x))
    return out


class _CoefHP(ops.AdamCoefBuffer):
    """Device-resident Adam coefficients (what the `_dc` entry points read) that still answer for the by-value fields the
    existing tests read back (`hp.eps`, `hp.weight_decay`)."""

    def __init__(self, hp, device):
        super().__init__(device)
        self.set(hp)
        for name, _ in hp._fields_:
            setattr(self, name, getattr(hp, name))


class _coef_adam_hp:
    """`ops.adam_hp` returns device-resident coefficients: every wrapper the existing Adam parity tests call then takes
    its `_dc` entry point, outside a captured graph, against the same oracle at the same tolerances."""

    def __init__(self, dev):
        self.dev = dev

    def __enter__(self):
        self.prev = prev = ops.adam_hp
        ops.adam_hp = lambda *a, **k: _CoefHP(prev(*a, **k), self.dev)

    def __exit__(self, *exc):
        ops.adam_hp = self.prev
        return False


class _Patch:
    """The two calls of `monkeypatch` that test_merged_fold_chain_equals_the_four_launch_chain uses, undone by `undo()`."""

    def __init__(self):
        self._undo = []

    def setattr(self, obj, name, value, raising=True):
        missing = object()
        old = getattr(obj, name, missing)
        self._undo.append((lambda: delattr(obj, name)) if old is missing else (lambda: setattr(obj, name, old)))
        setattr(obj, name, value)

    def setenv(self, name, value):
        import os

        old = os.environ.get(name)
        self._undo.append((lambda: os.environ.pop(name, None)) if old is None else (lambda: os.environ.__setitem__(name, old)))
        os.environ[name] = value

    def undo(self):
        for u in reversed(self._undo):
            u()
        self._undo.clear()


def _each_case(fn, fill, **fixed):
    """Every parametrization of an existing function, fills alternating from `fill`."""
    for i, kw in enumerate(ga.expand(fn)):
        run_guarded(fn, dict(kw, **fixed), ga.FILLS[(ga.FILLS.index(fill) + i) % 2])


@direct
def test_dc_scatter_adam_forms(dev, fill):
    """lr_adam_coef_store, lr_embed_scatter_adam_dc_f32, lr_embed_scatter_adam_lin_dc_f32: the by-value parity tests with
    device-resident coefficients."""
    ATTEMPTED["direct"] += 1
    with _coef_adam_hp(dev):
        _each_case(ops_cases.test_scatter_adam_matches_oracle_on_touched_rows, fill, dev=dev)
        _each_case(ops_cases.test_scatter_adam_lin_equals_two_scatter_adams, fill, dev=dev)


@direct
def test_dc_fm_rows_adam_and_dense_rows(dev, fill):
    """lr_fm_rows_adam_dc_f32, lr_adam_dense_rows_dc_f32: the by-value parity tests with device-resident coefficients."""
    ATTEMPTED["direct"] += 1
    with _coef_adam_hp(dev):
        _each_case(deepfm_cases.test_fm_rows_adam_matches_oracle, fill, dev=dev)
        _each_case(dense_adam_cases.test_rows_grad_compact_and_dense_table_pass, fill, dev=dev)


@direct
def test_dc_adam_dense(dev, fill):
    """lr_adam_dense_dc_f32 (the flat dense-parameter update of a captured step) against `ops_np.adam_step`, at the
    tolerances of test_ops_gpu.py::test_adam_dense_tf_semantics."""
    ATTEMPTED["direct"] += 1
    rng = np.random.default_rng(9)
    n = 300 * 16 + 4
    w = rng.standard_normal(n).astype(np.float32)
    m = (rng.standard_normal(n) * 0.01).astype(np.float32)
    v = (rng.random(n) * 0.01).astype(np.float32)
    g = rng.standard_normal(n).astype(np.float32)

    def body():
        wd, md, vd, gd = (gt(x, dev) for x in (w, m, v, g))
        coef = ops.AdamCoefBuffer(dev)
        coef.set(ops.adam_hp(lr=1e-2, step=2, eps=1e-5))
        ops.adam_dense_dc(wd, md, vd, gd, coef)
        w2, m2, v2 = ops_np.adam_step(w, m, v, g, 1e-2, 2, eps=1e-5)
        np.testing.assert_allclose(wd.cpu().numpy(), w2, rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(md.cpu().numpy(), m2, rtol=1e-4, atol=1e-6)
        np.testing.assert_array_equal(gd.cpu().numpy(), g)

    run_guarded(body, {}, fill)


@direct
def test_four_launch_fold_chain(dev, fill):
    """lr_deepfm_l1_fold_stats_f32, lr_deepfm_l1_fold_bias_f32: the existing merged-vs-chain test (its `monkeypatch` calls
    done and undone here), both arithmetics."""
    ATTEMPTED["direct"] += 1
    for arith in ("split_bf16", "f32_chain"):
        patch = _Patch()
        try:
            run_guarded(deepfm_cases.test_merged_fold_chain_equals_the_four_launch_chain, dict(dev=dev, monkeypatch=patch, arith=arith), fill)
        finally:
            patch.undo()


def _fm_case(K, dev):
    """The inputs of test_ops_gpu.py::test_fm_embed_fused_backward_adam (deep + linear + BatchNorm-fold terms)."""
    rng = np.random.default_rng(11 + K)
    V, B, F = 800, 300, 9
    table = (rng.standard_normal((V, K)) * 0.1).astype(np.float32)
    idx = ops_cases.zipf_ids(rng, V, (B, F))
    gdeep = (rng.standard_normal((B, F, K)) * 0.1).astype(np.float32)
    gpair = rng.standard_normal((B, K)).astype(np.float32)
    glin = rng.standard_normal((B, F)).astype(np.float32)
    bn_a = (rng.standard_normal((F, K)) * 0.05).astype(np.float32)
    bn_c = (rng.standard_normal((F, K)) * 0.05).astype(np.float32)
    return V, B, F, table, idx, gdeep, gpair, glin, bn_a, bn_c


@direct
def test_fm_embed_bwd_rows(dev, fill):
    """lr_fm_embed_bwd_rows_f32 (row-sharded tables: per-row gradients in run order, not applied) against the oracle of
    test_ops_gpu.py::test_fm_embed_fused_backward_adam.  That test checks the gradient through Adam's first moment at step 1
    from zero moments, m = (1 - beta1) * g, at rtol 1e-4 / atol 2e-6 (linear part: atol 1e-6): the same statement here."""
    ATTEMPTED["direct"] += 1

    def body(K):
        V, B, F, table, idx, gdeep, gpair, glin, bn_a, bn_c = _fm_case(K, dev)
        td = t(table, dev)
        fsum = ops.fm_embed_fwd(td, t(idx, dev), want_e=False)[2]
        seg = ops.build_segments(t(idx.reshape(-1), dev), V)
        ns = seg.count()
        rows = seg.rows[:ns].cpu().numpy()
        cache = ops.embed_gather(td, seg.rows[:ns].contiguous())
        grows, glin_rows = ops.fm_embed_bwd_rows(cache, t(gdeep, dev), t(gpair, dev), fsum, B, F, seg, glin=t(glin, dev),
                                                 bn_a=t(bn_a, dev), bn_c=t(bn_c, dev))
        e = table[idx]
        ge = ops_np.fm_pairwise_bwd(e.astype(np.float64), gpair.astype(np.float64)) + gdeep - bn_a[None] - bn_c[None] * e
        gd = ops_np.scatter_add_dense(V, idx, ge)
        z = np.zeros((len(rows), K))
        _, m2, _ = ops_np.adam_step(table[rows].astype(np.float64), z, z, gd[rows], 1e-3, 1, eps=1e-5)
        np.testing.assert_allclose(grows[:ns].cpu().numpy().astype(np.float64) * (1.0 - 0.9), m2, rtol=1e-4, atol=2e-6)
        gl = ops_np.scatter_add_dense(V, idx, glin[..., None])
        z1 = np.zeros((len(rows), 1))
        _, lm2, _ = ops_np.adam_step(z1, z1, z1, gl[rows], 1e-3, 1, eps=1e-5)
        np.testing.assert_allclose(glin_rows[:ns].cpu().numpy().astype(np.float64)[:, None] * (1.0 - 0.9), lm2, rtol=1e-4, atol=1e-6)

    for K in (16, 64, 128):
        run_guarded(body, dict(K=K), fill)


@direct
def test_fm_field_stats_slots(dev, fill):
    """lr_fm_field_stats_slots_f32 (the statistics read through the position -> cache-row map of a row-sharded step) on the
    inputs, against the fp64 shadow and at the tolerances of test_ops_gpu.py::test_fm_field_stats_equal_batch_statistics."""
    ATTEMPTED["direct"] += 1

    def body(K):
        rng = np.random.default_rng(K)
        sizes = [40, 25, 7, 300, 1]
        starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        V, F, B, C = int(starts[-1]), len(sizes), 512, 3
        table = rng.standard_normal((V, K)).astype(np.float32)
        idx = np.stack([rng.zipf(1.3, B) % sizes[f] + starts[f] for f in range(F)], axis=1).astype(np.int32)
        td = t(table, dev)
        seg = ops.build_segments(t(idx, dev).reshape(-1), V)
        ns = seg.count()
        cache = ops.embed_gather(td, seg.rows[:ns].contiguous())            # the step's row cache, in run order
        start = seg.start[:ns + 1].long()
        run_of = torch.repeat_interleave(torch.arange(ns, device=dev, dtype=torch.int32), start[1:] - start[:-1])
        slots = torch.zeros(B * F, dtype=torch.int32, device=dev)
        slots[seg.pos[:B * F].long()] = run_of
        partial = ga.PROXY.empty((F, C, 2, K), dtype=torch.float32, device=dev)
        ops._call("lr_fm_field_stats_slots_f32", ops._ptr(cache), K, ops._ptr(seg.rows), ops._ptr(seg.start), ops._ptr(seg.n_seg),
                  ops._ptr(t(starts, dev)), F, C, ops._ptr(partial), ops._ptr(seg.pos), ops._ptr(slots), ops._stream())
        tot = partial.double().sum(1)
        mean = tot[:, 0] / B
        var = torch.clamp(tot[:, 1] / B - mean * mean, min=0.0)
        e = table[idx].astype(np.float64).reshape(B, F * K)
        np.testing.assert_allclose(mean.reshape(-1).float().cpu().numpy(), e.mean(0), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(var.reshape(-1).float().cpu().numpy(), e.var(0), rtol=1e-4, atol=1e-6)

    for K in (16, 64):
        run_guarded(body, dict(K=K), fill)


@direct
def test_spmm_csr_plain_entry_point(dev, fill):
    """lr_spmm_csr_f32 called by name (the Python wrappers reach it only through the bucketed form's own fallback), on the
    inputs and at the tolerances of test_ops_gpu.py::test_spmm_csr."""
    ATTEMPTED["direct"] += 1
    import scipy.sparse as ssp

    def body(K):
        rng = np.random.default_rng(K)
        n = 3000
        A = ssp.random(n, n, density=0.004, format="csr", dtype=np.float32, random_state=1)
        A.sort_indices()
        X = rng.standard_normal((n, K)).astype(np.float32)
        rp, ci, va = A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.astype(np.float32)
        acc0 = rng.standard_normal((n, K)).astype(np.float32)
        acc = gt(acc0, dev)
        Y = ga.PROXY.empty((n, K), dtype=torch.float32, device=dev)
        rpd, cid, vad, Xd = t(rp, dev), t(ci, dev), t(va, dev), t(X, dev)
        ops._call("lr_spmm_csr_f32", ops._ptr(rpd), ops._ptr(cid), ops._ptr(vad), n, ops._ptr(Xd), K, ops._ptr(Y), ops._ptr(acc),
                  ops._stream())
        ref = ops_np.spmm_csr(rp, ci, va, X.astype(np.float64))
        np.testing.assert_allclose(Y.cpu().numpy(), ref, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(acc.cpu().numpy(), acc0 + ref, rtol=1e-5, atol=1e-5)

    for K in (16, 64, 128, 10):
        run_guarded(body, dict(K=K), fill)


@direct
def test_din_attention_one_call_backward(dev, fill):
    """lr_din_attn_pool_bwd_f32 (the one-call form of the C ABI; the Python wrapper calls the `_parts_` form) against the fp64
    autograd twin and at the tolerances of test_din_gpu.py::test_din_attention_fused_gather."""
    ATTEMPTED["direct"] += 1

    def body(K, B, L):
        V = 5000
        table, item, seq, lens, W1, b1, W2, b2 = din_cases.make_case(K, B, L, V, seed=K + B)
        gout = np.random.default_rng(1).standard_normal((B, K)).astype(np.float32)
        args = [t(x, dev) for x in (table, item, seq, lens, W1, b1, W2, b2)]
        _, attn = ops.din_attn_pool_fwd(*args)
        lib = _lib.load()
        E = ga.PROXY.empty
        f32 = dict(dtype=torch.float32, device=dev)
        ws = E(max(lib.lr_din_attn_ws_bytes(B, L, K, 16), 8), dtype=torch.uint8, device=dev)
        gq, gkey = E((B, K), **f32), E((B, L, K), **f32)
        gW1, gb1, gW2, gb2 = E(W1.shape, **f32), E(b1.shape, **f32), E(W2.shape, **f32), E(b2.shape, **f32)
        gd = t(gout, dev)
        ops._call("lr_din_attn_pool_bwd_f32", ops._ptr(args[0]), V, K, ops._ptr(args[1]), ops._ptr(args[2]), ops._ptr(args[3]), B, L,
                  ops._ptr(args[4]), ops._ptr(args[5]), ops._ptr(args[6]), ops._ptr(args[7]), 16, ops._ptr(attn), ops._ptr(gd),
                  ops._ptr(gq), ops._ptr(gkey), ops._ptr(gW1), ops._ptr(gb1), ops._ptr(gW2), ops._ptr(gb2), ops._ptr(ws), ws.numel(),
                  ops._stream())
        _, _, r_gq, r_gk, r_gp = din_cases.torch_ref(table, item, seq, lens, W1, b1, W2, b2, gout)
        np.testing.assert_allclose(gq.cpu().numpy(), r_gq, rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(gkey.cpu().numpy(), r_gk, rtol=1e-4, atol=1e-5)
        for got, want, name in ((gW1, r_gp[0], "gW1"), (gb1, r_gp[1], "gb1"), (gW2, r_gp[2], "gW2"), (gb2, r_gp[3], "gb2")):
            scale = max(1.0, float(np.abs(want).max()))
            np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-4, atol=1e-4 * scale, err_msg=name)

    for K, B, L in din_cases.test_din_attention_fused_gather.pytestmark[0].args[1]:
        run_guarded(body, dict(K=K, B=B, L=L), fill)



# ---- the coverage condition -----------------------------------------------------------------------------------------
_NO_WRITE_PATTERNS = [r"lr_abi_version", r"lr_strerror", r".*_bytes", r".*_supported", r".*_override", r".*_tile_cols",
                      r".*_plan_params", r".*_chunks", r".*_slabs", r".*_resident_blocks", r"lr_swing_lds_users",
                      r"lr_cf_select_max", r"lr_score_topk_filter_kp", r"lr_score_topk_test_mute", r"lr_graph_foreign_nodes",
                      r"lr_mfma_f32_probe", r"lr_probe_occupy", r"lr_clock_probe.*"]
NO_DEVICE_WRITES = sorted(n for n in _lib.SIGNATURES if any(re.fullmatch(p, n) for p in _NO_WRITE_PATTERNS))


def test_zz_every_writing_entry_point_ran_guarded():
    """Every `lr_*` entry point that launches a kernel was called under a guard by the cases above."""
    total = len(CASES) + 2 * len(DIRECT)
    ran = ATTEMPTED["rerun"] + ATTEMPTED["direct"]
    if ran != total:
        pytest.skip(f"only {ran} of the {total} cases of this module ran (deselected?): the coverage condition needs all of them")
    assert ATTEMPTED["unguarded"] == 0
    missing = sorted(set(_lib.SIGNATURES) - set(NO_DEVICE_WRITES) - ga.CALLED)
    assert not missing, f"writing entry points never called under a guard: {missing}"
