"""The guarded-allocation harness (tests/guarded_alloc.py) proves itself on CPU tensors, with the allocator told to guard CPU
allocations too: calling forms, dtypes, alignment, poison, the two overrun directions, case expansion against pytest's own,
and that every patch is undone.  These are the only places that damage a guard on purpose, and they do it through the
harness's own raw buffer: every store is in bounds of the real allocation.  No GPU kernel is involved."""
import sys

import numpy as np
import pytest
import torch

from librecommender_amd import ops
from librecommender_amd.layers import embedding
from tests import guarded_alloc as ga
from tests import test_ops_gpu as ops_cases

DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16, torch.int32, torch.int64, torch.int16, torch.int8,
          torch.uint8, torch.bool]
CPU = torch.device("cpu")


def guarded_cpu(fill):
    return ga.guarded(fill, guard_cpu=True, record=False)


def poison_of(dtype, fill):
    return torch.full((dtype.itemsize,), fill, dtype=torch.uint8).view(dtype)[0]


def body_offset(g, t):
    """Byte offset of `t`'s first element inside the raw buffer of the allocation that holds it."""
    for a in g.allocs:
        lo = a.raw.data_ptr()
        if lo <= t.data_ptr() < lo + a.raw.numel():
            return a, t.data_ptr() - lo
    raise AssertionError("tensor was not allocated by the guard")


@pytest.mark.parametrize("fill", ga.FILLS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_calling_form_gives_a_contiguous_aligned_poisoned_body(dtype, fill):
    with guarded_cpu(fill) as g:
        P = ops.torch
        assert P is ga.PROXY
        made = [
            (P.empty(7, dtype=dtype, device=CPU), (7,)),
            (P.empty((3, 5), dtype=dtype, device="cpu"), (3, 5)),
            (P.empty([3, 5], dtype=dtype, device=CPU), (3, 5)),
            (P.empty(2, 3, 4, dtype=dtype, device=CPU), (2, 3, 4)),
            (P.empty(torch.Size((4, 1)), dtype=dtype, device=CPU), (4, 1)),
            (P.empty((), dtype=dtype, device=CPU), ()),
            (P.empty((np.int64(6), 2), dtype=dtype, device=CPU), (6, 2)),
            (P.empty(size=(2, 2), dtype=dtype, device=CPU), (2, 2)),
            (P.empty_like(torch.zeros((5, 3), dtype=dtype)), (5, 3)),
            (P.empty_like(torch.zeros((5, 3)), dtype=dtype), (5, 3)),
        ]
        assert g.guarded == len(made) and g.unguarded == 0
        for t, shape in made:
            assert t.shape == shape and t.dtype == dtype and t.is_contiguous() and t.device == CPU
            assert t.storage_offset() == 0, "as for a real allocation: callers address flat buffers by storage_offset()"
            a, off = body_offset(g, t)
            assert off == a.guard and off % 256 == 0 and a.guard >= 64 * 1024
            assert a.nbytes == t.numel() * dtype.itemsize and a.raw.numel() == 2 * a.guard + a.nbytes
            assert bool((a.raw[:a.guard] == ga.GUARD_BYTE).all()) and bool((a.raw[a.guard + a.nbytes:] == ga.GUARD_BYTE).all())
            assert bool((a.raw[a.guard:a.guard + a.nbytes] == fill).all()), "the body of an `empty` holds the poison"
        g.check()


def test_poison_values_are_what_the_documentation_says():
    assert torch.isnan(poison_of(torch.float32, 0xFF)) and poison_of(torch.int32, 0xFF) == -1 and poison_of(torch.int64, 0xFF) == -1
    assert abs(float(poison_of(torch.float32, 0x5A)) - 1.5e16) < 0.05e16 and int(poison_of(torch.int32, 0x5A)) == 1_515_870_810


def test_guard_is_at_least_two_rows_and_256_aligned():
    assert ga.guard_bytes((10,), 4) == 64 * 1024
    assert ga.guard_bytes((3, 100_000), 4) == 800_000 + (-800_000) % 256
    assert ga.guard_bytes((3, 100_001), 4) % 256 == 0 and ga.guard_bytes((3, 100_001), 4) >= 2 * 100_001 * 4
    assert ga.guard_bytes((), 8) == 64 * 1024
    with guarded_cpu(0xFF) as g:
        t = ops.torch.empty((2, 50_000), dtype=torch.float32, device=CPU)
        a, off = body_offset(g, t)
        assert a.guard >= 2 * 50_000 * 4 and off % 256 == 0


@pytest.mark.parametrize("fill", ga.FILLS)
def test_value_factories_keep_their_value(fill):
    with guarded_cpu(fill) as g:
        P = ops.torch
        src = torch.arange(12, dtype=torch.int32).reshape(3, 4)
        cases = [
            (P.zeros(5, dtype=torch.int64, device=CPU), torch.zeros(5, dtype=torch.int64)),
            (P.zeros((2, 3), dtype=torch.float32, device=CPU), torch.zeros((2, 3))),
            (P.zeros((), device=CPU), torch.zeros(())),
            (P.ones((4,), dtype=torch.float32, device=CPU), torch.ones(4)),
            (P.ones(2, 2, dtype=torch.int32, device=CPU), torch.ones(2, 2, dtype=torch.int32)),
            (P.full((6,), -1, dtype=torch.int32, device=CPU), torch.full((6,), -1, dtype=torch.int32)),
            (P.full((2, 2), 0.5, device=CPU), torch.full((2, 2), 0.5)),
            (P.full((3,), 7, device=CPU), torch.full((3,), 7)),
            (P.full((3,), True, device=CPU), torch.full((3,), True)),
            (P.zeros_like(src), torch.zeros_like(src)),
            (P.ones_like(src), torch.ones_like(src)),
            (P.full_like(src, -1), torch.full_like(src, -1)),
            (P.zeros_like(src, dtype=torch.float32), torch.zeros_like(src, dtype=torch.float32)),
        ]
        assert g.guarded == len(cases) and g.unguarded == 0
        for got, want in cases:
            assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want)
        t = P.empty_like(src.t())           # a dense, non-contiguous source keeps its strides, as torch.empty_like does
        assert t.shape == (4, 3) and t.stride() == torch.empty_like(src.t()).stride()
        g.check()


def test_what_passes_through_and_what_is_counted():
    with ga.guarded(0xFF, record=False) as g:          # the production setting: CPU allocations are not guarded
        t = ops.torch.empty(5, dtype=torch.float32)
        assert g.guarded == 0 and g.unguarded == 0 and t.shape == (5,)
    with guarded_cpu(0xFF) as g:
        P = ops.torch
        z = P.empty(0, dtype=torch.float32, device=CPU)
        z2 = P.zeros((3, 0), dtype=torch.int32, device=CPU)
        assert z.numel() == 0 and z2.shape == (3, 0) and g.guarded == 0 and g.unguarded == 0, "zero-size passes through"
        if torch.cuda.is_available():      # pinning needs a device runtime
            P.empty(4, dtype=torch.float32, pin_memory=True)
            assert g.guarded == 0 and g.unguarded == 0
        out = P.empty(3, dtype=torch.float32, device=CPU, layout=torch.strided)
        assert out.shape == (3,) and g.guarded == 0 and g.unguarded == 1, "an unsupported form is passed through and counted"
        assert "layout" in g.unguarded_sites[0] and "test_guarded_alloc_cpu.py" in g.unguarded_sites[0]
        rg = P.zeros(3, device=CPU, requires_grad=True)
        assert rg.requires_grad and g.guarded == 1


def standin_double(P, x, rows_written=None, g=None):
    """Stand-in for a kernel wrapper: allocates its output as the package does and writes 2 * x row by row.  `rows_written`
    other than the row count models a kernel that skips its tail or runs one row over; the extra row is stored through
    the harness's raw buffer (in bounds of the real allocation)."""
    n, w = x.shape
    out = P.empty((n, w), dtype=x.dtype, device=x.device)
    rows = n if rows_written is None else rows_written
    for r in range(min(rows, n)):
        out[r] = 2 * x[r]
    if rows > n:
        a, _ = body_offset(g, out)
        rowb = w * x.dtype.itemsize
        a.raw[a.guard + n * rowb:a.guard + rows * rowb].view(x.dtype).fill_(3)
    return out


@pytest.mark.parametrize("fill", ga.FILLS)
def test_standin_op_right_short_and_long(fill):
    x = torch.arange(1, 13, dtype=torch.float32).reshape(4, 3)
    with guarded_cpu(fill) as g:
        out = standin_double(ops.torch, x)
        g.check()
        assert torch.equal(out, 2 * x)
    with guarded_cpu(fill) as g:                       # a skipped last row: the guards hold, the comparison does not
        out = standin_double(ops.torch, x, rows_written=3)
        g.check()
        assert torch.equal(out[:3], 2 * x[:3]) and not torch.equal(out, 2 * x)
        assert not np.allclose(out.numpy(), (2 * x).numpy(), rtol=1e-3, atol=1e-3)
    with guarded_cpu(fill) as g:                       # one row too many: the guard after the body catches it
        out = standin_double(ops.torch, x, rows_written=5, g=g)
        assert torch.equal(out, 2 * x)
        with pytest.raises(ga.GuardViolation) as e:
            g.check()
        msg = str(e.value)
        assert "guard after the body" in msg and "first changed byte 0 byte(s) past the end" in msg
        assert "test_guarded_alloc_cpu.py" in msg and "(4, 3)" in msg and "torch.float32" in msg


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32, torch.int64])
@pytest.mark.parametrize("fill", ga.FILLS)
def test_one_element_out_of_bounds_trips_check_on_the_right_side(dtype, fill):
    sz = dtype.itemsize
    with guarded_cpu(fill) as g:
        t = ops.torch.empty((5, 3), dtype=dtype, device=CPU)
        a, _ = body_offset(g, t)
        t[4, 2] = 1                                    # the last element INSIDE the body
        t[0, 0] = 1
        g.check()
        a.raw[a.guard + a.nbytes:a.guard + a.nbytes + sz].view(dtype).fill_(1)      # one element past the end
        with pytest.raises(ga.GuardViolation) as e:
            g.check()
        msg = str(e.value)
        assert "guard after the body" in msg and "first changed byte 0 byte(s) past the end" in msg and "before the start" not in msg
        assert "(5, 3)" in msg and str(dtype) in msg
        a.raw[a.guard + a.nbytes:a.guard + a.nbytes + sz] = ga.GUARD_BYTE
        g.check()
        a.raw[a.guard - sz:a.guard].view(dtype).fill_(1)                           # one element before the start
        with pytest.raises(ga.GuardViolation) as e:
            g.check()
        msg = str(e.value)
        assert "guard before the body" in msg and f"first changed byte {sz} byte(s) before the start" in msg
        assert "past the end" not in msg


def test_failure_names_the_allocating_line_inside_the_package():
    with guarded_cpu(0x5A) as g:
        tables = embedding.FieldTables(3, 4, 5, 8, CPU)
        sites = {a.site: a for a in g.allocs}
        embed_site = next(s for s, a in sites.items() if a.kind == "empty" and a.shape == (tables.V, 8))
        assert embed_site.startswith("librecommender_amd/layers/embedding.py:") and int(embed_site.split(":")[1]) > 0
        assert all(s.startswith("librecommender_amd/layers/embedding.py:") for s in sites)
        assert torch.isfinite(tables.embed).all() and (tables.embed.abs() < 10).all(), "the initialiser overwrote the poison"
        assert not tables.m.any() and g.unguarded == 0
        g.check()
        a = sites[embed_site]
        a.raw[a.guard + a.nbytes + 8] = 0
        with pytest.raises(ga.GuardViolation) as e:
            g.check()
        assert embed_site in str(e.value) and "first changed byte 8 byte(s) past the end" in str(e.value)


def _collected_params(names):
    """callspec.params of every collected item of tests/test_ops_gpu.py for the named functions, from pytest itself."""
    got = {n: [] for n in names}

    class Grab:
        def pytest_collection_modifyitems(self, items):
            for it in items:
                fn = it.originalname
                if fn in got:
                    got[fn].append(dict(it.callspec.params) if hasattr(it, "callspec") else {})

    rc = pytest.main(["--collect-only", "-q", "-p", "no:cacheprovider", ops_cases.__file__], plugins=[Grab()])
    assert rc == 0
    return got


def _frozen(dicts):
    return sorted(tuple(sorted(d.items())) for d in dicts)


def test_expand_reproduces_pytests_parametrization(capsys):
    names = ["test_pair_dot", "test_segments_bit_exact", "test_fm_embed_fused_backward_adam", "test_embed_gather_bit_exact",
             "test_adam_dense_tf_semantics"]
    want = _collected_params(names)
    capsys.readouterr()
    for n in names:
        mine = ga.expand(getattr(ops_cases, n))
        assert len(mine) == len(want[n]) > 0, n
        assert _frozen(mine) == _frozen(want[n]), n
    assert len(ga.expand(ops_cases.test_pair_dot)) == 3                          # one mark, one name
    assert len(ga.expand(ops_cases.test_segments_bit_exact)) == 12               # one mark, two names
    assert len(ga.expand(ops_cases.test_fm_embed_fused_backward_adam)) == 12     # stacked marks
    assert ga.expand(ops_cases.test_adam_dense_tf_semantics) == [{}]
    assert ga.case_id({"K": 16, "shape": (3, 4), "x": object()}) == "K=16,shape=3x4,x#object"


def test_proxy_leaves_everything_but_the_factories_alone():
    P = ga.PROXY
    assert P.Tensor is torch.Tensor and P.float32 is torch.float32 and P.int64 is torch.int64 and P.cuda is torch.cuda
    assert P.cuda.is_available is torch.cuda.is_available and P.no_grad is torch.no_grad and P.nn is torch.nn
    assert P.device is torch.device and P.from_numpy is torch.from_numpy and P.autograd is torch.autograd
    assert isinstance(torch.ones(1), P.Tensor)
    with pytest.raises(AttributeError):
        P.no_such_attribute
    t = P.empty(3, dtype=torch.float32)               # no guard active: the real factory
    assert t.shape == (3,) and not ga._ACTIVE


def test_patches_are_undone_on_exit_even_after_an_error():
    def package_torch():
        return {n: m.torch for n, m in sys.modules.items()
                if m is not None and (n == "librecommender_amd" or n.startswith("librecommender_amd.")) and hasattr(m, "torch")}

    with guarded_cpu(0xFF):
        inside = package_torch()
    assert len(inside) > 10 and all(v is ga.PROXY for v in inside.values()), "every package module sees the proxy"
    assert all(v is torch for v in package_torch().values())
    ops._WS_CACHE["stale"] = 1
    with pytest.raises(RuntimeError):
        with guarded_cpu(0x5A):
            assert "stale" not in ops._WS_CACHE and ops.torch is ga.PROXY
            ops._L1_WS["made inside"] = 1
            raise RuntimeError("boom")
    assert all(v is torch for v in package_torch().values()) and not ga._ACTIVE
    assert not ops._WS_CACHE and not ops._L1_WS, "scratch allocated under a guard does not outlive it"
    with guarded_cpu(0xFF) as outer:                  # nesting: the innermost guard allocates, the outer patch survives it
        with guarded_cpu(0x5A) as inner:
            ops.torch.empty(2, dtype=torch.int32, device=CPU)
        assert inner.guarded == 1 and outer.guarded == 0 and ops.torch is ga.PROXY
    assert ops.torch is torch


def test_recorder_records_only_while_a_guard_is_active():
    class FakeLib:
        def __init__(self):
            self.calls = []
            self.other = 5

        def lr_something(self, x):
            self.calls.append(x)
            return x + 1

    fake = FakeLib()
    rec = ga.LibRecorder(fake)
    before = set(ga.CALLED)
    assert rec.lr_something(1) == 2 and rec.other == 5
    assert ga.CALLED == before
    with guarded_cpu(0xFF):
        assert rec.lr_something(2) == 3
    assert ga.CALLED == before | {"lr_something"} and fake.calls == [1, 2]
    ga.CALLED.discard("lr_something")
