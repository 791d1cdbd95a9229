"""Poisoned, guarded device allocations for the kernel parity tests (a plain helper: no conftest, no plugin).

The package allocates every kernel output and workspace with a torch factory (`torch.empty` and friends).  In a test process
the caching allocator hands such a call either fresh zero pages or the block the same test has just freed, which often
still holds the previous, correct result, and it rounds blocks to 512 B and packs small ones together.  Three kinds of
memory-contract bug are therefore invisible to a parity test on ordinary allocations:

1. a kernel leaves part of an output unwritten (the test reads zeros, or the last call's right answer);
2. a kernel or wrapper relies on a workspace being zero where the header does not promise it;
3. a kernel stores a few elements before or after its output or workspace (the store lands in padding or in a neighbour
   nobody compares).

`guarded(fill)` makes all three visible.  While it is active, the name `torch` of every loaded `librecommender_amd.*`
module is a proxy that forwards everything to the real module except the factory functions `empty`, `zeros`, `ones`, `full`
and their `*_like` forms (the package uses no `Tensor.new_*` factory).  A device allocation of n bytes becomes one uint8
buffer `[guard | body | guard]`; the caller gets `body.view(dtype).reshape(shape)` (the body re-imported over a storage
of its own, so that `storage_offset()` is 0 as for a real allocation).  Guards are 0xA5 bytes, a multiple of
256 B wide (the body keeps the alignment include/libreco_hip.h asks for), at least 64 KiB and at least two rows of the
allocation, so that an overrun by a row or by a tile of rows lands in them.  The body of an `empty` is filled with `fill`:
0xFF (f32 NaN, int32 / int64 -1) or 0x5A (f32 1.5e16, int32 1,515,870,810: beyond any index a test uses).  Both are needed:
-1 is this project's own "dropped" / "empty slot" value and can pass for initialised memory.  `check()` verifies every guard
byte of every allocation made in the context.

What this cannot see: out-of-bounds READS.  Those need a device address sanitizer or page-fault (XNACK) runs, which the
shared MI355X machines do not allow; nothing here pretends to cover them.  A stray store that jumps over the guard (further
than 64 KiB and two rows from the allocation) is not seen either.

The module also holds the entry-point recorder (which `lr_*` functions ran while a guard was active) and `expand()`, which
turns the `parametrize` marks of an existing test function into the keyword dictionaries pytest would pass.
"""
from __future__ import annotations

import importlib
import itertools
import operator
import pkgutil
import sys
import types
from pathlib import Path

import torch as _torch

GUARD_BYTE = 0xA5
GUARD_MIN = 64 * 1024
ALIGN = 256
FILLS = (0xFF, 0x5A)

_PKG = "librecommender_amd"
_PKG_DIR = str(Path(__file__).resolve().parent.parent / _PKG)
_FACTORIES = ("empty", "zeros", "ones", "full", "empty_like", "zeros_like", "ones_like", "full_like")
_PLAIN_KW = {"dtype", "device", "requires_grad", "pin_memory"}

CALLED: set = set()          # every lr_* entry point called while a guard was active, over the whole session
_ACTIVE: list = []           # stack of active Guard objects (the innermost one allocates)


class GuardViolation(AssertionError):
    pass


def guard_bytes(shape, itemsize: int) -> int:
    """Width of one guard zone: a multiple of 256 B, >= 64 KiB and >= two rows (2 * shape[-1] * itemsize)."""
    row = int(shape[-1]) * int(itemsize) if len(shape) else 0
    need = max(GUARD_MIN, 2 * row)
    return (need + ALIGN - 1) // ALIGN * ALIGN


class _Alloc:
    __slots__ = ("raw", "guard", "nbytes", "shape", "dtype", "site", "kind")

    def __init__(self, raw, guard, nbytes, shape, dtype, site, kind):
        self.raw, self.guard, self.nbytes, self.shape, self.dtype, self.site, self.kind = raw, guard, nbytes, shape, dtype, site, kind

    def describe(self) -> str:
        return f"torch.{self.kind} of shape {tuple(self.shape)} {self.dtype} allocated at {self.site}"


def _site() -> str:
    """file:line of the allocating call: the innermost frame inside the package, else the first frame outside this file."""
    f = sys._getframe(1)
    first = None
    while f is not None:
        fn = f.f_code.co_filename
        if fn != __file__ and first is None:
            first = f"{fn}:{f.f_lineno}"
        if fn.startswith(_PKG_DIR):
            return f"{_PKG}/{Path(fn).relative_to(_PKG_DIR).as_posix()}:{f.f_lineno}"
        f = f.f_back
    return first or "?"


def _shape_of(args):
    """`empty(n)`, `empty((a, b))`, `empty([a, b])`, `empty(a, b)` -> tuple of ints; None if the form is not understood."""
    try:
        if len(args) == 1 and isinstance(args[0], (tuple, list, _torch.Size)):
            return tuple(operator.index(s) for s in args[0])
        if len(args) >= 1:
            return tuple(operator.index(s) for s in args)
    except TypeError:
        return None
    return None


class Guard:
    """One active guarded-allocation context; see the module docstring."""

    def __init__(self, fill: int, guard_cpu: bool = False):
        assert fill in FILLS, f"fill must be one of {[hex(f) for f in FILLS]}"
        self.fill = fill
        self.guard_cpu = guard_cpu
        self.allocs: list = []
        self.unguarded = 0
        self.unguarded_sites: list = []
        self.guarded = 0

    # ---- allocation -------------------------------------------------------------------------------------------------
    def _carve(self, kind, shape, dtype, device, strides=None):
        itemsize = _torch.empty((), dtype=dtype).element_size()
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * itemsize
        g = guard_bytes(shape, itemsize)
        raw = _torch.empty(2 * g + nbytes, dtype=_torch.uint8, device=device)
        raw.fill_(GUARD_BYTE)
        body = raw[g:g + nbytes]
        if kind.startswith("empty"):
            body.fill_(self.fill)
        # re-import the body as a tensor over a storage of its own (same memory, kept alive by the capsule): like a real
        # allocation its storage_offset() is 0, which callers that address a flat buffer by it rely on
        body = _torch.utils.dlpack.from_dlpack(_torch.utils.dlpack.to_dlpack(body))
        t = body.view(dtype)
        t = t.reshape(shape) if strides is None else t.as_strided(shape, strides)
        self.allocs.append(_Alloc(raw, g, nbytes, tuple(shape), dtype, _site(), kind))
        self.guarded += 1
        return t

    def factory(self, kind, args, kwargs):
        real = getattr(_torch, kind)
        like, full = kind.endswith("_like"), kind.startswith("full")
        a, kw = list(args), dict(kwargs)
        src = value = size = None
        try:
            if like:
                src = a.pop(0) if a else kw.pop("input")
                if full:
                    value = a.pop(0) if a else kw.pop("fill_value")
            elif full:
                size = a.pop(0) if a else kw.pop("size")
                value = a.pop(0) if a else kw.pop("fill_value")
            elif a:
                size, a = _shape_of(a), []
            else:
                size = kw.pop("size")
        except KeyError:
            return real(*args, **kwargs)          # a malformed call: the real factory words the error
        dev_kw = kw.get("device")
        if dev_kw is not None:
            device = _torch.device(dev_kw)
        elif like and isinstance(src, _torch.Tensor):
            device = src.device
        else:
            device = _torch.device("cpu")
        if (device.type == "cpu" and not self.guard_cpu) or kw.get("pin_memory"):
            return real(*args, **kwargs)

        def unguarded(why):
            self.unguarded += 1
            self.unguarded_sites.append(f"{_site()} torch.{kind}: {why}")
            return real(*args, **kwargs)

        if a:
            return unguarded("extra positional arguments")
        if device.type == "cuda" and _torch.cuda.is_current_stream_capturing():
            return unguarded("the stream is capturing a graph: the guard's fills would be recorded into it")
        extra = set(kw) - _PLAIN_KW
        if like and "memory_format" in extra and kw["memory_format"] in (_torch.preserve_format, _torch.contiguous_format):
            extra.discard("memory_format")
        if extra:
            return unguarded(f"keyword(s) {sorted(extra)}")
        strides = None
        if like:
            if not isinstance(src, _torch.Tensor):
                return unguarded("source is not a tensor")
            shape = tuple(src.shape)
            dtype = kw.get("dtype") or src.dtype
            if kw.get("memory_format", _torch.preserve_format) is _torch.preserve_format and not src.is_contiguous():
                meta = _torch.empty_like(_torch.empty_strided(shape, src.stride(), dtype=dtype, device="meta"))
                strides = tuple(meta.stride())
                if all(shape) and 1 + sum((n - 1) * st for n, st in zip(shape, strides)) != meta.numel():
                    return unguarded("source is not dense")
        else:
            shape = None if size is None else _shape_of([size])
            if shape is None:
                return unguarded("size form not understood")
            dtype = kw.get("dtype")
            if dtype is None:
                dtype = _torch.full((), value).dtype if full else _torch.get_default_dtype()
        if any(s == 0 for s in shape):
            return real(*args, **kwargs)
        t = self._carve(kind, shape, dtype, device, strides)
        if kind.startswith("zeros"):
            t.zero_()
        elif kind.startswith("ones"):
            t.fill_(1)
        elif full:
            t.fill_(value)
        if kw.get("requires_grad"):
            t.requires_grad_(True)
        return t

    # ---- verification -----------------------------------------------------------------------------------------------
    def check(self) -> None:
        """Synchronise and verify every guard byte of every allocation made so far; raises GuardViolation naming the
        allocation site, shape, dtype, side and offset of the first changed byte of every damaged allocation."""
        if not self.allocs:
            return
        devs = {a.raw.device for a in self.allocs if a.raw.device.type != "cpu"}
        for d in devs:
            _torch.cuda.synchronize(d)
        flags = [(a.raw[:a.guard] != GUARD_BYTE).any() | (a.raw[a.guard + a.nbytes:] != GUARD_BYTE).any() for a in self.allocs]
        if len({f.device for f in flags}) == 1:     # one transfer for all of them
            bad = _torch.stack(flags).cpu().tolist()
        else:
            bad = [bool(f) for f in flags]
        if not any(bad):
            return
        lines = []
        for a, b in zip(self.allocs, bad):
            if not b:
                continue
            for side, zone in (("before", a.raw[:a.guard]), ("after", a.raw[a.guard + a.nbytes:])):
                changed = (zone != GUARD_BYTE).nonzero().flatten()
                if changed.numel() == 0:
                    continue
                first, last = int(changed[0]), int(changed[-1])
                if side == "before":
                    where = (f"first changed byte {a.guard - first} byte(s) before the start of the body, "
                             f"nearest {a.guard - last} byte(s) before it")
                else:
                    where = (f"first changed byte {first} byte(s) past the end of the body, "
                             f"furthest {last} byte(s) past it")
                lines.append(f"guard {side} the body overwritten ({int(changed.numel())} byte(s)): {where}; {a.describe()}")
        raise GuardViolation("\n".join(lines))


class TorchProxy(types.ModuleType):
    """Stands in for the name `torch` inside the package: everything is the real module's except the factories."""

    def __init__(self):
        super().__init__("torch")
        for kind in _FACTORIES:
            self.__dict__[kind] = _make_factory(kind)

    def __getattr__(self, name):
        return getattr(_torch, name)


def _make_factory(kind):
    def factory(*args, **kwargs):
        if not _ACTIVE:
            return getattr(_torch, kind)(*args, **kwargs)
        return _ACTIVE[-1].factory(kind, args, kwargs)
    factory.__name__ = kind
    return factory


PROXY = TorchProxy()


# ---- entry-point recorder -------------------------------------------------------------------------------------------
class _RecordedFn:
    __slots__ = ("_fn", "_name")

    def __init__(self, fn, name):
        self._fn, self._name = fn, name

    def __call__(self, *args):
        if _ACTIVE:
            CALLED.add(self._name)
        return self._fn(*args)

    def __getattr__(self, name):
        return getattr(self._fn, name)


class LibRecorder:
    """Wraps the loaded ctypes library: records the name of every `lr_*` function called while a guard is active."""

    def __init__(self, lib):
        self.__dict__["_real"] = lib
        self.__dict__["_fns"] = {}

    def __getattr__(self, name):
        real = getattr(self._real, name)
        if not name.startswith("lr_"):
            return real
        fn = self._fns.get(name)
        if fn is None:
            fn = self._fns[name] = _RecordedFn(real, name)
        return fn

    def __setattr__(self, name, value):
        setattr(self._real, name, value)


# ---- the context manager --------------------------------------------------------------------------------------------
_IMPORTED_ALL = False


def _package_modules():
    """Every loaded `librecommender_amd.*` module whose global `torch` is the real module."""
    global _IMPORTED_ALL
    if not _IMPORTED_ALL:      # a module first imported INSIDE a guard would keep the real torch: import them all now
        pkg = importlib.import_module(_PKG)
        for info in pkgutil.walk_packages(pkg.__path__, _PKG + "."):
            if ".csrc" in info.name or info.name in sys.modules:
                continue
            try:
                importlib.import_module(info.name)
            except Exception:      # an optional dependency is missing: that module cannot allocate either
                pass
        _IMPORTED_ALL = True
    return [m for n, m in list(sys.modules.items())
            if m is not None and (n == _PKG or n.startswith(_PKG + ".")) and getattr(m, "torch", None) is _torch]


def _clear_scratch_caches():
    ops = sys.modules.get(_PKG + ".ops")
    for name in ("_WS_CACHE", "_L1_WS"):
        cache = getattr(ops, name, None)
        if isinstance(cache, dict):
            cache.clear()


class guarded:
    """`with guarded(0xFF) as g: ...; g.check()`.  Patches are undone on exit, whatever happened inside.

    `guard_cpu=True` guards CPU allocations too (the harness's own self-test); `record=False` leaves the C library alone
    (needed where it has not been built)."""

    def __init__(self, fill: int, guard_cpu: bool = False, record: bool = True):
        self.g = Guard(fill, guard_cpu)
        self.record = record
        self._patched: list = []
        self._lib_prev = None
        self._lib_mod = None

    def __enter__(self) -> Guard:
        _clear_scratch_caches()
        try:
            for m in _package_modules():
                m.torch = PROXY
                self._patched.append(m)
            if self.record:
                lib_mod = importlib.import_module(_PKG + "._lib")
                real = lib_mod.load()
                if not isinstance(real, LibRecorder):
                    self._lib_mod, self._lib_prev = lib_mod, real
                    lib_mod._lib = LibRecorder(real)
        except BaseException:
            self._undo()
            raise
        _ACTIVE.append(self.g)
        return self.g

    def _undo(self):
        if self._lib_mod is not None:
            self._lib_mod._lib = self._lib_prev
            self._lib_mod = None
        for m in self._patched:
            m.torch = _torch
        self._patched.clear()
        _clear_scratch_caches()

    def __exit__(self, *exc):
        _ACTIVE.remove(self.g)
        self._undo()
        return False


# ---- case expansion -------------------------------------------------------------------------------------------------
def _argnames(names):
    return [s.strip() for s in names.split(",") if s.strip()] if isinstance(names, str) else list(names)


def expand(fn):
    """The keyword dictionaries pytest passes to `fn` for its `parametrize` marks: the product of stacked marks, one
    empty dictionary for a function without marks.  `indirect` parametrization is not used by this suite and refused."""
    marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
    per_mark = []
    for m in marks:
        if m.kwargs.get("indirect"):
            raise NotImplementedError(f"{fn.__name__}: indirect parametrization")
        names = _argnames(m.args[0] if m.args else m.kwargs["argnames"])
        values = m.args[1] if len(m.args) > 1 else m.kwargs["argvalues"]
        rows = []
        for v in values:
            if hasattr(v, "values") and hasattr(v, "marks") and not isinstance(v, dict):      # pytest.param(...)
                v = v.values
            elif len(names) == 1:
                v = (v,)
            v = tuple(v)
            assert len(v) == len(names), (fn.__name__, names, v)
            rows.append(dict(zip(names, v)))
        per_mark.append(rows)
    out = []
    for combo in itertools.product(*reversed(per_mark)):      # the mark nearest the function varies fastest, as in pytest
        kw = {}
        for d in combo:
            kw.update(d)
        out.append(kw)
    return out


def case_id(kwargs: dict) -> str:
    """A readable id for one expanded case."""
    parts = []
    for k, v in kwargs.items():
        if isinstance(v, (int, float, bool, str, type(None))):
            parts.append(f"{k}={v}")
        elif isinstance(v, (tuple, list)) and len(v) <= 6 and all(isinstance(x, (int, float, bool, str, type(None))) for x in v):
            parts.append(f"{k}=" + "x".join(str(x) for x in v))
        else:
            parts.append(f"{k}#{type(v).__name__}")
    return ",".join(parts)
