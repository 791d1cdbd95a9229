"""The kernel and step cases of tests/test_wide_deep_gpu.py (both FTRL kernels on every stream shape, the argument errors and
the training steps), run again on poisoned, guarded device allocations (tests/guarded_alloc.py), every case under both fills.

A case asserts the existing function's own assertions, that every guard zone is intact afterwards and that no device
allocation of the package escaped the guard, as `run_guarded` of tests/test_memory_contract_gpu.py does.  The long-run
workspace of `lr_ftrl_rows_f32` is an `empty` of the package: it arrives filled with 0xFF or 0x5A, so a kernel that relied on
its contents would fail here.

This module's name matters: pytest collects tests/ in name order, and the coverage condition at the end of
tests/test_memory_contract_gpu.py asks that every writing entry point of `_lib.SIGNATURES` was called under a guard in the
session.  `lr_ftrl_rows_f32` and `lr_ftrl_dense_f32` are called under a guard here, before that module runs."""
import inspect

import pytest

from tests import guarded_alloc as ga
from tests import test_wide_deep_gpu as cases
from tests.test_wide_deep_gpu import feat_data  # noqa: F401  (the module fixture of the step cases)

pytestmark = pytest.mark.gpu

FUNCTIONS = [cases.test_rows_kernel, cases.test_rows_kernel_without_a_workspace, cases.test_empty_stream, cases.test_dense_kernel,
             cases.test_dense_kernel_on_an_unaligned_range, cases.test_first_dense_step_with_a_zero_gradient_zeroes_var,
             cases.test_two_runs_give_the_same_bits, cases.test_argument_errors, cases.test_training_steps]


def _build():
    out, ids = [], []
    for fn in FUNCTIONS:
        for kw in ga.expand(fn):
            for fill in ga.FILLS:
                out.append((fn, kw, fill))
                cid = ga.case_id({k: (cases._cfg_id(v) if k == "cfg" else v) for k, v in kw.items()})
                ids.append(f"{fn.__name__[5:]}[{cid}]-{fill:02X}")
    assert len(set(ids)) == len(ids)
    return out, ids


CASES, IDS = _build()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wide_deep_case_on_guarded_allocations(case, dev, feat_data):  # noqa: F811
    fn, kwargs, fill = case
    if "feat_data" in inspect.signature(fn).parameters:
        kwargs = dict(kwargs, feat_data=feat_data)
    with ga.guarded(fill) as g:
        fn(dev=dev, **kwargs)
        g.check()
        assert g.unguarded == 0, "device allocations that escaped the guard:\n" + "\n".join(g.unguarded_sites)
