"""The kernel, tail and step cases of tests/test_ncf_gpu.py (both pair kernels at every batch and width, the score kernel on
every stack, the argument errors, `DeepFMTail` in its `K > 0, F = 0` form and the training steps), run again on poisoned, guarded
device allocations (tests/guarded_alloc.py), every case under both fills.

A case asserts the existing function's own assertions, that every guard zone is intact afterwards and that no device
allocation of the package escaped the guard, as `run_guarded` of tests/test_memory_contract_gpu.py does.  The outputs the
wrappers allocate (`x`, `gmf`, the scores) and the step's persistent buffers are `empty`s of the package: they arrive filled
with 0xFF or 0x5A, so a kernel that left part of them unwritten, or wrote a row past them, would fail here.

This module's name matters: pytest collects tests/ in name order, and the coverage condition at the end of
tests/test_memory_contract_gpu.py asks that every writing entry point of `_lib.SIGNATURES` was called under a guard in the
session.  `lr_ncf_pair_fwd_f32`, `lr_ncf_pair_bwd_f32` and `lr_ncf_score_f32` are called under a guard here, before that module
runs."""
import pytest

from tests import guarded_alloc as ga
from tests import test_ncf_gpu as cases

pytestmark = pytest.mark.gpu

FUNCTIONS = [cases.test_pair_kernels, cases.test_pair_argument_errors, cases.test_score, cases.test_score_argument_errors,
             cases.test_tail_with_a_pair_term_and_no_linear_term, cases.test_training_steps,
             cases.test_other_steps_run_and_move_the_parameters]


def _flat(v):
    if isinstance(v, dict):
        return "+".join(f"{k}{_flat(x)}" for k, x in v.items()) or "none"
    if isinstance(v, (tuple, list)):
        return "x".join(_flat(x) for x in v)
    return str(v)


def _build():
    out, ids = [], []
    for fn in FUNCTIONS:
        for kw in ga.expand(fn):
            for fill in ga.FILLS:
                out.append((fn, kw, fill))
                ids.append(f"{fn.__name__[5:]}[{','.join(f'{k}={_flat(v)}' for k, v in kw.items())}]-{fill:02X}")
    assert len(set(ids)) == len(ids)
    return out, ids


CASES, IDS = _build()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_ncf_case_on_guarded_allocations(case, dev):
    fn, kwargs, fill = case
    with ga.guarded(fill) as g:
        fn(dev=dev, **kwargs)
        g.check()
        assert g.unguarded == 0, "device allocations that escaped the guard:\n" + "\n".join(g.unguarded_sites)
