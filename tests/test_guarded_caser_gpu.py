"""The kernel and step cases of tests/test_caser_gpu.py (the convolutions in both batch classes, exact ties, dead filters, bad
ids and the training steps), run again on poisoned, guarded device allocations (tests/guarded_alloc.py), every case under both
fills.

A case asserts the existing function's own assertions, that every guard zone is intact afterwards and that no device
allocation of the package escaped the guard, as `run_guarded` of tests/test_memory_contract_gpu.py does.

This module's name matters: pytest collects tests/ in name order, and the coverage condition at the end of
tests/test_memory_contract_gpu.py asks that every writing entry point of `_lib.SIGNATURES` was called under a guard in the
session.  `lr_caser_fwd_f32` and `lr_caser_bwd_f32` are called under a guard here, before that module runs."""
import pytest

from tests import guarded_alloc as ga
from tests import test_caser_gpu as cases

pytestmark = pytest.mark.gpu

FUNCTIONS = [cases.test_stack, cases.test_stack_wide_batches, cases.test_equal_positions_pool_to_the_first, cases.test_dead_filter,
             cases.test_bad_ids, cases.test_training_steps]


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
def test_caser_case_on_guarded_allocations(case, dev):
    fn, kwargs, fill = case
    with ga.guarded(fill) as g:
        fn(dev=dev, **kwargs)
        g.check()
        assert g.unguarded == 0, "device allocations that escaped the guard:\n" + "\n".join(g.unguarded_sites)
