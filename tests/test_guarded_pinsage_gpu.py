"""The kernel and step cases of tests/test_pinsage_gpu.py (the sampler with and without an exclusion, the weights, the tower in
every shape class, dropout, zero norms, bad rows and the training steps of both paradigms), run again on poisoned, guarded
device allocations (tests/guarded_alloc.py), every case under both fills.

A case asserts the existing function's own assertions, that every guard zone is intact afterwards and that no device
allocation of the package escaped the guard, as `run_guarded` of tests/test_memory_contract_gpu.py does.

This module's name matters: pytest collects tests/ in name order, and the coverage condition at the end of
tests/test_memory_contract_gpu.py asks that every writing entry point of `_lib.SIGNATURES` was called under a guard in the
session.  The `lr_pinsage_*` kernels are called under a guard here, before that module runs."""
import pytest

from tests import guarded_alloc as ga
from tests import test_pinsage_gpu as cases

pytestmark = pytest.mark.gpu

FUNCTIONS = [cases.test_neighbors, cases.test_neighbors_of_a_level_with_an_exclusion, cases.test_neighbors_outside_the_graph,
             cases.test_weights, cases.test_tower, cases.test_tower_wide_batch, cases.test_tower_dropout, cases.test_zero_norm_nodes,
             cases.test_bad_rows, cases.test_fused_and_composed_steps]


def _build():
    out, ids = [], []
    for fn in FUNCTIONS:
        for kw in ga.expand(fn):
            for fill in ga.FILLS:
                out.append((fn, kw, fill))
                ids.append(f"{fn.__name__[5:]}[{ga.case_id(kw)}]-{fill:02X}")
    assert len(set(ids)) == len(ids)
    return out, ids


CASES, IDS = _build()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_pinsage_case_on_guarded_allocations(case, dev):
    fn, kwargs, fill = case
    with ga.guarded(fill) as g:
        fn(dev=dev, **kwargs)
        g.check()
        assert g.unguarded == 0, "device allocations that escaped the guard:\n" + "\n".join(g.unguarded_sites)
