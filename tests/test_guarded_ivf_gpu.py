"""The kernel-level cases of tests/test_ivf_gpu.py (assignment, list build, centroid means, search with its filter and fill
cases, the full probe against the exact scan, same bits on two runs, the unsupported shapes and the whole training), run again
on poisoned, guarded device allocations (tests/guarded_alloc.py), every case under both fills.

A case asserts the existing function's own assertions, that every guard zone is intact afterwards and that no device
allocation of the package escaped the guard, as `run_guarded` of tests/test_memory_contract_gpu.py does.  Outputs, partial keys,
work-item counts and the sort's scratch are `empty` tensors of the package: they arrive filled with 0xFF or 0x5A, so an entry a
kernel left unwritten or read before writing would fail the comparison with the oracle here.

This module's name matters: pytest collects tests/ in name order, and the coverage condition at the end of
tests/test_memory_contract_gpu.py asks that every writing entry point of `_lib.SIGNATURES` was called under a guard in the
session.  `lr_ivf_assign_f32`, `lr_ivf_build_lists`, `lr_ivf_centroids_f32` and `lr_ivf_search_f32` are called under a guard
here, before that module runs."""
import pytest

from tests import guarded_alloc as ga
from tests import test_ivf_gpu as cases

pytestmark = pytest.mark.gpu

FUNCTIONS = [cases.test_assign, cases.test_build_lists, cases.test_centroids, cases.test_search,
             cases.test_search_consumed_list_empties_a_probed_list, cases.test_full_probe_equals_the_exact_scan,
             cases.test_two_runs_give_the_same_bits, cases.test_unsupported_shapes_raise_and_write_nothing,
             cases.test_training_on_a_separated_mixture]


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
def test_ivf_case_on_guarded_allocations(case, dev):
    fn, kwargs, fill = case
    with ga.guarded(fill) as g:
        fn(dev=dev, **kwargs)
        g.check()
        assert g.unguarded == 0, "device allocations that escaped the guard:\n" + "\n".join(g.unguarded_sites)
