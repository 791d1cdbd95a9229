"""The kernel-level cases of tests/test_eval_gpu.py (keys, rank statistics at every size and pattern, pointwise sums, listwise
metrics with the unsupported k, coverage, same bits on two runs), run again on poisoned, guarded device allocations
(tests/guarded_alloc.py), every case under both fills.

A case asserts the existing function's own assertions, that every guard zone is intact afterwards and that no device
allocation of the package escaped the guard, as `run_guarded` of tests/test_memory_contract_gpu.py does.  Keys, the NaN count,
the integer and fp64 outputs, the per-user rows, the coverage flags and count and both workspaces are `empty` tensors of the
package: they arrive filled with 0xFF or 0x5A, so an element a kernel left unwritten, a count added onto a word nobody zeroed
or a tile summary read before it was written would fail the comparison with the oracle here.

This module's name matters: pytest collects tests/ in name order, and the coverage condition at the end of
tests/test_memory_contract_gpu.py asks that every writing entry point of `_lib.SIGNATURES` was called under a guard in the
session.  `lr_eval_keys_f32`, `lr_eval_rank_stats`, `lr_eval_point_sums_f32`, `lr_eval_listwise` and `lr_eval_coverage_i32` are
called under a guard here, before that module runs."""
import pytest

from tests import guarded_alloc as ga
from tests import test_eval_gpu as cases

pytestmark = pytest.mark.gpu

FUNCTIONS = [cases.test_keys, cases.test_rank_stats, cases.test_rank_stats_argument_errors, cases.test_point_sums,
             cases.test_point_sums_nan_prediction_poisons_the_log_loss, cases.test_listwise,
             cases.test_listwise_unsupported_k_raises_and_writes_nothing, cases.test_coverage,
             cases.test_two_runs_give_the_same_bits]


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
def test_eval_case_on_guarded_allocations(case, dev):
    fn, kwargs, fill = case
    with ga.guarded(fill) as g:
        fn(dev=dev, **kwargs)
        g.check()
        assert g.unguarded == 0, "device allocations that escaped the guard:\n" + "\n".join(g.unguarded_sites)
