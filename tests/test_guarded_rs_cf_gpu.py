"""The kernel-level cases of tests/test_rs_cf_gpu.py (pair state, sums of squares, merge and refresh, the visible view,
predict, same bits on two runs, the argument errors and the oversize guard), run again on poisoned, guarded device allocations
(tests/guarded_alloc.py), every case under both fills.

A case asserts the existing function's own assertions, that every guard zone is intact afterwards and that no device
allocation of the package escaped the guard, as `run_guarded` of tests/test_memory_contract_gpu.py does.  The outputs of the
two-pass kernels and of the merge are `empty` tensors of the package: they arrive filled with 0xFF or 0x5A, so an entry that a
kernel left unwritten would fail the comparison with the oracle here.

This module's name matters: pytest collects tests/ in name order, and the coverage condition at the end of
tests/test_memory_contract_gpu.py asks that every writing entry point of `_lib.SIGNATURES` was called under a guard in the
session.  `lr_cf_pair_state_f32`, `lr_cf_sumsq_f32`, `lr_cf_state_merge_f32` and `lr_cf_predict_topk_f32` are called under a
guard here, before that module runs."""
import inspect

import pytest

from tests import guarded_alloc as ga
from tests import test_rs_cf_gpu as cases

pytestmark = pytest.mark.gpu

FUNCTIONS = [cases.test_pair_state, cases.test_sumsq, cases.test_merge_and_refresh, cases.test_visible_pairs,
             cases.test_update_of_the_empty_state_and_empty_delta, cases.test_predict, cases.test_two_runs_give_the_same_bits,
             cases.test_argument_errors, cases.test_oversize_raises_before_allocating,
             cases.test_update_equals_a_fit_on_the_union]


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
def test_rs_cf_case_on_guarded_allocations(case, dev, monkeypatch):
    fn, kwargs, fill = case
    if "monkeypatch" in inspect.signature(fn).parameters:
        kwargs = dict(kwargs, monkeypatch=monkeypatch)
    with ga.guarded(fill) as g:
        fn(dev=dev, **kwargs)
        g.check()
        assert g.unguarded == 0, "device allocations that escaped the guard:\n" + "\n".join(g.unguarded_sites)
