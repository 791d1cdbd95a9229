"""The kernel-level cases of tests/test_word2vec_gpu.py (walks, keep flags, pairs, targets, one window at every row-group
class, the two-run comparison), run again on poisoned, guarded device allocations (tests/guarded_alloc.py), every case under
both fills.

A case asserts the existing function's own assertions, that every guard zone is intact afterwards and that no device
allocation of the package escaped the guard, as `run_guarded` of tests/test_memory_contract_gpu.py does.

This module's name matters: pytest collects tests/ in name order, and the coverage condition at the end of
tests/test_memory_contract_gpu.py asks that every writing entry point of `_lib.SIGNATURES` was called under a guard in the
session.  The seven writing `lr_w2v_*` entry points are called under a guard here, before that module runs."""
import pytest

from tests import guarded_alloc as ga
from tests import test_word2vec_gpu as cases

pytestmark = pytest.mark.gpu

FUNCTIONS = [cases.test_walks, cases.test_keep_flags, cases.test_pairs, cases.test_targets, cases.test_one_window,
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
def test_word2vec_case_on_guarded_allocations(case, dev):
    fn, kwargs, fill = case
    with ga.guarded(fill) as g:
        fn(dev=dev, **kwargs)
        g.check()
        assert g.unguarded == 0, "device allocations that escaped the guard:\n" + "\n".join(g.unguarded_sites)
