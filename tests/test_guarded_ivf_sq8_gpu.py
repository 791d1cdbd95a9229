"""The kernel-level cases of tests/test_ivf_sq8_gpu.py (encoding, the code scan with its filter, fill and zero-scale cases, the
full refine against the Flat scan, the re-rank alone, same bits on two runs, the off-grid bound and the unsupported shapes), run
again on poisoned, guarded device allocations (tests/guarded_alloc.py), every case under both fills.

A case asserts the existing function's own assertions, that every guard zone is intact afterwards and that no device
allocation of the package escaped the guard, as tests/test_guarded_ivf_gpu.py does.  Codes, scales, candidate lists, partial
keys and outputs are `empty` tensors of the package: they arrive filled with 0xFF or 0x5A, so a code-row padding byte, a
candidate slot or an output entry a kernel left unwritten would fail the comparison with the oracle here.

This module's name matters: pytest collects tests/ in name order, and the coverage condition at the end of
tests/test_memory_contract_gpu.py asks that every writing entry point of `_lib.SIGNATURES` was called under a guard in the
session.  `lr_ivf_sq8_encode_f32`, `lr_ivf_sq8_search_f32` and `lr_ivf_rerank_f32` are called under a guard here, before that
module runs (`lr_ivf_sq8_supported` and `lr_ivf_sq8_search_ws_bytes` write nothing)."""
import pytest

from tests import guarded_alloc as ga
from tests import ivf_sq8_oracle as Q
from tests import test_ivf_sq8_gpu as cases

pytestmark = pytest.mark.gpu

FUNCTIONS = [cases.test_encode, cases.test_encode_hand_made_rows, cases.test_search,
             cases.test_search_consumed_list_empties_a_probed_list, cases.test_search_a_list_of_all_zero_rows,
             cases.test_full_refine_equals_flat, cases.test_rerank, cases.test_two_runs_give_the_same_bits,
             cases.test_off_grid_within_the_bound, cases.test_unsupported_shapes_raise_and_write_nothing]


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
def test_ivf_sq8_case_on_guarded_allocations(case, dev):
    fn, kwargs, fill = case
    if fn is cases.test_off_grid_within_the_bound:
        kwargs = dict(kwargs, off_grid=Q.off_grid_case())      # the fixture's value
    with ga.guarded(fill) as g:
        fn(dev=dev, **kwargs)
        g.check()
        assert g.unguarded == 0, "device allocations that escaped the guard:\n" + "\n".join(g.unguarded_sites)
