"""The kernel and model cases of tests/test_seq_attn_gpu.py (every shape class, saturated scores, a row with nothing allowed,
the inference form, and the training steps of the three nets), run again on poisoned, guarded device allocations
(tests/guarded_alloc.py), every case under both fills.

A case asserts the existing function's own assertions, that every guard zone is intact afterwards and that no device
allocation of the package escaped the guard, as `run_guarded` of tests/test_memory_contract_gpu.py does.

This module's name matters: pytest collects tests/ in name order, and the coverage condition at the end of
tests/test_memory_contract_gpu.py asks that every writing entry point of `_lib.SIGNATURES` was called under a guard in the
session.  `lr_seq_attn_fwd_f32` (with and without `saved`) and `lr_seq_attn_bwd_f32` are called under a guard here, before
that module runs."""
import pytest

from tests import guarded_alloc as ga
from tests import test_seq_attn_gpu as cases
from tests.seq_attn_oracle import sid

pytestmark = pytest.mark.gpu

FUNCTIONS = [cases.test_kernel_case, cases.test_saturated_scores, cases.test_row_with_nothing_allowed,
             cases.test_inference_form_writes_the_same_output, cases.test_training_steps]


def _build():
    out, ids = [], []
    for fn in FUNCTIONS:
        for kw in ga.expand(fn):
            for fill in ga.FILLS:
                out.append((fn, kw, fill))
                cid = ",".join(f"{k}={cases._case_id(v) if k == 'case' else sid(v)}" for k, v in kw.items())
                ids.append(f"{fn.__name__[5:]}[{cid}]-{fill:02X}")
    assert len(set(ids)) == len(ids)
    return out, ids


CASES, IDS = _build()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_seq_attn_case_on_guarded_allocations(case, dev):
    fn, kwargs, fill = case
    with ga.guarded(fill) as g:
        fn(dev=dev, **kwargs)
        g.check()
        assert g.unguarded == 0, "device allocations that escaped the guard:\n" + "\n".join(g.unguarded_sites)
