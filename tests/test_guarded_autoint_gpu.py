"""The kernel and step cases of tests/test_autoint_gpu.py (the stack in both batch classes, a single field, saturated scores,
the inference mode without acts, and the training steps), run again on poisoned, guarded device allocations
(tests/guarded_alloc.py), every case under both fills.

A case asserts the existing function's own assertions, that every guard zone is intact afterwards and that no device
allocation of the package escaped the guard, as `run_guarded` of tests/test_memory_contract_gpu.py does.

This module's name matters: pytest collects tests/ in name order, and the coverage condition at the end of
tests/test_memory_contract_gpu.py asks that every writing entry point of `_lib.SIGNATURES` was called under a guard in the
session.  `lr_autoint_fwd_f32` (with and without acts) and `lr_autoint_bwd_f32` are called under a guard here, before that
module runs."""
import inspect

import pytest

from tests import guarded_alloc as ga
from tests import test_autoint_gpu as cases
from tests.autoint_oracle import sid
from tests.test_autoint_gpu import feat_data  # noqa: F401  (the fixture the training steps take)

pytestmark = pytest.mark.gpu

FUNCTIONS = [cases.test_stack, cases.test_stack_wide_batches, cases.test_softmax_of_one_field, cases.test_saturated_softmax,
             cases.test_inference_mode_and_batch_independence, cases.test_training_steps]


def _build():
    out, ids = [], []
    for fn in FUNCTIONS:
        for kw in ga.expand(fn):
            for fill in ga.FILLS:
                out.append((fn, kw, fill))
                cid = ",".join(f"{k}={cases._cfg_id(v) if k == 'cfg' else sid(v)}" for k, v in kw.items())
                ids.append(f"{fn.__name__[5:]}[{cid}]-{fill:02X}")
    assert len(set(ids)) == len(ids)
    return out, ids


CASES, IDS = _build()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_autoint_case_on_guarded_allocations(case, dev, feat_data):  # noqa: F811
    fn, kwargs, fill = case
    if "feat_data" in inspect.signature(fn).parameters:
        kwargs = dict(kwargs, feat_data=feat_data)
    with ga.guarded(fill) as g:
        fn(dev=dev, **kwargs)
        g.check()
        assert g.unguarded == 0, "device allocations that escaped the guard:\n" + "\n".join(g.unguarded_sites)
