"""Initial tables drawn on the host with numpy (`libreco/utils/initializers.py`): the same generator calls in the same
order as the reference, so a seed gives the reference's tables bit for bit."""
import numpy as np


def truncated_normal(np_rng: np.random.Generator, shape, mean=0.0, scale=0.05, tolerance=5):
    """Normal(mean, scale) draws in float32; entries outside mean +- 2 scale are drawn again, at most `tolerance` rounds
    (whatever is still outside after that stays)."""
    shape = list(shape)
    n = int(shape[0]) if len(shape) == 1 else int(shape[0]) * int(shape[1])
    out = np_rng.normal(mean, scale, n).astype(np.float32)
    lo, hi = mean - 2 * scale, mean + 2 * scale
    for _ in range(tolerance):
        bad = (out > hi) | (out < lo)
        k = int(np.count_nonzero(bad))
        if k == 0:
            break
        out[bad] = np_rng.normal(mean, scale, k)
    return out.reshape(*shape)
