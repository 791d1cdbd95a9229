from .evaluate import evaluate, print_metrics

# The default of `evaluate(..., on_device=None)` / `print_metrics(..., on_device=None)`: False computes the metrics on the host
# (sklearn / numpy), True with the kernels of csrc/eval_metrics.hip.  `fit(..., eval_data=...)` follows it.
ON_DEVICE = False


def set_device_metrics(flag: bool) -> bool:
    """Set the module default `ON_DEVICE`; returns the previous value."""
    global ON_DEVICE
    prev, ON_DEVICE = ON_DEVICE, bool(flag)
    return prev


__all__ = ["evaluate", "print_metrics", "ON_DEVICE", "set_device_metrics"]
