"""FTRL-proximal for the wide side of Wide & Deep (`tf.train.FtrlOptimizer(lr, l1_regularization_strength=1e-3)`,
`training/tf_trainer.py:297-302`): the slots of a parameter and which of the two kernels of csrc/ftrl.hip it gets.

  * `dense=False`: a scalar-row table moves on the rows a stream touches (`ops.ftrl_rows`: TF's SparseApplyFtrl on the
    de-duplicated IndexedSlices), every other row and its slots stay as they are;
  * `dense=True`: every row moves every step with the gradient `scatter(stream) + l2_grad * w` (`ops.ftrl_dense`: TF's
    ApplyFtrl), the only form that carries a regulariser on the variable — the reason `reg` selects `dense_adam` in `RowAdam`;
  * `update_flat`: parameters with a dense gradient every step (the `wide_term` layer, `dense_linear_var`).

Slots are TF's: accumulator 0.1, linear 0 (`init_slots`).  An accumulator of 0 on an untouched row would make the quadratic
term of its first update sqrt(g*g)/lr alone — and 0/0 under a zero gradient."""
from __future__ import annotations

import torch

from .. import ops


class RowFtrl:
    def __init__(self, dense: bool = False, l2_grad: float = 0.0, l1: float = 1e-3, l2: float = 0.0):
        self.dense, self.l2_grad, self.l1, self.l2 = bool(dense), float(l2_grad or 0.0), float(l1), float(l2)
        if self.l2_grad and not self.dense:
            raise ValueError("a regulariser on the variable reaches every row each step: use the dense form with it")

    @staticmethod
    def init_slots(accum: torch.Tensor, linear: torch.Tensor) -> None:
        """TF's slot initialisation, in place."""
        accum.fill_(ops.FTRL_INIT_ACCUM)
        linear.zero_()

    def update(self, lr, seg, var, accum, linear, grad) -> None:
        """One step of the scalar-row table `var` [V, 1] from the per-position gradients `grad` [seg.n, 1]."""
        if not self.dense:
            ops.ftrl_rows(var, accum, linear, grad, seg, lr, self.l1, self.l2)
            return
        gd = torch.zeros_like(var)                       # the run sums scattered onto their rows, in the segments' fixed order
        ops.embed_scatter_add(gd.view(-1, 1), grad.view(-1, 1), seg, 1.0)
        ops.ftrl_dense(var, accum, linear, gd, lr, self.l1, self.l2, l2_grad_coef=2.0 * self.l2_grad)

    def update_flat(self, lr, var, accum, linear, grad) -> None:
        """One step of a flat range of parameters from their dense gradient."""
        ops.ftrl_dense(var, accum, linear, grad, lr, self.l1, self.l2)
