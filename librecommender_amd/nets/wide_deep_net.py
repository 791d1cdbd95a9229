"""Wide & Deep graph (`libreco/algorithms/wide_deep.py:151-178`) over the general feature embedding layer: the field matrix
E [B, F', K] is the deep input and the linear weights LIN [B, F'] the wide input ([user, item, plain sparse columns, pooled
multi-sparse fields, dense columns] under every combiner),

    logit = Dense(1, "wide_term")(LIN) + Dense(1, "deep_term")(dense_nn(E.flatten(1))).

Two optimisers per step (`training/tf_trainer.py:275-311`, `WideDeepTrainer`):
  * Adam at lr["deep"] on the K-wide table (row-wise, or TF1's dense form under `dense_adam` / `reg`, as in `FeatDeepFMNet`),
    `dense_embeds_var`, the MLP with its BatchNorms and `deep_term`;
  * FTRL-proximal at lr["wide"] with l1 = 1e-3 (csrc/ftrl.hip, `layers/ftrl.py`) on the `lin` table — `ops.ftrl_rows` on the
    segments the deep update builds; under `reg` every row gets the gradient 2 reg w and the dense form runs — and on
    `dense_linear_var` and the `wide_term` kernel and bias (`ops.ftrl_dense`).  Adam does not touch them: the wide parameters
    are one contiguous range of the flat buffer of `DenseParams` (`wide_span`) that `adam_step(skip=)` leaves out.

Where the FTRL slots live: the table's accumulator in `tables.lin_m` and its linear slot in `tables.lin_v`, those of the flat
wide range in the same range of `P.m` / `P.v`; accumulators start at 0.1 (TF's `initial_accumulator_value`).  The arrays
`opt::lin_m / opt::lin_v / opt::dense_m / opt::dense_v` of `FeatBase` therefore carry them through `save` and `rebuild_model`
unchanged, and rows a rebuilt model appends keep the 0.1 they were built with.

`reg` is the reference's l2 regulariser on the embedding variables, `dense_wide_var` and `dense_deep_var` included (their
gradients take 2 reg w here); the Dense layers have none.
"""
from __future__ import annotations

import torch

from ..layers import DenseStack, TFDense
from ..layers.ftrl import RowFtrl
from .feat_nets import _FeatNet
from .fm_nets import _FieldNet

DEFAULT_LR = {"wide": 0.01, "deep": 1e-4}


class WideDeepNet(_FeatNet):
    with_linear = True

    def __init__(self, spec, embed_size=16, hidden_units=(128, 64, 32), use_bn=True, dropout_rate=0.0, lr=None, epsilon=1e-5,
                 seed=42, device=None, dense_adam=False, reg=None, l1=1e-3):
        super().__init__(spec, embed_size, dict(lr or DEFAULT_LR), epsilon, seed, device, dense_adam, reg)
        P, F_ = self.P, spec.n_fields
        self.wide_term = TFDense(P, "wide_term", F_, 1)                   # directly behind `embedding/dense_linear_var`
        self.mlp = DenseStack(P, "deep", F_ * embed_size, hidden_units, use_bn, dropout_rate)
        self.deep_term = TFDense(P, "deep_term", self.mlp.n_out, 1)
        P.finalize()
        self.wide_span = P.span("embedding/dense_linear_var" if spec.n_dense_cols else self.wide_term.w, self.wide_term.b)
        self.ftrl = RowFtrl(dense=bool(self.reg), l2_grad=self.reg, l1=l1)
        t, (a, b) = self.tables, self.wide_span
        RowFtrl.init_slots(t.lin_m, t.lin_v)
        RowFtrl.init_slots(P.m[a:b], P.v[a:b])

    def _hp(self):
        from .. import ops

        return ops.adam_hp(self.lr["deep"], self.step, eps=self.epsilon, tf_style=True)

    def _logits(self, E, LIN, training):
        return (self.wide_term(LIN) + self.deep_term(self.mlp(E.flatten(1), training))).squeeze(1)

    @torch.no_grad()
    def forward(self, users, items, sparse=None, dense=None, **_):
        _, E, LIN = self.emb.forward(users, items, sparse, dense, grad=False)
        return self._logits(E, LIN, False)

    def _wide_rows(self, seg, gl):
        t = self.tables
        self.ftrl.update(self.lr["wide"], seg, t.lin, t.lin_m, t.lin_v, gl)

    def train_step(self, users, items, labels, sparse=None, dense=None, loss_type="cross_entropy", **_):
        self.step += 1
        P = self.P
        ctx, E, LIN = self.emb.forward(users, items, sparse, dense)
        P.zero_grad()
        loss = _FieldNet.loss_fn(self._logits(E, LIN, True), self._labels(labels), loss_type)
        loss.backward()
        with torch.no_grad():
            if self.reg and self.spec.n_dense_cols:
                for name in ("embedding/dense_embeds_var", "embedding/dense_linear_var"):
                    P[name].grad.add_(P[name], alpha=2.0 * self.reg)
            hp = self._hp()
            self.emb.apply_gradients(ctx, hp, self.dense_adam, self.reg, lin_update=self._wide_rows)
            P.adam_step(hp, skip=self.wide_span)
            a, b = self.wide_span
            self.ftrl.update_flat(self.lr["wide"], P.flat[a:b], P.m[a:b], P.v[a:b], P.grad[a:b])
        return loss.detach()
