"""What the id-window towers (`nets/rnn_nets.py`, `nets/wavenet_net.py`, `nets/caser_net.py`) share: row tables `seq_embeds_var` (pad row
`n_items`), `item_embeds_var` and `item_bias_var` as `NamedTables`, a `DenseParams` for everything else, the pointwise losses
against the item rows, and the TF1 Adam step of the tables from the window's and the batch's (id, gradient) streams.

A subclass builds `self.P`, `self.adam` and its attributes, calls `_init_tables`, and writes its own `train_step` around its
user side; the order of the `ops.*` calls within a step is the subclass's and is spelled out there.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .. import ops
from ..layers.embedding import glorot_uniform_
from ..layers.row_adam import NamedTables
from ..utils.device import to_device


class SeqTowerNet(NamedTables):
    bias_l2 = True           # whether a regulariser (dense Adam only) also decays `item_bias_var`

    def _init_tables(self, shapes, seed):
        """`shapes` {name: (rows, width)}, drawn in this order from one generator seeded with `seed`
        (tf.glorot_uniform_initializer), and a zero `item_bias_var` [n_items, 1]."""
        gen = torch.Generator(device=self.device)
        gen.manual_seed(seed)
        tables = {}
        for name, shape in shapes.items():
            tables[name] = torch.empty(shape, dtype=torch.float32, device=self.device)
            glorot_uniform_(tables[name], shape, gen)
        tables["item_bias_var"] = torch.zeros((self.n_items, 1), dtype=torch.float32, device=self.device)
        NamedTables.__init__(self, tables)

    def _i32(self, x):
        return to_device(x, self.device).to(torch.int32).contiguous()

    @torch.no_grad()
    def item_matrix(self):
        """[N, width] class rows (normalised if `norm_embed`) and [N] biases (dyn_embed_base.py:240-269)."""
        w = self.vars["item_embeds_var"]
        return (F.normalize(w, dim=1, eps=1e-12) if self.norm_embed else w), self.vars["item_bias_var"].view(-1)

    # ---- losses ---------------------------------------------------------------------------------
    def _item_leaves(self, items):
        w = self.vars["item_embeds_var"]
        q = ops.embed_gather(w, items.view(-1, 1)).view(-1, w.shape[1]).requires_grad_(True)
        b = self.vars["item_bias_var"].view(-1)[items.long()].requires_grad_(True)
        return q, b

    def _pointwise_torch(self, u, items, labels):
        """The pointwise losses with `norm_embed` (`rnn4rec.py:157-167`, `wave_net.py:145-152`): both sides l2-normalised."""
        q, b = self._item_leaves(items)
        s = (F.normalize(u, dim=1, eps=1e-12) * F.normalize(q, dim=1, eps=1e-12)).sum(1) + b
        if self.loss == "mse":
            loss = F.mse_loss(s, labels)
        else:
            bce = F.binary_cross_entropy_with_logits(s, labels, reduction="none")
            if self.loss == "focal":                                         # tfops/loss.py:56-62
                p = torch.sigmoid(s)
                bce = (labels * 0.25 + (1 - labels) * 0.75) * (1 - (labels * p + (1 - labels) * (1 - p))) ** 2.0 * bce
            loss = bce.mean()
        loss.backward()
        return loss.detach(), q.grad, b.grad

    def _pointwise(self, u, items, labels):
        """(loss, d loss / d item rows, d loss / d biases) of the user block `u` [B, width] against the batch's items, the
        gradient of `u` propagated: `ops.mf_score` with `u` as X, torch ops on the gathered rows under `norm_embed`."""
        if self.norm_embed:
            return self._pointwise_torch(u, items, labels)
        B, V = items.numel(), self.vars
        with torch.no_grad():
            slot = torch.arange(B, dtype=torch.int32, device=self.device)
            out = ops.mf_score(u.detach().contiguous(), V["item_embeds_var"], None, V["item_bias_var"].view(-1),
                               torch.zeros_like(slot), items, labels, self.loss, xidx=slot, mode="grad", gscale=1.0 / B)
            loss = out["loss"].sum() / B
        u.backward(out["gx"])
        return loss, out["gq"], out["g"]

    # ---- the tables' Adam step ------------------------------------------------------------------
    def _update_seq_and_items(self, hp, sid, gseq, items, gq, gb):
        """`seq_embeds_var` from the window's stream (`sid` [B * L], -1 = no row; `gseq` [B * L, width]), then
        `item_embeds_var` with its twin `item_bias_var` from the batch's items."""
        V, M, S = self.vars, self.m, self.v
        seg_s = self.adam.segments("seq", sid, self.n_items + 1)
        self.adam.update(hp, seg_s, V["seq_embeds_var"], M["seq_embeds_var"], S["seq_embeds_var"], gseq)
        seg_i = self.adam.segments("item", items, self.n_items)
        bias = (V["item_bias_var"], M["item_bias_var"], S["item_bias_var"], gb.contiguous())
        if self.bias_l2 or not (self.adam.dense and self.adam.l2):
            self.adam.update(hp, seg_i, V["item_embeds_var"], M["item_embeds_var"], S["item_embeds_var"], gq.contiguous(), lin=bias)
        else:       # the dense step of the twin as `RowAdam.update` makes it, without the l2 term
            self.adam.update(hp, seg_i, V["item_embeds_var"], M["item_embeds_var"], S["item_embeds_var"], gq.contiguous())
            ops.adam_dense(*bias[:3], hp, grows=ops.embed_segment_sum(bias[3].view(-1, 1), seg_i), seg=seg_i,
                           row_slot=self.adam.row_slot(bias[0]), l2=0.0)
