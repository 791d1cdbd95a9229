"""RNN4Rec graph (`libreco/algorithms/rnn4rec.py:151-237`): the user vector is Dense(embed_size) of the last state of a GRU /
LSTM stack over the rows of `seq_embeds_var` that the behaviour window names; the classes are the rows of `item_embeds_var`
(+ `item_bias_var`).

The first recurrent layer reads `seq_embeds_var` in place through the window's ids (csrc/rnn.hip, no [B, L, D] gather) and
its input gradient goes back to the table as one (id, gradient) stream, masked positions dropped with id -1.  The pointwise
losses are `ops.mf_score` with the user-vector block as X; `bpr` and `norm_embed` are composed from torch ops on the gathered
rows.  Variables and their TF1 Adam moments are `NamedTables`; recurrent, layer-norm and Dense parameters are `DenseParams`;
the tables, the pointwise losses and the tables' Adam step are `nets/seq_tower.py`'s.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .. import ops
from ..layers import DenseParams
from ..layers.recurrent import RnnStack
from ..layers.row_adam import RowAdam
from ..utils.device import to_device
from .seq_tower import SeqTowerNet

LOSSES = ("mse", "cross_entropy", "focal", "bpr")


class RNN4RecNet(SeqTowerNet):
    def __init__(self, n_items, embed_size=16, hidden_units=(16,), rnn_type="gru", use_layer_norm=False, dropout_rate=0.0,
                 norm_embed=False, max_seq_len=10, lr=1e-3, epsilon=1e-5, seed=42, device=None, dense_adam=False,
                 loss="cross_entropy", reg=None):
        if loss not in LOSSES:
            raise ValueError(f"loss must be one of {LOSSES}")
        self.device = device or torch.device("cuda")
        self.n_items, self.K, self.L = int(n_items), int(embed_size), int(max_seq_len)
        self.loss, self.norm_embed, self.lr, self.epsilon = loss, norm_embed, lr, epsilon
        # tf.keras.regularizers.l2(reg) on the three embedding variables adds 2 * reg * w to EVERY row's gradient each step
        # (tfops/configs.py:20-26): representable only with the dense TF1 update (layers/row_adam.py)
        self.adam = RowAdam(self.device, dense_adam, reg)
        self.P = DenseParams(self.device, seed)
        self.rnn = RnnStack(self.P, rnn_type, hidden_units[0], hidden_units, use_layer_norm, dropout_rate)
        self.P.add("dense/kernel", (self.rnn.n_out, self.K), "glorot_uniform")
        self.P.add("dense/bias", (self.K,), "zeros")
        self.P.finalize()
        self._init_tables({"seq_embeds_var": (self.n_items + 1, int(hidden_units[0])), "item_embeds_var": (self.n_items, self.K)},
                          seed)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(seed + 2)

    # ---- user side ------------------------------------------------------------------------------
    def _user(self, ids, lens, masks=None):
        """-> (Dense(last state) [B, K], the first layer's io)."""
        last, io = self.rnn(lens, table=self.vars["seq_embeds_var"], ids=ids, masks=masks)
        return torch.addmm(self.P["dense/bias"], last, self.P["dense/kernel"]), io

    @torch.no_grad()
    def embed_users(self, seqs, lens):
        u, _ = self._user(self._i32(seqs), self._i32(lens))
        return F.normalize(u, dim=1, eps=1e-12) if self.norm_embed else u

    # ---- losses ---------------------------------------------------------------------------------
    def _bpr_torch(self, u, pos, neg):
        """`rnn4rec.py:169-195`: -mean log sigmoid(b_p - b_n + <u, q_p - q_n>).  With `norm_embed` the reference normalises
        the item rows but takes the RAW user vector in the difference (rnn4rec.py:191 reads `self.user_embeds`)."""
        both = torch.cat([pos, neg])
        q, b = self._item_leaves(both)
        B = pos.numel()
        qn = F.normalize(q, dim=1, eps=1e-12) if self.norm_embed else q
        diff = b[:B] - b[B:] + (u * (qn[:B] - qn[B:])).sum(1)
        loss = -F.logsigmoid(diff).mean()
        loss.backward()
        return loss.detach(), both, q.grad, b.grad

    # ---- one step ---------------------------------------------------------------------------------
    def train_step(self, seqs, lens, items=None, labels=None, pos=None, neg=None, masks=None):
        """One step on a pointwise batch (`items`, `labels`) or, for `bpr`, on (`pos`, `neg`) pairs; `masks`: the dropout
        masks of `RnnStack.draw_masks` (drawn here when the net has a dropout rate)."""
        self.step += 1
        ids, ln = self._i32(seqs), self._i32(lens)
        B, L = ids.shape
        if masks is None and self.rnn.dropout_rate > 0:
            masks = self.rnn.draw_masks(B, self.gen)
        self.P.zero_grad()
        u, io = self._user(ids, ln, masks)
        if self.loss == "bpr":
            loss, it, gq, gb = self._bpr_torch(u, self._i32(pos), self._i32(neg))
        else:
            it = self._i32(items)
            loss, gq, gb = self._pointwise(u, it, to_device(labels, self.device).to(torch.float32).contiguous())
        with torch.no_grad():
            hp = ops.adam_hp(self.lr, self.step, eps=self.epsilon, tf_style=True)
            t = torch.arange(L, dtype=torch.int32, device=self.device)
            sid = torch.where(t[None, :] < ln.clamp(0, L)[:, None], ids, torch.full_like(ids, -1)).reshape(-1).contiguous()
            self._update_seq_and_items(hp, sid, io.gx.reshape(B * L, -1), it, gq, gb)
            self.P.adam_step(hp)
        return loss
