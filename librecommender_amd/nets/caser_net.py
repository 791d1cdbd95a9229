"""Caser graph (`libreco/algorithms/caser.py:135-221`): the user vector is the row of `user_embeds_var` next to
relu(Dense(embed_size)) of the concatenated outputs of L horizontal convolutions (kernel sizes 1 .. L, ReLU, a max over time)
and one vertical convolution (over the L positions, per embedding channel, ReLU) of the rows of `seq_embeds_var` that the
behaviour window names; the classes are the rows of `item_embeds_var` [n_items, 2K] (+ `item_bias_var`).

All L + 1 convolutions and the pools are one forward launch of csrc/caser.hip that reads `seq_embeds_var` in place through the
window's ids (no [B, L, K] gather, no pre-pool activation in HBM), and one backward call that writes the convolution gradients
straight into the flat gradient buffer of `DenseParams` (the convolution parameters are its first tensors: `conv_params` is a
slice of `P.flat`) and returns the input gradient as one (id, gradient) stream.  There is no sequence mask: pad positions
carry the pad row (id == n_items), take part in every convolution and in the pools, and the pad row is trained.  The Dense
layer is `torch.addmm` + relu on `DenseParams`.  The pointwise losses are `ops.mf_score` with the [B, 2K] user block as X;
`norm_embed` is composed from torch ops.  The tables, the pointwise losses and the tables' Adam step are
`nets/seq_tower.py`'s.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .. import ops
from ..layers import DenseParams
from ..layers.row_adam import RowAdam
from ..utils.device import to_device
from .seq_tower import SeqTowerNet

LOSSES = ("mse", "cross_entropy", "focal")
UNSUPPORTED = ("Caser supports a window (`recent_num`) from 1 to 64, an `embed_size` from 1 to 128 and `nh_filters` and "
               "`nv_filters` from 1 to 64 (the convolution kernels' limit), got {}, {}, {}, {}")


def conv_param_names(max_seq_len):
    """[(kernel name, bias name)] of the horizontal layers of kernel sizes 1 .. L and of the vertical layer, in graph order
    (Keras' default layer names)."""
    return [(f"conv1d{'' if i == 0 else f'_{i}'}/kernel", f"conv1d{'' if i == 0 else f'_{i}'}/bias") for i in range(max_seq_len + 1)]


class CaserNet(SeqTowerNet):
    bias_l2 = False          # the reference regularises item_embeds_var but not item_bias_var (caser.py:162-175)

    def __init__(self, n_users, n_items, embed_size=16, nh_filters=2, nv_filters=4, norm_embed=False, max_seq_len=10, lr=1e-3,
                 epsilon=1e-5, seed=42, device=None, dense_adam=False, loss="cross_entropy", reg=None):
        if loss not in LOSSES:
            raise ValueError(f"loss must be one of {LOSSES}")
        self.device = device or torch.device("cuda")
        self.n_users, self.n_items, self.K, self.L = int(n_users), int(n_items), int(embed_size), int(max_seq_len)
        self.nh, self.nv = int(nh_filters), int(nv_filters)
        self.loss, self.norm_embed, self.lr, self.epsilon = loss, norm_embed, lr, epsilon
        if not ops.caser_supported(self.L, self.K, self.nh, self.nv):
            raise ValueError(UNSUPPORTED.format(self.L, self.K, self.nh, self.nv))
        # tf.keras.regularizers.l2(reg) on the three embedding variables (not on item_bias_var) adds 2 * reg * w to EVERY row's
        # gradient each step: representable only with the dense TF1 update (layers/row_adam.py)
        self.adam = RowAdam(self.device, dense_adam, reg)
        self.P = DenseParams(self.device, seed)
        for i, (kn, bn) in enumerate(conv_param_names(self.L), 1):
            vertical = i == self.L + 1
            self.P.add(kn, (1, self.L, self.nv) if vertical else (i, self.K, self.nh), "glorot_uniform")
            self.P.add(bn, (self.nv if vertical else self.nh,), "zeros")
        self.width = self.L * self.nh + self.K * self.nv
        self.P.add("dense/kernel", (self.width, self.K), "glorot_uniform")
        self.P.add("dense/bias", (self.K,), "zeros")
        self.P.finalize()
        n_conv = ops.caser_param_floats(self.L, self.K, self.nh, self.nv)
        self.conv_params, self.conv_grad = self.P.flat[:n_conv], self.P.grad[:n_conv]
        assert self.P["dense/kernel"].data_ptr() == self.P.flat.data_ptr() + 4 * n_conv, "DenseParams / lr_caser layout"
        self._init_tables({"user_embeds_var": (self.n_users + 1, self.K), "seq_embeds_var": (self.n_items + 1, self.K),
                           "item_embeds_var": (self.n_items, 2 * self.K)}, seed)

    # ---- user side ------------------------------------------------------------------------------
    def _convs(self, ids, need_arg=True):
        return ops.caser_fwd(self.vars["seq_embeds_var"], ids, self.conv_params, self.nh, self.nv, need_arg)

    def _user_block(self, urow, feat):
        return torch.cat([urow, torch.relu(torch.addmm(self.P["dense/bias"], feat, self.P["dense/kernel"]))], dim=1)

    @torch.no_grad()
    def embed_users(self, users, seqs):
        """[B, 2K]: concat(user row, relu(Dense(convolution features))), l2-normalised if `norm_embed`."""
        feat, _ = self._convs(self._i32(seqs), need_arg=False)
        u = self._user_block(self.vars["user_embeds_var"][self._i32(users).long()], feat)
        return F.normalize(u, dim=1, eps=1e-12) if self.norm_embed else u

    # ---- one step ---------------------------------------------------------------------------------
    def train_step(self, users, seqs, items, labels):
        self.step += 1
        V, M, S = self.vars, self.m, self.v
        us, ids, it = self._i32(users), self._i32(seqs), self._i32(items)
        y = to_device(labels, self.device).to(torch.float32).contiguous()
        B, L = ids.shape
        self.P.zero_grad()
        feat, arg = self._convs(ids)
        urow = V["user_embeds_var"][us.long()].requires_grad_(True)
        feat.requires_grad_(True)
        loss, gq, gb = self._pointwise(self._user_block(urow, feat), it, y)
        with torch.no_grad():
            gx, _ = ops.caser_bwd(V["seq_embeds_var"], ids, self.conv_params, self.nh, self.nv, feat.detach(), arg,
                                  feat.grad.contiguous(), gparams=self.conv_grad)
            hp = ops.adam_hp(self.lr, self.step, eps=self.epsilon, tf_style=True)
            seg_u = self.adam.segments("user", us, self.n_users + 1)
            self.adam.update(hp, seg_u, V["user_embeds_var"], M["user_embeds_var"], S["user_embeds_var"], urow.grad.contiguous())
            inside = (ids >= 0) & (ids <= self.n_items)
            sid = torch.where(inside, ids, torch.full_like(ids, -1)).reshape(-1).contiguous()
            self._update_seq_and_items(hp, sid, gx.reshape(B * L, -1), it, gq, gb)
            self.P.adam_step(hp)
        return loss
