"""WaveNet graph (`libreco/algorithms/wave_net.py:139-222`, the TF2 branch): the user vector is the row of
`user_embeds_var` next to Dense(embed_size) of the max pool of a dilated causal convolution stack over the rows of
`seq_embeds_var` that the behaviour window names; the classes are the rows of `item_embeds_var` [n_items, 2K]
(+ `item_bias_var`).

The stack, the 1x1 layer and the pool are one forward launch of csrc/wavenet.hip that reads `seq_embeds_var` in place through
the window's ids (no [B, L, K] gather), and one backward call that writes the convolution gradients straight into the flat
gradient buffer of `DenseParams` (the convolution parameters are its first tensors: `conv_params` is a slice of `P.flat`) and
returns the input gradient as one (id, gradient) stream.  There is no sequence mask: pad positions carry the pad row
(id == n_items), take part in every layer and in the pool, and the pad row is trained.  The pointwise losses are
`ops.mf_score` with the [B, 2K] user block as X; `norm_embed` is composed from torch ops.  Variables and their TF1 Adam
moments are `NamedTables`; convolution and Dense parameters are `DenseParams`; the tables, the pointwise losses and the
tables' Adam step are `nets/seq_tower.py`'s.
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


def conv_param_names(n_blocks, n_layers_per_block):
    """[(kernel name, bias name)] of the dilated layers and the 1x1 layer, in graph order (Keras' default layer names)."""
    n = n_blocks * n_layers_per_block + 1
    return [(f"conv1d{'' if i == 0 else f'_{i}'}/kernel", f"conv1d{'' if i == 0 else f'_{i}'}/bias") for i in range(n)]


class WaveNetNet(SeqTowerNet):
    bias_l2 = False          # the reference regularises item_embeds_var but not item_bias_var (wave_net.py:169-179)

    def __init__(self, n_users, n_items, embed_size=16, n_filters=16, n_blocks=1, n_layers_per_block=4, norm_embed=False,
                 max_seq_len=10, lr=1e-3, epsilon=1e-5, seed=42, device=None, dense_adam=False, loss="cross_entropy", reg=None):
        if loss not in LOSSES:
            raise ValueError(f"loss must be one of {LOSSES}")
        self.device = device or torch.device("cuda")
        self.n_users, self.n_items, self.K, self.L = int(n_users), int(n_items), int(embed_size), int(max_seq_len)
        self.F, self.n_blocks, self.n_per_block = int(n_filters), int(n_blocks), int(n_layers_per_block)
        self.loss, self.norm_embed, self.lr, self.epsilon = loss, norm_embed, lr, epsilon
        if not ops.wavenet_supported(self.L, self.K, self.F, self.n_blocks, self.n_per_block):
            raise ValueError(f"WaveNet supports a window, `embed_size` and `n_filters` from 1 to 128 and at most 16 dilated "
                             f"layers (the kernels' limit), got {self.L}, {self.K}, {self.F}, {self.n_blocks} x {self.n_per_block}")
        # tf.keras.regularizers.l2(reg) on the three embedding variables (not on item_bias_var) adds 2 * reg * w to EVERY row's
        # gradient each step: representable only with the dense TF1 update (layers/row_adam.py)
        self.adam = RowAdam(self.device, dense_adam, reg)
        self.P = DenseParams(self.device, seed)
        names = conv_param_names(self.n_blocks, self.n_per_block)
        for i, (kn, bn) in enumerate(names):
            last = i == len(names) - 1
            self.P.add(kn, (1 if last else 2, self.K if i == 0 else self.F, self.F), "glorot_uniform")
            self.P.add(bn, (self.F,), "zeros")
        self.P.add("dense/kernel", (self.F, self.K), "glorot_uniform")
        self.P.add("dense/bias", (self.K,), "zeros")
        self.P.finalize()
        n_conv = ops.wavenet_param_floats(self.K, self.F, self.n_blocks, self.n_per_block)
        self.conv_params, self.conv_grad = self.P.flat[:n_conv], self.P.grad[:n_conv]
        assert self.P["dense/kernel"].data_ptr() == self.P.flat.data_ptr() + 4 * n_conv, "DenseParams / lr_wavenet layout"
        self._init_tables({"user_embeds_var": (self.n_users + 1, self.K), "seq_embeds_var": (self.n_items + 1, self.K),
                           "item_embeds_var": (self.n_items, 2 * self.K)}, seed)

    # ---- user side ------------------------------------------------------------------------------
    def _stack(self, ids):
        return ops.wavenet_fwd(self.vars["seq_embeds_var"], ids, self.conv_params, self.F, self.n_blocks, self.n_per_block)

    @torch.no_grad()
    def embed_users(self, users, seqs):
        """[B, 2K]: concat(user row, Dense(pool)), l2-normalised if `norm_embed`."""
        _, pooled, _ = self._stack(self._i32(seqs))
        u = torch.cat([self.vars["user_embeds_var"][self._i32(users).long()],
                       torch.addmm(self.P["dense/bias"], pooled, self.P["dense/kernel"])], dim=1)
        return F.normalize(u, dim=1, eps=1e-12) if self.norm_embed else u

    # ---- one step ---------------------------------------------------------------------------------
    def train_step(self, users, seqs, items, labels):
        self.step += 1
        V, M, S = self.vars, self.m, self.v
        us, ids, it = self._i32(users), self._i32(seqs), self._i32(items)
        y = to_device(labels, self.device).to(torch.float32).contiguous()
        B, L = ids.shape
        self.P.zero_grad()
        acts, pooled, arg = self._stack(ids)
        urow = V["user_embeds_var"][us.long()].requires_grad_(True)
        pooled.requires_grad_(True)
        u = torch.cat([urow, torch.addmm(self.P["dense/bias"], pooled, self.P["dense/kernel"])], dim=1)
        loss, gq, gb = self._pointwise(u, it, y)
        with torch.no_grad():
            gx, _ = ops.wavenet_bwd(V["seq_embeds_var"], ids, self.conv_params, self.F, self.n_blocks, self.n_per_block,
                                    acts, arg, pooled.grad.contiguous(), gparams=self.conv_grad)
            hp = ops.adam_hp(self.lr, self.step, eps=self.epsilon, tf_style=True)
            seg_u = self.adam.segments("user", us, self.n_users + 1)
            self.adam.update(hp, seg_u, V["user_embeds_var"], M["user_embeds_var"], S["user_embeds_var"], urow.grad.contiguous())
            inside = (ids >= 0) & (ids <= self.n_items)
            sid = torch.where(inside, ids, torch.full_like(ids, -1)).reshape(-1).contiguous()
            self._update_seq_and_items(hp, sid, gx.reshape(B * L, -1), it, gq, gb)
            self.P.adam_step(hp)
        return loss
