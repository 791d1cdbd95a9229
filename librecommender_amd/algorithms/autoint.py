"""`AutoInt` (`libreco/algorithms/autoint.py`, Song et al., "AutoInt: Automatic Feature Interaction Learning via
Self-Attentive Neural Networks"): the reference's constructor and checks over `FeatBase`'s `fit / predict / recommend_user /
save / load / rebuild_model`.  The interaction stack and the read-out run on csrc/autoint.hip (one forward launch, one backward
call, `nets/autoint_net.py`); full-catalogue scoring is the chunked forward in its inference mode.

Deliberate differences from the reference:
  (a) the attention is the Keras `MultiHeadAttention(use_bias=False)` branch of `layers/attention.py:67-101`; its TF1 branch is
      not provided;
  (b) `use_bn` and `dropout_rate` are accepted, stored and, as in the reference's graph, never used;
  (c) the default optimiser is TF1-style Adam on the rows a batch touches; `dense_adam=True` is the reference's TF1 semantics,
      and `reg` selects it;
  (d) more fields, a wider embedding or wider heads than the kernels take (`ops.autoint_supported`: 64 each, 8 heads, 8 layers)
      run the same net composed from torch ops (`net.fused` is False);
  (e) `tf_sess_config` is accepted and ignored; under a process group of more than one rank `fit` raises; `save_tf_variables` /
      `load_tf_variables` do not know this model's variables.
"""
from __future__ import annotations

import numpy as np

from ..bases.base import hip_device
from ..nets.autoint_net import FeatAutoIntNet
from .fm import _FMCommon


def attention_config(att_embed_size):
    """`tfops/configs.py:6-17`: nothing -> (8, 8, 8), an int -> one layer, a list or tuple -> one layer per entry."""
    if not att_embed_size:
        return (8, 8, 8)
    if isinstance(att_embed_size, (int, np.integer)) and not isinstance(att_embed_size, bool):
        return (int(att_embed_size),)
    if isinstance(att_embed_size, (list, tuple)):
        if not all(isinstance(h, (int, np.integer)) and not isinstance(h, bool) and h >= 1 for h in att_embed_size):
            raise ValueError(f"every entry of `att_embed_size` must be a positive int, got {att_embed_size}")
        return tuple(int(h) for h in att_embed_size)
    raise ValueError("att_embed_size must be int or list")


class AutoInt(_FMCommon):
    def __init__(self, task, data_info, loss_type="cross_entropy", embed_size=16, n_epochs=10, lr=0.001, lr_decay=False,
                 epsilon=1e-5, reg=None, batch_size=256, sampler="random", num_neg=1, use_bn=True, dropout_rate=None,
                 att_embed_size=(8, 8, 8), num_heads=2, use_residual=True, multi_sparse_combiner="sqrtn", seed=42,
                 lower_upper_bound=None, tf_sess_config=None, device="cuda", dense_adam=False):
        super().__init__(task, data_info, lower_upper_bound)
        self.all_args = locals()
        self._common(data_info, loss_type, embed_size, n_epochs, lr, lr_decay, epsilon, reg, batch_size, sampler, num_neg,
                     use_bn, dropout_rate, multi_sparse_combiner, seed, device, dense_adam)    # use_bn, dropout_rate: stored, unused
        self.att_head_dims = attention_config(att_embed_size)
        self.att_layer_num = len(self.att_head_dims)
        if not isinstance(num_heads, (int, np.integer)) or isinstance(num_heads, bool) or num_heads < 1:
            raise ValueError(f"`num_heads` must be a positive integer, got {num_heads}")
        self.num_heads, self.use_residual = int(num_heads), use_residual

    def build_model(self):
        self.device = hip_device(self._device_arg)
        self.net = FeatAutoIntNet(self._spec(), self.embed_size, self.att_head_dims, self.num_heads, self.use_residual, self.lr,
                                  self.epsilon, self.seed, self.device, self.dense_adam, self.reg)
