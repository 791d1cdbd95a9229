"""`Caser` (`libreco/algorithms/caser.py`): the sequence recommender of Tang & Wang built on horizontal and vertical
convolutions over the window's embedding rows, with the reference's constructor, checks, `fit / predict / recommend_user /
dyn_user_embedding` and checkpoints.  The L horizontal convolutions with their pools and the vertical convolution run on
csrc/caser.hip (one forward launch, one backward call, `nets/caser_net.py`), the exported embeddings are served by
`lr_score_topk_f32` like every `EmbedBase` model.  Dynamic inference (`recommend_user` with a `seq`, the window) is
`bases/dyn_embed_base.py`'s, the checkpoint arrays are its `SeqTowerCheckpoint`'s.

Deliberate differences from the reference:
  (a) there is no sequence mask, as in the reference: pad positions carry the pad row, take part in every convolution and
      pool, and the pad row is trained; a pool's gradient goes to the FIRST position that holds the maximum;
  (b) `use_bn` and `dropout_rate` are accepted, stored and, as in the reference's graph, never used: it builds neither a
      batch normalisation nor a dropout layer;
  (c) the default optimiser is TF1-style Adam on the rows a batch touches; `dense_adam=True` is the reference's TF1
      semantics, and `reg` needs it;
  (d) a window outside 1 to 64, an `embed_size` outside 1 to 128 or `nh_filters` / `nv_filters` outside 1 to 64 raise
      `ValueError` at `build_model` (`lr_caser_supported`);
  (e) `tf_sess_config` is accepted and ignored; `user_feats` is rejected (the model has no user features); under a process
      group of more than one rank `fit` raises;
  (f) the convolution shapes depend on the window: a checkpoint taken at another `recent_num` cannot be loaded.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from ..bases import DynEmbedBase
from ..bases.base import hip_device
from ..bases.dyn_embed_base import SeqTowerCheckpoint
from ..batch.sequence import get_recent_seqs
from ..layers.row_adam import REG_NEEDS_DENSE
from ..nets.caser_net import UNSUPPORTED, CaserNet
from ..utils.validate import check_seq_mode, dropout_config, reg_config


class Caser(SeqTowerCheckpoint, DynEmbedBase):
    uses_sequence = True
    takes_user_feats = False

    def __init__(self, task, data_info=None, loss_type="cross_entropy", embed_size=16, norm_embed=False, n_epochs=20, lr=0.001,
                 lr_decay=False, epsilon=1e-5, reg=None, batch_size=256, sampler="random", num_neg=1, use_bn=False,
                 dropout_rate=None, nh_filters=2, nv_filters=4, recent_num=10, random_num=None, seed=42,
                 lower_upper_bound=None, tf_sess_config=None, device="cuda", dense_adam=False):
        super().__init__(task, data_info, embed_size, lower_upper_bound)
        self.all_args = locals()
        self.loss_type, self.norm_embed = loss_type, norm_embed
        self.n_epochs, self.lr, self.lr_decay, self.epsilon = n_epochs, lr, lr_decay, epsilon
        self.reg = reg_config(reg)
        self.batch_size, self.sampler, self.num_neg = batch_size, sampler, num_neg
        self.dropout_rate, self.use_bn = dropout_config(dropout_rate), use_bn          # stored, unused (as in the reference)
        self.nh_filters, self.nv_filters, self.seed = nh_filters, nv_filters, seed
        self.seq_mode, self.max_seq_len = check_seq_mode(recent_num, random_num)
        self.recent_seqs, self.recent_seq_lens = get_recent_seqs(self.n_users, self.user_consumed, self.n_items,
                                                                 self.max_seq_len)
        self._device_arg, self.dense_adam = device, dense_adam
        self._check_params()
        if self.reg and not dense_adam:
            raise ValueError(REG_NEEDS_DENSE)
        self.net = None

    def _check_params(self):
        if self.loss_type not in ("cross_entropy", "focal"):
            raise ValueError("`loss_type` must be one of (`cross_entropy`, `focal`)")
        for name in ("nh_filters", "nv_filters"):
            v = getattr(self, name)
            if not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f"`{name}` must be a positive integer, got {v}")

    def build_model(self):
        self.device = hip_device(self._device_arg)
        if not ops.caser_supported(self.max_seq_len, self.embed_size, self.nh_filters, self.nv_filters):
            raise ValueError(UNSUPPORTED.format(self.max_seq_len, self.embed_size, self.nh_filters, self.nv_filters))
        self.net = CaserNet(self.n_users, self.n_items, self.embed_size, self.nh_filters, self.nv_filters, self.norm_embed,
                            self.max_seq_len, self.lr, self.epsilon, self.seed, self.device, self.dense_adam,
                            "mse" if self.task == "rating" else self.loss_type, reg=self.reg)

    def train_on_batch(self, b):
        self.apply_lr_schedule()
        return self.net.train_step(b.users, b.seqs.interacted_seq, b.items, b.labels)

    # ---- embeddings and dynamic inference --------------------------------------------------------
    def set_embeddings(self):
        """The OOV row of `user_embeds_var` becomes the mean user row (`dyn_embed_base.py:271-283`); users: the net on the
        cached recent windows."""
        uv = self.net.vars["user_embeds_var"]
        with torch.no_grad():
            uv[self.n_users] = uv[: self.n_users].mean(dim=0)
        self._export_with_bias(self.net.embed_users(np.arange(self.n_users, dtype=np.int32), self.recent_seqs[: self.n_users]))

    def _default_window(self, uid):
        return self.recent_seqs[[uid]]

    def dyn_user_embedding(self, user, user_feats=None, seq=None, include_bias=False, inner_id=False):
        self._check_dynamic(user, user_feats, seq)
        uid = int(self.convert_array_id(user, inner_id)[0])
        vec = self.net.embed_users(np.array([uid], dtype=np.int32), self._window(uid, seq, inner_id))[0].cpu().numpy()
        return np.append(vec, np.float32(1.0)) if include_bias else vec

    # ---- persistence ----------------------------------------------------------------------------
    def _check_window(self, arrays):
        """The horizontal layers are one per position of the window and the vertical kernel is [1, L, nv]: saved convolution
        tensors fit only the `recent_num` they were trained at."""
        for k, p in self.net.P.params.items():
            if k in arrays and tuple(arrays[k].shape) != tuple(p.shape):
                raise ValueError(f'the saved "{k}" has shape {tuple(arrays[k].shape)}, this model needs {tuple(p.shape)}: Caser\'s '
                                 f"convolution shapes depend on the window, so a checkpoint taken at another `recent_num` (or "
                                 f"other filter counts or `embed_size`) cannot be loaded; this model has recent_num="
                                 f"{self.max_seq_len}")
        extra = f"conv1d_{self.max_seq_len + 1}/kernel"
        if extra in arrays:
            raise ValueError(f'the saved model has a layer "{extra}": it was taken at a larger `recent_num` than this model\'s '
                             f"{self.max_seq_len} and cannot be loaded")

    def load_variables_np(self, arrays):
        self._check_window(arrays)
        super().load_variables_np(arrays)

    def rebuild_model(self, path, model_name, full_assign=True):
        """Retraining on merged data: users and items keep their ids (new ones are appended), so the first `n_users` /
        `n_items` rows of the tables are the saved ones; the pad rows of `seq_embeds_var` and `user_embeds_var` move from the
        old `n_items` / `n_users` to the new ones; convolution and Dense parameters have the same shapes (the same
        `recent_num`, or `ValueError`) and are copied.  With `full_assign` the Adam moments follow and the step count is
        restored."""
        arrays, old = self._begin_rebuild(path, model_name)
        self._check_window(arrays)
        n_users, n_items = int(old.n_users), int(old.n_items)
        n_old = {"user_embeds_var": n_users, "seq_embeds_var": n_items, "item_embeds_var": n_items, "item_bias_var": n_items}
        pad_moves = {"seq_embeds_var": (n_items, self.n_items), "user_embeds_var": (n_users, self.n_users)}
        self._take_over(arrays, n_old, pad_moves, full_assign)
