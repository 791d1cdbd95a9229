"""`RNN4Rec` (`libreco/algorithms/rnn4rec.py`): the session-based recommender of Hidasi et al. (GRU4Rec; an LSTM is also
offered), with the reference's constructor, checks, `fit / predict / recommend_user / dyn_user_embedding` and checkpoints.
The recurrent layers run on csrc/rnn.hip (one forward and one backward call per layer, `nets/rnn_nets.py`), the exported
embeddings are served by `lr_score_topk_f32` like every `EmbedBase` model.  Dynamic inference (`recommend_user` with a `seq`,
the window) is `bases/dyn_embed_base.py`'s, the checkpoint arrays are its `SeqTowerCheckpoint`'s.

Deliberate differences from the reference:
  (a) the arithmetic is the reference's TF2 branch (Keras `GRU` / `LSTM` under a sequence mask); its TF1 branch
      (`MultiRNNCell` + `dynamic_rnn`, other cell equations) is not provided;
  (b) dropout is this package's own definition (one mask per sample and layer, constant over time);
  (c) the default optimiser is TF1-style Adam on the rows a batch touches; `dense_adam=True` is the reference's TF1
      semantics, and `reg` needs it;
  (d) `hidden_units` and the implied input width outside `lr_rnn_supported` (1 to 128) raise `ValueError` at `build_model`;
  (e) `tf_sess_config` is accepted and ignored; `user_feats` is rejected (the model has no user features); under a process
      group of more than one rank `fit` raises.
"""
from __future__ import annotations

import numpy as np

from .. import ops
from ..bases import DynEmbedBase
from ..bases.base import hip_device
from ..bases.dyn_embed_base import SeqTowerCheckpoint
from ..batch.sequence import get_recent_seqs
from ..layers.row_adam import REG_NEEDS_DENSE
from ..nets.rnn_nets import RNN4RecNet
from ..utils.validate import check_seq_mode, dropout_config, hidden_units_config, reg_config


class RNN4Rec(SeqTowerCheckpoint, DynEmbedBase):
    uses_sequence = True
    takes_user_feats = False

    def __init__(self, task, data_info=None, loss_type="cross_entropy", rnn_type="gru", embed_size=16, norm_embed=False,
                 n_epochs=20, lr=0.001, lr_decay=False, epsilon=1e-5, reg=None, batch_size=256, sampler="random", num_neg=1,
                 dropout_rate=None, hidden_units=16, use_layer_norm=False, recent_num=10, random_num=None, seed=42,
                 lower_upper_bound=None, tf_sess_config=None, device="cuda", dense_adam=False):
        super().__init__(task, data_info, embed_size, lower_upper_bound)
        self.all_args = locals()
        self.loss_type, self.rnn_type, self.norm_embed = loss_type, rnn_type.lower(), norm_embed
        self.n_epochs, self.lr, self.lr_decay, self.epsilon = n_epochs, lr, lr_decay, epsilon
        self.hidden_units = hidden_units_config(hidden_units)
        self.reg = reg_config(reg)
        self.batch_size, self.sampler, self.num_neg = batch_size, sampler, num_neg
        self.dropout_rate = dropout_config(dropout_rate)
        self.use_ln, self.seed = use_layer_norm, seed
        self.seq_mode, self.max_seq_len = check_seq_mode(recent_num, random_num)
        self.recent_seqs, self.recent_seq_lens = get_recent_seqs(self.n_users, self.user_consumed, self.n_items,
                                                                 self.max_seq_len)
        self._device_arg, self.dense_adam = device, dense_adam
        self._check_params()
        if self.reg and not dense_adam:
            raise ValueError(REG_NEEDS_DENSE)
        self.net = None

    def _check_params(self):
        if self.rnn_type not in ("lstm", "gru"):
            raise ValueError("`rnn_type` must either be `lstm` or `gru`")
        if self.loss_type not in ("cross_entropy", "bpr", "focal"):
            raise ValueError("`loss_type` must be one of (`cross_entropy`, `focal`, `bpr`)")

    def build_model(self):
        self.device = hip_device(self._device_arg)
        dims = [self.hidden_units[0], *self.hidden_units]
        for d, h in zip(dims[:-1], dims[1:]):
            if not ops.rnn_supported(self.rnn_type, d, h):
                raise ValueError(f"RNN4Rec supports `hidden_units` from 1 to 128 per layer (the recurrent kernels' limit), "
                                 f"got {self.hidden_units}")
        self.net = RNN4RecNet(self.n_items, self.embed_size, self.hidden_units, self.rnn_type, self.use_ln, self.dropout_rate,
                              self.norm_embed, self.max_seq_len, self.lr, self.epsilon, self.seed, self.device, self.dense_adam,
                              "mse" if self.task == "rating" else self.loss_type, reg=self.reg)

    def train_on_batch(self, b):
        self.apply_lr_schedule()
        s = b.seqs
        if hasattr(b, "item_pairs"):
            return self.net.train_step(s.interacted_seq, s.interacted_len, pos=b.item_pairs[0], neg=b.item_pairs[1])
        return self.net.train_step(s.interacted_seq, s.interacted_len, items=b.items, labels=b.labels)

    # ---- embeddings and dynamic inference --------------------------------------------------------
    def set_embeddings(self):
        """Users: the net on the cached recent windows."""
        self._export_with_bias(self.net.embed_users(self.recent_seqs[: self.n_users], self.recent_seq_lens[: self.n_users]))

    def _default_window(self, uid):
        return self.recent_seqs[[uid]]

    def _window_len(self, uid, seq):
        """[1] steps of the window `_window` builds: those of `seq` that fit, or the cached length; no history is the one-step
        sequence [pad]."""
        if seq is None or len(seq) == 0:
            return self.recent_seq_lens[[uid]]
        return np.array([max(min(len(seq), self.max_seq_len), 1)], dtype=np.int32)

    def dyn_user_embedding(self, user, user_feats=None, seq=None, include_bias=False, inner_id=False):
        self._check_dynamic(user, user_feats, seq)
        uid = int(self.convert_array_id(user, inner_id)[0])
        vec = self.net.embed_users(self._window(uid, seq, inner_id), self._window_len(uid, seq))[0].cpu().numpy()
        return np.append(vec, np.float32(1.0)) if include_bias else vec

    # ---- persistence ----------------------------------------------------------------------------
    def rebuild_model(self, path, model_name, full_assign=True):
        """Retraining on merged data: items keep their ids (new ones are appended), so the first `n_items` rows of the three
        tables are the saved ones; the pad row of `seq_embeds_var` moves from the old `n_items` to the new one; recurrent,
        layer-norm and Dense parameters have the same shapes and are copied.  With `full_assign` the Adam moments follow
        and the step count is restored."""
        arrays, old = self._begin_rebuild(path, model_name)
        n_old = int(old.n_items)
        self._take_over(arrays, dict.fromkeys(self.net.vars, n_old), {"seq_embeds_var": (n_old, self.n_items)}, full_assign)
