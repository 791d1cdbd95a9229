"""`WaveNet` (`libreco/algorithms/wave_net.py`): the sequence recommender built on the dilated causal convolutions of van den
Oord et al., with the reference's constructor, checks, `fit / predict / recommend_user / dyn_user_embedding` and checkpoints.
The convolution stack, the 1x1 layer and the pool run on csrc/wavenet.hip (one forward launch, one backward call,
`nets/wavenet_net.py`), the exported embeddings are served by `lr_score_topk_f32` like every `EmbedBase` model.

Deliberate differences from the reference:
  (a) the arithmetic is the reference's TF2 branch (Keras `Conv1D` with padding="causal" and a dilation rate); its TF1 branch
      (`tf.layers.conv1d`, which drops the dilation) is not provided;
  (b) `use_bn` and `dropout_rate` are accepted, stored and, as in the reference's graph, never used: it builds neither a
      batch normalisation nor a dropout layer;
  (c) the default optimiser is TF1-style Adam on the rows a batch touches; `dense_adam=True` is the reference's TF1
      semantics, and `reg` needs it;
  (d) a window, `embed_size` or `n_filters` outside 1 to 128, or more than 16 dilated layers, raise `ValueError` at
      `build_model` (`lr_wavenet_supported`);
  (e) `tf_sess_config` is accepted and ignored; `user_feats` is rejected (the model has no user features); under a process
      group of more than one rank `fit` raises.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from ..bases import EmbedBase
from ..bases.base import hip_device
from ..batch.sequence import get_recent_seqs
from ..layers.row_adam import REG_NEEDS_DENSE
from ..nets.wavenet_net import WaveNetNet
from ..utils.validate import check_seq_mode, dropout_config, reg_config

PAD_TABLES = ("seq_embeds_var", "user_embeds_var")


class WaveNet(EmbedBase):
    uses_sequence = True

    def __init__(self, task, data_info=None, loss_type="cross_entropy", embed_size=16, norm_embed=False, n_epochs=20, lr=0.001,
                 lr_decay=False, epsilon=1e-5, reg=None, batch_size=256, sampler="random", num_neg=1, dropout_rate=None,
                 use_bn=False, n_filters=16, n_blocks=1, n_layers_per_block=4, recent_num=10, random_num=None, seed=42,
                 lower_upper_bound=None, tf_sess_config=None, device="cuda", dense_adam=False):
        super().__init__(task, data_info, embed_size, lower_upper_bound)
        self.all_args = locals()
        self.loss_type, self.norm_embed = loss_type, norm_embed
        self.n_epochs, self.lr, self.lr_decay, self.epsilon = n_epochs, lr, lr_decay, epsilon
        self.reg = reg_config(reg)
        self.batch_size, self.sampler, self.num_neg = batch_size, sampler, num_neg
        self.dropout_rate, self.use_bn = dropout_config(dropout_rate), use_bn          # stored, unused (as in the reference)
        self.n_filters, self.n_blocks, self.n_layers_per_block, self.seed = n_filters, n_blocks, n_layers_per_block, seed
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
        for name in ("n_filters", "n_blocks", "n_layers_per_block"):
            v = getattr(self, name)
            if not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f"`{name}` must be a positive integer, got {v}")

    def build_model(self):
        self.device = hip_device(self._device_arg)
        if not ops.wavenet_supported(self.max_seq_len, self.embed_size, self.n_filters, self.n_blocks, self.n_layers_per_block):
            raise ValueError(f"WaveNet supports a window, `embed_size` and `n_filters` from 1 to 128 and at most 16 dilated "
                             f"layers (the convolution kernels' limit), got {self.max_seq_len}, {self.embed_size}, "
                             f"{self.n_filters}, {self.n_blocks} x {self.n_layers_per_block}")
        self.net = WaveNetNet(self.n_users, self.n_items, self.embed_size, self.n_filters, self.n_blocks, self.n_layers_per_block,
                              self.norm_embed, self.max_seq_len, self.lr, self.epsilon, self.seed, self.device, self.dense_adam,
                              "mse" if self.task == "rating" else self.loss_type, reg=self.reg)

    def train_on_batch(self, b):
        self.apply_lr_schedule()
        return self.net.train_step(b.users, b.seqs.interacted_seq, b.items, b.labels)

    # ---- embeddings (`bases/dyn_embed_base.py:240-285`) ------------------------------------------
    def set_embeddings(self):
        """The OOV row of `user_embeds_var` becomes the mean user row; users: the net on the cached recent windows, a column
        of ones appended (the item side carries `item_bias_var` there); items: `item_embeds_var` rows + the bias column."""
        uv = self.net.vars["user_embeds_var"]
        with torch.no_grad():
            uv[self.n_users] = uv[: self.n_users].mean(dim=0)
        ue = self.net.embed_users(np.arange(self.n_users, dtype=np.int32), self.recent_seqs[: self.n_users])
        w, bias = self.net.item_matrix()
        self.user_embeds = torch.cat([ue, torch.ones_like(ue[:, :1])], dim=1).contiguous()
        self.item_embeds = torch.cat([w, bias.view(-1, 1)], dim=1).contiguous()

    def convert_array_id(self, user, inner_id):
        assert np.isscalar(user), f"User to convert must be scalar, got: {user}"
        if inner_id:
            if not isinstance(user, (int, np.integer)):
                raise ValueError(f"`inner id` user must be int, got {user}")
            return np.array([user if 0 <= user < self.n_users else self.n_users])
        return np.array([self.data_info.user2id.get(user, self.n_users)])

    def _window(self, uid, seq, inner_id):
        """[1, L] window (`recommendation/preprocess.py:7-23,79-85`): the last L entries of `seq` (unknown items become the
        pad id), padded with the pad id, or the user's cached recent window."""
        L, N = self.max_seq_len, self.n_items
        if seq is None or len(seq) == 0:
            return self.recent_seqs[[uid]]
        ids = list(seq) if inner_id else [self.data_info.item2id.get(i, N) for i in seq]
        ids = [i if 0 <= i < N else N for i in ids[-min(L, len(ids)):]]
        out = np.full((1, L), N, dtype=np.int32)
        out[0, : len(ids)] = ids
        return out

    def dyn_user_embedding(self, user, user_feats=None, seq=None, include_bias=False, inner_id=False):
        from ..recommendation import check_dynamic_rec_feats

        if user_feats is not None:
            raise ValueError("`WaveNet` has no user features: `user_feats` is not supported")
        check_dynamic_rec_feats(self.model_name, user, user_feats, seq)
        uid = int(self.convert_array_id(user, inner_id)[0])
        vec = self.net.embed_users(np.array([uid], dtype=np.int32), self._window(uid, seq, inner_id))[0].cpu().numpy()
        return np.append(vec, np.float32(1.0)) if include_bias else vec

    def recommend_user(self, user, n_rec, user_feats=None, seq=None, cold_start="average", inner_id=False,
                       filter_consumed=True, random_rec=False):
        if user_feats is not None:
            raise ValueError("`WaveNet` has no user features: `user_feats` is not supported")
        if seq is None:
            return super().recommend_user(user, n_rec, cold_start, inner_id, filter_consumed, random_rec)
        from ..recommendation import check_dynamic_rec_feats, recommend_from_embedding

        check_dynamic_rec_feats(self.model_name, user, user_feats, seq)
        vec = torch.from_numpy(self.dyn_user_embedding(user, None, seq, include_bias=True, inner_id=inner_id)).view(1, -1)
        uid = int(self.convert_array_id(user, inner_id)[0])
        recs = recommend_from_embedding(self, [uid], n_rec, None, self.item_embeds, filter_consumed, random_rec,
                                        user_vectors=vec)[0]
        return {user: recs if inner_id else np.array([self.data_info.id2item[i] for i in recs.tolist()])}

    # ---- persistence ----------------------------------------------------------------------------
    def variables_np(self):
        out = {}
        for k, v in self.net.vars.items():
            out[f"embedding/{k}"] = (v.view(-1) if k == "item_bias_var" else v).cpu().numpy()
        out.update({k: p.detach().cpu().numpy() for k, p in self.net.P.params.items()})
        return out

    def optimizer_arrays(self):
        P = self.net.P
        return {**self.net.optimizer_arrays(), "opt::dense_m": P.m.cpu().numpy(), "opt::dense_v": P.v.cpu().numpy()}

    def load_variables_np(self, arrays):
        with torch.no_grad():
            for k, var in self.net.vars.items():
                if f"embedding/{k}" in arrays:
                    var.copy_(torch.from_numpy(arrays[f"embedding/{k}"]).view_as(var))
            for k, p in self.net.P.params.items():
                if k in arrays:
                    p.copy_(torch.from_numpy(arrays[k]))

    def rebuild_model(self, path, model_name, full_assign=True):
        """Retraining on merged data: users and items keep their ids (new ones are appended), so the first `n_users` /
        `n_items` rows of the tables are the saved ones; the pad rows of `seq_embeds_var` and `user_embeds_var` move from the
        old `n_items` / `n_users` to the new ones; convolution and Dense parameters have the same shapes and are copied.  With
        `full_assign` the Adam moments follow and the step count is restored."""
        arrays, old = self._begin_rebuild(path, model_name)
        net = self.net
        n_old = {"user_embeds_var": int(old.n_users), "seq_embeds_var": int(old.n_items), "item_embeds_var": int(old.n_items),
                 "item_bias_var": int(old.n_items)}
        n_new = {"user_embeds_var": self.n_users, "seq_embeds_var": self.n_items}
        net.take_over(arrays, lambda k: f"embedding/{k}", lambda k: n_old[k], full_assign)
        with torch.no_grad():
            for name in PAD_TABLES:
                pad_sets = [(net.vars[name], f"embedding/{name}")]
                if full_assign:
                    pad_sets += [(net.m[name], f"opt::m_{name}"), (net.v[name], f"opt::v_{name}")]
                for dst, key in pad_sets:
                    if key in arrays:
                        dst[n_new[name]] = torch.from_numpy(arrays[key][n_old[name]]).to(dst.device)
            P = net.P
            same = all(k in arrays and tuple(arrays[k].shape) == tuple(p.shape) for k, p in P.params.items())
            for k, p in P.params.items():
                if k in arrays and tuple(arrays[k].shape) == tuple(p.shape):
                    p.copy_(torch.from_numpy(arrays[k]))
                else:
                    print(f'variable "{k}" is not in the saved model or changed its shape, will be skipped.')
            if full_assign and same and "opt::dense_m" in arrays and arrays["opt::dense_m"].shape == tuple(P.m.shape):
                P.m.copy_(torch.from_numpy(arrays["opt::dense_m"]))
                P.v.copy_(torch.from_numpy(arrays["opt::dense_v"]))
