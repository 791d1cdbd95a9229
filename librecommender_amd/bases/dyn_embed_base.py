"""Embedding models whose user vector can be recomputed at serving time from a behaviour sequence and / or overridden user
features (`libreco/bases/dyn_embed_base.py:17-322`): `RNN4Rec`, `WaveNet`, `Caser`, `YouTubeRetrieval`, `TwoTower`.  The id
conversion, the dynamic branch of `recommend_user`, the sequence window, the user-feature override and the export tail of
`set_embeddings` live here; a model supplies `dyn_user_embedding` (its one call into the net) and, if it takes sequences,
`_default_window`.

`SeqTowerCheckpoint` is the checkpoint surface of the models whose net is a `nets.seq_tower.SeqTowerNet` (`NamedTables` +
`DenseParams`): `RNN4Rec`, `WaveNet` and `Caser`.
"""
from __future__ import annotations

import numpy as np
import torch

from ..feature_override import override_dense, override_sparse
from ..recommendation import check_dynamic_rec_feats, recommend_from_embedding
from .embed_base import EmbedBase


class DynEmbedBase(EmbedBase):
    takes_user_feats = True          # False: the model has no user features, `user_feats` raises

    def convert_array_id(self, user, inner_id):
        """One raw (or inner) user id -> `[inner id]`; unknown users map to the OOV id (`dyn_embed_base.py:60-72`)."""
        assert np.isscalar(user), f"User to convert must be scalar, got: {user}"
        if inner_id:
            if not isinstance(user, (int, np.integer)):
                raise ValueError(f"`inner id` user must be int, got {user}")
            return np.array([user if 0 <= user < self.n_users else self.n_users])
        return np.array([self.data_info.user2id.get(user, self.n_users)])

    def _check_dynamic(self, user, user_feats, seq):
        if user_feats is not None and not self.takes_user_feats:
            raise ValueError(f"`{self.model_name}` has no user features: `user_feats` is not supported")
        check_dynamic_rec_feats(self.model_name, user, user_feats, seq)

    def dyn_user_embedding(self, user, user_feats=None, seq=None, include_bias=False, inner_id=False):
        raise NotImplementedError

    def recommend_user(self, user, n_rec, user_feats=None, seq=None, cold_start="average", inner_id=False,
                       filter_consumed=True, random_rec=False):
        """`dyn_embed_base.py:74-164`: the exported embeddings unless `user_feats` or `seq` is given; then ONE user, served
        from the vector `dyn_user_embedding` computes."""
        if user_feats is None and seq is None:
            return super().recommend_user(user, n_rec, cold_start, inner_id, filter_consumed, random_rec)
        self._check_dynamic(user, user_feats, seq)
        vec = torch.from_numpy(self.dyn_user_embedding(user, user_feats, seq, include_bias=True, inner_id=inner_id)).view(1, -1)
        uid = int(self.convert_array_id(user, inner_id)[0])
        recs = recommend_from_embedding(self, [uid], n_rec, None, self.item_embeds, filter_consumed, random_rec,
                                        user_vectors=vec)[0]
        return {user: recs if inner_id else np.array([self.data_info.id2item[i] for i in recs.tolist()])}

    # ---- the inputs of one user ----------------------------------------------------------------------
    def _pad_window(self, ids):
        """[1, L] int32: the last L of the inner item ids `ids`, out-of-range ones turned into the pad id `n_items`, which
        also fills the tail."""
        L, N = self.max_seq_len, self.n_items
        ids = [i if 0 <= i < N else N for i in ids[-L:]]
        out = np.full((1, L), N, dtype=np.int32)
        out[0, : len(ids)] = ids
        return out

    def _default_window(self, uid):
        """The [1, L] window of a user for whom no `seq` is given."""
        raise NotImplementedError

    def _window(self, uid, seq, inner_id):
        """[1, L] window (`recommendation/preprocess.py:7-23,79-85`): the last L entries of `seq` (raw ids unless `inner_id`,
        unknown items become the pad id), or without one the model's `_default_window`."""
        if seq is None or len(seq) == 0:
            return self._default_window(uid)
        return self._pad_window(list(seq) if inner_id else [self.data_info.item2id.get(i, self.n_items) for i in seq])

    def _user_feature_rows(self, uid, user_feats):
        """(sparse, dense): the stored feature rows of `uid`, each None when the data has none, with `user_feats` {column:
        value} written over them (`dyn_embed_base.py:190-215`)."""
        d = self.data_info
        sp = de = None
        if d.user_sparse_unique is not None:
            sp = d.user_sparse_unique[[uid]]
            if user_feats:
                sp = override_sparse(d, sp, user_feats, d.user_sparse_col.name)
        if d.user_dense_unique is not None:
            de = d.user_dense_unique[[uid]]
            if user_feats:
                de = override_dense(d, de, user_feats, d.user_dense_col.name)
        return sp, de

    def _export_with_bias(self, ue):
        """`dyn_embed_base.py:240-269` for a model with `item_bias_var`: users get a column of ones, the items' rows carry
        their bias there."""
        w, bias = self.net.item_matrix()
        self.user_embeds = torch.cat([ue, torch.ones_like(ue[:, :1])], dim=1).contiguous()
        self.item_embeds = torch.cat([w, bias.view(-1, 1)], dim=1).contiguous()


class SeqTowerCheckpoint:
    """Checkpoint arrays of a model on a `SeqTowerNet`: tables as `embedding/<name>` (`item_bias_var` flat), Dense parameters
    under their own names, moments as `opt::m_<name>` / `opt::v_<name>` and `opt::dense_m` / `opt::dense_v`."""

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

    def _take_over(self, arrays, n_old, pad_moves, full_assign):
        """Retraining on merged data: ids keep their place, so the first `n_old[table]` rows of every table are the saved
        ones; `pad_moves` {table: (old pad row, new pad row)} carries the pad rows behind them to their new place; the Dense
        parameters have the same shapes and are copied.  With `full_assign` the Adam moments follow and the step count is
        restored."""
        net = self.net
        net.take_over(arrays, lambda k: f"embedding/{k}", lambda k: n_old[k], full_assign)
        with torch.no_grad():
            for name, (old_row, new_row) in pad_moves.items():
                pad_sets = [(net.vars[name], f"embedding/{name}")]
                if full_assign:
                    pad_sets += [(net.m[name], f"opt::m_{name}"), (net.v[name], f"opt::v_{name}")]
                for dst, key in pad_sets:
                    if key in arrays:
                        dst[new_row] = torch.from_numpy(arrays[key][old_row]).to(dst.device)
        net.P.take_over(arrays, full_assign)
