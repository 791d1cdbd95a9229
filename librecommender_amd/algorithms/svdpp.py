"""`SVDpp` (`libreco/algorithms/svdpp.py`): SVD whose user vector is z_u = p_u + |N(u)|^-1/2 sum_{j in N(u)} y_j, with
N(u) the last `recent_num` consumed items of the user (all of them for `recent_num=None`; the `sqrtn` combiner of
`safe_embedding_lookup_sparse`: a repeated item counts twice, an empty history gives z_u = p_u).

A training step pools the histories of the batch's distinct users (`lr_svdpp_pool_f32`), scores the samples against their
user's slot of that block (`lr_mf_score_f32`), sums the user-side gradient per distinct user and hands it to every y row of
that user's history through the slot (`lr_svdpp_hist_grad_f32`): no per-entry gradient buffer exists.  The reference pools
ALL users every step; the rows outside the batch receive no gradient, so the result is the same.  The
export (`set_embeddings`) pools all users.  The other deliberate differences are those of algorithms/svd.py."""
from __future__ import annotations

from .svd import SvdBase, history_csr


class SVDpp(SvdBase):
    with_history = True

    def __init__(self, task, data_info, loss_type="cross_entropy", embed_size=16, n_epochs=20, lr=0.001, lr_decay=False,
                 epsilon=1e-5, reg=None, batch_size=256, sampler="random", num_neg=1, seed=42, recent_num=30,
                 lower_upper_bound=None, tf_sess_config=None, device="cuda", dense_adam=False):
        super().__init__(task, data_info, embed_size, lower_upper_bound)
        self.all_args = locals()
        self.recent_num = recent_num
        self._init_common(loss_type, n_epochs, lr, lr_decay, epsilon, reg, batch_size, sampler, num_neg, seed, device, dense_adam)
        self.sparse_interaction = None          # (hist_ptr, hist_idx), built at the first `fit` (`svdpp.py:150-151`)

    def _set_sparse_interaction(self):
        """`svdpp.py:178-194` as a CSR: (int64 [n_users + 1], int32 [nnz])."""
        return history_csr(self.user_consumed, self.n_users, self.recent_num)

    def build_model(self):
        super().build_model()
        if self.sparse_interaction is not None:
            self.net.set_history(*self.sparse_interaction)

    def fit(self, train_data, neg_sampling, verbose=1, shuffle=True, eval_data=None, metrics=None, k=10,
            eval_batch_size=8192, eval_user_num=None, num_workers=0):
        if self.sparse_interaction is None:
            self.sparse_interaction = self._set_sparse_interaction()
            if self.net is not None:
                self.net.set_history(*self.sparse_interaction)
        super().fit(train_data, neg_sampling, verbose, shuffle, eval_data, metrics, k, eval_batch_size, eval_user_num,
                    num_workers)

    def _user_vectors(self):
        return self.net.pooled_all()

    def load_state_arrays(self, arrays):
        # a full checkpoint restores the variables; the histories come from this `data_info`
        if self.sparse_interaction is None:
            self.sparse_interaction = self._set_sparse_interaction()
            self.net.set_history(*self.sparse_interaction)
        super().load_state_arrays(arrays)

    def rebuild_model(self, path, model_name, full_assign=False):
        self.sparse_interaction = self._set_sparse_interaction()          # from the merged `user_consumed`
        self._rebuild(path, model_name, full_assign)
