"""`ALS` (`libreco/algorithms/als.py`): alternating least squares, explicit (rating) and implicit (ranking), with the
reference's constructor, checks and checkpoints.  Each half-sweep runs on the device (csrc/als.hip via
`ops.als_half_sweep`); there is no CPU solver.

Deliberate differences from the reference:
  (a) `fit` leaves `train_data.sparse_interaction.data` alone (the reference turns it into the confidence in place, so its
      second `fit` on the same set compounds `alpha`);
  (b) both CSRs have shape (n_users, n_items): an id without a training interaction is a zero-degree row;
  (c) `n_threads` is accepted and ignored;
  (d) under a process group of more than one rank `fit` raises, as `Base.fit` does for models without a sharded net;
  (e) `embed_size` above 128 raises `ValueError` (the per-row K x K system is solved in LDS).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import ops
from ..bases import EmbedBase
from ..bases.base import hip_device
from ..evaluation.evaluate import print_metrics
from ..utils.initializers import truncated_normal
from ..utils.misc import time_block
from ..utils.validate import check_fitting

CG_STEPS = 3      # `_als.pyx:als_update` passes cg_steps = 3


class ALS(EmbedBase):
    def __init__(self, task, data_info, embed_size=16, n_epochs=10, reg=None, alpha=10, use_cg=True, n_threads=1,
                 seed=42, lower_upper_bound=None):
        super().__init__(task, data_info, embed_size, lower_upper_bound)
        self.all_args = locals()
        self.n_epochs = n_epochs
        self.reg = self._check_reg(reg)
        self.alpha = alpha
        self.use_cg = use_cg
        self.n_threads = n_threads
        self.seed = seed
        if not ops.als_supported(embed_size):
            raise ValueError(f"ALS supports `embed_size` up to 128 (the per-row system is solved in LDS), got {embed_size}")

    @staticmethod
    def _check_reg(reg):
        if not isinstance(reg, float) or reg <= 0.0:
            raise ValueError(f"`reg` must be float and positive, got {reg}")
        return reg

    def initial_tables(self):
        """The reference's draws (`als.py:build_model`): users, then items, from one generator seeded with `seed`."""
        rng = np.random.default_rng(self.seed)
        u = truncated_normal(rng, shape=[self.n_users, self.embed_size], mean=0.0, scale=0.03)
        i = truncated_normal(rng, shape=[self.n_items, self.embed_size], mean=0.0, scale=0.03)
        return u, i

    def build_model(self):
        self.device = hip_device("cuda")
        u, i = self.initial_tables()
        self.user_embeds = torch.from_numpy(u).to(self.device)
        self.item_embeds = torch.from_numpy(i).to(self.device)

    def train_on_batch(self, batch):
        raise NotImplementedError("ALS trains by whole half-sweeps, not by batches")

    def set_embeddings(self):
        pass

    def _device_csr(self, train_data):
        """(rowptr, col, val) of the user x item matrix and of its transpose on the device, shapes (n_users, n_items) and
        (n_items, n_users); val is the confidence alpha r + 1 (ranking) or the rating, computed in f32 as the reference."""
        csr = train_data.sparse_interaction
        dev, nu, ni = self.device, self.n_users, self.n_items
        indptr = np.asarray(csr.indptr, dtype=np.int64)
        rp = np.full(nu + 1, indptr[-1] if len(indptr) else 0, dtype=np.int64)
        rp[: len(indptr)] = indptr
        rowptr_u = torch.from_numpy(rp).to(dev)
        col_u = torch.from_numpy(np.asarray(csr.indices, dtype=np.int32)).to(dev)
        val_u = torch.from_numpy(np.asarray(csr.data, dtype=np.float32)).to(dev)   # a copy: the caller's data stays
        if self.task == "ranking":
            val_u = val_u * self.alpha + 1
        nnz = col_u.numel()
        rows_u = torch.repeat_interleave(torch.arange(nu, device=dev, dtype=torch.int64), rowptr_u[1:] - rowptr_u[:-1],
                                         output_size=nnz)
        order = torch.argsort(col_u.to(torch.int64) * nu + rows_u)
        col_i = rows_u[order].to(torch.int32).contiguous()
        val_i = val_u[order].contiguous()
        rowptr_i = torch.zeros(ni + 1, dtype=torch.int64, device=dev)
        rowptr_i[1:] = torch.cumsum(torch.bincount(col_u.to(torch.int64), minlength=ni), 0)
        return (rowptr_u, col_u, val_u.contiguous()), (rowptr_i, col_i, val_i)

    def _half_sweep(self, csr, plan, X, Y):
        implicit = self.task == "ranking"
        G0 = ops.als_gram(Y, self.reg, implicit)
        fail = ops.als_half_sweep(*csr, X, Y, G0, implicit, self.use_cg, plan, CG_STEPS)
        if fail is not None:
            bad = torch.nonzero(fail).flatten()
            if bad.numel():
                m = int(bad[0])
                raise ValueError(f"cython_lapack.posv failed (err={int(fail[m])}) on row {m}. "
                                 "Try increasing the regularization parameter.")

    def fit(self, train_data, neg_sampling, verbose=1, shuffle=True, eval_data=None, metrics=None, k=10,
            eval_batch_size=8192, eval_user_num=None, **kwargs):
        check_fitting(self, train_data, eval_data, neg_sampling, k)
        from .. import distributed as D

        if D.active() is not None:
            raise RuntimeError(f"{self.model_name}: multi-GPU `fit` (torch.distributed is initialised with more than one "
                               "rank) is implemented for TwoTower, LightGCN, FM / DeepFM with plain sparse columns and DIN "
                               "on pure ids; run this model in a single process")
        if verbose > 0:
            self.show_start_time()
        if not self.model_built:
            self.build_model()
            self.model_built = True
        # a second fit continues from the current tables, without their OOV rows
        self.user_embeds = self.user_embeds[: self.n_users].contiguous()
        self.item_embeds = self.item_embeds[: self.n_items].contiguous()
        user_csr, item_csr = self._device_csr(train_data)
        user_plan = ops.als_plan(user_csr[0], self.embed_size)
        item_plan = ops.als_plan(item_csr[0], self.embed_size)
        for epoch in range(1, self.n_epochs + 1):
            with time_block(f"Epoch {epoch}", verbose):
                self._half_sweep(user_csr, user_plan, self.user_embeds, self.item_embeds)
                self._half_sweep(item_csr, item_plan, self.item_embeds, self.user_embeds)
                torch.cuda.synchronize(self.device)
            if verbose > 1:
                self.assign_embedding_oov()
                print_metrics(model=self, neg_sampling=neg_sampling, eval_data=eval_data, metrics=metrics,
                              eval_batch_size=eval_batch_size, k=k, sample_user_num=eval_user_num, seed=self.seed)
                print("=" * 30)
                self.user_embeds = self.user_embeds[: self.n_users].contiguous()
                self.item_embeds = self.item_embeds[: self.n_items].contiguous()
        self.after_fit()

    def rebuild_model(self, path, model_name):
        """`als.py:rebuild_model`: fresh (larger) tables, the saved rows copied in without their OOV row."""
        self.model_built = True
        self.build_model()
        saved = np.load(os.path.join(path, f"{model_name}.npz"))
        for name, key in (("user_embeds", "user_embed"), ("item_embeds", "item_embed")):
            old = torch.from_numpy(saved[key][:-1]).to(self.device)
            getattr(self, name)[: old.shape[0]] = old
