"""`SageBase` (`libreco/bases/sage_base.py`): the neighbour-sampling graph models.  The reference assembles every batch on the
host (`graph/neighbor_walk.py`, `sampling/random_walks.py`, `batch/collators.py:322-396`: Python `random` per sampled
neighbour and per walk step); here start nodes, walk pairs, negatives, neighbours and the whole tower run on the device
(csrc/sage.hip, nets/sage_net.py).  Every draw is a function of (seed, global step, coordinates): two runs
give the same bits.  `full_inference` is accepted and has no effect; `remove_edges` is read by PinSage's net under i2i only (the
reference's non-DGL GraphSage never reads either).  A subclass names its net through `net_class`."""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import ops
from ..evaluation.evaluate import print_metrics
from ..nets.graph_nets import cosine_warm_restart_lr
from ..nets.sage_net import cumulative_table
from ..utils.misc import time_block
from ..utils.validate import check_fitting
from .base import hip_device
from .embed_base import EmbedBase
from .word2vec_base import flatten_lists


class SageBase(EmbedBase):
    def __init__(self, task, data_info, loss_type="cross_entropy", paradigm="i2i", embed_size=16, n_epochs=20, lr=0.001,
                 lr_decay=False, epsilon=1e-8, amsgrad=False, reg=None, batch_size=256, num_neg=1, dropout_rate=0.0,
                 remove_edges=False, num_layers=2, num_neighbors=3, num_walks=10, sample_walk_len=5, margin=1.0,
                 sampler="random", start_node="random", focus_start=False, seed=42, device="cuda", lower_upper_bound=None,
                 full_inference=False, fused=True):
        super().__init__(task, data_info, embed_size, lower_upper_bound)
        self.loss_type, self.paradigm, self.n_epochs, self.lr, self.lr_decay = loss_type, paradigm, n_epochs, lr, lr_decay
        self.epsilon, self.amsgrad, self.reg, self.batch_size, self.num_neg = epsilon, amsgrad, reg, batch_size, num_neg
        self.dropout_rate, self.remove_edges, self.num_layers, self.num_neighbors = dropout_rate, remove_edges, num_layers, num_neighbors
        self.num_walks, self.sample_walk_len, self.margin, self.sampler = num_walks, sample_walk_len, margin, sampler
        self.start_node, self.focus_start, self.full_inference, self.seed = start_node, focus_start, full_inference, seed
        self.fused, self._device_arg = fused, device
        self.net = None
        self.last_epoch_loss = None
        self._check_params()

    def _check_params(self):
        if self.task != "ranking":
            raise ValueError(f"`{self.model_name}` is only suitable for ranking")
        if self.paradigm not in ("u2i", "i2i"):
            raise ValueError("`paradigm` must either be `u2i` or `i2i`")
        if self.loss_type not in ("cross_entropy", "focal", "bpr", "max_margin"):
            raise ValueError(f"unsupported `loss_type`: {self.loss_type}")
        if self.paradigm == "i2i" and self.start_node not in ("random", "unpopular"):
            raise ValueError("`start_nodes` must either be `random` or `unpopular`")
        if not self.sampler:
            raise ValueError(f"`{self.model_name}` must use negative sampling, make sure data "
                             f"only contains positive samples when using negative sampling.")

    def _check_trainer_params(self):
        """`training/torch_trainer.py:200-223`."""
        assert 0 < self.num_neg < self.n_items, (f"`num_neg` should be positive and smaller than total items, "
                                                 f"got {self.num_neg}, {self.n_items}")
        if self.paradigm == "u2i" and self.sampler not in ("random", "unconsumed", "popular"):
            raise ValueError(f"`sampler` must be one of (`random`, `unconsumed`, `popular`) for u2i, got {self.sampler}")
        if self.paradigm == "i2i" and self.sampler not in ("random", "out-batch", "popular"):
            raise ValueError(f"`sampler` must be one of (`random`, `out-batch`, `popular`) for i2i, got {self.sampler}")

    # ---- the graph and the sampling tables ------------------------------------------------------------------------
    def sage_graph(self):
        """The two CSRs on the device, lists as `data_info` holds them (duplicates kept)."""
        d, dev = self.data_info, self.device
        uidx, uptr = flatten_lists([d.user_consumed.get(u, ()) for u in range(self.n_users)])
        iidx, iptr = flatten_lists([d.item_consumed.get(i, ()) for i in range(self.n_items)])
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        return ops.SageGraph(t(iptr), t(iidx), t(uptr), t(uidx))

    def _sampling_tables(self):
        d, dev = self.data_info, self.device
        freq = np.asarray([len(set(d.item_consumed.get(i, ()))) for i in range(self.n_items)], dtype=np.float64)
        self._neg_cum = self._start_cum = None
        if self.sampler == "popular":                        # `neg_probs_from_frequency`, temperature 0.75
            self._neg_cum = torch.from_numpy(cumulative_table(freq ** 0.75)).to(dev)
        if self.paradigm == "i2i" and self.start_node == "unpopular":      # `pos_probs_from_frequency`, alpha 1e-3
            prob = freq / self.n_users
            with np.errstate(divide="ignore", invalid="ignore"):
                w = np.where(prob > 0, (np.sqrt(prob / 1e-3) + 1) * (1e-3 / prob), 0.0)
            self._start_cum = torch.from_numpy(cumulative_table(w)).to(dev)

    def net_kwargs(self):
        """The feature layout of `data_info` for `SageNet`."""
        from ..utils.validate import sparse_feat_size

        d = self.data_info
        u2i = self.paradigm == "u2i"
        has_sparse, has_dense = bool(d.sparse_col.name), bool(d.dense_col.name)
        return dict(
            n_sparse_rows=sparse_feat_size(d) if has_sparse else 0, n_dense_rows=len(d.dense_col.name) if has_dense else 0,
            item_sparse=d.item_sparse_unique, item_dense=d.item_dense_unique, item_dense_cols=list(d.item_dense_col.index),
            user_sparse=d.user_sparse_unique if u2i else None, user_dense=d.user_dense_unique if u2i else None,
            user_dense_cols=list(d.user_dense_col.index))

    def net_class(self):
        """The net of the model and its keyword arguments beyond `SageNet`'s (a subclass with another tower overrides it)."""
        from ..nets.sage_net import SageNet

        return SageNet, {}

    def build_model(self):
        SageNet, extra = self.net_class()
        self._check_trainer_params()
        self.device = hip_device(self._device_arg)
        kw = self.net_kwargs()
        # what neither the fused nor the composed tower serves: the samplers' own ranges (fan-out, levels, dropout columns)
        if not (1 <= self.num_neighbors <= 10 and 0 <= self.num_layers <= 3 and 1 <= self.embed_size <= 128):
            raise ValueError(f"{self.model_name}: `num_layers` must be from 0 to 3, `num_neighbors` from 1 to 10 and "
                             f"`embed_size` from 1 to 128 (the device samplers' ranges), got {self.num_layers}, "
                             f"{self.num_neighbors} and {self.embed_size}")
        self.net = SageNet(self.paradigm, self.n_users, self.n_items, self.embed_size, self.num_layers, self.num_neighbors,
                           self.dropout_rate, self.device, self.sage_graph(), seed=self.seed, lr=self.lr, epsilon=self.epsilon,
                           reg=self.reg, amsgrad=self.amsgrad, margin=self.margin, fused=self.fused, **kw, **extra)
        self._sampling_tables()

    def train_on_batch(self, batch):
        raise NotImplementedError(f"{self.model_name} samples its batches on the device, not from collated batches")

    # ---- one step ---------------------------------------------------------------------------------------------------
    def sample_i2i(self, size, step):
        """(items, items_pos, items_neg) of one step: start nodes, walk pairs, negatives that avoid both ends of a pair."""
        net = self.net
        starts = ops.sage_starts(size, self.n_items, self.seed, step, self.device, cum=self._start_cum)
        items, pos = ops.sage_pairs(starts, net.graph, self.num_walks, self.sample_walk_len, self.focus_start, self.seed, step)
        in_batch = None
        if self.sampler == "out-batch":
            in_batch = torch.zeros(self.n_items, dtype=torch.uint8, device=self.device)
            in_batch[items.long()] = 1
            in_batch[pos.long()] = 1
        neg = ops.sage_negatives(items, pos, self.num_neg, self.n_items, self.sampler, self.seed, step, cum=self._neg_cum,
                                 in_batch=in_batch)
        return items, pos, neg

    def sample_u2i_negatives(self, users, pos, step):
        if self.sampler == "popular":
            return ops.sage_negatives(None, pos, self.num_neg, self.n_items, "popular", self.seed, step, cum=self._neg_cum)
        seed = (int(self.seed) * 1000003 + int(step)) & ((1 << 63) - 1)
        if self.sampler == "unconsumed":
            return ops.sample_negatives(pos, self.num_neg, self.n_items, seed, users=users, consumed_ptr=self._cptr,
                                        consumed_idx=self._cidx)
        return ops.sample_negatives(pos, self.num_neg, self.n_items, seed)

    def current_lr(self, epoch, batch, n_batches):
        if not self.lr_decay:
            return self.lr
        return cosine_warm_restart_lr(self.lr, (epoch - 1) + batch / n_batches)

    def fit(self, train_data, neg_sampling, verbose=1, shuffle=True, eval_data=None, metrics=None, k=10,
            eval_batch_size=8192, eval_user_num=None, num_workers=0):
        check_fitting(self, train_data, eval_data, neg_sampling, k)
        if not neg_sampling:
            raise ValueError(f"`{self.model_name}` must use negative sampling, make sure data "
                             f"only contains positive samples when using negative sampling.")
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
        dev, bs = self.device, int(self.batch_size)
        users_np = np.asarray(train_data.user_indices).astype(np.int32)
        items_np = np.asarray(train_data.item_indices).astype(np.int32)
        n = len(users_np)
        n_batches = max(1, math.ceil(n / bs))
        if self.paradigm == "u2i" and self.sampler == "unconsumed":
            csr = train_data.sparse_interaction.sorted_indices()
            rp = np.full(self.n_users + 1, csr.indptr[-1] if len(csr.indptr) else 0, dtype=np.int64)
            rp[: len(csr.indptr)] = csr.indptr
            self._cptr = torch.from_numpy(rp).to(dev)
            self._cidx = torch.from_numpy(np.asarray(csr.indices, dtype=np.int32)).to(dev)
        rng = np.random.default_rng(self.seed)
        for epoch in range(1, self.n_epochs + 1):
            with time_block(f"Epoch {epoch}", verbose):
                losses = []
                if self.paradigm == "u2i":
                    order = rng.permutation(n) if shuffle else np.arange(n)
                    users = torch.from_numpy(users_np[order]).to(dev)
                    items = torch.from_numpy(items_np[order]).to(dev)
                for b in range(n_batches):
                    lr = self.current_lr(epoch, b, n_batches)
                    step = self.net.step + 1
                    size = min(bs, n - b * bs)
                    if self.paradigm == "u2i":
                        q, pos = users[b * bs:b * bs + size].contiguous(), items[b * bs:b * bs + size].contiguous()
                        neg = self.sample_u2i_negatives(q, pos, step)
                    else:
                        q, pos, neg = self.sample_i2i(size, step)
                        if q.numel() == 0:               # no start node of the batch can walk anywhere
                            self.net.step += 1
                            continue
                    losses.append(self.net.train_step(self.loss_type, q, pos, neg, lr=lr))
                torch.cuda.synchronize(dev)
            if losses:
                self.last_epoch_loss = float(torch.stack(losses).mean())
                if verbose > 0:
                    print(f"\t train_loss: {self.last_epoch_loss:.4f}")
            if verbose > 1:
                self.prepare_for_eval()
                print_metrics(model=self, neg_sampling=neg_sampling, eval_data=eval_data, metrics=metrics,
                              eval_batch_size=eval_batch_size, k=k, sample_user_num=eval_user_num, seed=self.seed)
                print("=" * 30)
        self.after_fit()

    # ---- export -----------------------------------------------------------------------------------------------------
    def set_embeddings(self):
        """Item rows: the tower over all items in inference mode, neighbours drawn at a fixed step number (two calls give the
        same bits; the reference draws them unseeded).  User rows: the user tower (u2i) or the mean of the item rows over the
        consumed list in one `lr_spmm_csr_f32` (i2i; a user without items gets a zero row)."""
        net = self.net
        self.item_embeds = net.item_embeddings()
        if self.paradigm == "u2i":
            self.user_embeds = net.user_embeddings()
            return
        idx, ptr = flatten_lists([self.user_consumed.get(u, ()) for u in range(self.n_users)])
        lens = np.diff(ptr)
        val = np.repeat(1.0 / np.maximum(lens, 1), lens).astype(np.float32)
        ptr, idx, val = (torch.from_numpy(a).to(self.device) for a in (ptr, idx, val))
        self.user_embeds = ops.spmm_csr(ptr, idx, val, self.item_embeds)

    # ---- persistence ------------------------------------------------------------------------------------------------
    def variables_np(self):
        return {"sage/table": self.net.E.cpu().numpy(), "sage/params": self.net.P.cpu().numpy()}

    def optimizer_arrays(self):
        n = self.net
        out = {"opt::m": n.m.cpu().numpy(), "opt::v": n.v.cpu().numpy(), "opt::pm": n.pm.cpu().numpy(),
               "opt::pv": n.pv.cpu().numpy(), "opt::step": np.asarray(n.step, dtype=np.int64)}
        if n.vmax is not None:
            out["opt::vmax"], out["opt::pvmax"] = n.vmax.cpu().numpy(), n.pvmax.cpu().numpy()
        return out

    def load_variables_np(self, arrays):
        with torch.no_grad():
            if "sage/table" in arrays:
                self.net.E.copy_(torch.from_numpy(arrays["sage/table"]))
                self.net.P.copy_(torch.from_numpy(arrays["sage/params"]))

    def rebuild_model(self, path, model_name):
        raise NotImplementedError(f"{self.model_name} does not support retraining on merged data (`rebuild_model`)")
