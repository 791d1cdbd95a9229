"""`BPR` (`libreco/algorithms/bpr.py`): Bayesian personalised ranking by matrix factorisation, with the reference's
constructor, checks and checkpoints.  Both training modes run on the device (csrc/bpr.hip); there is no CPU engine.

`use_tf=False` replaces the loop of `_bpr.pyx` (sgd / momentum / adam over (user, positive, negative) triples).  The
reference walks the samples one after the other; here an epoch is cut into windows of `batch_size` consecutive samples
(DESIGN.md §7.4): every c = 1 / (1 + exp(d)) and every gradient of a window (the `reg` term too) comes from the tables as
they stood when the window began, and each touched row then takes the reference's optimiser step once per occurrence in
ascending sample order.  `batch_size=1` is the reference's loop at `num_threads=1`; two runs give the same bits.

`use_tf=True` (the default) replaces the TF graph: mean(-log sigmoid(d)) over the pairwise collators' batches, TF1 Adam on
the touched rows (or on every row with `dense_adam=True`).

Deliberate differences from the reference:
  (a) the window instead of the sample sequence (`use_tf=False`), see above;
  (b) the engine's negatives come from the device sampler (`ops.sample_negatives`, "unconsumed" rules, a pure function of
      (seed, epoch, position)), not from the reference's `mt19937` stream, which also never ends on a user who consumed
      every item;
  (c) `tf_sess_config` and `num_threads` are accepted and ignored; `reg` in the mini-batch mode needs `dense_adam=True`
      (an l2 on the whole variables moves every row every step);
  (d) under a process group of more than one rank `fit` raises;
  (e) `embed_size` above 255 raises `ValueError` (a row and its optimiser state live in one wave's registers).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from .. import ops
from ..bases import EmbedBase
from ..bases.base import hip_device
from ..evaluation.evaluate import print_metrics
from ..layers.embedding import glorot_uniform_
from ..layers.row_adam import REG_NEEDS_DENSE, NamedTables, RowAdam
from ..utils.device import to_device
from ..utils.initializers import truncated_normal
from ..utils.misc import time_block
from ..utils.validate import check_fitting, reg_config

OPTIMIZERS = ("sgd", "momentum", "adam")
N_STATES = {"sgd": 0, "momentum": 1, "adam": 2}
SAVED = {"user": "embedding/user_embeds_var", "item": "embedding/item_embeds_var", "bias": "embedding/item_bias_var"}


class BprNet(NamedTables):
    """The variables of `bpr.py:161-204` (`user_embeds_var [n_users, K]`, `item_embeds_var [n_items, K]`,
    `item_bias_var [n_items]`, glorot-uniform) with their Adam moments, and one training step on a batch of triples."""

    def __init__(self, n_users, n_items, K, lr, epsilon, reg, norm_embed, dense_adam, seed, device):
        self.n_users, self.n_items, self.K, self.device = int(n_users), int(n_items), int(K), device
        self.lr, self.epsilon, self.norm_embed = lr, epsilon, norm_embed
        # tf.keras.regularizers.l2(reg) on the variables adds 2 * reg * w to EVERY row's gradient each step
        # (tfops/configs.py:20-26): representable only with the dense TF1 update (layers/row_adam.py)
        self.adam = RowAdam(device, dense_adam, reg)
        gen = torch.Generator(device=device)
        gen.manual_seed(seed)
        tables = {}
        for name, shape in (("user", (self.n_users, K)), ("item", (self.n_items, K)), ("bias", (self.n_items,))):
            t = torch.empty((shape[0], shape[1] if len(shape) == 2 else 1), dtype=torch.float32, device=device)
            glorot_uniform_(t, shape, gen)
            tables[name] = t
        super().__init__(tables)

    def _grads(self, u, p, q):
        """(mean loss, gu [B, K], gi [2 B, K], gb [2 B]): item rows interleaved positive, negative per sample."""
        U, I, b = self.vars["user"], self.vars["item"], self.vars["bias"]
        B = u.numel()
        if not self.norm_embed:
            out = ops.bpr_triple_score(U, I, u, p, q, mode="grad", ibias=b.view(-1), gscale=1.0 / B)
            return out["loss"].sum() / B, out["gu"], out["gi"], out["gb"]
        # off the hot path: l2-normalised rows (`bpr.py:196-199`) and their backward as torch ops on the gathered rows
        items2 = torch.stack([p, q], 1).reshape(-1, 1).contiguous()
        ur = ops.embed_gather(U, u.view(-1, 1)).view(B, self.K).requires_grad_(True)
        ir = ops.embed_gather(I, items2).view(2 * B, self.K).requires_grad_(True)
        br = b.view(-1)[items2.view(-1).long()].requires_grad_(True)
        un, inn = F.normalize(ur, dim=1, eps=1e-12), F.normalize(ir, dim=1, eps=1e-12).view(B, 2, self.K)
        bb = br.view(B, 2)
        d = bb[:, 0] - bb[:, 1] + (un * (inn[:, 0] - inn[:, 1])).sum(1)
        loss = -F.logsigmoid(d).mean()                          # tfops/loss.py:23
        loss.backward()
        return loss.detach(), ur.grad.contiguous(), ir.grad.contiguous(), br.grad.contiguous()

    def train_step(self, users, pos, neg):
        self.step += 1
        u, p, q = (to_device(x, self.device).to(torch.int32).contiguous() for x in (users, pos, neg))
        loss, gu, gi, gb = self._grads(u, p, q)
        with torch.no_grad():
            hp = ops.adam_hp(self.lr, self.step, eps=self.epsilon, tf_style=True)
            seg_u = self.adam.segments("user", u, self.n_users)
            seg_i = self.adam.segments("item", torch.stack([p, q], 1).reshape(-1).contiguous(), self.n_items)
            V, M, S = self.vars, self.m, self.v
            self.adam.update(hp, seg_u, V["user"], M["user"], S["user"], gu)
            self.adam.update(hp, seg_i, V["item"], M["item"], S["item"], gi, lin=(V["bias"], M["bias"], S["bias"], gb))
        return loss


class BPR(EmbedBase):
    def __init__(self, task="ranking", data_info=None, loss_type="bpr", embed_size=16, norm_embed=False, n_epochs=20, lr=0.001,
                 lr_decay=False, epsilon=1e-5, reg=None, batch_size=256, sampler="random", num_neg=1, use_tf=True, seed=42,
                 lower_upper_bound=None, tf_sess_config=None, optimizer="adam", num_threads=1, device="cuda", dense_adam=False):
        super().__init__(task, data_info, embed_size, lower_upper_bound)
        assert task == "ranking", "BPR is only suitable for ranking"
        assert loss_type == "bpr", "BPR should use bpr loss"
        if optimizer not in OPTIMIZERS:
            raise ValueError("optimizer must be one of these: (`sgd`, `momentum`, `adam`)")
        if not isinstance(embed_size, (int, np.integer)) or not 1 <= embed_size <= 255:
            raise ValueError(f"BPR supports `embed_size` from 1 to 255 (a row and its optimiser state are held in one wave's "
                             f"registers), got {embed_size}")
        self.all_args = locals()
        self.loss_type, self.norm_embed = loss_type, norm_embed
        self.n_epochs, self.lr, self.lr_decay, self.epsilon = n_epochs, lr, lr_decay, epsilon
        self.reg = reg_config(reg) if use_tf else reg           # bpr.py:126
        self.batch_size, self.sampler, self.num_neg = batch_size, sampler, num_neg
        self.use_tf, self.seed, self.optimizer, self.num_threads = use_tf, seed, optimizer, num_threads
        self._device_arg, self.dense_adam = device, dense_adam
        if use_tf and self.reg and not dense_adam:
            raise ValueError(REG_NEEDS_DENSE)
        self.net = None
        self._U = self._I = None            # engine tables [n, K + 1]
        self._state = None                  # engine optimiser state {"u": [...], "i": [...]}, allocated in `fit`
        self._restored_state = None         # set by `rebuild_model`, taken by the next `fit`
        self._epochs_done = 0
        self.last_epoch_triples = None      # (users, positives, negatives) of the engine's last epoch, device int32

    # ---- model ----------------------------------------------------------------------------------
    def initial_tables(self):
        """The reference's draws (`bpr.py:143-159`): users, then items, from one generator seeded with `seed`; the user
        bias column is 1, the item bias column 0."""
        rng = np.random.default_rng(self.seed)
        K = self.embed_size
        u = truncated_normal(rng, shape=(self.n_users, K + 1), mean=0.0, scale=0.03)
        u[:, K] = 1.0
        i = truncated_normal(rng, shape=(self.n_items, K + 1), mean=0.0, scale=0.03)
        i[:, K] = 0.0
        return u, i

    def build_model(self):
        self.device = hip_device(self._device_arg)
        if self.use_tf:
            self.net = BprNet(self.n_users, self.n_items, self.embed_size, self.lr, self.epsilon, self.reg, self.norm_embed,
                              self.dense_adam, self.seed, self.device)
        else:
            u, i = self.initial_tables()
            self._U = torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32)).to(self.device)
            self._I = torch.from_numpy(np.ascontiguousarray(i, dtype=np.float32)).to(self.device)

    def _new_state(self):
        n = N_STATES[self.optimizer]
        return {"u": [torch.zeros_like(self._U) for _ in range(n)], "i": [torch.zeros_like(self._I) for _ in range(n)]}

    def train_on_batch(self, b):
        self.apply_lr_schedule()
        return self.net.train_step(b.queries, b.item_pairs[0], b.item_pairs[1])

    def set_embeddings(self):
        """`bpr.py:381-395`: [n, K + 1] tables, the user's last column 1.0, the item's last column its bias."""
        if self.use_tf:
            U, I, b = self.net.vars["user"], self.net.vars["item"], self.net.vars["bias"]
            if self.norm_embed:
                U, I = F.normalize(U, dim=1, eps=1e-12), F.normalize(I, dim=1, eps=1e-12)
            self.user_embeds = torch.cat([U, torch.ones_like(U[:, :1])], dim=1).contiguous()
            self.item_embeds = torch.cat([I, b.view(-1, 1)], dim=1).contiguous()
        else:
            self.user_embeds, self.item_embeds = self._U.clone(), self._I.clone()

    # ---- the engine -----------------------------------------------------------------------------
    def _consumed_csr(self, train_data):
        csr = train_data.sparse_interaction.sorted_indices()
        indptr = np.asarray(csr.indptr, dtype=np.int64)
        rp = np.full(self.n_users + 1, indptr[-1] if len(indptr) else 0, dtype=np.int64)
        rp[: len(indptr)] = indptr
        return (torch.from_numpy(rp).to(self.device),
                torch.from_numpy(np.asarray(csr.indices, dtype=np.int32)).to(self.device))

    def engine_window(self, users, pos, neg, items2, epoch, bufs, builders):
        """One window: score the triples against the tables as they stand, then the ordered update of the touched item rows
        (which reads the user rows, still untouched) and of the touched user rows (which reads only the stash)."""
        st = self._state
        out = ops.bpr_triple_score(self._U, self._I, users, pos, neg, mode="stash", want_loss=False, out=bufs)
        seg_i = builders[1].build(items2)
        seg_u = builders[0].build(users)
        reg = self.reg or 0.0
        ops.bpr_row_update(self.optimizer, self._I, seg_i, out["c"], self._U, self.lr, reg, epoch, *st["i"], users=users)
        ops.bpr_row_update(self.optimizer, self._U, seg_u, out["c"], out["gu"], self.lr, reg, epoch, *st["u"])

    def engine_epoch(self, users, pos, neg, epoch):
        """An epoch over the given device int32 triples in windows of `batch_size`."""
        n, W, D = users.numel(), int(self.batch_size), self.embed_size + 1
        W = max(1, min(W, n))
        bufs = {"c": torch.empty(W, dtype=torch.float32, device=self.device),
                "gu": torch.empty((W, D), dtype=torch.float32, device=self.device)}
        builders = (ops.SegmentBuilder(W, self.n_users, self.device), ops.SegmentBuilder(2 * W, self.n_items, self.device))
        items2 = torch.stack([pos, neg], 1).reshape(-1).contiguous()
        for a in range(0, n, W):
            self.engine_window(users[a:a + W], pos[a:a + W], neg[a:a + W], items2[2 * a:2 * (a + W)], epoch, bufs, builders)

    def _fit_engine(self, train_data, neg_sampling, verbose, shuffle, eval_data, metrics, k, eval_batch_size, eval_user_num):
        if self.batch_size < 1:
            raise ValueError("`batch_size` (the window) must be at least 1")
        # a second fit continues from the current tables with fresh optimiser state, as the reference's `_fit_cython`
        self._state = self._restored_state if self._restored_state is not None else self._new_state()
        self._restored_state = None
        cptr, cidx = self._consumed_csr(train_data)
        users_np = np.asarray(train_data.user_indices).astype(np.int32)
        items_np = np.asarray(train_data.item_indices).astype(np.int32)
        for epoch in range(1, self.n_epochs + 1):
            u_np, i_np = users_np, items_np
            if shuffle:                                       # `utils/misc.py:shuffle_data`: one permutation per epoch
                mask = self.data_info.np_rng.permutation(range(len(users_np)))
                u_np, i_np = users_np[mask], items_np[mask]
            users = torch.from_numpy(np.ascontiguousarray(u_np)).to(self.device)
            pos = torch.from_numpy(np.ascontiguousarray(i_np)).to(self.device)
            with time_block(f"Epoch {epoch}", verbose):
                neg = ops.sample_negatives(pos, 1, self.n_items, self.negative_seed(epoch), users=users, consumed_ptr=cptr,
                                           consumed_idx=cidx)
                self.engine_epoch(users, pos, neg, epoch)
                torch.cuda.synchronize(self.device)
            self.last_epoch_triples = (users, pos, neg)
            self._epochs_done = epoch
            if verbose > 1:
                self.prepare_for_eval()
                print_metrics(model=self, neg_sampling=neg_sampling, eval_data=eval_data, metrics=metrics,
                              eval_batch_size=eval_batch_size, k=k, sample_user_num=eval_user_num, seed=self.seed)
                print("=" * 30)

    def negative_seed(self, epoch):
        """The device sampler's seed of an epoch: a function of (`seed`, epoch) alone."""
        return (int(self.seed) * 1000003 + int(epoch)) & ((1 << 63) - 1)

    def fit(self, train_data, neg_sampling, verbose=1, shuffle=True, eval_data=None, metrics=None, k=10,
            eval_batch_size=8192, eval_user_num=None, num_workers=0):
        if self.use_tf:
            return super().fit(train_data, neg_sampling, verbose, shuffle, eval_data, metrics, k, eval_batch_size,
                               eval_user_num, num_workers)
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
        self._fit_engine(train_data, neg_sampling, verbose, shuffle, eval_data, metrics, k, eval_batch_size, eval_user_num)
        self.after_fit()

    # ---- persistence ----------------------------------------------------------------------------
    def variables_np(self):
        if self.use_tf:
            return {SAVED[k]: (v.view(-1) if k == "bias" else v).cpu().numpy() for k, v in self.net.vars.items()}
        return {"engine/user_table": self._U.cpu().numpy(), "engine/item_table": self._I.cpu().numpy()}

    def optimizer_arrays(self):
        if self.use_tf:
            return self.net.optimizer_arrays()
        out = {"opt::epochs": np.asarray(self._epochs_done, dtype=np.int64)}
        for side in "ui":
            for n, s in enumerate((self._state or {}).get(side, [])):
                out[f"opt::{side}{n}"] = s.cpu().numpy()
        return out

    def load_variables_np(self, arrays):
        with torch.no_grad():
            if self.use_tf:
                for k, name in SAVED.items():
                    if name in arrays:
                        self.net.vars[k].copy_(torch.from_numpy(arrays[name]).view_as(self.net.vars[k]))
            else:
                if "engine/user_table" in arrays:
                    self._U.copy_(torch.from_numpy(arrays["engine/user_table"]))
                    self._I.copy_(torch.from_numpy(arrays["engine/item_table"]))

    def rebuild_model(self, path, model_name, full_assign=True):
        """Retraining on merged data: a freshly built, larger model takes over the saved rows (ids keep their place, new ones
        are appended) and, with `full_assign`, their optimiser state; new ids keep fresh draws and zero state."""
        arrays, old = self._begin_rebuild(path, model_name)
        nu, ni = int(old.n_users), int(old.n_items)
        if self.use_tf:
            self.net.take_over(arrays, SAVED.get, lambda k: nu if k == "user" else ni, full_assign)
            return
        # the engine's tables and optimiser states under their saved names; the states have no moments of their own
        tables, n_old = {"engine/user_table": self._U, "engine/item_table": self._I}, {"engine/user_table": nu, "engine/item_table": ni}
        if full_assign and all(f"opt::{s}{n}" in arrays for s in "ui" for n in range(N_STATES[self.optimizer])):
            self._restored_state = self._new_state()
            for side, n_side in (("u", nu), ("i", ni)):
                for n, s in enumerate(self._restored_state[side]):
                    tables[f"opt::{side}{n}"], n_old[f"opt::{side}{n}"] = s, n_side
        # `full_assign` above decides whether the states are among `tables`; `take_over`'s own flag only concerns the m / v
        # moments and the step count, which this holder does not have
        NamedTables(tables, m={}, v={}).take_over(arrays, lambda k: k, n_old.get, False)
