"""`SVD` (`libreco/algorithms/svd.py`): the biased matrix factorisation s = bu[u] + bi[i] + <p_u, q_i> for the `rating`
(mean squared error) and `ranking` (cross entropy or focal loss) tasks, with the reference's constructor, checks and
checkpoints.  `SvdNet` is also the net of `SVDpp` (algorithms/svdpp.py), where the user vector is the pooled
z_u = p_u + |N(u)|^-1/2 sum_{j in N(u)} y_j.  Score, loss and gradients run on the device (csrc/svd.hip).

Deliberate differences from the reference:
  (a) the default optimiser is TF1-style Adam on the rows a batch touches; `dense_adam=True` is the reference's TF1
      semantics (every row of every variable decays and moves every step).  `reg` needs it: an l2 on the whole variables
      moves every row every step;
  (b) SVD++ pools the histories of the batch's distinct users, not of all users, in a training step (the export pools all);
  (c) `tf_sess_config` is accepted and ignored;
  (d) `embed_size` above the library's limit (`lr_svd_supported`: 512) raises `ValueError` (a row lives in one wave's
      registers);
  (e) under a process group of more than one rank `fit` raises.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from .. import ops
from ..bases import EmbedBase
from ..bases.base import hip_device
from ..layers.embedding import glorot_uniform_
from ..layers.row_adam import REG_NEEDS_DENSE, NamedTables, RowAdam
from ..utils.device import to_device
from ..utils.validate import reg_config

VAR_KEYS = ("bu", "pu", "bi", "qi", "yj")


def max_embed_size():
    """The widest row the kernels of csrc/svd.hip take, asked of the library (`lr_svd_supported`): the one definition."""
    lo, hi = 1, 2
    while ops.svd_supported(hi):
        lo, hi = hi, hi * 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ops.svd_supported(mid) else (lo, mid)
    return lo


def check_embed_size(name, embed_size):
    if not isinstance(embed_size, (int, np.integer)) or embed_size < 1 or not ops.svd_supported(embed_size):
        raise ValueError(f"{name} supports `embed_size` from 1 to {max_embed_size()} (a row is held in one wave's registers), "
                         f"got {embed_size}")


def check_loss_type(task, loss_type):
    if task == "ranking" and loss_type not in ("cross_entropy", "focal"):        # fm.py:29
        raise ValueError(f"unsupported `loss_type`: {loss_type}")


def history_csr(user_consumed, n_users, recent_num):
    """`svdpp.py:178-188`: the last `recent_num` consumed items of every user (all of them for None), repeats kept, as
    (int64 [n_users + 1], int32 [nnz])."""
    assert recent_num is None or (isinstance(recent_num, int) and recent_num > 0), "`recent_num` must be None or positive int"
    ptr = np.zeros(n_users + 1, dtype=np.int64)
    parts = []
    for u in range(n_users):
        items = user_consumed.get(u, ()) if hasattr(user_consumed, "get") else user_consumed[u]
        u_data = items if recent_num is None else items[-recent_num:]
        ptr[u + 1] = ptr[u] + len(u_data)
        parts.append(np.asarray(u_data, dtype=np.int32))
    idx = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)
    return ptr, np.ascontiguousarray(idx, dtype=np.int32)


class SvdNet(NamedTables):
    """The variables of `svd.py:109-136` / `svdpp.py:108-131,198-213` (`bu [n_users]`, `bi [n_items]` zero; `pu`, `qi` and
    for SVD++ `yj [n_items, K]` glorot-uniform) with their Adam moments, and one training step on a pointwise batch."""

    def __init__(self, n_users, n_items, K, lr, epsilon, reg, norm_embed, dense_adam, seed, device, loss, with_history=False):
        self.n_users, self.n_items, self.K, self.device = int(n_users), int(n_items), int(K), device
        self.lr, self.epsilon, self.norm_embed = lr, epsilon, norm_embed
        self.loss, self.with_history = loss, with_history
        # tf.keras.regularizers.l2(reg) on the variables adds 2 * reg * w to EVERY row's gradient each step
        # (tfops/configs.py:20-26): representable only with the dense TF1 update (layers/row_adam.py)
        self.adam = RowAdam(device, dense_adam, reg)
        gen = torch.Generator(device=device)
        gen.manual_seed(seed)
        tables = {}
        for name in VAR_KEYS if with_history else VAR_KEYS[:4]:
            n = self.n_users if name in ("bu", "pu") else self.n_items
            if name in ("bu", "bi"):                                        # tf.zeros_initializer
                tables[name] = torch.zeros((n, 1), dtype=torch.float32, device=device)
            else:
                t = torch.empty((n, self.K), dtype=torch.float32, device=device)
                glorot_uniform_(t, (n, self.K), gen)
                tables[name] = t
        super().__init__(tables)
        self.hist_ptr = self.hist_idx = None

    # ---- the histories of SVD++ -----------------------------------------------------------------
    def set_history(self, ptr, idx):
        self.hist_ptr = torch.from_numpy(np.ascontiguousarray(ptr, dtype=np.int64)).to(self.device)
        self.hist_idx = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(self.device)
        if self.hist_idx.numel() == 0:          # a valid pointer for the kernels
            self.hist_idx = torch.zeros(1, dtype=torch.int32, device=self.device)[:0]

    def pooled_all(self):
        """z over all users (`svdpp.py:196-214`), the export."""
        return ops.svdpp_pool(self.vars["pu"], self.vars["yj"], self.hist_ptr, self.hist_idx)

    def _entries(self, seg_u, n):
        """The concatenated history entries of the batch's distinct users: (y row, user slot) per entry.  Index plumbing on
        torch ops; the entry count is the step's one host read."""
        ar = torch.arange(n, device=self.device)
        valid = ar < seg_u.n_seg.long()
        rows = torch.where(valid, seg_u.rows[:n].long(), torch.zeros_like(ar)).clamp_(0, self.n_users - 1)
        begin = self.hist_ptr[rows]
        lens = torch.where(valid, self.hist_ptr[rows + 1] - begin, torch.zeros_like(begin))
        end = torch.cumsum(lens, 0)
        E = int(end[-1])
        if E == 0:
            return None, None
        ent_slot = torch.repeat_interleave(ar, lens, output_size=E)
        ent_pos = torch.arange(E, device=self.device) - (end - lens)[ent_slot] + begin[ent_slot]
        return self.hist_idx[ent_pos].contiguous(), ent_slot.to(torch.int32).contiguous()

    # ---- one step ---------------------------------------------------------------------------------
    def _norm_grads(self, u, i, y):
        """Off the hot path: l2-normalised rows (`svd.py:138-141`) and their backward as torch ops on the gathered rows."""
        B = u.numel()
        pr = ops.embed_gather(self.vars["pu"], u.view(-1, 1)).view(B, self.K).requires_grad_(True)
        qr = ops.embed_gather(self.vars["qi"], i.view(-1, 1)).view(B, self.K).requires_grad_(True)
        bur = self.vars["bu"].view(-1)[u.long()].requires_grad_(True)
        bir = self.vars["bi"].view(-1)[i.long()].requires_grad_(True)
        s = bur + bir + (F.normalize(pr, dim=1, eps=1e-12) * F.normalize(qr, dim=1, eps=1e-12)).sum(1)
        if self.loss == "mse":
            loss = F.mse_loss(s, y)
        else:
            bce = F.binary_cross_entropy_with_logits(s, y, reduction="none")
            if self.loss == "focal":                                        # tfops/loss.py:56-62
                p = torch.sigmoid(s)
                bce = (y * 0.25 + (1 - y) * 0.75) * (1 - (y * p + (1 - y) * (1 - p))) ** 2.0 * bce
            loss = bce.mean()
        loss.backward()
        return loss.detach(), pr.grad.contiguous(), qr.grad.contiguous(), bur.grad.contiguous(), bir.grad.contiguous()

    def train_step(self, users, items, labels):
        self.step += 1
        u, i = (to_device(x, self.device).to(torch.int32).contiguous() for x in (users, items))
        y = to_device(labels, self.device).to(torch.float32).contiguous()
        B = u.numel()
        V, M, S = self.vars, self.m, self.v
        with torch.no_grad():
            seg_u = self.adam.segments("user", u, self.n_users, self.with_history)      # (with the positions' run numbers)
        gbi = None
        if self.with_history:
            with torch.no_grad():
                z, scale = ops.svdpp_pool(V["pu"], V["yj"], self.hist_ptr, self.hist_idx, rows=seg_u.rows, n_rows_dev=seg_u.n_seg,
                                          n_rows=B, want_scale=True)
                out = ops.mf_score(z, V["qi"], V["bu"], V["bi"], u, i, y, self.loss, xidx=seg_u.slots, mode="grad",
                                   gscale=1.0 / B)
        elif self.norm_embed:
            loss, gx, gq, gbu, gbi = self._norm_grads(u, i, y)
            out = None
        else:
            with torch.no_grad():
                out = ops.mf_score(V["pu"], V["qi"], V["bu"], V["bi"], u, i, y, self.loss, mode="grad", gscale=1.0 / B)
        if out is not None:
            loss, gx, gq, gbu = out["loss"].sum() / B, out["gx"], out["gq"], out["g"]
            gbi = gbu
        with torch.no_grad():
            hp = ops.adam_hp(self.lr, self.step, eps=self.epsilon, tf_style=True)
            if self.with_history:           # the y side first: it reads the per-user sums of this step's gx
                ent_idx, ent_slot = self._entries(seg_u, B)
                if ent_idx is not None:
                    G = ops.embed_segment_sum(gx, seg_u)
                    seg_y = self.adam.segments("hist", ent_idx, self.n_items)
                    if self.adam.dense:     # the per-row sums come from the history kernel, not from `embed_segment_sum`
                        grows = ops.svdpp_hist_grad(G, scale, ent_slot, seg_y)
                        ops.adam_dense(V["yj"], M["yj"], S["yj"], hp, grows=grows, seg=seg_y, row_slot=self.adam.row_slot(V["yj"]),
                                       l2=self.adam.l2)
                    else:
                        ops.svdpp_hist_grad(G, scale, ent_slot, seg_y, Y=V["yj"], m=M["yj"], v=S["yj"], hp=hp)
                elif self.adam.dense:
                    self.adam.update_all_rows(hp, V["yj"], M["yj"], S["yj"])
            seg_i = self.adam.segments("item", i, self.n_items)
            self.adam.update(hp, seg_u, V["pu"], M["pu"], S["pu"], gx, lin=(V["bu"], M["bu"], S["bu"], gbu))
            self.adam.update(hp, seg_i, V["qi"], M["qi"], S["qi"], gq, lin=(V["bi"], M["bi"], S["bi"], gbi))
        return loss


class SvdBase(EmbedBase):
    """What `SVD` and `SVDpp` share: the step, the export, checkpoints and retraining."""
    with_history = False
    default_full_assign = True

    def _init_common(self, loss_type, n_epochs, lr, lr_decay, epsilon, reg, batch_size, sampler, num_neg, seed, device, dense_adam):
        check_embed_size(self.model_name, self.embed_size)
        check_loss_type(self.task, loss_type)
        self.loss_type = loss_type
        self.n_epochs, self.lr, self.lr_decay, self.epsilon = n_epochs, lr, lr_decay, epsilon
        self.reg = reg_config(reg)
        self.batch_size, self.sampler, self.num_neg, self.seed = batch_size, sampler, num_neg, seed
        self._device_arg, self.dense_adam = device, dense_adam
        if self.reg and not dense_adam:
            raise ValueError(REG_NEEDS_DENSE)
        self.net = None

    def build_model(self):
        self.device = hip_device(self._device_arg)
        self.net = SvdNet(self.n_users, self.n_items, self.embed_size, self.lr, self.epsilon, self.reg,
                          getattr(self, "norm_embed", False), self.dense_adam, self.seed, self.device,
                          "mse" if self.task == "rating" else self.loss_type, with_history=self.with_history)

    def train_on_batch(self, b):
        self.apply_lr_schedule()
        return self.net.train_step(b.users, b.items, b.labels)

    def _user_vectors(self):
        p = self.net.vars["pu"]
        return F.normalize(p, dim=1, eps=1e-12) if getattr(self, "norm_embed", False) else p

    def set_embeddings(self):
        """`svd.py:146-160`, `svdpp.py:164-176`: user rows [x | bu | 1], item rows [q | 1 | bi]."""
        V = self.net.vars
        x, q = self._user_vectors(), V["qi"]
        if getattr(self, "norm_embed", False):
            q = F.normalize(q, dim=1, eps=1e-12)
        self.user_embeds = torch.cat([x, V["bu"].view(-1, 1), torch.ones_like(x[:, :1])], dim=1).contiguous()
        self.item_embeds = torch.cat([q, torch.ones_like(q[:, :1]), V["bi"].view(-1, 1)], dim=1).contiguous()

    # ---- persistence ----------------------------------------------------------------------------
    def variables_np(self):
        return {f"embedding/{k}_var": (v.view(-1) if k in ("bu", "bi") else v).cpu().numpy() for k, v in self.net.vars.items()}

    def optimizer_arrays(self):
        return self.net.optimizer_arrays()

    def load_variables_np(self, arrays):
        with torch.no_grad():
            for k, var in self.net.vars.items():
                if f"embedding/{k}_var" in arrays:
                    var.copy_(torch.from_numpy(arrays[f"embedding/{k}_var"]).view_as(var))

    def _rebuild(self, path, model_name, full_assign):
        """Retraining on merged data: a freshly built, larger model takes over the saved rows (ids keep their place, new ones
        are appended) and, with `full_assign`, their optimiser state; new ids keep fresh draws and zero state."""
        arrays, old = self._begin_rebuild(path, model_name)
        self.net.take_over(arrays, lambda k: f"embedding/{k}_var",
                           lambda k: int(old.n_users if k in ("bu", "pu") else old.n_items), full_assign)


class SVD(SvdBase):
    def __init__(self, task, data_info, loss_type="cross_entropy", embed_size=16, norm_embed=False, n_epochs=20, lr=0.001,
                 lr_decay=False, epsilon=1e-5, reg=None, batch_size=256, sampler="random", num_neg=1, seed=42,
                 lower_upper_bound=None, tf_sess_config=None, device="cuda", dense_adam=False):
        super().__init__(task, data_info, embed_size, lower_upper_bound)
        self.all_args = locals()
        self.norm_embed = norm_embed
        self._init_common(loss_type, n_epochs, lr, lr_decay, epsilon, reg, batch_size, sampler, num_neg, seed, device, dense_adam)

    def rebuild_model(self, path, model_name, full_assign=True):
        self._rebuild(path, model_name, full_assign)
