"""GraphSage (`libreco/algorithms/torch_modules/graphsage_module.py:13-140`, there `GraphSageModel`) on the HIP path
(csrc/sage.hip).

* One stacked table  E = [sparse_embeds | dense_embeds | item_embeds | user_embeds (u2i)]  and one flat parameter buffer
  P = [item pack | user pack (u2i)]: a pack is proj W^T, proj b, then per layer W^T, b (`ops.sage_param_floats`).
* A node's input is T slots (row of E, scale): its sparse-feature rows, its dense rows scaled by the node's dense values, its id
  row.  The slot tables of all items (and users) are built once and indexed by the sampled ids.
* The tower is `lr_sage_fwd_f32` / `lr_sage_bwd_f32` (one launch each per tower batch; nothing but repr is kept between them).
  With `fused=False`, or outside `ops.sage_supported`, the same parameters run composed from torch ops under autograd, on the
  same sampled ids and the same dropout flags (`lr_sage_dropout_u8`).
* The slot-row gradients reach E through `Segments` / `embed_segment_sum`; E and P take torch's dense Adam
  (`lr_adam_dense_f32`, `weight_decay = reg`, optional AMSGrad), every row decaying its moments each step.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from .. import ops

INFERENCE_STEP = 1 << 40          # the step number of the neighbour draws behind the exported item embeddings


def xavier_uniform(rng, fan_out, fan_in, gain=1.0):
    bound = gain * math.sqrt(6.0 / (fan_in + fan_out))
    return ((rng.random((fan_out, fan_in)) * 2.0 - 1.0) * bound).astype(np.float32)


def cumulative_table(weights: np.ndarray) -> np.ndarray:
    """int64 [n]: the cumulative weights scaled to 2^32; a draw r picks the first entry with cum > r."""
    w = np.where(np.isfinite(weights) & (weights > 0), weights, 0.0).astype(np.float64)
    cs = np.cumsum(w)
    if len(cs) == 0 or cs[-1] <= 0:
        return np.full(len(w), 1 << 32, dtype=np.int64)
    cum = np.floor(cs / cs[-1] * 4294967296.0).astype(np.int64)
    cum[np.flatnonzero(w > 0)[-1]:] = 1 << 32
    return cum


class _Side:
    """The slot tables of one node family: rows int32 [n + 1, T] and scale f32 [n + 1, T] (or None); row n is the node
    outside the family: rows of -1."""

    def __init__(self, n, id_off, sparse, sparse_off, dense, dense_cols, dense_off, device):
        cols, scales = [], []
        if sparse is not None:
            cols.append(np.asarray(sparse[:n], dtype=np.int64) + sparse_off)
            scales.append(np.ones((n, sparse.shape[1]), dtype=np.float32))
        if dense is not None:
            cols.append(np.broadcast_to(np.asarray(dense_cols, dtype=np.int64) + dense_off, (n, len(dense_cols))))
            scales.append(np.asarray(dense[:n], dtype=np.float32))
        cols.append(np.arange(n, dtype=np.int64)[:, None] + id_off)
        scales.append(np.ones((n, 1), dtype=np.float32))
        rows = np.concatenate(cols, axis=1)
        rows = np.concatenate([rows, np.full((1, rows.shape[1]), -1)]).astype(np.int32)
        self.n, self.T = n, rows.shape[1]
        self.rows = torch.from_numpy(rows).to(device)
        self.scale = None
        if dense is not None:
            sc = np.concatenate([np.concatenate(scales, axis=1), np.zeros((1, self.T), dtype=np.float32)])
            self.scale = torch.from_numpy(np.ascontiguousarray(sc)).to(device)

    def slots(self, ids: torch.Tensor):
        i = ids.long()
        i = torch.where((i >= 0) & (i < self.n), i, torch.full_like(i, self.n))
        return self.rows[i].contiguous(), (None if self.scale is None else self.scale[i].contiguous())


class _Tower:
    """One tower batch between its forward and its backward."""

    def __init__(self, net, rows, scale, pack, L, n, step, train, fused):
        self.net, self.rows, self.scale, self.pack, self.L, self.n, self.step, self.train = net, rows, scale, pack, L, n, step, train
        self.fused = fused
        p = net.dropout if train else 0.0
        if fused:
            self.repr = ops.sage_fwd(net.E, rows, scale, net.P[pack], L, n, p, net.seed, step, train)
        else:
            self._x = ops.embed_gather(net.E, rows.clamp(min=0).contiguous())
            self._x.requires_grad_(train)
            self._p = net.P[pack].detach().clone().requires_grad_(train)
            with torch.set_grad_enabled(train):
                self._out = net.composed(self._x, rows, scale, self._p, L, n, p, step)
            self.repr = self._out.detach()

    def backward(self, grepr):
        """-> (grow [nodes, T, K], gparams of the pack)"""
        net = self.net
        if self.fused:
            grow, gp, _ = ops.sage_bwd(net.E, self.rows, self.scale, net.P[self.pack], self.L, self.n, grepr.contiguous(),
                                       net.dropout, net.seed, self.step)
            return grow, gp
        self._out.backward(grepr)
        return self._x.grad, self._p.grad


class SageNet:
    def __init__(self, paradigm, n_users, n_items, embed_size, num_layers, num_neighbors, dropout_rate, device, graph,
                 n_sparse_rows=0, n_dense_rows=0, item_sparse=None, item_dense=None, item_dense_cols=(), user_sparse=None,
                 user_dense=None, user_dense_cols=(), seed=42, lr=1e-3, epsilon=1e-8, reg=None, amsgrad=False, margin=1.0,
                 fused=True):
        self.paradigm, self.n_users, self.n_items, self.K = paradigm, n_users, n_items, int(embed_size)
        self.L, self.n, self.dropout = int(num_layers), int(num_neighbors), float(dropout_rate or 0.0)
        self.device, self.graph, self.seed = device, graph, int(seed)
        self.lr, self.epsilon, self.reg, self.margin = lr, epsilon, float(reg or 0.0), margin
        self._want_fused = bool(fused)
        K, rng = self.K, np.random.default_rng(seed)
        u2i = paradigm == "u2i"
        # the stacked table
        self.sparse_off, self.dense_off = 0, n_sparse_rows
        self.item_off = n_sparse_rows + n_dense_rows
        self.user_off = self.item_off + n_items
        sizes = [n_sparse_rows, n_dense_rows, n_items] + ([n_users] if u2i else [])
        self.E = torch.from_numpy(np.concatenate([xavier_uniform(rng, v, K) for v in sizes if v])).to(device).contiguous()
        self.items = _Side(n_items, self.item_off, item_sparse, self.sparse_off, item_dense, item_dense_cols, self.dense_off, device)
        self.users = (_Side(n_users, self.user_off, user_sparse, self.sparse_off, user_dense, user_dense_cols, self.dense_off,
                            device) if u2i else None)
        self._init_packs(rng, u2i)
        self.m, self.v = torch.zeros_like(self.E), torch.zeros_like(self.E)
        self.pm, self.pv = torch.zeros_like(self.P), torch.zeros_like(self.P)
        self.vmax = torch.zeros_like(self.E) if amsgrad else None
        self.pvmax = torch.zeros_like(self.P) if amsgrad else None
        self._row_slot = torch.full((self.E.shape[0],), -1, dtype=torch.int32, device=device)
        self.step = 0

    def _init_packs(self, rng, u2i):
        """The parameter packs `P`, their slices and whether each tower runs fused (a subclass with other towers overrides it)."""
        K, device = self.K, self.device
        Ti = self.items.T
        relu_gain = math.sqrt(2.0)
        pack = [xavier_uniform(rng, K, Ti * K).T.reshape(-1), np.zeros(K, dtype=np.float32)]
        for l in range(self.L):
            pack += [xavier_uniform(rng, K, 2 * K, 1.0 if l == self.L - 1 else relu_gain).T.reshape(-1), np.zeros(K, dtype=np.float32)]
        n_item_pack = sum(len(p) for p in pack)
        self.item_pack = slice(0, n_item_pack)
        self.user_pack = None
        if u2i:
            Tu = self.users.T
            pack += [xavier_uniform(rng, K, Tu * K).T.reshape(-1), np.zeros(K, dtype=np.float32)]
            self.user_pack = slice(n_item_pack, n_item_pack + Tu * K * K + K)
        self.P = torch.from_numpy(np.concatenate(pack).astype(np.float32)).to(device).contiguous()
        self.item_fused = self._want_fused and ops.sage_supported(K, Ti, self.L, self.n)
        self.user_fused = self._want_fused and u2i and ops.sage_supported(K, self.users.T, 0, 1)

    # ---- sampling -----------------------------------------------------------------------------
    def tree_ids(self, targets: torch.Tensor, step: int) -> torch.Tensor:
        """The node ids of all levels of the targets' trees, level-major (int32 [B N])."""
        levels, cur = [targets], targets
        for level in range(self.L):
            cur = ops.sage_neighbors(cur, self.graph, self.n, self.seed, step, level).view(-1)
            levels.append(cur)
        return torch.cat(levels) if self.L else targets

    # ---- the tower, composed from torch ops ---------------------------------------------------
    def composed(self, x, rows, scale, params, L, n, p, step):
        """The tower of csrc/sage.hip from torch ops: `x` [nodes, T, K] the gathered slot rows (rows < 0 hold garbage)."""
        K, T = self.K, rows.shape[1]
        x = x * (rows >= 0).unsqueeze(-1)
        if scale is not None:
            x = x * scale.unsqueeze(-1)
        o = T * K * K
        h0 = x.flatten(1) @ params[:o].view(T * K, K) + params[o:o + K]
        o += K
        B = rows.shape[0] // ops.sage_tree_nodes(L, n)
        h, at = [], 0
        for k in range(L + 1):
            cnt = B * (n ** k if L else 1)
            h.append(h0[at:at + cnt])
            at += cnt
        inv_keep = float(np.float32(1.0 / (1.0 - p))) if p > 0 else 1.0

        def drop(t, layer, level, role):
            if p <= 0:
                return t
            keep = ops.sage_dropout_mask(t.shape[0], K, p, self.seed, step, layer, level, role, t.device)
            return torch.where(keep.bool(), t * inv_keep, torch.zeros_like(t))

        for l in range(L):
            Wt, b = params[o:o + 2 * K * K].view(2 * K, K), params[o + 2 * K * K:o + 2 * K * K + K]
            o += 2 * K * K + K
            nxt = []
            for k in range(L - l):
                zs = drop(h[k], l, k, 0)
                zn = drop(h[k + 1], l, k + 1, 1).view(-1, n, K).sum(1) / n
                out = torch.cat([zs, zn], dim=1) @ Wt + b
                nxt.append(F.relu(out) if l < L - 1 else out)
            h = nxt
        return h[0]

    def item_tower(self, targets, step, train):
        rows, scale = self.items.slots(self.tree_ids(targets, step))
        return _Tower(self, rows, scale, self.item_pack, self.L, self.n, step, train, self.item_fused)

    def i2i_tower(self, queries, items_pos, items_neg, step):
        """The three item towers of an i2i step as one batch."""
        return self.item_tower(torch.cat([queries, items_pos, items_neg]).contiguous(), step, True)

    def user_tower(self, users, step, train):
        rows, scale = self.users.slots(users)
        return _Tower(self, rows, scale, self.user_pack, 0, 1, step, train, self.user_fused)

    # ---- losses (`training/torch_trainer.py:237-282`, `torchops/loss.py`) ----------------------
    def _loss(self, loss_type, q, pos, neg):
        repeat = loss_type in ("bpr", "max_margin")
        f = len(neg) // len(pos)
        ps = (q * pos).sum(1)
        if f == 1:
            ns = (q * neg).sum(1)
        else:
            ns = torch.einsum("ik,ijk->ij", q, neg.view(len(pos), f, -1)).reshape(-1)
            if repeat:
                ps = ps.repeat_interleave(f)
        if loss_type in ("cross_entropy", "focal"):
            logits = torch.cat([ps, ns])
            lab = torch.cat([torch.ones_like(ps), torch.zeros_like(ns)])
            each = F.binary_cross_entropy_with_logits(logits, lab, reduction="none")
            if loss_type == "focal":
                prob = torch.sigmoid(logits)
                p_t = lab * prob + (1 - lab) * (1 - prob)
                each = (lab * 0.25 + (1 - lab) * 0.75) * (1.0 - p_t) ** 2.0 * each
            return each.mean() if self.paradigm == "u2i" else each.sum()
        if loss_type == "bpr":
            return -F.logsigmoid(ps - ns).mean()
        return F.margin_ranking_loss(ps, ns, torch.ones_like(ps), margin=self.margin)

    # ---- training -----------------------------------------------------------------------------
    def train_step(self, loss_type, queries, items_pos, items_neg, lr=None):
        """One optimiser step on int32 device ids: `queries` are users (u2i) or items (i2i), `items_neg` holds a whole number
        of negatives per positive.  The three item towers run as one batch."""
        self.step += 1
        step, nq, npos = self.step, queries.numel(), items_pos.numel()
        if self.paradigm == "u2i":
            qt = self.user_tower(queries, step, True)
            it = self.item_tower(torch.cat([items_pos, items_neg]).contiguous(), step, True)
            q = qt.repr.clone().requires_grad_(True)
            r = it.repr.clone().requires_grad_(True)
            loss = self._loss(loss_type, q, r[:npos], r[npos:])
        else:
            qt = None
            it = self.i2i_tower(queries, items_pos, items_neg, step)
            r = it.repr.clone().requires_grad_(True)
            loss = self._loss(loss_type, r[:nq], r[nq:nq + npos], r[nq + npos:])
        loss.backward()
        with torch.no_grad():
            gP = torch.zeros_like(self.P)
            grow, gp = it.backward(r.grad)
            gP[self.item_pack] = gp
            idx, grads = [it.rows.reshape(-1)], [grow.reshape(-1, self.K)]
            if qt is not None:
                grow_u, gp_u = qt.backward(q.grad)
                gP[self.user_pack] = gp_u
                idx.append(qt.rows.reshape(-1))
                grads.append(grow_u.reshape(-1, self.K))
            idx, grads = torch.cat(idx).contiguous(), torch.cat(grads).contiguous()
            hp = ops.adam_hp(self.lr if lr is None else lr, self.step, eps=self.epsilon, weight_decay=self.reg, tf_style=False)
            seg = ops.build_segments(idx, self.E.shape[0])
            gsum = ops.embed_segment_sum(grads, seg)
            ops.adam_dense(self.E, self.m, self.v, hp, grows=gsum, seg=seg, row_slot=self._row_slot, vmax=self.vmax)
            ops.adam_dense(self.P.view(-1, 1), self.pm.view(-1, 1), self.pv.view(-1, 1), hp, grows=gP.view(-1, 1),
                           vmax=None if self.pvmax is None else self.pvmax.view(-1, 1))
        return loss.detach()

    # ---- export -------------------------------------------------------------------------------
    @torch.no_grad()
    def item_embeddings(self, batch=4096):
        out = []
        for a in range(0, self.n_items, batch):
            ids = torch.arange(a, min(a + batch, self.n_items), dtype=torch.int32, device=self.device)
            out.append(self.item_tower(ids, INFERENCE_STEP + a // batch, False).repr)
        return torch.cat(out).contiguous()

    @torch.no_grad()
    def user_embeddings(self, batch=8192):
        out = []
        for a in range(0, self.n_users, batch):
            ids = torch.arange(a, min(a + batch, self.n_users), dtype=torch.int32, device=self.device)
            out.append(self.user_tower(ids, INFERENCE_STEP, False).repr)
        return torch.cat(out).contiguous()
