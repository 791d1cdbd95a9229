"""PinSage (`libreco/algorithms/torch_modules/pinsage_module.py:8-96`, there `PinSageModel`) on the HIP path
(csrc/pinsage.hip), built on `SageNet`: the stacked table, the slot tables, the losses, the Adam path and the
export loop are its.

* A node's neighbours are the most visited items of short random walks (`lr_pinsage_neighbors_i32`), at most `num_neighbors`
  of them; the trees keep GraphSage's exact fan-out, an unused child slot holding id -1 (slot rows of -1) and weight 0.  The
  importance weights are `ops.pinsage_weights` of the visit counts.
* A pack is proj W^T, proj b, per layer Q^T, bq, W^T, bw, then the head G1^T, b1, G2^T (`ops.pinsage_param_floats`); the user
  tower of u2i is the pack of zero layers (proj, U1, U2).
* With `remove_edges` (i2i) the query block of a step excludes its positive from the neighbours of the query item, wherever the
  query item stands in its own tree; the positives', the negatives' and the exported trees exclude nothing.
* The towers are `lr_pinsage_fwd_f32` / `lr_pinsage_bwd_f32`; with `fused=False`, or outside `ops.pinsage_supported`, the same
  parameters run composed from torch ops under autograd on the same ids, weights and dropout flags.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from .. import ops
from .sage_net import SageNet, xavier_uniform


class _PinTower:
    """One tower batch between its forward and its backward."""

    def __init__(self, net, rows, scale, weights, pack, L, n, step, train, fused):
        self.net, self.rows, self.scale, self.weights, self.pack = net, rows, scale, weights, pack
        self.L, self.n, self.step, self.train, self.fused = L, n, step, train, fused
        p = net.dropout if train else 0.0
        if fused:
            self.repr = ops.pinsage_fwd(net.E, rows, scale, weights, net.P[pack], L, n, p, net.seed, step, train)
        else:
            self._x = ops.embed_gather(net.E, rows.clamp(min=0).contiguous())
            self._x.requires_grad_(train)
            self._p = net.P[pack].detach().clone().requires_grad_(train)
            with torch.set_grad_enabled(train):
                self._out = net.composed(self._x, rows, scale, weights, self._p, L, n, p, step)
            self.repr = self._out.detach()

    def backward(self, grepr):
        """-> (grow [nodes, T, K], gparams of the pack)"""
        net = self.net
        if self.fused:
            grow, gp, _ = ops.pinsage_bwd(net.E, self.rows, self.scale, self.weights, net.P[self.pack], self.L, self.n,
                                          grepr.contiguous(), net.dropout, net.seed, self.step)
            return grow, gp
        self._out.backward(grepr)
        return self._x.grad, self._p.grad


class PinSageNet(SageNet):
    def __init__(self, *args, num_walks=10, neighbor_walk_len=2, termination_prob=0.5, remove_edges=False, **kwargs):
        self.num_walks, self.walk_len = int(num_walks), int(neighbor_walk_len)
        self.termination_prob, self.remove_edges = float(termination_prob), bool(remove_edges)
        super().__init__(*args, **kwargs)

    def _init_packs(self, rng, u2i):
        K, gain = self.K, math.sqrt(2.0)
        zeros = lambda: np.zeros(K, dtype=np.float32)  # noqa: E731
        lin = lambda fan_in, g=gain: xavier_uniform(rng, K, fan_in, g).T.reshape(-1)  # noqa: E731
        Ti = self.items.T
        pack = [lin(Ti * K), zeros()]
        for _ in range(self.L):
            pack += [lin(K), zeros(), lin(2 * K), zeros()]
        pack += [lin(K), zeros(), lin(K, 1.0)]
        n_item_pack = sum(len(p) for p in pack)
        self.item_pack, self.user_pack = slice(0, n_item_pack), None
        if u2i:
            pack += [lin(self.users.T * K), zeros(), lin(K), zeros(), lin(K, 1.0)]
            self.user_pack = slice(n_item_pack, sum(len(p) for p in pack))
        self.P = torch.from_numpy(np.concatenate(pack).astype(np.float32)).to(self.device).contiguous()
        self.item_fused = self._want_fused and ops.pinsage_supported(K, Ti, self.L, self.n)
        self.user_fused = self._want_fused and u2i and ops.pinsage_supported(K, self.users.T, 0, 1)

    # ---- sampling -----------------------------------------------------------------------------
    def tree(self, targets: torch.Tensor, step: int, exclude: torch.Tensor = None):
        """(ids int32 [B N], weights f32 [B (N - 1)] or None) of the targets' trees, level-major; `exclude` int32 [B] (-1: nothing)
        is removed from the neighbours of a node that equals its tree's target."""
        levels, weights, cur = [targets], [], targets
        for level in range(self.L):
            ids, counts = ops.pinsage_neighbors(cur, self.graph, self.n, self.num_walks, self.walk_len, self.termination_prob,
                                                self.seed, step, level, tree_target=None if exclude is None else targets,
                                                tree_exclude=exclude)
            cur = ids.view(-1)
            levels.append(cur)
            weights.append(ops.pinsage_weights(counts).view(-1))
        if not self.L:
            return targets, None
        return torch.cat(levels), torch.cat(weights)

    def tree_ids(self, targets, step):
        return self.tree(targets, step)[0]

    # ---- the tower, composed from torch ops ---------------------------------------------------
    def composed(self, x, rows, scale, weights, params, L, n, p, step):
        """The tower of csrc/pinsage.hip from torch ops: `x` [nodes, T, K] the gathered slot rows (rows < 0 hold garbage)."""
        K, T = self.K, rows.shape[1]
        x = x * (rows >= 0).unsqueeze(-1)
        if scale is not None:
            x = x * scale.unsqueeze(-1)
        o = T * K * K
        h0 = x.flatten(1) @ params[:o].view(T * K, K) + params[o:o + K]
        o += K
        B = rows.shape[0] // ops.sage_tree_nodes(L, n)
        h, w, at = [], [None], 0
        for k in range(L + 1):
            cnt = B * (n ** k if L else 1)
            h.append(h0[at:at + cnt])
            if k:
                w.append(weights[at - B:at - B + cnt].to(h0.dtype))
            at += cnt
        inv_keep = float(np.float32(1.0 / (1.0 - p))) if p > 0 else 1.0
        for l in range(L):
            Qt, bq = params[o:o + K * K].view(K, K), params[o + K * K:o + K * K + K]
            o += K * K + K
            Wt, bw = params[o:o + 2 * K * K].view(2 * K, K), params[o + 2 * K * K:o + 2 * K * K + K]
            o += 2 * K * K + K
            nxt = []
            for k in range(L - l):
                nb = F.relu(h[k + 1] @ Qt + bq)
                if p > 0:
                    keep = ops.sage_dropout_mask(nb.shape[0], K, p, self.seed, step, l, k + 1, 1, nb.device)
                    nb = torch.where(keep.bool(), nb * inv_keep, torch.zeros_like(nb))
                agg = (nb * w[k + 1].unsqueeze(-1)).view(-1, n, K).sum(1)
                z = F.relu(torch.cat([h[k], agg], dim=1) @ Wt + bw)
                norm = z.norm(dim=1, keepdim=True)
                nxt.append(z / torch.where(norm == 0, torch.ones_like(norm), norm))
            h = nxt
        G1t, b1 = params[o:o + K * K].view(K, K), params[o + K * K:o + K * K + K]
        G2t = params[o + K * K + K:o + 2 * K * K + K].view(K, K)
        return F.relu(h[0] @ G1t + b1) @ G2t

    def item_tower(self, targets, step, train, exclude=None):
        ids, weights = self.tree(targets, step, exclude)
        rows, scale = self.items.slots(ids)
        return _PinTower(self, rows, scale, weights, self.item_pack, self.L, self.n, step, train, self.item_fused)

    def user_tower(self, users, step, train):
        rows, scale = self.users.slots(users)
        return _PinTower(self, rows, scale, None, self.user_pack, 0, 1, step, train, self.user_fused)

    def i2i_exclude(self, queries, items_pos, items_neg):
        """int32 [batch of the three towers]: the positive on the query block, -1 elsewhere (None without `remove_edges`)."""
        if not self.remove_edges:
            return None
        rest = torch.full((items_pos.numel() + items_neg.numel(),), -1, dtype=torch.int32, device=queries.device)
        return torch.cat([items_pos[:queries.numel()], rest]).contiguous()

    def i2i_tower(self, queries, items_pos, items_neg, step):
        targets = torch.cat([queries, items_pos, items_neg]).contiguous()
        return self.item_tower(targets, step, True, self.i2i_exclude(queries, items_pos, items_neg))
