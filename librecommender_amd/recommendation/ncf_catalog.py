"""Full-catalogue scoring of NCF without the B x N pair rows.

The first Dense layer of NCF's MLP sees concat[u | i], so with the input BatchNorm folded in (W1', b1') it splits into a
user part and an item part,  z1 = (u @ W1'[:K] + b1') + (i @ W1'[K:]) = P_u + Q_i,  and the GMF term is bilinear,
sum_k u_k i_k wg_k = ((u * wg) @ I^T).  The item side Q is computed once for the catalogue and kept until the net changes;
a pair then costs the MLP tail behind z1: `ops.pair_mlp` (csrc/pair_mlp.hip) where the stack is three relu layers of compiled
widths — the fold of `CatalogScorer._fused_tail` with the output layer's MLP weights `out.w[K:]` —, else the net's own forward
(`ops.ncf_score`, csrc/ncf.hip, where the stack is inside its envelope) over chunks of the materialised pairs.  Either way the
scores equal `net.forward` on the pairs up to f32 re-association (tests: 1e-4, as for `CatalogScorer`)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from .. import ops


class NCFCatalogScorer:
    pair_chunk = 1 << 22        # materialised pairs per forward on the chunked branch

    def __init__(self, model):
        self.model, self.net, self.device = model, model.net, model.device
        self._cache_key, self._item = None, None

    def _fused_tail(self, s, t):
        """(W2', b2', v3, c3) of  deep = relu(relu(z1) @ W2' + b2') @ v3 + c3, or None (see `CatalogScorer._fused_tail`)."""
        net, mlp, P = self.net, self.net.mlp, self.net.P
        if len(mlp.layers) != 3 or mlp.act is not F.relu or not net.tables.embed.is_cuda:
            return None
        W2, b2 = P[mlp.layers[1].w].detach(), P[mlp.layers[1].b].detach()
        W3, b3 = P[mlp.layers[2].w].detach(), P[mlp.layers[2].b].detach()
        if not ops.pair_mlp_supported(*W2.shape):
            return None
        wo_mlp = P[net.out.w].detach().view(-1)[net.K:]
        W2f, b2f = (W2, b2) if s[0] is None else ((W2 * s[0][:, None]).contiguous(), b2 + t[0] @ W2)
        W3f, b3f = (W3, b3) if s[1] is None else (W3 * s[1][:, None], b3 + t[1] @ W3)
        return W2f, b2f.contiguous(), (W3f @ wo_mlp).contiguous(), float(b3f @ wo_mlp)

    @torch.no_grad()
    def _item_side(self):
        """(fold, I, Q) cached per state of the net: I the catalogue's item rows, Q = I @ W1'[K:]."""
        net = self.net
        key = (net.step, net.P.flat._version, self.model.n_items)
        if self._item is None or self._cache_key != key:
            t, K = net.tables, net.K
            fold = net.inference_fold()
            I = t.embed[t.item_off: t.item_off + self.model.n_items]
            self._item, self._cache_key = (fold, I, I @ fold[0][0][K:]), key
        return self._item

    @torch.no_grad()
    def scores(self, user_ids, user_feats=None) -> torch.Tensor:
        """[B, n_items] logits of every (user, catalogue item) pair; `user_feats` has nothing to override on pure ids."""
        net, t, K = self.net, self.net.tables, self.net.K
        (W, b, s, tt, wg, wd, c), I, Q = self._item_side()
        users = torch.as_tensor(np.asarray(user_ids, dtype=np.int64), device=self.device)
        B, N = len(users), I.shape[0]
        fused = self._fused_tail(s, tt)
        if fused is None:
            out = torch.empty((B, N), dtype=torch.float32, device=self.device)
            flat, ub = out.view(-1), max(1, self.pair_chunk // max(1, N))
            items = torch.arange(N, device=self.device, dtype=torch.int32)
            for s0 in range(0, B, ub):
                u = users[s0:s0 + ub].to(torch.int32)
                flat[s0 * N:(s0 + len(u)) * N] = net.forward(u.repeat_interleave(N), items.repeat(len(u)))
            return out
        u = t.embed[t.user_off + users]
        out = (u * wg) @ I.T + c
        W2f, b2f, v3, c3 = fused
        ops.pair_mlp((u @ W[0][:K] + b[0]).contiguous(), Q, W2f, b2f, v3, c3, out, accumulate=True)
        return out
