"""NCF graph (`libreco/algorithms/ncf.py:113-150` of the reference; He et al., "Neural Collaborative Filtering"):

    u = user_embeds_var[user]      i = item_embeds_var[item]           (K wide, glorot, one OOV row each)
    gmf = u * i                    mlp = dense_nn(concat[u | i])       logit = Dense(1)(concat[gmf | mlp])

Both variables are views of one `FieldTables.embed` allocation ([user rows | item rows], no sparse rows, no linear twins), so
one gather, one segment build and one row update serve a batch.  Feature columns of a `DatasetFeat` are ignored, as in the
reference.

The fused step (cross entropy, row-wise Adam, no `reg`, at least two layers, 2K % 32 == 0, compiled widths) runs without
autograd:  `ops.ncf_pair_fwd` (csrc/ncf.hip: both rows gathered, x = [u | i] and the exact product gmf = u * i) ->
`BlockFirstLayer` on the row-major block re-cut into 32-wide pieces (input BatchNorm folded, MFMA) -> `DeepFMTail` in its
`K > 0, F = 0` form, whose head weights [pair | deep] are NCF's [gmf | mlp] -> the first layer's backward -> `ops.ncf_pair_bwd_`
(the GMF path joins the MLP's row gradient) -> `RowAdam.update` on the segments of the id block -> `DenseParams.adam_step`.
It is the shape of `FeatDeepFMNet._block_step` without the linear term; the DeepFM pairwise kernels are not used: they form
0.5((u+i)^2 - u^2 - i^2), which is u * i only up to an error of order eps * u^2.

Everything else (`focal`, `mse`, `dense_adam` / `reg`, one layer, other K, `fused=False`) is the autograd composition in the
shape of `TwoTowerNet.train_step`.  `forward` is one `ops.ncf_score` launch where the stack is inside its envelope, else the
same composition in inference mode."""
from __future__ import annotations

import torch

from .. import ops
from ..layers import DenseParams, DenseStack, FieldTables, TFDense
from ..layers.row_adam import RowAdam
from ..utils.device import to_device
from .fm_nets import _FieldNet


class NCFNet:
    def __init__(self, n_users, n_items, embed_size=16, hidden_units=(128, 64, 32), use_bn=True, dropout_rate=0.0, lr=0.01,
                 epsilon=1e-5, seed=42, device=None, dense_adam=False, reg=None, fused=True):
        from ..layers.dense import BlockFirstLayer
        from ..layers.tail import DeepFMTail

        self.device = device or torch.device("cuda")
        self.K = K = int(embed_size)
        hidden_units = [int(h) for h in hidden_units]
        self.tables = FieldTables(n_users, n_items, 0, K, self.device, seed, with_linear=False)
        self.P = P = DenseParams(self.device, seed)
        self.mlp = DenseStack(P, "mlp", 2 * K, hidden_units, use_bn, dropout_rate)
        self.out = TFDense(P, "out", K + self.mlp.n_out, 1)
        P.finalize()
        self.reg = float(reg or 0.0)
        self.adam = RowAdam(self.device, bool(dense_adam or self.reg), self.reg)   # `reg` only exists under TF1's dense update
        self.lr, self.epsilon, self.step = lr, epsilon, 0
        self.fused = bool(fused and not self.adam.dense and len(hidden_units) >= 2 and (2 * K) % 32 == 0
                          and BlockFirstLayer.supported(32, hidden_units[0]) and DeepFMTail.supported(self.mlp))
        self.score_kernel = bool(self.tables.embed.is_cuda and ops.ncf_score_supported(K, hidden_units))
        self._blk, self._score_args = {}, None

    @property
    def dense_adam(self):
        return self.adam.dense

    def _hp(self):
        return ops.adam_hp(self.lr, self.step, eps=self.epsilon, tf_style=True)

    def _i32(self, x):
        return to_device(x, self.device).to(torch.int32)

    def pair_rows(self, users, items) -> torch.Tensor:
        """[B, 2] int32 global rows (user row, item row) of the pairs."""
        t = self.tables
        return torch.stack([self._i32(users).view(-1) + t.user_off, self._i32(items).view(-1) + t.item_off], dim=1).contiguous()

    def assign_oov(self, sparse_oov_rows=None):
        """OOV rows := mean of the real rows (`bases/tf_base.py:310-353`)."""
        t = self.tables
        with torch.no_grad():
            t.embed[t.user_off + t.n_users] = t.embed[t.user_off: t.user_off + t.n_users].mean(dim=0)
            t.embed[t.item_off + t.n_items] = t.embed[t.item_off: t.item_off + t.n_items].mean(dim=0)

    # ---- the graph under torch ----------------------------------------------------------------------------------------------
    def _logits(self, u, i, training):
        h = self.mlp(torch.cat([u, i], dim=1), training)
        return self.out(torch.cat([u * i, h], dim=1)).squeeze(1)

    def inference_fold(self):
        """(W, b, s, t, wg, wd, c) of `ops.ncf_score`: the input BatchNorm folded into the first layer as
        `CatalogScorer._first_layer` does, each hidden BatchNorm's inference affine behind its relu as (s_l, t_l) (None without
        BatchNorm), the output layer split into its GMF and MLP weights, and its bias as a host float."""
        mlp, P, K = self.mlp, self.P, self.K
        W = [P[l.w].detach() for l in mlp.layers]
        b = [P[l.b].detach() for l in mlp.layers]

        def affine(bn):
            sc = P[bn.gamma].detach() * torch.rsqrt(bn.moving_var + bn.eps)
            return sc, P[bn.beta].detach() - bn.moving_mean * sc

        if mlp.bn_in is not None:
            sc, sh = affine(mlp.bn_in)
            W[0], b[0] = (W[0] * sc[:, None]).contiguous(), b[0] + sh @ W[0]
        s, t = [], []
        for bn in mlp.bns:
            st = (None, None) if bn is None else affine(bn)
            s.append(st[0])
            t.append(st[1])
        wo = P[self.out.w].detach().view(-1)
        return W, b, s, t, wo[:K], wo[K:], float(P[self.out.b].detach())

    @torch.no_grad()
    def forward(self, users, items, **_):
        t = self.tables
        idx = self.pair_rows(users, items)
        if self.score_kernel:
            key = (self.step, self.P.flat._version)                 # the fold (and the bias read-back) once per state
            if self._score_args is None or self._score_args[0] != key:
                self._score_args = (key, self.inference_fold())
            return ops.ncf_score(t.embed, idx[:, 0].contiguous(), idx[:, 1].contiguous(), *self._score_args[1])
        rows = ops.embed_gather(t.embed, idx)
        return self._logits(rows[:, 0], rows[:, 1], False)

    # ---- training ---------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _fused_step(self, idx, labels):
        from ..layers.dense import BlockFirstLayer
        from ..layers.tail import DeepFMTail

        P, mlp, t, K, dev = self.P, self.mlp, self.tables, self.K, self.device
        B, Pn = idx.shape[0], 2 * K // 32
        st = self._blk.get(B)
        if st is None:
            f32 = dict(dtype=torch.float32, device=dev)
            st = self._blk[B] = dict(
                l1=BlockFirstLayer(P, mlp.bn_in, mlp.layers[0], Pn, 32, B, dev, layout="rowmajor"),
                tail=DeepFMTail(P, mlp, None, self.out, 0, K, dev),
                gbuf=torch.empty((B * Pn + 1, 32), **f32), x=torch.empty((B, 2 * K), **f32), gmf=torch.empty((B, K), **f32))
        x, gmf = ops.ncf_pair_fwd(t.embed, idx, st["x"], st["gmf"])
        z1 = st["l1"].forward(x)
        loss, gl, gz1, sgz1 = st["tail"].run(z1, gmf, None, labels)
        st["l1"].backward(gz1, sgz1, st["gbuf"])
        G = st["gbuf"][: B * Pn].view(B, 2 * K)                       # d loss / d x through the MLP (BatchNorm terms included)
        ops.ncf_pair_bwd_(x, gl, P[self.out.w].view(-1)[:K], G)       # + the GMF path: ncf.py:137, the output layer's first K weights
        hp = self._hp()
        self.adam.update(hp, t.segments(idx), t.embed, t.m, t.v, G.view(-1, K))
        P.adam_step(hp)
        return loss

    def train_step(self, users, items, labels, sparse=None, dense=None, loss_type="cross_entropy", **_):
        self.step += 1
        t = self.tables
        idx = self.pair_rows(users, items)
        labels = to_device(labels, self.device, torch.float32)
        if self.fused and loss_type == "cross_entropy":
            return self._fused_step(idx, labels)
        rows = ops.embed_gather(t.embed, idx)
        rows.requires_grad_(True)
        self.P.zero_grad()
        loss = _FieldNet.loss_fn(self._logits(rows[:, 0], rows[:, 1], True), labels, loss_type)
        loss.backward()
        with torch.no_grad():
            hp = self._hp()
            self.adam.update(hp, t.segments(idx), t.embed, t.m, t.v, rows.grad.view(-1, self.K))
            self.P.adam_step(hp)
        return loss.detach()
