"""AutoInt graph (`libreco/algorithms/autoint.py:146-168`): the field matrix E [B, T, K] of the general feature embedding layer
([user, item, sparse..., dense...], multi-sparse fields pooled), `len(head_dims)` layers of bias-free multi-head self-attention
over the field axis (`layers/attention.py:67-101`, the Keras `MultiHeadAttention` branch) with an optional residual, and
Dense(1) of the flattened result.  No linear tables, no batch normalisation, no dropout (the reference stores `use_bn` and
`dropout_rate` and builds neither layer).

Fused path (`net.fused`): the stack and the read-out are one forward launch of csrc/autoint.hip on E and one backward call that
writes the attention and Dense gradients straight into the flat gradient buffer of `DenseParams` (their tensors are one
contiguous slice of `P.flat`: `stack_params`); the loss and its gradient with respect to the logits are `_FieldNet.loss_fn` in
torch on the logits as a leaf; d loss / d E goes back to the tables through `FeatEmbedding.apply_gradients` with explicit
gradients.  Inference writes nothing but the logits.

Composed path (a shape outside `ops.autoint_supported`, row-sharded tables, or `fused=False`): the same parameters under
`seq_nets.multi_head_attention` and `TFDense` with autograd, finished by `_FeatNet._finish`.
"""
from __future__ import annotations

import torch

from .. import ops
from ..layers import TFDense
from ..utils.device import to_device
from .feat_nets import _FeatNet
from .fm_nets import _FieldNet
from .seq_nets import multi_head_attention

MHA_KERNELS = ("query", "key", "value", "attention_output")


def mha_layer_names(n_layers):
    """Keras' default names of the attention layers, in graph order."""
    return [f"multi_head_attention{'' if i == 0 else f'_{i}'}" for i in range(n_layers)]


class FeatAutoIntNet(_FeatNet):
    with_linear = False

    def __init__(self, spec, embed_size=16, head_dims=(8, 8, 8), num_heads=2, use_residual=True, lr=1e-3, epsilon=1e-5,
                 seed=42, device=None, dense_adam=False, reg=None, fused=True, **shard):
        super().__init__(spec, embed_size, lr, epsilon, seed, device, dense_adam, reg, **shard)
        P, K, H = self.P, embed_size, int(num_heads)
        self.T, self.H, self.head_dims, self.residual = spec.n_fields, H, tuple(int(h) for h in head_dims), bool(use_residual)
        # Keras keeps the projections 3-D: [K, H, hd] and [H, hd, K].  Row-major that is the [K, H hd] / [H hd, K] the kernels
        # and `multi_head_attention` read, and `DenseParams` takes Keras' fans from the 3-D shape
        self.layer_names = mha_layer_names(len(self.head_dims))
        for name, hd in zip(self.layer_names, self.head_dims):
            for w in MHA_KERNELS[:3]:
                P.add(f"{name}/{w}/kernel", (K, H, hd), "glorot_uniform")
            P.add(f"{name}/attention_output/kernel", (H, hd, K), "glorot_uniform")
        self.readout = TFDense(P, "dense", self.T * K, 1)
        P.finalize()
        self.fused = bool(fused and self.kern is None and self.device.type == "cuda"
                          and ops.autoint_supported(self.T, K, H, self.head_dims))
        if self.fused:
            # `FeatEmbedding` may have put `embedding/dense_embeds_var` in front: the kernels' slice starts at the first projection
            first = P[f"{self.layer_names[0]}/query/kernel"]
            start = (first.data_ptr() - P.flat.data_ptr()) // 4
            n = ops.autoint_param_floats(self.T, K, H, self.head_dims)
            assert start + n == P.flat.numel() and P["dense/bias"].data_ptr() == P.flat.data_ptr() + 4 * (start + n - 4), \
                "DenseParams / lr_autoint layout"
            self.stack_params, self.stack_grad = P.flat[start:start + n], P.grad[start:start + n]

    # ---- the composed stack ------------------------------------------------------------------------
    def _logits(self, E):
        P, K = self.P, self.K
        a = E
        for name, hd in zip(self.layer_names, self.head_dims):
            M = self.H * hd
            y = multi_head_attention(a, a, P[f"{name}/query/kernel"].view(K, M), P[f"{name}/key/kernel"].view(K, M),
                                     P[f"{name}/value/kernel"].view(K, M), P[f"{name}/attention_output/kernel"].view(M, K),
                                     self.H, None)
            a = a + y if self.residual else y
        return self.readout(a.flatten(1)).squeeze(1)

    @torch.no_grad()
    def forward(self, users, items, sparse=None, dense=None, **_):
        _, E, _ = self.emb.forward(users, items, sparse, dense, grad=False)
        if not self.fused:
            return self._logits(E)
        return ops.autoint_fwd(E.contiguous(), self.stack_params, self.H, self.head_dims, self.residual, want_acts=False)[0]

    def train_step(self, users, items, labels, sparse=None, dense=None, loss_type="cross_entropy", **_):
        self.step += 1
        if not self.fused:
            ctx, E, _ = self.emb.forward(users, items, sparse, dense)
            self.P.zero_grad()
            return self._finish(ctx, _FieldNet.loss_fn(self._logits(E), self._labels(labels), loss_type))
        P, s = self.P, self.spec
        with torch.no_grad():
            ctx, E, _ = self.emb.forward(users, items, sparse, dense, grad=False)
            E = E.contiguous()
            P.zero_grad()
            logits, acts, saved = ops.autoint_fwd(E, self.stack_params, self.H, self.head_dims, self.residual)
        logits.requires_grad_(True)
        loss = _FieldNet.loss_fn(logits, self._labels(labels), loss_type)
        loss.backward()
        with torch.no_grad():
            dE, _ = ops.autoint_bwd(E, self.stack_params, self.H, self.head_dims, self.residual, acts, saved,
                                    logits.grad.contiguous(), gparams=self.stack_grad)
            Fp, nq = ctx.idx_plain.shape[1], len(ctx.pooled_idx)
            grads = (dE[:, :Fp].contiguous(), None, [dE[:, Fp + q].contiguous() for q in range(nq)], [])
            if s.n_dense_cols:                                         # features.py:121-148: dense_embeds_var[f] * value
                dv = to_device(dense, self.device, torch.float32)
                P["embedding/dense_embeds_var"].grad.copy_(torch.einsum("bf,bfk->fk", dv, dE[:, Fp + nq:]))
            hp = self._hp()
            self.emb.apply_gradients(ctx, hp, self.dense_adam, self.reg, None, grads)
            P.adam_step(hp)
        return loss.detach()
