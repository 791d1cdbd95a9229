"""`tf_rnn` of the reference's TF2 branch (`libreco/layers/recurrent.py:27-45`): a stack of Keras `GRU` / `LSTM` layers with
`return_sequences=True` under a sequence mask, optionally each followed by `LayerNormalization` (epsilon 1e-3) and tanh, of
which the last step's output is the result.

One layer is one forward and one backward call of csrc/rnn.hip (`ops.rnn_layer_fwd` / `ops.rnn_layer_bwd`); the layer norm
between the layers is torch.  Parameters carry the Keras shapes (kernel [D, G H], recurrent_kernel [H, G H], bias [2, 3H]
for the GRU and [4H] for the LSTM) and initialisers (glorot-uniform, orthogonal, zeros with the LSTM's forget gate at one).

Dropout is this package's own definition: one mask per sample and layer, constant over time, on the layer's
input and on the state that feeds the recurrent product."""
from __future__ import annotations

from typing import Optional, Sequence

import torch
import torch.nn.functional as F

from .. import ops
from .dense import DenseParams

LN_EPS = 1e-3          # tf.keras.layers.LayerNormalization's default


class RnnLayerIO:
    """What one kernel layer reads besides its weights, and for the table form what its backward leaves behind (`gx`)."""

    def __init__(self, cell, lens, act, table=None, ids=None, in_mask=None, rec_mask=None):
        self.cell, self.lens, self.act = cell, lens, bool(act)
        self.table, self.ids, self.in_mask, self.rec_mask = table, ids, in_mask, rec_mask
        self.gx = None


class _RnnLayerFn(torch.autograd.Function):
    """hs = layer(x or table[ids]); the table form has no input tensor: its gx [B, L, D] is left in `io.gx`."""

    @staticmethod
    def forward(ctx, x, W, U, b, io):
        x = None if x is None else x.contiguous()
        hs, saved = ops.rnn_layer_fwd(io.cell, W, U, b, io.lens, x=x, table=io.table, ids=io.ids, in_mask=io.in_mask,
                                      rec_mask=io.rec_mask, act=io.act)
        ctx.io = io
        ctx.save_for_backward(x, W, U, hs, saved)
        return hs

    @staticmethod
    def backward(ctx, ghs):
        x, W, U, hs, saved = ctx.saved_tensors
        io = ctx.io
        gx, gW, gU, gb = ops.rnn_layer_bwd(io.cell, W, U, io.lens, hs, saved, ghs.contiguous(), x=x, table=io.table, ids=io.ids,
                                           in_mask=io.in_mask, rec_mask=io.rec_mask, act=io.act)
        if x is None:
            io.gx = gx
            gx = None
        return gx, gW, gU, gb, None


def rnn_layer(x, W, U, b, io: RnnLayerIO) -> torch.Tensor:
    return _RnnLayerFn.apply(x, W, U, b, io)


def _suffix(i):
    return "" if i == 0 else f"_{i}"


class RnnStack:
    """`hidden_units[i]` units in layer i; layer 0 reads `d_in` inputs.  Parameter names follow the Keras layout
    (`gru/gru_cell/kernel`, `gru_1/gru_cell_1/recurrent_kernel`, `layer_normalization/gamma`, ...)."""

    def __init__(self, P: DenseParams, cell: str, d_in: int, hidden_units: Sequence[int], use_layer_norm=False,
                 dropout_rate: float = 0.0):
        if cell not in ops.RNN_CELLS:
            raise ValueError("`rnn_type` must either be `lstm` or `gru`")
        self.P, self.cell, self.use_ln, self.dropout_rate = P, cell, bool(use_layer_norm), float(dropout_rate or 0.0)
        self.dims = [int(d_in), *[int(h) for h in hidden_units]]
        G = 3 if cell == "gru" else 4
        self.layers, self.lns = [], []
        for i, (d, h) in enumerate(zip(self.dims[:-1], self.dims[1:])):
            if not ops.rnn_supported(cell, d, h):
                raise ValueError(f"{cell} layer {i}: {d} inputs and {h} units are outside what the recurrent kernels take "
                                 "(1 to 128 each)")
            scope = f"{cell}{_suffix(i)}/{cell}_cell{_suffix(i)}"
            w = P.add(f"{scope}/kernel", (d, G * h), "glorot_uniform")
            u = P.add(f"{scope}/recurrent_kernel", (h, G * h), "orthogonal")
            b = P.add(f"{scope}/bias", (2, G * h), "zeros") if cell == "gru" else P.add(f"{scope}/bias", (G * h,), "lstm_bias")
            self.layers.append((w, u, b))
            if self.use_ln:
                ln = f"layer_normalization{_suffix(i)}"
                self.lns.append((P.add(f"{ln}/gamma", (h,), "ones"), P.add(f"{ln}/beta", (h,), "zeros")))
        self.n_out = self.dims[-1]

    def draw_masks(self, B, gen):
        """[(in_mask [B, D_i], rec_mask [B, H_i])] per layer: Bernoulli(1 - p) / (1 - p)."""
        keep = 1.0 - self.dropout_rate
        out = []
        for d, h in zip(self.dims[:-1], self.dims[1:]):
            dev = self.P.device
            out.append(tuple((torch.rand((B, n), device=dev, generator=gen) < keep).float().div_(keep) for n in (d, h)))
        return out

    def __call__(self, lens, x=None, table=None, ids=None, masks=None):
        """-> (the last step's output [B, H_last], the first layer's `RnnLayerIO`).  `masks`: `draw_masks` in training."""
        P, out, first = self.P, x, None
        for i, (w, u, b) in enumerate(self.layers):
            im, rm = masks[i] if masks is not None else (None, None)
            io = RnnLayerIO(self.cell, lens, not self.use_ln, in_mask=im, rec_mask=rm)
            if i == 0 and x is None:
                io.table, io.ids = table, ids
            first = first or io
            out = rnn_layer(out, P[w], P[u], P[b], io)
            last = i == len(self.layers) - 1
            if last:
                out = out[:, -1]
            if self.use_ln:
                g, be = self.lns[i]
                out = torch.tanh(F.layer_norm(out, (out.shape[-1],), P[g], P[be], LN_EPS))
        return out, first
