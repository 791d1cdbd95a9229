"""CPU oracle of the FTRL-proximal kernels (csrc/ftrl.hip) and of one Wide & Deep training step (nets/wide_deep_net.py).

The arithmetic is TF1's ApplyFtrl / SparseApplyFtrl with lr_power = -0.5 and no l2 shrinkage
(`tf.train.FtrlOptimizer(lr, l1_regularization_strength=1e-3)`, `training/tf_trainer.py:297-302`), in f64:

  ftrl_elem / ftrl_dense   the update on every element, g = grad + l2_grad_coef * var
  ftrl_rows                de-duplicate the (id, gradient) stream by summing, then the update on the touched rows only
  kernel_case, KERNEL_CASES, oracle_rows   the seeded f32 inputs of tests/test_wide_deep_gpu.py and their f64 results, computed
                           once per case and never changed
  WideDeepOracle           one whole step in torch f64 autograd composed from plain ops: forward, loss, Adam on the deep side,
                           FTRL on the wide side, BatchNorm moving statistics (`libreco/algorithms/wide_deep.py:151-178`,
                           `WideDeepTrainer`)
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32
INIT_ACCUM = 0.1


# ---- the update ----------------------------------------------------------------------------------------------------------
def ftrl_elem(var, accum, linear, g, lr, l1=1e-3, l2=0.0):
    """-> (var, accum, linear) after one update with gradient g; every argument f64 (arrays or scalars)."""
    var, accum, linear, g = (np.asarray(x, dtype=np.float64) for x in (var, accum, linear, g))
    new_accum = accum + g * g
    linear = linear + g - (np.sqrt(new_accum) - np.sqrt(accum)) / lr * var
    quadratic = np.sqrt(new_accum) / lr + 2.0 * l2
    with np.errstate(divide="ignore", invalid="ignore"):
        var = np.where(np.abs(linear) > l1, (np.sign(linear) * l1 - linear) / quadratic, 0.0)
    return var, new_accum, linear


def ftrl_dense(var, accum, linear, grad, lr, l1=1e-3, l2=0.0, l2_grad_coef=0.0):
    var = np.asarray(var, dtype=np.float64)
    return ftrl_elem(var, accum, linear, np.asarray(grad, dtype=np.float64) + l2_grad_coef * var, lr, l1, l2)


def scatter_sum(V, ids, grad):
    """(dense [V] sum of the stream's gradients per row, sorted touched rows); ids outside [0, V) are dropped."""
    ids = np.asarray(ids).reshape(-1).astype(np.int64)
    ok = (ids >= 0) & (ids < V)
    out = np.zeros(V, dtype=np.float64)
    np.add.at(out, ids[ok], np.asarray(grad, dtype=np.float64).reshape(-1)[ok])
    return out, np.unique(ids[ok])


def ftrl_rows(var, accum, linear, ids, grad, lr, l1=1e-3, l2=0.0):
    """-> (var, accum, linear, touched rows): rows outside the stream keep their values."""
    var, accum, linear = (np.array(x, dtype=np.float64).reshape(-1) for x in (var, accum, linear))
    gsum, rows = scatter_sum(len(var), ids, grad)
    var[rows], accum[rows], linear[rows] = ftrl_elem(var[rows], accum[rows], linear[rows], gsum[rows], lr, l1, l2)
    return var, accum, linear, rows


# ---- seeded kernel cases ---------------------------------------------------------------------------------------------------
def _runs_stream(rng, lengths, V):
    """ids of a stream whose run of row r has exactly lengths[r] positions, shuffled."""
    ids = np.repeat(np.arange(len(lengths)), lengths)
    assert len(lengths) <= V
    return rng.permutation(ids).astype(np.int32)


def kernel_case(name, long_run, chunk):
    """dict(ids int32 [n], grad f32 [n], var / accum / linear f32 [V], lr, l1, l2) of a named case; `long_run` and `chunk` are
    the kernel's two constants (`ops.FTRL_LONG_RUN`, `ops.FTRL_CHUNK`)."""
    rng = np.random.default_rng([7, sum(map(ord, name))])
    lr, l1, l2 = 0.01, 1e-3, 0.0
    fresh = False
    if name == "collide":                      # V = 7, n = 64: everything collides, every run below the long threshold
        V, ids = 7, rng.integers(0, 7, 64).astype(np.int32)
        assert np.bincount(ids, minlength=7).max() <= long_run
    elif name == "random":                     # mostly runs of one
        V, ids = 5000, rng.integers(0, 5000, 4096).astype(np.int32)
    elif name == "boundaries":                 # runs of exactly T, T + 1, one chunk, one chunk + 1, three chunks + 5
        V = 9
        ids = _runs_stream(rng, [long_run, long_run + 1, chunk, chunk + 1, 3 * chunk + 5, 1, 2], V)
    elif name == "two_valued":                 # a two-valued column at batch 8192: two runs of about 4096 positions
        V, ids = 3, rng.integers(0, 2, 8192).astype(np.int32)
    elif name == "dropped":                    # ids of -1 and >= V mixed in
        V = 300
        ids = rng.integers(0, V, 2048).astype(np.int32)
        ids[rng.random(2048) < 0.2] = -1
        ids[rng.random(2048) < 0.2] = V + rng.integers(0, 50)
        ids[:chunk] = 5                        # and one long run among them
    elif name == "l1_zero":
        V, ids, l1 = 200, rng.integers(0, 200, 1500).astype(np.int32), 0.0
    elif name == "l2":
        V, ids, l2 = 200, rng.integers(0, 200, 1500).astype(np.int32), 0.05
    elif name == "threshold":                  # fresh slots and zero weights: linear = the summed gradient, on both sides of l1
        V, fresh = 400, True
        ids = np.concatenate([np.arange(V), rng.integers(0, V, 400)]).astype(np.int32)
    else:
        raise KeyError(name)
    n = len(ids)
    grad = (rng.standard_normal(n) * 0.3).astype(F32)
    var = rng.uniform(-0.5, 0.5, V).astype(F32)
    accum = (INIT_ACCUM + rng.random(V) * (rng.random(V) < 0.5)).astype(F32)       # half fresh, half used
    linear = (rng.standard_normal(V) * (accum > F32(INIT_ACCUM))).astype(F32)
    if fresh:
        var[10:], accum[:], linear[:] = 0.0, INIT_ACCUM, 0.0                       # rows 0..9 keep a random weight
        grad = rng.uniform(-2e-3, 2e-3, n).astype(F32)                             # |sum| on both sides of l1 = 1e-3
        grad[ids < 5] = 0.0                                                         # a zero gradient on touched rows: var -> 0.0
    return dict(name=name, V=V, ids=ids, grad=grad, var=var, accum=accum, linear=linear, lr=lr, l1=l1, l2=l2)


KERNEL_CASES = ("collide", "random", "boundaries", "two_valued", "dropped", "l1_zero", "l2", "threshold")


@functools.lru_cache(maxsize=None)
def oracle_rows(name, long_run, chunk):
    """(case, (var, accum, linear, touched rows) in f64, run length of every row)."""
    c = kernel_case(name, long_run, chunk)
    out = ftrl_rows(c["var"], c["accum"], c["linear"], c["ids"], c["grad"], c["lr"], c["l1"], c["l2"])
    ok = (c["ids"] >= 0) & (c["ids"] < c["V"])
    return c, out, np.bincount(c["ids"][ok], minlength=c["V"])


def dense_case(n, coef):
    rng = np.random.default_rng([11, n])
    return dict(var=rng.uniform(-0.5, 0.5, n).astype(F32), accum=(INIT_ACCUM + rng.random(n)).astype(F32),
                linear=rng.standard_normal(n).astype(F32), grad=(rng.standard_normal(n) * 0.3).astype(F32), lr=0.01, l1=1e-3,
                l2=0.0, coef=coef)


# ---- one Wide & Deep step ----------------------------------------------------------------------------------------------------
def export_state(net):
    """What `WideDeepOracle` starts from: the net's tables, dense parameters and BatchNorm statistics as CPU f64 tensors."""
    t = net.tables
    cpu = lambda x: x.detach().cpu().double().clone()
    st = dict(embed=cpu(t.embed), lin=cpu(t.lin), offs=(t.user_off, t.item_off, t.sparse_off),
              params={k: cpu(p) for k, p in net.P.params.items()}, bn={})
    for key, bn in [("bn_in", net.mlp.bn_in)] + [(f"bn{i}", b) for i, b in enumerate(net.mlp.bns, start=1)]:
        if bn is not None:
            st["bn"][key] = (cpu(bn.moving_mean), cpu(bn.moving_var))
    return st


class _Adam:
    """TF1 Adam with the constants the kernels use (b, 1 - b and eps formed in f32), on a dense gradient; `rows`: the rows that
    move (row-wise form), None: every element."""

    def __init__(self, lr, eps):
        self.lr, self.eps, self.state = lr, float(F32(eps)), {}
        self.b1, self.b2 = float(F32(0.9)), float(F32(0.999))
        self.omb1, self.omb2 = float(F32(1) - F32(0.9)), float(F32(1) - F32(0.999))

    def step(self, key, p, g, t, rows=None):
        m, v = self.state.setdefault(key, (torch.zeros_like(p), torch.zeros_like(p)))
        lr_t = self.lr * math.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        sel = slice(None) if rows is None else rows
        m[sel] = m[sel] * self.b1 + g[sel] * self.omb1
        v[sel] = v[sel] * self.b2 + g[sel] * g[sel] * self.omb2
        p[sel] = p[sel] - lr_t * (m[sel] / (v[sel].sqrt() + self.eps))


class WideDeepOracle:
    """`spec`: the net's `FeatSpec` (field layout only); `state`: `export_state(net)` before the first step."""

    WIDE = ("embedding/dense_linear_var", "wide_term/kernel", "wide_term/bias")

    def __init__(self, state, spec, n_layers, use_bn=True, lr=None, epsilon=1e-5, reg=None, dense_adam=False, l1=1e-3):
        self.spec, self.n_layers, self.use_bn = spec, n_layers, use_bn
        self.lr, self.reg, self.l1 = dict(lr), float(reg or 0.0), l1
        self.dense_adam = bool(dense_adam or reg)
        self.embed, self.lin = state["embed"].clone(), state["lin"].clone().reshape(-1)
        self.offs = state["offs"]
        self.P = {k: v.clone() for k, v in state["params"].items()}
        self.bn = {k: (m.clone(), v.clone()) for k, (m, v) in state["bn"].items()}
        self.adam, self.t = _Adam(self.lr["deep"], epsilon), 0
        self.accum = {"lin": torch.full_like(self.lin, INIT_ACCUM)}
        self.linear = {"lin": torch.zeros_like(self.lin)}
        for k in self.WIDE:
            if k in self.P:
                self.accum[k], self.linear[k] = torch.full_like(self.P[k], INIT_ACCUM), torch.zeros_like(self.P[k])

    # -- forward -----------------------------------------------------------------------------------------------------------
    def _bn(self, x, key, P, training):
        gamma, beta = P[f"deep/{key}/gamma"], P[f"deep/{key}/beta"]
        mm, mv = self.bn[key]
        if training:
            var, mean = torch.var_mean(x, dim=0, unbiased=False)
            with torch.no_grad():
                mm.mul_(0.99).add_(mean * 0.01)
                mv.mul_(0.99).add_(var * 0.01)
        else:
            mean, var = mm, mv
        return (x - mean) * (gamma * torch.rsqrt(var + 1e-3)) + beta

    def _pool(self, table, fi, oov):
        e = table[fi]                                                  # [B, n, ...]
        keep = (fi != oov).to(e.dtype)
        tot = (e * keep.reshape(keep.shape + (1,) * (e.dim() - 2))).sum(dim=1)
        if self.spec.combiner in ("mean", "sqrtn"):
            n = keep.sum(dim=1)
            n = n.sqrt() if self.spec.combiner == "sqrtn" else n
            n = n.reshape((-1,) + (1,) * (tot.dim() - 1))
            tot = torch.where(n > 0, tot / n.clamp_min(1e-30), torch.zeros_like(tot))
        return tot

    def _ids(self, users, items, sparse):
        s, (uo, io, so) = self.spec, self.offs
        cols = [torch.as_tensor(users).long().view(-1, 1) + uo, torch.as_tensor(items).long().view(-1, 1) + io]
        sp = torch.as_tensor(sparse).long() if s.n_sparse_cols else None
        if s.plain_cols:
            cols.append(sp[:, s.plain_cols] + so)
        fields = [(sp[:, o:o + n] + so, oov + so) for o, n, oov in zip(s.field_offset, s.field_len, s.field_oov)]
        return torch.cat(cols, dim=1), fields

    def logits(self, embed, lin, P, users, items, sparse, dense, training):
        idx, fields = self._ids(users, items, sparse)
        parts, lparts = [embed[idx]], [lin[idx]]
        for fi, oov in fields:
            parts.append(self._pool(embed, fi, oov)[:, None, :])
            lparts.append(self._pool(lin, fi, oov)[:, None])
        if self.spec.n_dense_cols:
            dv = torch.as_tensor(dense).double()
            parts.append(dv[:, :, None] * P["embedding/dense_embeds_var"][None])
            lparts.append(dv * P["embedding/dense_linear_var"][None])
        E, LIN = torch.cat(parts, dim=1), torch.cat(lparts, dim=1)
        wide = LIN @ P["wide_term/kernel"] + P["wide_term/bias"]
        x = E.flatten(1)
        if self.use_bn:
            x = self._bn(x, "bn_in", P, training)
        for i in range(1, self.n_layers + 1):
            x = x @ P[f"deep/deep_layer{i}/kernel"] + P[f"deep/deep_layer{i}/bias"]
            if i != self.n_layers:
                x = F.relu(x)
                if self.use_bn:
                    x = self._bn(x, f"bn{i}", P, training)
        deep = x @ P["deep_term/kernel"] + P["deep_term/bias"]
        return (wide + deep).squeeze(1), idx, fields

    @staticmethod
    def loss_fn(logits, labels, loss_type):
        if loss_type == "cross_entropy":
            return F.binary_cross_entropy_with_logits(logits, labels)
        if loss_type == "focal":
            w = labels * 0.25 + (1 - labels) * 0.75
            p = torch.sigmoid(logits)
            p_t = labels * p + (1 - labels) * (1 - p)
            return (w * (1 - p_t) ** 2.0 * F.binary_cross_entropy_with_logits(logits, labels, reduction="none")).mean()
        return F.mse_loss(logits, labels)

    def forward(self, users, items, sparse=None, dense=None):
        with torch.no_grad():
            return self.logits(self.embed, self.lin, self.P, users, items, sparse, dense, False)[0]

    # -- one step ----------------------------------------------------------------------------------------------------------
    def train_step(self, users, items, labels, sparse=None, dense=None, loss_type="cross_entropy"):
        self.t += 1
        embed, lin = self.embed.clone().requires_grad_(True), self.lin.clone().requires_grad_(True)
        P = {k: v.clone().requires_grad_(True) for k, v in self.P.items()}
        logits, idx, fields = self.logits(embed, lin, P, users, items, sparse, dense, True)
        loss = self.loss_fn(logits, torch.as_tensor(labels).double(), loss_type)
        loss.backward()
        touched = torch.unique(torch.cat([idx.reshape(-1)] + [fi.reshape(-1) for fi, _ in fields]))
        reg2 = 2.0 * self.reg
        with torch.no_grad():
            # Adam, the deep side
            ge = embed.grad + reg2 * self.embed if self.dense_adam else embed.grad
            self.adam.step("embed", self.embed, ge, self.t, None if self.dense_adam else touched)
            for k, p in self.P.items():
                if k in self.WIDE:
                    continue
                g = P[k].grad + (reg2 * p if k == "embedding/dense_embeds_var" else 0.0)
                self.adam.step(k, p, g, self.t)
            # FTRL, the wide side: rows of the stream, or every row under `reg`
            lw = self.lr["wide"]
            rows = slice(None) if self.reg else touched
            out = ftrl_elem(self.lin[rows].numpy(), self.accum["lin"][rows].numpy(), self.linear["lin"][rows].numpy(),
                            (lin.grad + reg2 * self.lin)[rows].numpy(), lw, self.l1)
            for dst, src in zip((self.lin, self.accum["lin"], self.linear["lin"]), out):
                dst[rows] = torch.from_numpy(src)
            for k in self.WIDE:
                if k not in self.P:
                    continue
                g = P[k].grad + (reg2 * self.P[k] if k == "embedding/dense_linear_var" else 0.0)
                out = ftrl_elem(self.P[k].numpy(), self.accum[k].numpy(), self.linear[k].numpy(), g.numpy(), lw, self.l1)
                for dst, src in zip((self.P[k], self.accum[k], self.linear[k]), out):
                    dst.copy_(torch.from_numpy(src))
        return float(loss.detach())
