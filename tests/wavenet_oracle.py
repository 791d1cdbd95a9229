"""CPU oracle of the WaveNet stack and of WaveNet's training step (csrc/wavenet.hip, nets/wavenet_net.py).

The arithmetic is the reference's TF2 branch, `libreco/algorithms/wave_net.py:181-222` with `layers/convolutional.py`: Keras
`Conv1D(kernel_size=2, padding="causal", dilation_rate=2**i, activation=relu)` layers, a `Conv1D(kernel_size=1)` with ReLU, a
max pool over the whole window and one Dense layer; there is no sequence mask.

  stack_forward / stack_backward   numpy, "f64" or "f32" arithmetic.  The backward is hand-derived and takes the ReLU pattern
                                   (acts > 0) and the pool's `arg` as inputs: a unit within rounding of 0 and a near-tie in the
                                   pool are legitimate subgradients either way, so a result is judged against the backward of
                                   ITS OWN pattern
  NetTwin                          torch-CPU f64 autograd twin of `WaveNetNet.train_step` (F.conv1d on a left-padded input) with
                                   TF1 Adam
  stack_case, step_*               the seeded inputs shared by tests/test_wavenet_cpu.py and tests/test_wavenet_gpu.py
  check_stack                      the tolerance both files use
"""
from __future__ import annotations

import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32
B1, B2 = 0.9, 0.999
DATA = os.path.join(os.path.dirname(__file__), "golden", "sample_movielens_rating.dat")


def _dt(variant):
    return np.float64 if variant == "f64" else F32


def max_diff(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max()) if np.size(a) else 0.0


def dilation(j, n_per_block):
    return 2 ** (j % n_per_block)


def _shift(a, d):
    """a[t - d] with zeros for t < d (Keras padding="causal")."""
    out = np.zeros_like(a)
    if d < a.shape[1]:
        out[:, d:] = a[:, : a.shape[1] - d]
    return out


# ---- the stack, numpy ------------------------------------------------------------------------------------------------
def stack_forward(x, layers, n_per_block, variant="f64"):
    """x [B, L, D]; `layers` = [(K [2, C, F], b [F])] * n_layers + [(K [1, F, F], b)] -> (acts: the post-ReLU output of every
    layer, pooled [B, F], arg [B, F]: the smallest t that attains the maximum, torch's `max(dim)` rule)."""
    dt = _dt(variant)
    a, acts = x.astype(dt), []
    for j, (K, b) in enumerate(layers):
        K, b = K.astype(dt), b.astype(dt)
        if K.shape[0] == 2:
            z = _shift(a, dilation(j, n_per_block)) @ K[0] + a @ K[1] + b
        else:
            z = a @ K[0] + b
        a = np.maximum(z, 0)
        acts.append(a)
    return acts, a.max(axis=1), a.argmax(axis=1).astype(np.int32)


def stack_backward(x, layers, n_per_block, acts, pattern, arg, gpooled, variant="f64"):
    """Hand-derived backward from gpooled [B, F] -> (gx [B, L, D], [(gK, gb)] per layer).  `acts`: the forward's layer outputs
    (the inputs of the weight gradients); `pattern` [bool [B, L, F]] per layer: where ReLU passes the gradient (its derivative
    at 0 is 0); `arg` [B, F]: the position the pool's gradient goes to."""
    dt = _dt(variant)
    B, L, _ = x.shape
    nF = gpooled.shape[1]
    dz = np.zeros((B, L, nF), dtype=dt)
    bi, fi = np.meshgrid(np.arange(B), np.arange(nF), indexing="ij")
    dz[bi, np.asarray(arg), fi] = gpooled.astype(dt)
    dz = dz * pattern[-1]
    grads = [None] * len(layers)
    gx = None
    for j in range(len(layers) - 1, -1, -1):
        K = layers[j][0].astype(dt)
        a_in = (x if j == 0 else acts[j - 1]).astype(dt)
        C = a_in.shape[2]
        flat_dz = dz.reshape(B * L, nF)
        gb = flat_dz.sum(0)
        if K.shape[0] == 2:
            d = dilation(j, n_per_block)
            gK = np.stack([_shift(a_in, d).reshape(B * L, C).T @ flat_dz, a_in.reshape(B * L, C).T @ flat_dz])
            da = dz @ K[1].T
            if d < L:
                da[:, : L - d] += dz[:, d:] @ K[0].T                  # da[t] = K[1] dz[t] + K[0] dz[t + d]
        else:
            gK = (a_in.reshape(B * L, C).T @ flat_dz)[None]
            da = dz @ K[0].T
        grads[j] = (gK, gb)
        if j > 0:
            dz = da * pattern[j - 1]
        else:
            gx = da
    return gx, grads


# ---- seeded stack cases ----------------------------------------------------------------------------------------------
# (B, L, D, F, n_blocks, n_per_block)
STACK_SHAPES = [(1, 1, 1, 1, 1, 1), (37, 2, 3, 5, 1, 2), (37, 10, 16, 16, 1, 4), (300, 10, 20, 16, 2, 2), (37, 50, 64, 64, 1, 6),
                (5, 128, 8, 128, 1, 8), (300, 7, 128, 16, 1, 3), (37, 7, 16, 128, 2, 3)]
# batches past 2 x 512 samples, where a workgroup owns more than one sample (and, the second, as many as its LDS budget holds)
WIDE_SHAPES = [(2100, 3, 4, 128, 1, 2), (16400, 2, 3, 16, 1, 1)]
TABLE_ROWS = 50
# seed 0 unless named here: the only unit of the single-element case is dead at seeds 0 and 1 (everything compared would be 0)
CASE_SEEDS = {(1, 1, 1, 1, 1, 1): 2}


def layer_shapes(D, nF, n_blocks, n_per_block):
    n = n_blocks * n_per_block
    return [((2, D if j == 0 else nF, nF), (nF,)) for j in range(n)] + [((1, nF, nF), (nF,))]


def pack_params(layers):
    """The flat parameter buffer of `lr_wavenet_*`: kernel, bias, kernel, ... every tensor padded to a multiple of 4 floats."""
    out = []
    for K, b in layers:
        for t in (K, b):
            flat = np.asarray(t, dtype=F32).reshape(-1)
            out.append(np.concatenate([flat, np.zeros(-flat.size % 4, dtype=F32)]))
    return np.concatenate(out)


def unpack_params(flat, D, nF, n_blocks, n_per_block):
    """-> ([(K, b)], the gap elements concatenated)."""
    out, gaps, off = [], [], 0
    for ks, bs in layer_shapes(D, nF, n_blocks, n_per_block):
        pair = []
        for s in (ks, bs):
            n = int(np.prod(s))
            pair.append(flat[off:off + n].reshape(s))
            gaps.append(flat[off + n: off + n + (-n % 4)])
            off += n + (-n % 4)
        out.append(tuple(pair))
    assert off == flat.size
    return out, np.concatenate(gaps)


def stack_case(B, L, D, nF, n_blocks, n_per_block, seed=None):
    """dict of f32 / int32 arrays: a table of 50 rows + the pad row (id 50, an ordinary row: it takes part), Zipf ids with
    repeats, the first windows ending in 0, 1, L - 1 and L pad ids (as many of them as B allows), weights, an upstream
    gradient for the pool."""
    if seed is None:
        seed = CASE_SEEDS.get((B, L, D, nF, n_blocks, n_per_block), 0)
    rng = np.random.default_rng([seed, B, L, D, nF, n_blocks, n_per_block])
    V = TABLE_ROWS
    table = rng.standard_normal((V + 1, D)).astype(F32)
    ids = (rng.zipf(1.5, (B, L)) % V).astype(np.int32)
    for i, n_pad in enumerate([0, 1, L - 1, L][:B]):
        ids[i, L - n_pad:] = V
    layers = []
    for ks, bs in layer_shapes(D, nF, n_blocks, n_per_block):
        layers.append(((rng.standard_normal(ks) / np.sqrt(ks[0] * ks[1])).astype(F32), (rng.standard_normal(bs) * 0.1).astype(F32)))
    return dict(table=table, ids=ids, V=V + 1, layers=layers, npb=n_per_block, shape=(B, L, D, nF, n_blocks, n_per_block),
                seed=seed, custom=False, gpooled=rng.standard_normal((B, nF)).astype(F32))


def inside(c, ids=None):
    """[B, L, 1] bool: the id names a table row.  Any other id is never dereferenced: a zero input row whose gradient is 0."""
    ids = c["ids"] if ids is None else ids
    return ((ids >= 0) & (ids < c["V"]))[:, :, None]


def case_input(c, ids=None):
    """x [B, L, D]: the rows the ids name, zeros for an id outside [0, V)."""
    ids = c["ids"] if ids is None else ids
    inside = (ids >= 0) & (ids < c["V"])
    return np.where(inside[:, :, None], c["table"][np.where(inside, ids, 0)], 0).astype(F32)


@functools.lru_cache(maxsize=None)
def _cached_forward(shape, seed, variant):
    c = stack_case(*shape, seed=seed)
    return stack_forward(case_input(c), c["layers"], c["npb"], variant)


def forward_oracle(c, variant, ids=None):
    """The forward of a case in one arithmetic; computed once per (shape, seed, variant) for the case's own ids and weights
    (a test that edits a case sets `custom`)."""
    if ids is None and not c["custom"]:
        return _cached_forward(c["shape"], c["seed"], variant)
    return stack_forward(case_input(c, ids), c["layers"], c["npb"], variant)


# ---- the tolerance shared by the CPU and the GPU file ----------------------------------------------------------------
def delta_bound(want64, want32, n_layers):
    """The project's rule for long f32 sums (`_delta_rule` of tests/test_svd_gpu.py): 10 x the oracle's own f32 / f64 gap on
    this very case, and no tighter than one f32 ulp of the largest value compared per layer passed through, the least any
    f32 implementation can incur."""
    top = float(np.abs(want64).max()) if np.size(want64) else 0.0
    return max(10 * max_diff(want32, want64), n_layers * float(np.spacing(F32(top))))


def delta_rule(got, want64, want32, n_layers, what):
    bound = delta_bound(want64, want32, n_layers)
    gap = max_diff(got, want64)
    print(f"WAVENET-FIGURE {what} delta={max_diff(want32, want64):.3e} got={gap:.3e} bound={bound:.3e}")
    assert np.isfinite(np.asarray(got)).all() and gap <= bound, what
    return bound


def check_stack(got, c, what, ids=None):
    """`got` = dict(acts [n + 1, B, L, F], pooled, arg, gx, gparams (flat)) of a case.
    Forward: every layer of acts, and pooled, against f64 by the delta rule.  arg: the f64 value at the device's arg is within
    the pool's bound of the f64 maximum, and where the f64 maximum leads the runner-up by more than the bound, arg is the f64
    first argmax.  Backward: gx and every parameter gradient against the f64 backward run with the result's own ReLU pattern
    and arg; the alignment gaps of gparams are 0."""
    B, L, D, nF, nb, npb = c["shape"]
    x = case_input(c, ids)
    a64, p64, arg64 = forward_oracle(c, "f64", ids)
    a32, p32, _ = forward_oracle(c, "f32", ids)
    n = len(c["layers"])
    acts = np.asarray(got["acts"])
    assert acts.shape == (n, B, L, nF)
    for j in range(n):
        delta_rule(acts[j], a64[j], a32[j], j + 1, f"{what} acts[{j}]")
    bound = delta_rule(got["pooled"], p64, p32, n, f"{what} pooled")
    arg = np.asarray(got["arg"])
    assert arg.shape == (B, nF) and arg.dtype == np.int32 and (arg >= 0).all() and (arg < L).all()
    bi, fi = np.meshgrid(np.arange(B), np.arange(nF), indexing="ij")
    last = a64[-1]
    assert (p64 - last[bi, arg, fi] <= bound).all(), f"{what} arg value"
    if L > 1:
        rest = last.copy()
        rest[bi, arg64, fi] = -np.inf
        clear = p64 - rest.max(axis=1) > bound
        assert np.array_equal(arg[clear], arg64[clear]), f"{what} arg"
    pattern = [acts[j] > 0 for j in range(n)]
    gx64, g64 = stack_backward(x, c["layers"], npb, a64, pattern, arg, c["gpooled"], "f64")
    gx32, g32 = stack_backward(x, c["layers"], npb, a32, pattern, arg, c["gpooled"], "f32")
    delta_rule(got["gx"], gx64 * inside(c, ids), gx32 * inside(c, ids), n, f"{what} gx")
    assert not np.asarray(got["gx"])[~inside(c, ids)[:, :, 0]].any(), f"{what} gx at ids outside the table"
    grads, gaps = unpack_params(np.asarray(got["gparams"]), D, nF, nb, npb)
    assert not gaps.any(), f"{what} gaps"
    for j in range(n):
        delta_rule(grads[j][0], g64[j][0], g32[j][0], n, f"{what} gK[{j}]")
        delta_rule(grads[j][1], g64[j][1], g32[j][1], n, f"{what} gb[{j}]")


def oracle_result(c, variant, ids=None):
    """What a device run returns, from the oracle in one arithmetic (its own pattern and arg)."""
    x = case_input(c, ids)
    acts, pooled, arg = forward_oracle(c, variant, ids)
    gx, grads = stack_backward(x, c["layers"], c["npb"], acts, [a > 0 for a in acts], arg, c["gpooled"], variant)
    return dict(acts=np.stack(acts), pooled=pooled, arg=arg, gx=gx * inside(c, ids), gparams=pack_params(grads))


# ---- the net's training step, torch f64 ------------------------------------------------------------------------------
TABLE_NAMES = ("user_embeds_var", "seq_embeds_var", "item_embeds_var", "item_bias_var")
REG_NAMES = TABLE_NAMES[:3]                  # wave_net.py:169-196: `item_bias_var` has no regulariser


def conv_names(n_blocks, n_per_block):
    return [f"conv1d{'' if i == 0 else f'_{i}'}" for i in range(n_blocks * n_per_block + 1)]


class NetTwin:
    """`WaveNetNet` in torch-CPU f64 with autograd: `weights` = {name: f32 array} of the four tables (`item_bias_var`
    [n_items, 1]) and of every dense parameter under the net's names.  TF1 Adam: the rows a batch touches (every id of the
    window, the pad id included) or, `dense`, every row, with the l2 term 2 * reg * w of `tf.keras.regularizers.l2` on the three
    embedding tables; dense parameters always whole."""

    def __init__(self, weights, n_blocks, n_per_block, loss, lr, epsilon=1e-5, dense=False, reg=None, norm_embed=False):
        self.w = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in weights.items()}
        self.m = {k: torch.zeros_like(v) for k, v in self.w.items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.w.items()}
        self.nb, self.npb, self.loss, self.lr, self.eps = n_blocks, n_per_block, loss, lr, epsilon
        self.dense, self.reg, self.norm_embed, self.step = dense, reg or 0.0, norm_embed, 0

    def stack(self, w, seqs, pre=None):
        """-> the last layer's output [B, F, L]; `pre` (a list) collects every layer's pre-activation."""
        a = w["seq_embeds_var"][torch.as_tensor(np.asarray(seqs)).long()].transpose(1, 2)          # [B, C, L]
        names = conv_names(self.nb, self.npb)
        for j, name in enumerate(names):
            K, b = w[f"{name}/kernel"], w[f"{name}/bias"]
            d = dilation(j, self.npb) if j < len(names) - 1 else 1
            z = F.conv1d(F.pad(a, ((K.shape[0] - 1) * d, 0)), K.permute(2, 1, 0), b, dilation=d)
            if pre is not None:
                pre.append(z.detach())
            a = torch.relu(z)
        return a

    def user_vectors(self, w, users, seqs):
        pooled = self.stack(w, seqs).max(dim=2).values
        return torch.cat([w["user_embeds_var"][torch.as_tensor(np.asarray(users)).long()],
                          pooled @ w["dense/kernel"] + w["dense/bias"]], dim=1)

    def loss_of(self, w, users, seqs, items, labels):
        u = self.user_vectors(w, users, seqs)
        it = torch.as_tensor(np.asarray(items)).long()
        y = torch.tensor(np.asarray(labels), dtype=torch.float64)
        q = w["item_embeds_var"][it]
        if self.norm_embed:
            u, q = F.normalize(u, dim=1, eps=1e-12), F.normalize(q, dim=1, eps=1e-12)
        s = (u * q).sum(1) + w["item_bias_var"].view(-1)[it]
        if self.loss == "mse":
            return F.mse_loss(s, y)
        bce = F.binary_cross_entropy_with_logits(s, y, reduction="none")
        if self.loss == "focal":                                  # tfops/loss.py:56-62
            p = torch.sigmoid(s)
            bce = (y * 0.25 + (1 - y) * 0.75) * (1 - (y * p + (1 - y) * (1 - p))) ** 2.0 * bce
        return bce.mean()

    def margins(self, seqs):
        """(the smallest non-zero |pre-activation| of any layer, the smallest lead of a pooled maximum over the values of its
        column that differ from it) at the current weights: how far the batch is from a flipped ReLU / a flipped argmax."""
        pre = []
        last = self.stack(self.w, seqs, pre).numpy()
        z = np.abs(np.concatenate([p.numpy().reshape(-1) for p in pre]))
        lead = last.max(axis=2, keepdims=True) - last
        return float(z[z > 0].min()), float(lead[lead > 0].min()) if (lead > 0).any() else np.inf

    def train_step(self, users, seqs, items, labels):
        self.step += 1
        w = {k: v.clone().requires_grad_(True) for k, v in self.w.items()}
        loss = self.loss_of(w, users, seqs, items, labels)
        loss.backward()
        touched = {"user_embeds_var": np.unique(users), "seq_embeds_var": np.unique(seqs), "item_embeds_var": np.unique(items),
                   "item_bias_var": np.unique(items)}
        lr_t = self.lr * np.sqrt(1.0 - B2 ** self.step) / (1.0 - B1 ** self.step)
        for k, p in self.w.items():
            g = w[k].grad if w[k].grad is not None else torch.zeros_like(p)
            if k in TABLE_NAMES and not self.dense:
                rows = torch.as_tensor(touched[k]).long()
            else:
                rows = slice(None)
                if k in REG_NAMES and self.reg:
                    g = g + 2.0 * self.reg * p
            m, v = self.m[k], self.v[k]
            m[rows] = B1 * m[rows] + (1 - B1) * g[rows]
            v[rows] = B2 * v[rows] + (1 - B2) * g[rows] ** 2
            p[rows] = p[rows] - lr_t * m[rows] / (torch.sqrt(v[rows]) + self.eps)
        return float(loss.detach())


# ---- seeded training-step cases --------------------------------------------------------------------------------------
# small on purpose: Adam turns a flipped ReLU into an O(lr) difference, so the batches must keep every pre-activation and
# every pool lead well away from the forward's rounding (test_wavenet_cpu.py asserts a factor of 100), which only a net
# with few units can promise.  K and F are no multiples of 4: every tensor of the parameter buffer is followed by a gap.
STEP_SHAPE = dict(n_users=12, n_items=20, K=6, F=3, L=4, B=6, lr=0.01)
STEP_SEED = 50          # chosen on the CPU: the margins of test_wavenet_cpu.py hold with room (a factor of 500)
# (loss, dense_adam, reg, norm_embed, n_blocks, n_per_block)
STEP_CONFIGS = [("cross_entropy", False, None, False, 1, 2), ("focal", False, None, False, 1, 2), ("mse", False, None, False, 1, 2),
                ("cross_entropy", True, 0.01, False, 1, 2), ("cross_entropy", False, None, True, 1, 2),
                ("focal", False, None, False, 2, 2)]


def step_batches(n=3, seed=None):
    """n batches of (users, seqs [B, L] padded with the pad id n_items: windows ending in 0, 1, L - 1 and L pad ids, items,
    labels)."""
    S = STEP_SHAPE
    N, L, B = S["n_items"], S["L"], S["B"]
    rng = np.random.default_rng([5, STEP_SEED if seed is None else seed])
    out = []
    for _ in range(n):
        seqs = (rng.zipf(1.5, (B, L)) % N).astype(np.int32)
        for i, n_pad in enumerate([0, 1, L - 1, L]):
            seqs[i, L - n_pad:] = N
        out.append(dict(users=(rng.zipf(1.5, B) % S["n_users"]).astype(np.int32), seqs=seqs,
                        items=(rng.zipf(1.5, B) % N).astype(np.int32), labels=rng.integers(0, 2, B).astype(F32)))
    return out


def step_weights(n_blocks, n_per_block, seed=None):
    """Seeded f32 weights under the net's parameter names (shared with tests/test_wavenet_gpu.py)."""
    S = STEP_SHAPE
    rng = np.random.default_rng([7, STEP_SEED if seed is None else seed])
    N, K, nF = S["n_items"], S["K"], S["F"]
    w = {"user_embeds_var": rng.standard_normal((S["n_users"] + 1, K)) * 0.3, "seq_embeds_var": rng.standard_normal((N + 1, K)) * 0.5,
         "item_embeds_var": rng.standard_normal((N, 2 * K)) * 0.3, "item_bias_var": rng.standard_normal((N, 1)) * 0.1}
    for name, (ks, bs) in zip(conv_names(n_blocks, n_per_block), layer_shapes(K, nF, n_blocks, n_per_block)):
        w[f"{name}/kernel"] = rng.standard_normal(ks) / np.sqrt(ks[0] * ks[1]) * 1.5
        w[f"{name}/bias"] = rng.standard_normal(bs) * 0.1
    w["dense/kernel"], w["dense/bias"] = rng.standard_normal((nF, K)) * 0.3, rng.standard_normal(K) * 0.1
    return {k: v.astype(F32) for k, v in w.items()}


def step_forward_bound(w, n_blocks, n_per_block, seqs):
    """The forward bound of `check_stack` (the largest over the layers) measured on a step batch at the weights `w`."""
    names = conv_names(n_blocks, n_per_block)
    layers = [(np.asarray(w[f"{n}/kernel"]), np.asarray(w[f"{n}/bias"])) for n in names]
    x = np.asarray(w["seq_embeds_var"])[seqs]
    a64, _, _ = stack_forward(x, layers, n_per_block, "f64")
    a32, _, _ = stack_forward(x, layers, n_per_block, "f32")
    return max(delta_bound(a64[j], a32[j], j + 1) for j in range(len(layers)))
