"""f64 numpy model of NCF (He et al. 2017), written from the reference's graph (`libreco/algorithms/ncf.py`: two embedding
lookups, gmf = u * i, mlp = dense_nn(concat[u | i]), logit = Dense(1)(concat[gmf | mlp])) and its `dense_nn` (input BatchNorm;
Dense -> relu -> BatchNorm per hidden layer; the last layer bare), with seeded f32 case builders for the kernels of
csrc/ncf.hip.

  pair_case / pair_ref          the front and back of the two-field step (`lr_ncf_pair_fwd_f32`, `lr_ncf_pair_bwd_f32`)
  score_case / score_ref        the inference tower of `lr_ncf_score_f32`, in f64 and in numpy f32 (the delta rule's yardstick)
  score_lds_bytes               the LDS a stack needs under the layout the header states: the envelope, restated
  NCFOracle                     forward (training / inference BatchNorm), loss, every gradient, one whole step: TF-style Adam on
                                the touched rows (duplicates summed first) and on the dense parameters, BatchNorm moving averages
  tail                          everything behind the first Dense layer (what `DeepFMTail` computes), forward and backward
"""
from __future__ import annotations

import functools

import numpy as np

F32 = np.float32
BN_EPS, BN_MOMENTUM = 1e-3, 0.99
B1, B2 = 0.9, 0.999


# ---- BatchNorm -------------------------------------------------------------------------------------------------------------
def bn_train(x, gamma, beta):
    mean, var = x.mean(0), x.var(0)                       # biased variance, like tf.nn.moments
    inv = 1.0 / np.sqrt(var + BN_EPS)
    xhat = (x - mean) * inv
    return gamma * xhat + beta, (xhat, inv, gamma), mean, var


def bn_train_bwd(gy, cache):
    xhat, inv, gamma = cache
    gx = gamma * inv * (gy - gy.mean(0) - xhat * (gy * xhat).mean(0))
    return gx, (gy * xhat).sum(0), gy.sum(0)


def bn_eval(x, gamma, beta, mean, var):
    return (x - mean) / np.sqrt(var + BN_EPS) * gamma + beta


def loss_and_gl(logits, labels, loss_type="cross_entropy"):
    """(mean loss, d loss / d logit)."""
    n = len(logits)
    if loss_type == "cross_entropy":                      # sigmoid cross entropy with logits, mean over the batch
        loss = np.maximum(logits, 0) - logits * labels + np.log1p(np.exp(-np.abs(logits)))
        return loss.mean(), (1.0 / (1.0 + np.exp(-logits)) - labels) / n
    if loss_type == "mse":
        return ((logits - labels) ** 2).mean(), 2.0 * (logits - labels) / n
    raise ValueError(loss_type)


# ---- names of the dense parameters, as `DenseStack(P, "mlp", ...)` and `TFDense(P, "out", ...)` register them ---------------------
def kernel(i):
    return f"mlp/mlp_layer{i}/kernel"


def bias(i):
    return f"mlp/mlp_layer{i}/bias"


def bn_names(key):
    return f"mlp/{key}/gamma", f"mlp/{key}/beta"


def tail(P, n_layers, use_bn, z1, gmf, labels=None, training=True, bn_stats=None, loss_type="cross_entropy"):
    """Everything behind the first Dense layer, whose output `z1` is: relu -> BatchNorm -> Dense ... (the last Dense bare), then
    logit = concat[gmf | mlp] @ out/kernel + out/bias.  With `labels`: the loss and the gradients of z1, gmf and of every
    parameter touched; `stats` holds the batch statistics of every BatchNorm passed (training), `margin` the smallest |input| of
    any relu: the distance of the batch from a kink of the model, where its gradient jumps."""
    L, z, caches, stats, margin = n_layers, z1, [], {}, np.inf
    for i in range(1, L):
        margin = min(margin, float(np.abs(z).min()))
        a = np.maximum(z, 0.0)
        if use_bn:
            g, b = (P[k] for k in bn_names(f"bn{i}"))
            if training:
                y, cache, mean, var = bn_train(a, g, b)
                stats[f"bn{i}"] = (mean, var)
            else:
                y, cache = bn_eval(a, g, b, *bn_stats[f"bn{i}"]), None
        else:
            y, cache = a, None
        caches.append((z, y, cache))
        z = y @ P[kernel(i + 1)] + P[bias(i + 1)]
    wo, bo = P["out/kernel"].reshape(-1), P["out/bias"].reshape(-1)[0]
    concat = np.concatenate([gmf, z], axis=1)
    logits = concat @ wo + bo
    out = dict(logits=logits, stats=stats, margin=margin)
    if labels is None:
        return out
    loss, gl = loss_and_gl(logits, labels, loss_type)
    grads = {"out/kernel": (concat.T @ gl).reshape(-1, 1), "out/bias": np.array([gl.sum()])}
    gcat = gl[:, None] * wo[None, :]
    K = gmf.shape[1]
    ggmf, gz = gcat[:, :K], gcat[:, K:]
    for i in range(L - 1, 0, -1):
        zin, y, cache = caches[i - 1]
        grads[kernel(i + 1)], grads[bias(i + 1)] = y.T @ gz, gz.sum(0)
        gy = gz @ P[kernel(i + 1)].T
        if cache is not None:
            gy, dgamma, dbeta = bn_train_bwd(gy, cache)
            grads[bn_names(f"bn{i}")[0]], grads[bn_names(f"bn{i}")[1]] = dgamma, dbeta
        gz = gy * (zin > 0)
    out.update(loss=loss, gl=gl, gz1=gz, ggmf=ggmf, grads=grads)
    return out


class NCFOracle:
    """`state`: dict(embed [V, K], P {name: array}, bn {key: (moving mean, moving var)}) as `export_state` returns it."""

    def __init__(self, state, K, n_layers, use_bn, lr, eps=1e-5):
        f64 = lambda a: np.array(a, dtype=np.float64)
        self.embed = f64(state["embed"])
        self.P = {k: f64(v) for k, v in state["P"].items()}
        self.bn = {k: (f64(m), f64(v)) for k, (m, v) in state["bn"].items()}
        self.K, self.L, self.use_bn, self.lr, self.eps, self.step = K, n_layers, use_bn, lr, eps, 0
        self.m, self.v = np.zeros_like(self.embed), np.zeros_like(self.embed)
        self.margin = np.inf                # the smallest |relu input| any training batch has seen (see `tail`)
        self.Pm = {k: np.zeros_like(v) for k, v in self.P.items()}
        self.Pv = {k: np.zeros_like(v) for k, v in self.P.items()}

    def _first(self, x, training):
        """z1 = Dense1(BN_in(x)); returns (z1, the Dense's input, the BatchNorm's cache, its batch statistics)."""
        P, cache, stats = self.P, None, None
        xb = x
        if self.use_bn:
            g, b = (P[k] for k in bn_names("bn_in"))
            if training:
                xb, cache, mean, var = bn_train(x, g, b)
                stats = (mean, var)
            else:
                xb = bn_eval(x, g, b, *self.bn["bn_in"])
        return xb @ P[kernel(1)] + P[bias(1)], xb, cache, stats

    def forward(self, rows):
        """Inference logits of the pairs `rows` [n, 2] (global rows; one outside the table reads as a zero row)."""
        rows = np.asarray(rows)
        ok = (rows >= 0) & (rows < len(self.embed))
        e = np.where(ok[:, :, None], self.embed[np.where(ok, rows, 0)], 0.0)
        u, i = e[:, 0], e[:, 1]
        z1 = self._first(np.concatenate([u, i], axis=1), False)[0]
        return tail(self.P, self.L, self.use_bn, z1, u * i, training=False, bn_stats=self.bn)["logits"]

    def gradients(self, rows, labels, loss_type="cross_entropy"):
        """(loss, per-position row gradients [B, 2, K], {name: gradient}, {key: batch statistics}) in training mode."""
        rows, K = np.asarray(rows), self.K
        u, i = self.embed[rows[:, 0]], self.embed[rows[:, 1]]
        x = np.concatenate([u, i], axis=1)
        z1, xb, cache, stats_in = self._first(x, True)
        t = tail(self.P, self.L, self.use_bn, z1, u * i, np.asarray(labels, dtype=np.float64), loss_type=loss_type)
        grads, gz1 = t["grads"], t["gz1"]
        self.margin = min(self.margin, t["margin"])
        grads[kernel(1)], grads[bias(1)] = xb.T @ gz1, gz1.sum(0)
        gx = gz1 @ self.P[kernel(1)].T
        stats = dict(t["stats"])
        if cache is not None:
            gx, dgamma, dbeta = bn_train_bwd(gx, cache)
            grads[bn_names("bn_in")[0]], grads[bn_names("bn_in")[1]] = dgamma, dbeta
            stats["bn_in"] = stats_in
        ge = np.stack([gx[:, :K] + t["ggmf"] * i, gx[:, K:] + t["ggmf"] * u], axis=1)
        return t["loss"], ge, grads, stats

    def _adam(self, w, m, v, g, lr_t):
        m[...] = B1 * m + (1 - B1) * g
        v[...] = B2 * v + (1 - B2) * g * g
        w[...] = w - lr_t * m / (np.sqrt(v) + self.eps)

    def train_step(self, rows, labels, loss_type="cross_entropy"):
        """One step: TF1 Adam (lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), epsilon outside the root) on the rows the batch touches
        with duplicates summed first, and on every dense parameter; the moving averages take the batch statistics."""
        rows = np.asarray(rows)
        loss, ge, grads, stats = self.gradients(rows, labels, loss_type)
        self.step += 1
        lr_t = self.lr * np.sqrt(1 - B2 ** self.step) / (1 - B1 ** self.step)
        gsum = np.zeros_like(self.embed)
        np.add.at(gsum, rows.reshape(-1), ge.reshape(-1, self.K))
        touched = np.unique(rows)
        w, m, v = self.embed[touched], self.m[touched], self.v[touched]
        self._adam(w, m, v, gsum[touched], lr_t)
        self.embed[touched], self.m[touched], self.v[touched] = w, m, v
        for k in self.P:
            self._adam(self.P[k], self.Pm[k], self.Pv[k], grads[k].reshape(self.P[k].shape), lr_t)
        for k, (mean, var) in stats.items():
            mm, mv = self.bn[k]
            self.bn[k] = (mm * BN_MOMENTUM + mean * (1 - BN_MOMENTUM), mv * BN_MOMENTUM + var * (1 - BN_MOMENTUM))
        return float(loss)


KINK_MARGIN = 1e-5


@functools.lru_cache(maxsize=None)
def step_batches(K, hidden, use_bn, n_steps=3, B=200, state_seed=31, lr=0.01):
    """(state, [(users, items, labels)] x n_steps) for the training-step tests: pairs with duplicates over users < 30 and
    items < 45, so that the rows above stay untouched.

    The gradient of a relu net jumps where a relu's input crosses zero.  A batch whose f64 forward puts some input within f32
    rounding of zero (a sum of up to 128 O(1) terms: a few 1e-7, plus the 1e-6 the parameters of two f32 Adam steps differ by)
    cannot be matched by ANY f32 implementation: whichever side its rounding falls on, that sample's whole contribution to
    the gradient is there or not.  Some 150,000 relu inputs pass in three steps at B = 200, so such a batch is no rarity.  The
    batches are therefore the first seed's whose smallest |relu input| over all steps of the ORACLE's run is at least
    KINK_MARGIN = 1e-5, ten times that rounding; the choice reads nothing from the code under test."""
    state = random_state(state_seed, N_USERS, N_ITEMS, K, hidden, use_bn)
    for seed in range(3, 200):
        rng = np.random.default_rng(seed)
        batches = [(rng.integers(0, 30, B), rng.integers(0, 45, B), rng.integers(0, 2, B).astype(F32)) for _ in range(n_steps)]
        oracle = NCFOracle(state, K, len(hidden), use_bn, lr)
        for users, items, labels in batches:
            oracle.train_step(np.stack([users, N_USERS + 1 + items], axis=1), labels)
        if oracle.margin >= KINK_MARGIN:
            return state, batches
    raise AssertionError("no seed keeps the batches away from the relu kinks")


def export_state(net):
    """The state of an `NCFNet` as numpy arrays."""
    bns = [("bn_in", net.mlp.bn_in)] + [(f"bn{i}", bn) for i, bn in enumerate(net.mlp.bns, start=1)]
    return dict(embed=net.tables.embed.detach().cpu().numpy().copy(),
                P={k: p.detach().cpu().numpy().copy() for k, p in net.P.params.items()},
                bn={k: (bn.moving_mean.cpu().numpy().copy(), bn.moving_var.cpu().numpy().copy()) for k, bn in bns if bn is not None})


def random_state(seed, n_users, n_items, K, hidden, use_bn):
    """A seeded f32 state with every BatchNorm away from its initial values (the affines and moving averages matter)."""
    rng = np.random.default_rng(seed)
    f = lambda *s, lo=-0.5, hi=0.5: rng.uniform(lo, hi, s).astype(F32)
    P, bn, d = {}, {}, 2 * K
    if use_bn:
        P["mlp/bn_in/gamma"], P["mlp/bn_in/beta"] = f(d, lo=0.5, hi=1.5), f(d)
        bn["bn_in"] = (f(d, lo=-0.2, hi=0.2), f(d, lo=0.5, hi=1.5))
    for i, h in enumerate(hidden, start=1):
        lim = np.sqrt(6.0 / (d + h))
        P[kernel(i)], P[bias(i)] = f(d, h, lo=-lim, hi=lim), f(h, lo=-0.1, hi=0.1)
        if use_bn and i < len(hidden):
            P[f"mlp/bn{i}/gamma"], P[f"mlp/bn{i}/beta"] = f(h, lo=0.5, hi=1.5), f(h)
            bn[f"bn{i}"] = (f(h, lo=0.0, hi=0.3), f(h, lo=0.5, hi=1.5))
        d = h
    P["out/kernel"], P["out/bias"] = f(K + d, 1), f(1)
    return dict(embed=f(n_users + 1 + n_items + 1, K), P=P, bn=bn)


def inference_fold(state, K, n_layers, use_bn, dtype=np.float64):
    """(W, b, s, t, wg, wd, c) of `lr_ncf_score_f32` from a state: the input BatchNorm folded into the first layer, each hidden
    BatchNorm as the affine behind its relu."""
    P = {k: np.asarray(v, dtype=dtype) for k, v in state["P"].items()}
    W = [P[kernel(i)] for i in range(1, n_layers + 1)]
    b = [P[bias(i)] for i in range(1, n_layers + 1)]
    s, t = [None] * n_layers, [None] * n_layers
    if use_bn:
        def aff(key):
            mean, var = (np.asarray(a, dtype=dtype) for a in state["bn"][key])
            sc = P[bn_names(key)[0]] / np.sqrt(var + dtype(BN_EPS))
            return sc, P[bn_names(key)[1]] - mean * sc

        sc, sh = aff("bn_in")
        W[0], b[0] = W[0] * sc[:, None], b[0] + sh @ W[0]
        for i in range(1, n_layers):
            s[i - 1], t[i - 1] = aff(f"bn{i}")
    wo = P["out/kernel"].reshape(-1)
    return W, b, s, t, wo[:K], wo[K:], P["out/bias"].reshape(-1)[0]


# ---- kernel cases ----------------------------------------------------------------------------------------------------------
N_USERS, N_ITEMS = 37, 53


def special_pairs(n_users=N_USERS, n_items=N_ITEMS):
    """Global (user row, item row) pairs every case opens with: both OOV rows, a duplicate pair, one id outside the table."""
    io = n_users + 1
    V = io + n_items + 1
    return np.array([[n_users, io + n_items], [3, io + 5], [3, io + 5], [V, io + 7], [4, -1]], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def pair_case(B, K, seed=0):
    """Seeded f32 inputs of the pair kernels.  Magnitudes: |gl wg x| <= 0.25 against 1 <= |G| <= 2, so that G + (gl wg) x does not
    cancel and a relative tolerance alone is meaningful."""
    rng = np.random.default_rng(1000 * B + K + seed)
    V = N_USERS + 1 + N_ITEMS + 1
    idx = np.stack([rng.integers(0, N_USERS + 1, B), N_USERS + 1 + rng.integers(0, N_ITEMS + 1, B)], axis=1).astype(np.int32)
    sp = special_pairs()
    if B >= len(sp):
        idx[:len(sp)] = sp
    else:
        idx[:B] = sp[[0, 3, 4][:B]] if B <= 3 else sp[:B]
    table = rng.uniform(-0.5, 0.5, (V, K)).astype(F32)
    G = (rng.uniform(1.0, 2.0, (B, 2 * K)) * rng.choice([-1.0, 1.0], (B, 2 * K))).astype(F32)
    return dict(V=V, K=K, B=B, table=table, idx=idx, gl=rng.uniform(-1, 1, B).astype(F32), wg=rng.uniform(-0.5, 0.5, K).astype(F32), G=G)


def gather(table, rows, dtype):
    rows = np.asarray(rows)
    ok = (rows >= 0) & (rows < len(table))
    return np.where(ok[..., None], table[np.where(ok, rows, 0)].astype(dtype), dtype(0))


def pair_ref(c):
    """x, gmf in numpy f32 (compared by bits) and G in f64."""
    e = gather(c["table"], c["idx"], F32)
    u, i = e[:, 0], e[:, 1]
    x, gmf = np.concatenate([u, i], axis=1), u * i
    cg = c["gl"].astype(np.float64)[:, None] * c["wg"].astype(np.float64)[None, :]
    G = c["G"].astype(np.float64) + np.concatenate([cg * i, cg * u], axis=1)
    return x, gmf, G


SCORE_STACKS = [(16,), (32, 16), (128, 64, 32), (64, 64, 64, 16), (256, 16)]
SCORE_KS = [4, 16, 64]
SCORE_NS = [1, 63, 64, 65, 130, 4097]


def score_lds_bytes(K, widths):
    """Bytes of LDS of `lr_ncf_score_f32` (include/libreco_hip.h): every layer's weights [d_in][width rounded up to 32] and two
    activation tiles of 68-float rows, one as tall as max(2K, the widths of the even layers), one as tall as those of the odd."""
    d, floats, rows = 2 * K, 0, [2 * K, 0]
    for l, w in enumerate(widths):
        floats += d * (-(-w // 32) * 32)
        rows[(l + 1) & 1] = max(rows[(l + 1) & 1], w)
        d = w
    return 4 * (floats + 68 * sum(rows))


def score_envelope(K, widths):
    return bool(K % 4 == 0 and 4 <= K <= 128 and 1 <= len(widths) <= 4 and all(w % 16 == 0 and 16 <= w <= 256 for w in widths)
                and score_lds_bytes(K, widths) <= 160 * 1024)


@functools.lru_cache(maxsize=None)
def score_case(K, widths, affine, n=max(SCORE_NS)):
    """Seeded f32 inputs of the score kernel for `n` pairs; a case of fewer pairs is a prefix of this one (same weights)."""
    L = len(widths)
    st = random_state(7 + 13 * K + len(widths), N_USERS, N_ITEMS, K, widths, affine)
    W, b, s, t, wg, wd, c = inference_fold(st, K, L, affine, dtype=F32)
    rng = np.random.default_rng(99 + K)
    users = rng.integers(0, N_USERS + 1, n).astype(np.int32)
    items = (N_USERS + 1 + rng.integers(0, N_ITEMS + 1, n)).astype(np.int32)
    sp = special_pairs()
    users[1:1 + len(sp)], items[1:1 + len(sp)] = sp[:, 0], sp[:, 1]          # (pair 0 stays an ordinary one: n = 1)
    as32 = lambda xs: [None if x is None else np.ascontiguousarray(x, dtype=F32) for x in xs]
    return dict(K=K, widths=widths, table=st["embed"], users=users, items=items, W=as32(W), b=as32(b), s=as32(s), t=as32(t),
                wg=np.ascontiguousarray(wg, dtype=F32), wd=np.ascontiguousarray(wd, dtype=F32), c=float(c))


@functools.lru_cache(maxsize=None)
def _score_ref(K, widths, affine, dtype):
    c = score_case(K, widths, affine)
    dt = np.dtype(dtype).type
    e_u, e_i = gather(c["table"], c["users"], dt), gather(c["table"], c["items"], dt)
    h = np.concatenate([e_u, e_i], axis=1)
    L = len(widths)
    for l in range(L):
        h = h @ c["W"][l].astype(dt) + c["b"][l].astype(dt)
        if l < L - 1:
            h = np.maximum(h, dt(0))
            if c["s"][l] is not None:
                h = h * c["s"][l].astype(dt) + c["t"][l].astype(dt)
    return ((e_u * e_i) @ c["wg"].astype(dt) + h @ c["wd"].astype(dt) + dt(c["c"])).astype(dt)


def score_ref(K, widths, affine, dtype="f64"):
    """The scores of the whole case (computed once per case and precision, shared, read-only)."""
    out = _score_ref(K, tuple(widths), bool(affine), "float64" if dtype == "f64" else "float32")
    out.setflags(write=False)
    return out
