"""CPU restatement of BPR, the yardstick of tests/test_bpr_cpu.py and tests/test_bpr_gpu.py.

(i) The engine (`libreco/algorithms/_bpr.pyx:116-399`) under the window semantics of DESIGN.md §7.4: an epoch's samples
are cut into windows of `window` consecutive samples; inside a window d (`_bpr.pyx:161-166`), c = 1 / (1 + exp(d)) and
every gradient (`:168-179`, the `reg` term included) come from the tables as they stood when the window began; each
touched row then takes the reference's optimiser step (sgd `:181-190`, momentum `:273-280`, adam `:376-399`, bias
correction by the epoch) once per occurrence in ascending sample order, positives and negatives of an item in one chain.
With `window=1` this is the reference's loop at `num_threads=1`.  Rows are independent once the gradients are fixed, so
the chains are walked level by level (the k-th occurrence of every row together); that is the same arithmetic in the same
per-row order.  Two variants of the intermediates: "f64" rounds where the C code does (float products c * x, double
`- reg * x`, `lr * g`, Adam in double, every store f32), "f32" keeps every intermediate in f32 as the device does.

(ii) The mini-batch mode (`libreco/algorithms/bpr.py:161-204`, `libreco/tfops/loss.py:23`): loss, autograd gradients and
the TF1 Adam step (`tf.train.AdamOptimizer`, sparse rows or dense) in torch on the CPU.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
OPTIMIZERS = ("sgd", "momentum", "adam")
MOMENTUM, RHO1, RHO2 = 0.9, 0.9, 0.999      # bpr.py:319, _bpr.pyx:51-52


def truncated_normal_tables(n_users, n_items, embed_size, seed):
    """`bpr.py:143-159`: users then items from one generator, scale 0.03, user bias column 1, item bias column 0
    (`libreco/utils/initializers.py:4-21`: f32 draws, up to five redraws of what lies outside two standard deviations)."""
    rng = np.random.default_rng(seed)

    def tn(shape, scale=0.03):
        x = rng.normal(0.0, scale, int(np.prod(shape))).astype(F32)
        for _ in range(5):
            bad = np.logical_or(x > 2 * scale, x < -2 * scale)
            if not bad.any():
                break
            x[bad] = rng.normal(0.0, scale, int(bad.sum()))
        return x.reshape(shape)

    U = tn((n_users, embed_size + 1))
    U[:, embed_size] = 1.0
    I = tn((n_items, embed_size + 1))
    I[:, embed_size] = 0.0
    return U, I


def new_state(optimizer, U, I):
    n = {"sgd": 0, "momentum": 1, "adam": 2}[optimizer]
    return {"u": [np.zeros_like(U) for _ in range(n)], "i": [np.zeros_like(I) for _ in range(n)]}


def triple_score(U, I, users, pos, neg, variant="f64", ibias=None):
    """(d, c, -log sigmoid(d), p - q) of the samples; `variant` as in the module docstring."""
    u, diff = U[users], I[pos] - I[neg]                     # float - float (`_bpr.pyx:163-165`)
    if variant == "f64":
        d = (u.astype(np.float64) * diff.astype(np.float64)).sum(1)
        if ibias is not None:
            d = d + ibias[pos].astype(np.float64) - ibias[neg]
        with np.errstate(over="ignore"):
            c = 1.0 / (1.0 + np.exp(d))
        loss = np.maximum(-d, 0.0) + np.log1p(np.exp(-np.abs(d)))
        return d, c, loss, diff
    d = (u * diff).sum(1, dtype=F32)
    if ibias is not None:
        d = d + (ibias[pos] - ibias[neg])
    with np.errstate(over="ignore"):
        c = F32(1) / (F32(1) + np.exp(d))
    loss = np.maximum(-d, F32(0)) + np.log1p(np.exp(-np.abs(d)))
    return d, c, loss, diff


def _step(optimizer, variant, x, st, gdir, x0, lr, reg, epoch):
    """One optimiser step of the rows `x` (f32, [n, cols]) with gradient gdir - reg * x0; returns the new (x, st)."""
    if variant == "f64":
        g = (gdir.astype(np.float64) - reg * x0.astype(np.float64)).astype(F32)          # `_bpr.pyx:169-179`
        if optimizer == "sgd":
            return (x.astype(np.float64) + lr * g.astype(np.float64)).astype(F32), st     # `:181-183`
        if optimizer == "momentum":
            v = (MOMENTUM * st[0].astype(np.float64) + lr * g.astype(np.float64)).astype(F32)   # `:274`
            return x + v, [v]                                                             # `:275` float + float
        m = (RHO1 * st[0].astype(np.float64) + (1.0 - RHO1) * g.astype(np.float64)).astype(F32)        # `:377`
        h = (RHO2 * st[1].astype(np.float64) + (1.0 - RHO2) * g.astype(np.float64) ** 2).astype(F32)   # `:378`
        um = (m.astype(np.float64) / (1.0 - RHO1 ** epoch)).astype(F32)                    # `:379`
        uh = (h.astype(np.float64) / (1.0 - RHO2 ** epoch)).astype(F32)                    # `:380`
        x = (x.astype(np.float64) + lr * um.astype(np.float64) / (np.sqrt(uh.astype(np.float64)) + 1e-8)).astype(F32)
        return x, [m, h]
    lr, reg = F32(lr), F32(reg)
    g = gdir - reg * x0
    if optimizer == "sgd":
        return x + lr * g, st
    if optimizer == "momentum":
        v = F32(MOMENTUM) * st[0] + lr * g
        return x + v, [v]
    m = F32(RHO1) * st[0] + F32(1.0 - RHO1) * g
    h = F32(RHO2) * st[1] + F32(1.0 - RHO2) * (g * g)
    bc1, bc2 = F32(1.0 - RHO1 ** epoch), F32(1.0 - RHO2 ** epoch)
    return x + lr * (m / bc1) / (np.sqrt(h / bc2) + F32(1e-8)), [m, h]


def _chains(optimizer, variant, table, states, ids, gdir, cols, lr, reg, epoch, chain, reg_term):
    """Walk every row's chain: `ids` [n] in sample order, `gdir` [n, cols] the c-part of each occurrence's gradient."""
    n = len(ids)
    order = np.argsort(ids, kind="stable")
    sorted_ids = ids[order]
    first = np.r_[True, sorted_ids[1:] != sorted_ids[:-1]]
    start = np.maximum.accumulate(np.where(first, np.arange(n), 0))
    rank = np.arange(n) - start                               # k-th occurrence of its row, ascending sample order
    if chain == "descending":
        last = np.r_[sorted_ids[1:] != sorted_ids[:-1], True]
        end = np.minimum.accumulate(np.where(last, np.arange(n), n)[::-1])[::-1]
        rank = end - np.arange(n)
    elif chain != "ascending":
        raise ValueError(chain)
    snap = table[:, :cols].copy() if reg_term == "stale" else None
    for level in range(int(rank.max()) + 1 if n else 0):
        sel = order[rank == level]
        rows = ids[sel]
        x = table[rows, :cols]
        x0 = snap[rows] if snap is not None else x
        st = [s[rows, :cols] for s in states]
        x, st = _step(optimizer, variant, x, st, gdir[sel], x0, lr, reg, epoch)
        table[rows, :cols] = x
        for s, v in zip(states, st):
            s[rows, :cols] = v


def engine_epoch(optimizer, users, pos, neg, U, I, state, lr, reg, epoch, window, variant="f64", chain="ascending",
                 reg_term="stale"):
    """One epoch over the given triples, in place on U, I (f32 [n, K + 1]) and `state` (`new_state`).  `chain` and
    `reg_term` exist so that the tests can show that the other readings of the semantics differ measurably."""
    assert U.dtype == F32 and I.dtype == F32 and variant in ("f64", "f32")
    K = U.shape[1] - 1
    reg = reg or 0.0
    for a in range(0, len(users), window):
        u, p, q = users[a:a + window], pos[a:a + window], neg[a:a + window]
        _, c, _, diff = triple_score(U, I, u, p, q, variant)
        c = c.astype(F32)[:, None]
        urows = U[u]
        g_user = (c * diff)[:, :K]                            # float * float (`_bpr.pyx:169`)
        g_item = np.empty((2 * len(u), K + 1), dtype=F32)
        g_item[0::2] = c * urows                              # `:172-175`
        g_item[1::2] = -c * urows                             # `:176-179`
        items2 = np.stack([p, q], 1).reshape(-1)
        _chains(optimizer, variant, I, state["i"], items2, g_item, K + 1, lr, reg, epoch, chain, reg_term)
        _chains(optimizer, variant, U, state["u"], u, g_user, K, lr, reg, epoch, chain, reg_term)


def pair_auc(U, I, users, pos, seed=0):
    """Share of (user, positive) pairs scored above one random item each (ties count half)."""
    rng = np.random.default_rng(seed)
    rnd = rng.integers(0, I.shape[0], size=len(users))
    sp = (U[users].astype(np.float64) * I[pos]).sum(1)
    sr = (U[users].astype(np.float64) * I[rnd]).sum(1)
    return float(((sp > sr) + 0.5 * (sp == sr)).mean())


# ---- (ii) the mini-batch mode ------------------------------------------------------------
def minibatch_step(params, adam, users, pos, neg, lr, step, epsilon=1e-5, reg=None, norm_embed=False, dense=False):
    """One step of `bpr.py:161-204` + `tf.train.AdamOptimizer(lr, epsilon=epsilon)` in torch-CPU f64 autograd with f32
    stores.  `params` = {"user" [nu, K], "item" [ni, K], "bias" [ni]} f32 numpy, `adam` = {name: (m, v)}; both updated in
    place.  `dense`: TF1's dense apply (every row decays and moves); otherwise only the rows of the batch (the package's
    row-wise default).  `reg`: `tf.keras.regularizers.l2` on the three whole variables (`tfops/configs.py:reg_config`),
    only meaningful with `dense`.  Returns the loss (without the reg term, as the reference prints it)."""
    import torch

    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    iu, ip, iq = (torch.as_tensor(np.asarray(a, dtype=np.int64)) for a in (users, pos, neg))
    u, p, q = t["user"][iu], t["item"][ip], t["item"][iq]
    if norm_embed:                                            # `bpr.py:196-199`, `utils/misc.py:normalize_embeds` (tf.linalg.l2_normalize)
        u, p, q = (x * torch.rsqrt(torch.clamp((x * x).sum(1, keepdim=True), min=1e-12)) for x in (u, p, q))
    d = t["bias"][ip] - t["bias"][iq] + (u * (p - q)).sum(1)   # `bpr.py:201-203`
    loss = -torch.nn.functional.logsigmoid(d).mean()           # `tfops/loss.py:23`
    total = loss
    if reg:
        total = total + sum(reg * (x * x).sum() for x in t.values())
    total.backward()
    b1, b2 = 0.9, 0.999
    lr_t = lr * np.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step)
    touched = {"user": np.unique(users), "item": np.unique(np.r_[pos, neg]), "bias": np.unique(np.r_[pos, neg])}
    for name, w in params.items():
        g = t[name].grad.numpy().astype(F32)
        m, v = adam[name]
        rows = slice(None) if dense else touched[name]
        gm = g[rows]
        m[rows] = (b1 * m[rows].astype(np.float64) + (1.0 - b1) * gm).astype(F32)
        v[rows] = (b2 * v[rows].astype(np.float64) + (1.0 - b2) * gm.astype(np.float64) ** 2).astype(F32)
        w[rows] = (w[rows].astype(np.float64) - lr_t * m[rows] / (np.sqrt(v[rows].astype(np.float64)) + epsilon)).astype(F32)
    return float(loss.detach())


# ---- shared cases ------------------------------------------------------------------------
WINDOW_LR = {"sgd": 0.05, "momentum": 0.01, "adam": 0.001}


def window_case(K, optimizer, seed=0, n_users=300, n_items=200, W=4096, head_share=0.06):
    """One window from non-zero states: every row many times, item 0 the positive of about `head_share` of the samples;
    tables N(0, 0.3), first moments N(0, 0.01), second moments |N(0, 1e-3)|."""
    rng = np.random.default_rng(seed)
    users = rng.integers(0, n_users, W).astype(np.int32)
    pos = rng.integers(1, n_items, W).astype(np.int32)
    pos[rng.random(W) < head_share] = 0
    neg = ((pos + rng.integers(1, n_items, W)) % n_items).astype(np.int32)
    U = rng.normal(0, 0.3, (n_users, K + 1)).astype(F32)
    U[:, K] = 1.0
    I = rng.normal(0, 0.3, (n_items, K + 1)).astype(F32)
    state = new_state(optimizer, U, I)
    for side in "ui":
        for n, s in enumerate(state[side]):
            s[:] = np.abs(rng.normal(0, 1e-3, s.shape)) if n == 1 else rng.normal(0, 0.01, s.shape)
        if side == "u":
            for s in state[side]:
                s[:, K] = 0.0                                 # the user bias column has no state: it is never written
    return users, pos, neg, U, I, state


def copy_case(U, I, state):
    return U.copy(), I.copy(), {k: [s.copy() for s in v] for k, v in state.items()}


def case_arrays(U, I, state):
    return [U, I, *state["u"], *state["i"]]


def max_diff(a, b):
    return max(float(np.abs(x.astype(np.float64) - y).max()) for x, y in zip(a, b))


def unconsumed_negatives(rng, users, n_items, consumed_sets):
    """One uniform negative per sample outside the user's consumed set (`_bpr.pyx:153-155`)."""
    neg = rng.integers(0, n_items, len(users))
    while True:
        bad = np.fromiter((neg[j] in consumed_sets[u] for j, u in enumerate(users)), dtype=bool, count=len(users))
        if not bad.any():
            return neg.astype(np.int32)
        neg[bad] = rng.integers(0, n_items, int(bad.sum()))


def quality_engine(optimizer, users, items, n_users, n_items, consumed_sets, eval_users, eval_items, seed, lr, K=16,
                   n_epochs=6, window=256, reg=0.0):
    """Pair AUC on the held-out pairs after `n_epochs` of the windowed engine (f64 variant) from the reference's draws."""
    U, I = truncated_normal_tables(n_users, n_items, K, seed)
    state = new_state(optimizer, U, I)
    rng = np.random.default_rng(seed)
    for epoch in range(1, n_epochs + 1):
        mask = rng.permutation(len(users))
        u, p = users[mask], items[mask]
        q = unconsumed_negatives(rng, u, n_items, consumed_sets)
        engine_epoch(optimizer, u, p, q, U, I, state, lr, reg, epoch, window, "f64")
    return pair_auc(U, I, eval_users, eval_items, seed=0)


def quality_minibatch(users, items, n_users, n_items, eval_users, eval_items, seed, lr=0.001, K=16, n_epochs=6, batch=256):
    """The same figure for the mini-batch mode: glorot-uniform variables, random negatives (!= positive), row-wise Adam."""
    rng = np.random.default_rng(seed)

    def glorot(shape):
        lim = np.sqrt(6.0 / (shape[0] + shape[-1])) if len(shape) == 2 else np.sqrt(6.0 / (2 * shape[0]))
        return rng.uniform(-lim, lim, shape).astype(F32)

    params = {"user": glorot((n_users, K)), "item": glorot((n_items, K)), "bias": glorot((n_items,))}
    adam = {k: (np.zeros_like(v), np.zeros_like(v)) for k, v in params.items()}
    step = 0
    for _ in range(n_epochs):
        mask = rng.permutation(len(users))
        for a in range(0, len(users), batch):
            u, p = users[mask[a:a + batch]], items[mask[a:a + batch]]
            q = ((p + rng.integers(1, n_items, len(p))) % n_items).astype(np.int32)
            step += 1
            minibatch_step(params, adam, u, p, q, lr, step)
    U = np.concatenate([params["user"], np.ones((n_users, 1), F32)], 1)
    I = np.concatenate([params["item"], params["bias"][:, None]], 1)
    return pair_auc(U, I, eval_users, eval_items, seed=0)
