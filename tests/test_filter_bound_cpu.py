"""The inequality the filtered scoring form rests on (csrc/score_topk.hip, "Filtered scoring"), checked in numpy: for f32 vectors
u, i with elements rounded to bf16 (round to nearest even) and products accumulated in f32,

    | sum_k bf(u_k) bf(i_k)  -  sum_k u_k i_k |  <=  0.004 |u| |i|      (kFiltDelta)

so that  approx + 0.004 |u| |i|  is an upper bound of the exact score — on random vectors, on vectors built so that every element
sits just below / above its bf16 rounding midpoint (the worst case of the rounding), and on wide dynamic ranges.  The kernel adds the
term with both norms rounded UP to bf16 (and the item norm computed from the rounded row, inflated by 1 + 2^-8): also checked.

Below the normal range (`check_scaled`, the power-of-two sweeps): the squares of a norm underflow, and the term with them, while
the rounding error of `approx` stays — the kernel replaces a norm it cannot trust by a floor (kFiltMinN2 / kFiltNormFloor), and
the sweep holds the bound to `>= exact` for every pair, with the kernel's own f32 norms and no additive slack."""
import numpy as np
import pytest

DELTA = 0.004               # kFiltDelta
MIN_N2 = 2.0 ** -64         # kFiltMinN2 (csrc/score_topk.hip): an f32 squared norm below it is not trusted ...
NORM_FLOOR = 2.0 ** -20     # kFiltNormFloor: ... and the row enters the bound with this norm instead


def bf16_rne(x: np.ndarray) -> np.ndarray:
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) << np.uint64(16)
    return r.astype(np.uint32).view(np.float32)


def bf16_up(x: np.ndarray) -> np.ndarray:          # x >= 0
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + np.where(b & np.uint64(0xFFFF), np.uint64(0x10000), np.uint64(0))) >> np.uint64(16)) << np.uint64(16)
    return r.astype(np.uint32).view(np.float32)


def approx_f32(ub, ib):
    """f32 accumulation of exact bf16 x bf16 products in a fixed order (the MFMA's own order differs: any order is within
    K 2^-24 sum |products|, which the 2 % spare of DELTA covers)."""
    acc = np.zeros(ub.shape[:-1], np.float32)
    for k in range(ub.shape[-1]):
        acc = (acc + (ub[..., k] * ib[..., k]).astype(np.float32)).astype(np.float32)
    return acc


def check(u, i):
    u, i = np.asarray(u, np.float32), np.asarray(i, np.float32)
    ub, ib = bf16_rne(u), bf16_rne(i)
    exact = (u.astype(np.float64) * i.astype(np.float64)).sum(-1)
    appr = approx_f32(ub, ib).astype(np.float64)
    nu = np.sqrt((u.astype(np.float64) ** 2).sum(-1))
    ni = np.sqrt((i.astype(np.float64) ** 2).sum(-1))
    assert np.all(np.abs(appr - exact) <= DELTA * nu * ni * (1 - 0.015) + 1e-300), float(np.max(np.abs(appr - exact) / (nu * ni + 1e-300)))
    # the kernel's term: delta |u| (f32 norm x 1.0009765625, rounded up) times |i| (norm of the ROUNDED row x 1.00390625, rounded up)
    du = bf16_up((np.float32(DELTA) * np.sqrt((u * u).sum(-1, dtype=np.float32)) * np.float32(1.0009765625)).astype(np.float32))
    ni_k = bf16_up((np.sqrt((ib * ib).sum(-1, dtype=np.float32)) * np.float32(1.00390625)).astype(np.float32))
    bound = appr + du.astype(np.float64) * ni_k.astype(np.float64) * (1 - 2.0 ** -20)      # (one more f32 rounding of the sum)
    assert np.all(bound >= exact), float(np.min(bound - exact))
    assert np.all(du.astype(np.float64) >= DELTA * nu * (1 - 1e-6)) and np.all(ni_k.astype(np.float64) >= ni * (1 - 1e-6))


def test_bound_on_random_vectors():
    rng = np.random.default_rng(0)
    for D in (36, 64, 100, 128):
        u = rng.standard_normal((2000, D)).astype(np.float32)
        i = rng.standard_normal((2000, D)).astype(np.float32)
        check(u, i)
        check(u * np.exp(rng.standard_normal((2000, D))).astype(np.float32), i * np.exp(2 * rng.standard_normal((2000, D))).astype(np.float32))
        check(u * 1e-12, i * 1e-12)
        check(u * 1e12, i * 1e12)


def test_bound_at_the_rounding_midpoints():
    """Every element of u just BELOW its bf16 midpoint (rounds down by almost half an ulp), every element of i just ABOVE (rounds
    up), all products of one sign: the rounding errors add up coherently — the worst case the constant has to cover."""
    rng = np.random.default_rng(1)
    for D in (64, 128):
        for sign in (1.0, -1.0):
            m_u = rng.integers(0, 128, (500, D)).astype(np.float64)      # 7 explicit mantissa bits of bf16
            m_i = rng.integers(0, 128, (500, D)).astype(np.float64)
            e_u = rng.integers(-3, 4, (500, D)).astype(np.float64)
            e_i = rng.integers(-3, 4, (500, D)).astype(np.float64)
            u = (1 + m_u / 128 + (1 / 256) * (1 - 2.0 ** -10)) * 2.0 ** e_u       # just below the midpoint between two bf16 values
            i = (1 + m_i / 128 + (1 / 256) * (1 + 2.0 ** -10)) * 2.0 ** e_i       # just above
            check(u.astype(np.float32), (sign * i).astype(np.float32))
            check((sign * i).astype(np.float32), u.astype(np.float32))


def test_bf16_helpers():
    mid = np.float32(1.00390625)                    # halfway between the bf16 values 1 and 1 + 2^-7
    x = np.array([1.0, mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(2)), 3.0e38, 0.0, 1e-30], np.float32)
    r = bf16_rne(x)
    assert r[0] == 1.0 and r[1] == 1.0 and r[2] == 1.0 and r[3] == np.float32(1.0078125)      # ties to even, below, above the midpoint
    up = bf16_up(np.array([1.0, 1.0000001, 2.5, 0.0], np.float32))
    assert up[0] == 1.0 and up[1] == np.float32(1.0078125) and up[2] == 2.5 and up[3] == 0.0
    assert np.all(bf16_up(np.abs(x)) >= np.abs(x))


# ---- below the normal range ---------------------------------------------------------------------------------------------------
F32_MIN = np.float32(2.0 ** -126)


def _ftz(x):
    """Subnormal f32 values flushed to 0."""
    x = np.asarray(x, np.float32)
    return np.where(np.abs(x) < F32_MIN, np.float32(0), x)


def _sum_f32(terms, flush):
    """Sequential f32 sum over the last axis.  `flush`: the pessimistic model of what nobody has measured — whether the MFMA and
    v_dot2 flush subnormal bf16 operands, subnormal products and subnormal f32 sums.  Taken as flushed, every one of them is 0: a
    flushed operand removes its product, a subnormal partial sum restarts at 0.  Both models (IEEE gradual underflow as numpy
    computes it, and everything flushed) are checked; the hardware lies between them."""
    acc = np.zeros(terms.shape[:-1], np.float32)
    for k in range(terms.shape[-1]):
        acc = (acc + terms[..., k]).astype(np.float32)
        if flush:
            acc = _ftz(acc)
    return acc


def norm2_f32(x, flush):
    """The kernels' squared norms: f32 squares summed in f32 (`un2`: an fma chain over the f32 user row; `rn2`: v_dot2 over the
    bf16 item row).  Rounding every square on its own (and flushing it) loses at least what either instruction loses."""
    x = _ftz(x) if flush else np.asarray(x, np.float32)
    sq = (x * x).astype(np.float32)
    return _sum_f32(_ftz(sq) if flush else sq, flush)


def floored(n2):
    """Mirror of the kernel's rule (kFiltMinN2): the rows whose computed squared norm is replaced by the floor.  (NaN: not.)"""
    return n2 < np.float32(MIN_N2)


def kernel_bound(u, i, flush, floor=True):
    """The filter's bound as the kernel forms it, in f32: approx + bf16_up(delta |u|) x bf16_up(|i|), a norm that `floored` names
    replaced by NORM_FLOOR.  Returns (bound, uncertifiable, un2, rn2): `uncertifiable` is the kernel's OTHER rule, an item row
    whose squared norm is not finite certifies nobody (`bad_norm`)."""
    ub, ib = bf16_rne(u), bf16_rne(i)
    if flush:
        ub, ib = _ftz(ub), _ftz(ib)
    prod = (ub * ib).astype(np.float32)                  # bf16 x bf16: exact in f32 unless it underflows
    appr = _sum_f32(_ftz(prod) if flush else prod, flush)
    un2, rn2 = norm2_f32(u, flush), norm2_f32(bf16_rne(i), flush)
    nu = (np.float32(DELTA) * np.sqrt(un2) * np.float32(1.0009765625)).astype(np.float32)
    ni = (np.sqrt(rn2) * np.float32(1.00390625)).astype(np.float32)
    if floor:
        nu = np.where(floored(un2), np.float32(DELTA) * np.float32(NORM_FLOOR), nu)
        ni = np.where(floored(rn2), np.float32(NORM_FLOOR), ni)
    du, ni_k = bf16_up(nu), bf16_up(ni)
    term = (du * ni_k).astype(np.float32)
    if flush:
        du, ni_k = _ftz(du), _ftz(ni_k)
        term = _ftz((du * ni_k).astype(np.float32))
    bound = appr.astype(np.float64) + term.astype(np.float64) * (1 - 2.0 ** -20)       # (one more f32 rounding of the sum)
    if flush:                                            # a subnormal sum may come out as 0: the worse of the two
        bound = np.where((np.abs(bound) < 2.0 ** -126) & (bound > 0), 0.0, bound)
    return bound, ~(rn2 < np.inf), un2, rn2


def check_scaled(u, i, a, b, floor=True):
    """The pair (u 2^a, i 2^b): the bound holds, or the kernel certifies nobody — under both underflow models."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        us, it = np.ldexp(np.asarray(u, np.float32), a).astype(np.float32), np.ldexp(np.asarray(i, np.float32), b).astype(np.float32)
        exact = (us.astype(np.float64) * it.astype(np.float64)).sum(-1)
        for flush in (False, True):
            bound, uncert, un2, rn2 = kernel_bound(us, it, flush, floor)
            ok = uncert | (bound >= exact)
            assert np.all(ok), (a, b, flush, int((~ok).sum()), float(np.min((bound - exact)[~ok])))
            # the floor costs nothing in the working range: no row of squared norm >= 2^-60 is touched
            for x, n2 in ((us, un2), (it, rn2)):
                true_n2 = (x.astype(np.float64) ** 2).sum(-1)
                assert not np.any(floored(n2) & (true_n2 >= 2.0 ** -60)), (a, b, flush)


def _sweep_pairs():
    steps = range(0, -141, -10)
    return [(a, b) for a in steps for b in steps] + [(a, -a) for a in range(-100, 101, 10) if a]


def _sweep_vectors():
    rng = np.random.default_rng(5)
    out = []
    for D in (64, 100, 128):
        out.append((rng.standard_normal((150, D)).astype(np.float32), rng.standard_normal((150, D)).astype(np.float32)))
    for D in (64, 128):                                  # the midpoint vectors of test_bound_at_the_rounding_midpoints
        for sign in (1.0, -1.0):
            m_u, m_i = rng.integers(0, 128, (100, D)).astype(np.float64), rng.integers(0, 128, (100, D)).astype(np.float64)
            e_u, e_i = rng.integers(-3, 4, (100, D)).astype(np.float64), rng.integers(-3, 4, (100, D)).astype(np.float64)
            u = (1 + m_u / 128 + (1 / 256) * (1 - 2.0 ** -10)) * 2.0 ** e_u
            i = sign * (1 + m_i / 128 + (1 / 256) * (1 + 2.0 ** -10)) * 2.0 ** e_i
            out += [(u.astype(np.float32), i.astype(np.float32)), (i.astype(np.float32), u.astype(np.float32))]
    return out


def test_bound_over_power_of_two_scales_down_to_underflow():
    """u 2^a, i 2^b for a, b = 0, -10 .. -140 and for a + b = 0 up to |a| = 100: wherever the squares of a norm underflow (elements
    below about 2^-75: the term vanishes while approx keeps its rounding error) the floored norm keeps the bound a bound."""
    for u, i in _sweep_vectors():
        for a, b in _sweep_pairs():
            check_scaled(u, i, a, b)


def test_the_sweep_fails_without_the_floor():
    """The kernel before kFiltMinN2 (the mirror switched off): the same sweep finds pairs whose bound is below the exact score —
    tiny users against ordinary items, ordinary users against tiny items, as in the issue's table."""
    u, i = _sweep_vectors()[-1]
    for a, b in ((-80, 0), (-80, 40), (0, -80), (40, -80)):
        with pytest.raises(AssertionError):
            check_scaled(u, i, a, b, floor=False)
    for a, b in ((0, 0), (-40, -40)):                    # (the working range never needed it)
        check_scaled(u, i, a, b, floor=False)


def test_all_zero_rows_keep_a_bound_and_a_tiny_one():
    """Padding and OOV rows are all-zero: approx = exact = 0.  Their norm is floored like any other below 2^-64, which leaves them a
    valid bound of delta |u| 2^-20 — nothing that outranks a real candidate — and never one that certifies nobody (0 x inf = NaN was
    possible with a norm of 0 against a user whose squared norm overflows)."""
    rng = np.random.default_rng(6)
    u = rng.standard_normal((50, 64)).astype(np.float32)
    z = np.zeros((50, 64), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for scale in (1.0, 2.0 ** -30, 2.0 ** 30, 2.0 ** 100):
            us = (u * np.float32(scale)).astype(np.float32)
            for flush in (False, True):
                b_item, uncert, _, _ = kernel_bound(us, z, flush)             # zero ITEM rows
                assert not uncert.any() and np.all(b_item >= 0.0)
                nu = np.sqrt((us.astype(np.float64) ** 2).sum(-1))
                assert np.all(b_item <= 2.0 ** -27 * nu) or scale == 2.0 ** 100          # (|u|^2 overflows f32 there: bound = inf)
                b_user, uncert, _, _ = kernel_bound(z, us, flush)             # zero USER rows: every score is 0
                assert np.all(b_user >= 0.0) and not np.isnan(b_user).any()
