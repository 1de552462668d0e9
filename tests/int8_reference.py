"""Host model of the int8 predict kernel (csrc/gpb_sliced.hip, option key 51) for the tests — a helper module, not a test file:
numpy and Python integers restate, bit for bit, what the device makes of the fp64 L^-1 it slices (GPEngine.get("Linv")) and of the
fixed-point K* its digit planes hold (GPEngine.get("Kstar", W) after a sliced batch), for D = 6 or 7 digit planes.

What the code does, in its order:
  * e = sl_exponent(m): frexp(m) = (f, ex), e = ex if f <= 0.99 else ex + 1.  Row j: m = max |Linv[j, 0..j]|; GP: m = c.
  * a[j, k] = rint(Linv[j, k] 2^(8D - 1 - e_j)) on the lower triangle (round to nearest even, __double2ll_rn), 0 above it;
    b[k, w] = Kfix[k, w] 2^(8D - 1 - e_c), an integer already (asserted).
  * digit t of an integer = byte t of (a + 0x80..80) XOR 0x80..80, read as a signed byte.  |a| <= 0.99 2^(8D - 1) keeps the round
    trip exact; the top digit then lies in [-127, 127] (0.99 x 128 = 126.7, plus the carry of the digits below), every digit in
    [-128, 127], every digit product within 2^14.
  * S_l[j, w] = sum_k sum_{ta + tb = l} a_ta[j, k] b_tb[k, w], exact (float64 matmuls of digit planes: every partial sum is below
    2^31); the D levels l = D - 1 .. 2D - 2 are kept.
  * Horner from the lowest kept level: t = S_{D-1}; t = t / 256 + S_l (the kernel's fma(t, 1/256, S_l): the product is exact,
    one rounding per level), then v = t 2^(e_j - 14) 2^(e_c) (exact).
  * sum of squares in the padded design's row order.  A design of N points is stored in Np = 64 ceil(N / 64) rows, at rows
    [pad, pad + N), pad = 16 floor((Np - N) / 16) (pad_front, csrc/gpb_internal.h); the other rows have v = 0 and only decide
    which 64-row block a design row falls in.  Per 64-row block and walker: two 32-row halves (the waves wm even and odd); in a
    half, lane half q = 0, 1 chains the rows (r & 3) + 8 (r >> 2) + 4 q, r = 0..15, through sum = fma(v, v, sum) from 0; the two
    chains are added, then the two halves (even + odd).  k_finalize (csrc/gpb_predict.hip): s = 0; s += partial[block] over the
    Np / 64 blocks in order; var = (amp + noise) - s.
  * amp = exp(theta[0]) and noise = exp(theta[d + 1]) are computed on the HOST by the C library's exp (gpb_gp_set_theta) and
    copied to the device; engine_exp below is that same function (math.exp).  numpy's exp is its own vector routine and differs
    from it in the last bit on some of the tests' thetas (tests/test_int8_reference.py counts them), so the model does not use it.

fma(v, v, sum) is emulated as ONE correctly rounded operation: Dekker's exact product and two exact sums give the candidate, and
wherever the candidate lies within 1e-6 of a rounding boundary (or v is tiny) the element is redone as
float(Fraction(v) ** 2 + Fraction(sum)); exact=True takes the Fraction route for every element.
"""
import math
from fractions import Fraction

import numpy as np

NP_MAX = 16384                      # SL_NP_MAX: D x Np x 2^14 < 2^31
MUTANTS = ("drop_pair", "truncate", "skip_kstep", "swap_rows", "move_row")


def engine_exp(x):
    """exp as gpb_gp_set_theta takes it: the C library's, on the host"""
    return math.exp(float(x))


def sl_exponent(m):
    """power-of-two exponent e with m <= 0.99 2^e (m > 0); scalars or arrays"""
    f, ex = np.frexp(m)
    return np.where(f <= 0.99, ex, ex + 1)


def padded_size(N):
    return -(-int(N) // 64) * 64


def pad_front(Np, N):
    return ((int(Np) - int(N)) // 16) * 16


def half_word(D):
    return int("80" * D, 16)


def digits(a, D):
    """the D signed radix-256 digits of int64 a, least significant first, as int64 arrays"""
    a = np.asarray(a, dtype=np.int64)
    h = np.uint64(half_word(D))
    u = (a.view(np.uint64) + h) ^ h
    return [((u >> np.uint64(8 * t)) & np.uint64(0xFF)).astype(np.uint8).view(np.int8).astype(np.int64) for t in range(D)]


def undigits(dg):
    """sum_t digit_t 256^t as Python integers (object array)"""
    out = np.zeros(dg[0].shape, dtype=object)
    for t, d in enumerate(dg):
        out = out + d.astype(object) * (256 ** t)
    return out


def row_exponents(Linv):
    """e_j and the frexp fraction it was decided on, from max |Linv[j, 0..j]|"""
    N = Linv.shape[0]
    m = np.empty(N)
    for r0 in range(0, N, 2048):
        r1 = min(N, r0 + 2048)
        blk = np.abs(Linv[r0:r1, :r1])
        blk[np.arange(r1)[None, :] > np.arange(r0, r1)[:, None]] = 0.0
        m[r0:r1] = blk.max(axis=1)
    assert np.all(m > 0)
    return sl_exponent(m).astype(np.int64), np.frexp(m)[0]


def round_operand(Linv_rows, e_rows, D, r0, truncate=False):
    """a[j, k] of rows r0.. (columns 0..r1) as int64"""
    r1 = r0 + Linv_rows.shape[0]
    x = np.ldexp(Linv_rows[:, :r1], ((8 * D - 1) - e_rows)[:, None].astype(np.int32))
    x[np.arange(r1)[None, :] > np.arange(r0, r1)[:, None]] = 0.0
    x = np.trunc(x) if truncate else np.rint(x)
    assert np.all(np.abs(x) < 2.0 ** (8 * D - 1))
    return x.astype(np.int64)


def fixed_kstar(K, c, D):
    """K* rounded to the (8D - 1)-bit fixed point of the planes (the CPU tier's stand-in for the device's read-back)"""
    ec = int(sl_exponent(c))
    return np.ldexp(np.rint(np.ldexp(np.asarray(K, float), (8 * D - 1) - ec)), ec - (8 * D - 1))


def level_sums(Linv, Kfix, c, D, truncate=False, drop_pair=None, zero_k=None, chunk=1024):
    """S[l, j, w] for ALL levels l = 0 .. 2D - 2 (float64 holding exact integers), e_j, e_c.  Linv [N, N] (lower triangle used),
    Kfix [nw, N].  drop_pair = (ta, tb) leaves one digit product out; zero_k = (k0, k1) the design rows k0 <= k < k1 of K*."""
    N, nw = Linv.shape[0], Kfix.shape[0]
    ec = int(sl_exponent(c))
    bf = np.ldexp(np.ascontiguousarray(Kfix.T, dtype=np.float64), (8 * D - 1) - ec)
    assert np.array_equal(bf, np.rint(bf)), "K* is not on the fixed-point grid of the planes"
    assert np.all(np.abs(bf) < 2.0 ** (8 * D - 1))
    if zero_k is not None:
        bf = bf.copy()
        bf[zero_k[0]:zero_k[1]] = 0.0
    Bcat = np.concatenate([d.astype(np.float64) for d in digits(bf.astype(np.int64), D)], axis=1)        # [N, D nw]
    ej, _ = row_exponents(Linv)
    S = np.zeros((2 * D - 1, N, nw))
    for r0 in range(0, N, chunk):
        r1 = min(N, r0 + chunk)
        Ad = digits(round_operand(Linv[r0:r1], ej[r0:r1], D, r0, truncate), D)
        for ta in range(D):
            prod = Ad[ta].astype(np.float64) @ Bcat[:r1]
            for tb in range(D):
                if drop_pair == (ta, tb):
                    continue
                S[ta + tb, r0:r1] += prod[:, tb * nw:(tb + 1) * nw]
    return S, ej, ec


def horner(S, ej, ec, D):
    """the device's v [N, nw] from the kept levels, and max |S_l| over them"""
    kept = S[D - 1:]
    smax = float(np.max(np.abs(kept)))
    assert smax < 2.0 ** 31, "an int32 level sum would wrap"
    t = kept[0].copy()
    for l in range(1, D):
        t = t / 256.0 + kept[l]
    return np.ldexp(t, (ej - 14 + ec)[:, None].astype(np.int32)), smax


# ------------------------------------------------------------------------------------------------ fma(v, v, s), correctly rounded
def fma_sq_exact(v, s):
    return float(Fraction(float(v)) ** 2 + Fraction(float(s)))


def fma_sq(v, s, exact=False):
    """round(v^2 + s), one rounding, elementwise"""
    v = np.asarray(v, dtype=np.float64)
    s = np.asarray(s, dtype=np.float64)
    if exact:
        return np.array([fma_sq_exact(a, b) for a, b in zip(v.ravel(), s.ravel())]).reshape(v.shape)
    with np.errstate(all="ignore"):
        cc = 134217729.0 * v                                    # Veltkamp split, Dekker product: v^2 = p + e exactly
        hi = cc - (cc - v)
        lo = v - hi
        p = v * v
        e = ((hi * hi - p) + 2.0 * hi * lo) + lo * lo
        h = p + s                                               # p + s = h + l exactly
        bb = h - p
        l = (p - (h - bb)) + (s - bb)
        t = l + e
        r = h + t                                               # candidate; h + t = r + err exactly
        b2 = r - h
        err = (h - (r - b2)) + (t - b2)
        half = 0.5 * np.spacing(np.abs(r))
        doubt = (np.abs(np.abs(err) - half) <= 1e-6 * half) | ((np.frexp(r)[0] == 0.5) & (err != 0.0))
        doubt |= (v != 0.0) & (np.abs(v) < 1e-120)
        doubt |= ~np.isfinite(r)
    if np.any(doubt):
        r = r.copy()
        idx = np.flatnonzero(doubt)
        rf, vf, sf = r.reshape(-1), v.reshape(-1), np.broadcast_to(s, v.shape).reshape(-1)
        for i in idx:
            rf[i] = fma_sq_exact(vf[i], sf[i])
    return r


# ------------------------------------------------------------------------------------------------ the order of the sums
def chain_rows(Np):
    """idx[block, half, q, step]: the padded row each step of each chain takes (-1: none); 17 steps, the last one unused"""
    nblk = Np // 64
    r = np.arange(16)
    idx = np.full((nblk, 2, 2, 17), -1, dtype=np.int64)
    for half in range(2):
        for q in range(2):
            idx[:, half, q, :16] = (np.arange(nblk) * 64)[:, None] + 32 * half + (r & 3) + 8 * (r >> 2) + 4 * q
    return idx


def device_sumsq(V, N, order=None, exact=False):
    """s[w] as k_finalize forms it from the device's partials; V [N, nw]"""
    Np = padded_size(N)
    pad = pad_front(Np, N)
    nw = V.shape[1]
    Vp = np.zeros((Np + 1, nw))                                 # row Np: the v = 0 of a step that takes no row
    Vp[pad:pad + N] = V
    idx = chain_rows(Np) if order is None else order
    idx = np.where(idx < 0, Np, idx)
    acc = np.zeros(idx.shape[:3] + (nw,))
    for step in range(idx.shape[3]):
        rows = idx[..., step]
        if np.all(rows == Np):
            continue
        acc = fma_sq(Vp[rows], acc, exact)
    halves = acc[:, :, 0] + acc[:, :, 1]                        # sum += __shfl_xor(sum, 32)
    part = halves[:, 0] + halves[:, 1]                          # even wave row + what the odd one handed over
    s = np.zeros(nw)
    for i in range(part.shape[0]):
        s = s + part[i]
    return s


def exact_sumsq(V):
    """sum_j V[j, w]^2 as Fractions"""
    mant, ex = np.frexp(V)
    mi = np.ldexp(mant, 53).astype(np.int64).astype(object)
    sh = 2 * (ex.astype(np.int64) - 53)
    low = int(sh.min())
    tot = np.left_shift(mi * mi, (sh - low).astype(object)).sum(axis=0)
    scale = Fraction(2) ** low
    return [Fraction(int(x)) * scale for x in np.atleast_1d(tot)]


class Model:
    """what predict_model returns: v [N, nw] (the device's v), var_bits [nw] (the device's variance, bit for bit), sumsq_exact and
    var_exact (Fractions), B [nw] (the first-order rounding bound), smax = max |S_l| over the kept levels, frac (the frexp
    fractions the row exponents were decided on)"""


def predict_model(Linv, Kfix, amp, noise, D, mutant=None, exact=False):
    """One GP: Linv [N, N] as the slicer reads it, Kfix [nw, N] the fixed-point K* of nw walkers, amp and noise as the engine
    holds them.  mutant: one of MUTANTS, a deliberately wrong model for the resolving-power tests."""
    assert D in (6, 7) and mutant in (None,) + MUTANTS
    N = Linv.shape[0]
    Np = padded_size(N)
    assert Np <= NP_MAX, "above SL_NP_MAX the engine stays on the fp64 kernel"
    pad = pad_front(Np, N)
    kw = {}
    if mutant == "drop_pair":
        kw["drop_pair"] = (D - 1, 0)
    if mutant == "truncate":
        kw["truncate"] = True
    if mutant == "skip_kstep":                                  # the first 32-deep K-step that holds design rows
        k0 = (pad // 32) * 32
        kw["zero_k"] = (max(0, k0 - pad), k0 + 32 - pad)
    S, ej, ec = level_sums(Linv, Kfix, amp, D, **kw)
    out = Model()
    out.S, out.ej, out.ec = S, ej, ec
    out.v, out.smax = horner(S, ej, ec, D)
    out.frac = row_exponents(Linv)[1]
    order = None
    if mutant == "swap_rows":                                   # the first design row and the next row of its chain change places
        order = chain_rows(Np)
        b, half, q, st = (int(x[0]) for x in np.nonzero(order == pad))
        order[b, half, q, [st, st + 1]] = order[b, half, q, [st + 1, st]]
    if mutant == "move_row":                                    # the first row of the block behind the first design row's is summed
        order = chain_rows(Np)                                  # at the end of that block instead: a padding offset off by one row
        b = pad // 64
        assert b + 1 < order.shape[0]
        order[b, 1, 1, 16] = order[b + 1, 0, 0, 0]
        order[b + 1, 0, 0, 0] = -1
    s = device_sumsq(out.v, N, order, exact)
    out.var_bits = (amp + noise) - s
    out.sumsq_exact = exact_sumsq(out.v)
    out.var_exact = [Fraction(amp) + Fraction(noise) - q for q in out.sumsq_exact]
    nI64 = Np // 64
    out.B = np.array([(nI64 + 24) * 2.0 ** -53 * (amp + noise + float(q)) for q in out.sumsq_exact])
    return out


def error_over_bound(var_device, model):
    """|var_device - var_exact| / B per walker"""
    return np.array([float(abs(Fraction(float(x)) - e)) / b for x, e, b in zip(var_device, model.var_exact, model.B)])


def problem(N, d, P, kind, W, seed, sn2=0.05, c=1.0):
    """the synthetic GPs of tests/test_gpu_sliced.py and tests/test_gpu_predict_int8x7.py (the same draws for the same seed)"""
    from gpbayestools_hic_amd import synth
    rng = np.random.default_rng(seed)
    X = synth.lhs(N, d, seed=seed)
    Z = np.sin(X @ rng.standard_normal((d, P))).T + 0.05 * rng.standard_normal((P, N))
    th = synth.fixed_theta(d, P, ell=1.2, noise=sn2)
    th[:, 0] = np.log(c) + 0.1 * rng.standard_normal(P)
    Xs = rng.random((W, d))
    k = min(W, N, 16)
    Xs[:k] = X[:k]                                            # queries ON design points: the smallest variances
    return X, Z, th, Xs


def worst_corner(th, X, Xs):
    """the corner of the search box of test_the_worst_corner_of_the_search_box: c = e^3, sn2 = 1e-2, l = 8, queries beside design points"""
    th = th.copy(); Xs = Xs.copy()
    th[:, 0], th[:, -1] = 3.0, np.log(1e-2)
    th[:, 1:-1] = np.log(8.0)
    Xs[:64] = X[:64] + 1e-6
    return th, Xs
