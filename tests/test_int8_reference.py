"""
CPU tier: the host model of the int8 predict kernel (tests/int8_reference.py) against exact integer and rational arithmetic, and
its resolving power — every way the kernel could be subtly wrong that the model can imitate must change the bits the model
predicts, or tests/test_gpu_int8_exact.py (which holds the device to those bits) would not see it.
"""
from fractions import Fraction

import numpy as np
import pytest
from scipy.linalg import solve_triangular

import int8_reference as R
from oracle import gp_oracle as O


def _gp(N, d, P, kind, W, seed, corner=False, p=0):
    """Linv (from the oracle's factor), fp64 K* [W, N], amp, noise of GP p"""
    X, Z, th, Xs = R.problem(N, d, P, kind, W, seed)
    if corner:
        th, Xs = R.worst_corner(th, X, Xs)
    kid = O.KIND_NAMES[kind]
    L, _ = O.gp_factor(X, Z[p], th[p], kid, 0.1)
    Linv = solve_triangular(L, np.eye(N), lower=True)
    return Linv, O.kernel_cross(Xs, X, th[p], kid), R.engine_exp(th[p, 0]), R.engine_exp(th[p, -1])


@pytest.mark.parametrize("D", [6, 7])
def test_digits_round_trip_up_to_the_headroom_rule(D):
    """every |a| <= 0.99 2^(8D - 1) splits into D signed bytes and back exactly.  The top digit reaches +-127, not +-64:
    0.99 x 2^(8D - 1) / 256^(D - 1) = 126.7, and the digits below can carry one into it; the 0.01 of headroom is what keeps that
    carry from making it 128 — without it (a = 2^(8D - 1) - 1) the round trip fails."""
    bits = 8 * D - 1
    top = int(0.99 * 2.0 ** bits)
    rng = np.random.default_rng(D)
    a = np.concatenate([
        np.array([0, 1, -1, top, -top, top - 1, 1 - top, 127, 128, -128, -129, 0x7F7F7F7F7F7F, -0x808080808080, 0x808080808080]),
        rng.integers(-top, top + 1, 200000),
        (rng.integers(-top, top + 1, 1000) >> rng.integers(0, bits, 1000)),
        np.array([s * (1 << k) + o for k in range(bits) for s in (1, -1) for o in (-1, 0, 1) if abs(s * (1 << k) + o) <= top]),
    ]).astype(np.int64)
    a = a[np.abs(a) <= top]
    dg = R.digits(a, D)
    assert len(dg) == D
    for d in dg:
        assert d.min() >= -128 and d.max() <= 127
    assert dg[-1].min() >= -127 and dg[-1].max() <= 127
    assert dg[-1].max() == 127 and dg[-1].min() == -127        # reached at the extremes
    assert np.all(R.undigits(dg) == a.astype(object))
    over = np.array([2 ** bits - 1], dtype=np.int64)
    assert R.undigits(R.digits(over, D))[0] != int(over[0])


@pytest.mark.parametrize("D", [6, 7])
def test_all_levels_sum_to_the_big_integer_product(D):
    Linv, K, c, sn2 = _gp(200, 5, 2, "RBF", 8, seed=4)
    S, ej, ec = R.level_sums(Linv, R.fixed_kstar(K, c, D), c, D)
    a = R.round_operand(Linv, ej, D, 0).astype(object)
    b = np.rint(np.ldexp(R.fixed_kstar(K, c, D).T, 8 * D - 1 - ec)).astype(np.int64).astype(object)
    exact = a.dot(b)
    total = sum(S[l].astype(np.int64).astype(object) * 256 ** l for l in range(2 * D - 1))
    assert np.all(total == exact)


@pytest.mark.parametrize("D", [6, 7])
def test_the_dropped_levels_and_the_distance_from_exact_arithmetic(D):
    """Every digit lies in [-128, 127], so a digit product is at most 2^14 in magnitude; level l < D has l + 1 digit pairs and k
    runs over at most Np rows, so |S_l| <= (l + 1) Np 2^14 and the levels below D - 1 weigh at most
    sum_{l < D - 1} (l + 1) Np 2^14 256^l units of the integer product.  Horner adds D - 1 roundings of at most 2^-53 |t|
    each; rounding L^-1 and K* to their grids moves a product sum by at most sum_k (ua/2 |K*| + ub/2 |a| ua)."""
    N, nw = 128, 4
    Linv, K, c, sn2 = _gp(N, 5, 2, "RBF", nw, seed=11)
    Np = R.padded_size(N)
    bits = 8 * D - 1
    Kfix = R.fixed_kstar(K, c, D)
    S, ej, ec = R.level_sums(Linv, Kfix, c, D)
    v, smax = R.horner(S, ej, ec, D)
    allsum = sum(S[l].astype(np.int64).astype(object) * 256 ** l for l in range(2 * D - 1))
    kept = sum(S[l].astype(np.int64).astype(object) * 256 ** l for l in range(D - 1, 2 * D - 1))
    drop_bound = sum((l + 1) * Np * 2 ** 14 * 256 ** l for l in range(D - 1))
    assert np.all(np.abs(allsum - kept) <= drop_bound)
    for l in range(D - 1):
        assert np.max(np.abs(S[l])) <= (l + 1) * Np * 2 ** 14
    a = R.round_operand(Linv, ej, D, 0)
    worst = 0.0
    for j in range(N):
        ua = Fraction(2) ** (int(ej[j]) - bits)
        ub = Fraction(2) ** (ec - bits)
        for w in range(nw):
            exact = sum(Fraction(float(Linv[j, k])) * Fraction(float(K[w, k])) for k in range(j + 1))
            rounding = sum(ua / 2 * Fraction(float(K[w, k])) + ub / 2 * abs(int(a[j, k])) * ua for k in range(j + 1))
            bound = drop_bound * ua * ub + rounding + (D - 1) * Fraction(2) ** -52 * abs(Fraction(float(v[j, w])))
            err = abs(Fraction(float(v[j, w])) - exact)
            assert err <= bound, (j, w, float(err), float(bound))
            worst = max(worst, float(err / bound))
    print(f"D = {D}: max |v - exact| / bound = {worst:.3f}, max |S_l| / 2^31 = {smax / 2 ** 31:.2e}")


def test_the_emulated_fma_is_correctly_rounded():
    rng = np.random.default_rng(0)
    v = rng.standard_normal(20000) * np.exp(rng.uniform(-40, 3, 20000))
    s = np.abs(rng.standard_normal(20000)) * np.exp(rng.uniform(-40, 3, 20000))
    # exact ties and near ties: v^2 = half an ulp of s, s with an even and an odd last bit, and one ulp of v to either side
    tv = [2.0 ** -26, 2.0 ** -26, np.nextafter(2.0 ** -26, 1), np.nextafter(2.0 ** -26, 0), 2.0 ** -26 * 3, 0.0, 1e-130, 3.0]
    ts = [2.0, 2.0 + 2.0 ** -51, 2.0, 2.0 + 2.0 ** -51, 8.0 + 2.0 ** -49, 0.0, 1.0, np.nextafter(16.0, 0) - 9.0]
    v, s = np.r_[v, tv, v[:3000]], np.r_[s, ts, np.zeros(3000)]
    fast = R.fma_sq(v, s)
    assert np.array_equal(fast, R.fma_sq(v, s, exact=True))
    assert R.fma_sq(np.array([2.0 ** -26]), np.array([2.0]))[0] == 2.0                            # tie: to even
    assert R.fma_sq(np.array([2.0 ** -26]), np.array([2.0 + 2.0 ** -51]))[0] == 2.0 + 2.0 ** -50
    assert np.mean(v * v + s != fast) > 0.01                   # two roundings are not one
    import math
    if hasattr(math, "fma"):
        assert np.array_equal(fast, np.array([math.fma(a, a, b) for a, b in zip(v, s)]))


def test_the_vector_route_and_the_fraction_route_give_one_model():
    Linv, K, c, sn2 = _gp(200, 5, 2, "Matern25", 6, seed=4)
    for D in (6, 7):
        Kfix = R.fixed_kstar(K, c, D)
        a, b = R.predict_model(Linv, Kfix, c, sn2, D), R.predict_model(Linv, Kfix, c, sn2, D, exact=True)
        assert np.array_equal(a.var_bits, b.var_bits)
        assert R.error_over_bound(a.var_bits, a).max() < 1.0   # the device's order of sums lies inside the rounding bound
        # the exact sum of squares against plain Fractions
        assert a.sumsq_exact[0] == sum(Fraction(float(x)) ** 2 for x in a.v[:, 0])


def test_the_engines_exp_is_the_c_librarys_not_numpys():
    """gpb_gp_set_theta computes amp = exp(theta[0]) and noise = exp(theta[d + 1]) with the host C library's exp; the model takes
    math.exp, the same function.  numpy's exp (its own vector routine) is NOT a stand-in: on the thetas the GPU tier runs it
    differs from the C library's in the last bit for some (exp(-0.008455845566983857) is one), never by more."""
    import test_gpu_int8_exact as G
    n = differ = 0
    for th in G.all_thetas():
        for x in np.r_[th[:, 0], th[:, -1]]:
            a, b = float(np.exp(x)), R.engine_exp(x)
            assert abs(a - b) <= np.spacing(b)
            differ += a != b
            n += 1
    print(f"numpy's exp differs from the C library's on {differ} of {n} theta entries")
    assert n > 100


INPUTS = {"worst corner, N = 500": (500, 5, 3, "RBF", 256, 9, True), "plain, N = 1000": (1000, 15, 4, "RBF", 515, 1515, False)}


@pytest.mark.parametrize("D", [7, 6])
@pytest.mark.parametrize("name", list(INPUTS))
def test_resolving_power(name, D):
    """what makes the GPU tier worth having: each imitation of a subtly wrong kernel changes the predicted bits of at least one
    of 16 walkers (8 beside design points, 8 anywhere) — a dropped lowest digit pair, truncation of L^-1, a skipped K-step, two
    rows of a chain swapped, one row summed in the neighbouring 64-row block"""
    N, d, P, kind, W, seed, corner = INPUTS[name]
    Linv, K, c, sn2 = _gp(N, d, P, kind, W, seed, corner)
    ws = np.r_[0:8, 64:72]
    Kfix = R.fixed_kstar(K[ws], c, D)
    good = R.predict_model(Linv, Kfix, c, sn2, D)
    assert good.smax < 2.0 ** 31
    assert R.error_over_bound(good.var_bits, good).max() < 1.0
    print(f"\n{name}, D = {D}: headroom max |S_l| / 2^31 = {good.smax / 2 ** 31:.1e}")
    shares = {}
    for mutant in R.MUTANTS:
        bad = R.predict_model(Linv, Kfix, c, sn2, D, mutant=mutant)
        changed = bad.var_bits != good.var_bits
        shift = np.abs(np.array([float(x - y) for x, y in zip(bad.sumsq_exact, good.sumsq_exact)])) / good.B
        shares[mutant] = float(np.mean(changed))
        print(f"  {mutant:10s}: bits changed for {int(changed.sum()):2d} of {len(ws)} walkers; "
              f"shift of sum v^2 in units of B: {shift.min():.2g} .. {shift.max():.2g}")
    for mutant, share in shares.items():
        assert share > 0, f"{mutant} changes no bit of any modelled walker on '{name}'"
