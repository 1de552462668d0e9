"""
GPU tier: the int8 predict kernel (csrc/gpb_sliced.hip, gpb_ctx_option 51) against an exact host integer model, BIT FOR BIT.

Integer sums are exact, so given the fp64 L^-1 the slicer reads (GPEngine.get("Linv")) and the fixed-point K* its planes hold
(GPEngine.get("Kstar", W) after a sliced batch), every v[j, w] the kernel forms, and every one of the ~18 + Np / 64 fp64 additions
behind it, is determined: tests/int8_reference.py restates them, and the predictive variance the device returns must EQUAL the
model's (np.array_equal: no tolerance).  The secondary check |var - var_exact| <= B = (Np / 64 + 24) 2^-53 (c + sn2 + sum v^2)
— the first-order bound of the 18 + Np / 64 + 2 roundings with a slack of 4 — tells the reader of a failure which side to
suspect: inside B but not equal means an order or padding detail of the model (or a defect of a few ulps in the kernel: look at
the model first), outside B means the kernel is wrong.  tests/test_int8_reference.py shows that bit equality resolves a dropped
digit pair, a truncated operand, a skipped K-step and a misplaced row, which the bound does not.

This file pins a context's own launch.  Chain launches, the shared multi-emulator launch and compacted batches expose no variance
to read; they stay covered by transitivity: the tests that give them the own launch's bits (tests/test_gpu_predict_int8x7.py,
tests/test_gpu_sliced.py, tests/test_gpu_multi_emulator.py) stand as they are.

Every test sets option 51 itself (the suite also runs with GPB_PREDICT_SLICED=0).  GPB_INT8_EXACT_REPORT=<file> appends one line per
case: walkers compared, bit-equal, max err / B, max |S_l| / 2^31, wall time (profiles/r10_int8_exact.txt is such a run).
"""
import os
import time

import numpy as np
import pytest

import int8_reference as R

pytestmark = pytest.mark.gpu

DEPTH = {3: 7, 2: 6}            # option 51 value -> digit planes (2: six planes with the theta rule off)

SHAPES = [                      # the shapes of test_seven_planes_against_the_oracle
    (1000, 15, 4, "RBF", 515),
    (320, 20, 3, "Matern15", 130),
    (65, 3, 2, "Matern25", 1),
    (40, 4, 2, "RBF", 70),
    (900, 12, 3, "RBF", 300),
    (2048, 20, 10, "RBF", 256),
    (640, 8, 9, "RBF", 1024),
]
BIG = (4096, 20, 2, "Matern25", 130)
DEPTH6_SHAPES = [SHAPES[0], SHAPES[3], SHAPES[4]]
EDGE = (500, 5, 3, "RBF", 256)
EDGES = ["worst_corner", "short_scales", "c0.995", "c1.99", "c1", "c_exp-3"]

_fractions = []                 # frexp fractions of the row maxima of every modelled L^-1 (the row-exponent branch test)


def shape_problem(shape):
    N, d, P, kind, W = shape
    return R.problem(N, d, P, kind, W, seed=N + W)


def edge_problem(edge):
    """(X, Z, theta, Xs, kernel) of a theta edge, on the design of test_the_worst_corner_of_the_search_box"""
    N, d, P, kind, W = EDGE
    X, Z, th, Xs = R.problem(N, d, P, kind, W, seed=9)
    if edge == "worst_corner":
        th, Xs = R.worst_corner(th, X, Xs)
    elif edge == "short_scales":                              # the Matern families' lower bound, 1e-3 x extent: difference form
        kind = "Matern15"
        th[:, 1:-1] = np.log(1e-3)
    else:
        th[:, 0] = {"c0.995": np.log(0.995), "c1.99": np.log(1.99), "c1": 0.0, "c_exp-3": -3.0}[edge]
    return X, Z, th, Xs, kind


def all_thetas():
    """every theta this file hands to the engine (tests/test_int8_reference.py checks numpy's exp against the engine's on them)"""
    out = [shape_problem(s)[2] for s in SHAPES + [BIG]]
    out += [edge_problem(e)[2] for e in EDGES]
    out += [R.problem(N, 4, 1, "RBF", 64, seed=N)[2] for N in (16384, 16385)]
    return out


def modelled_walkers(N, W, count=32):
    """every walker where N <= 1100; else `count` of them: the first, the last, one in every 64-wide tile of the ragged last
    super-block (4 tiles), the rest drawn"""
    if N <= 1100 or W <= count:
        return np.arange(W)
    last0 = ((W - 1) // 256) * 256
    must = {0, W - 1} | {min(t + 17, W - 1) for t in range(last0, W, 64)} | set(range(last0, W, 64))
    rest = [int(w) for w in np.random.default_rng(N + W).permutation(W) if w not in must]
    return np.array(sorted(must | set(rest[:max(0, count - len(must))])))


def report(line):
    print(line)
    path = os.environ.get("GPB_INT8_EXACT_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def check_against_model(eng, name, th, Xs, code, walkers=None, t0=None):
    """predict Xs at option value `code`, read back what the kernel read, model it, hold the variance to the model's bits.
    Returns (mean, variance)."""
    t0 = time.time() if t0 is None else t0
    D = DEPTH[code]
    W = len(Xs)
    eng.tune("predict_sliced", code)
    m, v = eng.predict(Xs)
    Linv = eng.get("Linv")
    Ks = eng.get("Kstar", W)
    ws = modelled_walkers(eng.N, W) if walkers is None else np.asarray(walkers)
    compared = equal = 0
    worst, worst_bad, smax, bad = 0.0, 0.0, 0.0, []
    for p in range(eng.P):
        amp, noise = R.engine_exp(th[p, 0]), R.engine_exp(th[p, -1])
        mod = R.predict_model(Linv[p], Ks[p][ws], amp, noise, D)
        _fractions.append(mod.frac)
        same = v[ws, p] == mod.var_bits
        ratio = R.error_over_bound(v[ws, p], mod)
        compared += len(ws); equal += int(same.sum())
        worst, smax = max(worst, float(ratio.max())), max(smax, mod.smax)
        worst_bad = max(worst_bad, float(ratio[~same].max())) if not same.all() else worst_bad
        for i in np.flatnonzero(~same)[:4]:
            bad.append(f"GP {p} walker {int(ws[i])}: device {v[ws[i], p]!r} model {mod.var_bits[i]!r} err/B {ratio[i]:.3g}")
    report(f"{name:44s} D={D} Np={R.padded_size(eng.N):5d} GPs={eng.P:2d} walkers compared {compared:5d} bit-equal {equal:5d} "
           f"max err/B {worst:.3f} max|S_l|/2^31 {smax / 2 ** 31:.2e} wall {time.time() - t0:.1f}s")
    assert smax < 2.0 ** 31                                     # exact arithmetic: no int32 level sum wrapped on this input
    verdict = (f"the worst of them {worst_bad:.3g} B from exact arithmetic, " +
               ("outside the rounding bound: the kernel is wrong" if worst_bad > 1.0 else
                "inside the rounding bound: an order or padding detail of the model, or a kernel defect of a few ulps"))
    assert equal == compared, f"{compared - equal} of {compared} variances differ from the model's bits ({verdict}): " + "; ".join(bad)
    assert worst <= 1.0
    return m, v


def _engine(X, Z, th, kind):
    from gpbayestools_hic_amd import GPEngine
    eng = GPEngine(0)
    eng.set_data(X, Z, kind, alpha=0.1); eng.set_theta(th); eng.factor()
    return eng


@pytest.mark.parametrize("shape", SHAPES + [BIG], ids=lambda s: "N%d-P%d-%s-W%d" % (s[0], s[2], s[3], s[4]))
def test_seven_planes_bit_for_bit(shape):
    t0 = time.time()
    X, Z, th, Xs = shape_problem(shape)
    eng = _engine(X, Z, th, shape[3])
    check_against_model(eng, "seven planes N=%d d=%d P=%d %s W=%d" % shape, th, Xs, 3, t0=t0)
    eng.close()


@pytest.mark.parametrize("shape", DEPTH6_SHAPES, ids=lambda s: "N%d-P%d-%s-W%d" % (s[0], s[2], s[3], s[4]))
def test_six_planes_bit_for_bit(shape):
    """option value 2: six planes, K* rounded to 47 bits by the + 2^52 trick"""
    t0 = time.time()
    X, Z, th, Xs = shape_problem(shape)
    eng = _engine(X, Z, th, shape[3])
    check_against_model(eng, "six planes N=%d d=%d P=%d %s W=%d" % shape, th, Xs, 2, t0=t0)
    eng.close()


@pytest.mark.parametrize("edge", EDGES)
def test_theta_edges_bit_for_bit(edge):
    t0 = time.time()
    X, Z, th, Xs, kind = edge_problem(edge)
    eng = _engine(X, Z, th, kind)
    amps = np.array([R.engine_exp(x) for x in th[:, 0]])
    f = np.frexp(amps)[0]
    if edge == "short_scales":
        assert np.all(eng.get("form") == 1)                    # the difference form of the distances
    if edge in ("c0.995", "c1.99"):
        assert np.all(f > 0.99)                                # the ex + 1 branch of the column scale
    if edge == "c1":
        assert np.all(amps == 1.0)
    check_against_model(eng, "edge " + edge, th, Xs, 3, t0=t0)
    if edge == "short_scales":                                 # K* is mostly zero digits here
        Ks = eng.get("Kstar", len(Xs))
        assert np.mean(Ks == 0.0) > 0.9
    eng.close()


def test_both_branches_of_the_row_exponent_were_modelled():
    """a condition on the inputs, read off the L^-1 the device holds so that it cannot lapse: among the modelled rows some have a
    frexp fraction above 0.99 (e_j = ex + 1) and some one in (0.98, 0.99] (e_j = ex, at the edge); ~1.4 % should lie above"""
    if not _fractions:                                         # run on its own: model one case first
        X, Z, th, Xs = shape_problem(SHAPES[0])
        eng = _engine(X, Z, th, SHAPES[0][3])
        check_against_model(eng, "seven planes (for the row exponents)", th, Xs[:8], 3)
        eng.close()
    f = np.concatenate(_fractions)
    above, edge = int(np.sum(f > 0.99)), int(np.sum((f > 0.98) & (f <= 0.99)))
    report(f"row exponents: {len(f)} modelled rows, {above} with fraction > 0.99 ({100.0 * above / len(f):.2f} %), {edge} in (0.98, 0.99]")
    assert above >= 1 and edge >= 1


def test_switching_depth_on_one_factorisation():
    """7 -> 6 -> 7 planes with no factor() between: sliced_prepare re-slices L^-1 when the depth changes"""
    X, Z, th, Xs = shape_problem(SHAPES[1])
    eng = _engine(X, Z, th, SHAPES[1][3])
    eng.tune("predict_sliced", 3)
    m1, v1 = eng.predict(Xs)
    m2, v2 = check_against_model(eng, "depth switch 7 -> 6", th, Xs, 2)
    eng.tune("predict_sliced", 3)
    m3, v3 = eng.predict(Xs)
    assert np.array_equal(v3, v1) and np.array_equal(m3, m1)
    assert not np.array_equal(v2, v1)
    check_against_model(eng, "depth switch 6 -> 7", th, Xs, 3)
    eng.close()


def test_a_growing_batch_keeps_the_bits_of_its_first_rows():
    """64 rows, then 700: the batch capacity grows after a sliced batch and the planes of K*^T are allocated anew"""
    N, d, P, kind = 320, 6, 3, "RBF"
    X, Z, th, Xs = R.problem(N, d, P, kind, 700, seed=77)
    eng = _engine(X, Z, th, kind)
    eng.tune("predict_sliced", 3)
    m64, v64 = eng.predict(Xs[:64])
    m, v = check_against_model(eng, "batch grown 64 -> 700", th, Xs, 3)
    assert np.array_equal(v[:64], v64) and np.array_equal(m[:64], m64)
    m64b, v64b = eng.predict(Xs[:64])
    assert np.array_equal(v64b, v64) and np.array_equal(m64b, m64)
    eng.close()


# ------------------------------------------------------------------------------------------------ the size limit
def test_the_largest_design_the_int8_kernel_takes():
    """Np = 16384 = SL_NP_MAX, where D x Np x 2^14 = 0.875 x 2^31: an ordinary well-conditioned design; the model, not the
    device, says how close to 2^31 the level sums came.  W = 64; eight walkers modelled (131 072 emulated fmas)."""
    t0 = time.time()
    N, W = 16384, 64
    X, Z, th, Xs = R.problem(N, 4, 1, "RBF", W, seed=N)
    eng = _engine(X, Z, th, "RBF")
    eng.tune("predict_sliced", 0)
    m64, v64 = eng.predict(Xs)
    ws = np.array([0, 5, 16, 31, 32, 40, 57, 63])
    m, v = check_against_model(eng, "the size limit N=16384 d=4 P=1 RBF W=64", th, Xs, 3, walkers=ws, t0=t0)
    assert not np.array_equal(v, v64)                          # the int8 kernel ran
    assert np.max(np.abs(v - v64) / v64) < 1e-10
    eng.close()


def test_the_first_design_above_the_limit_stays_on_the_fp64_kernel():
    """N = 16385 pads to Np = 16448 > SL_NP_MAX (the design is padded to a multiple of 64 rows): sliced_applies sends every
    option value to the fp64 kernel"""
    N, W = 16385, 64
    assert R.padded_size(N) > R.NP_MAX and R.padded_size(N - 1) == R.NP_MAX
    X, Z, th, Xs = R.problem(N, 4, 1, "RBF", W, seed=N)
    eng = _engine(X, Z, th, "RBF")
    eng.tune("predict_sliced", 3)
    m3, v3 = eng.predict(Xs)
    eng.tune("predict_sliced", 0)
    m0, v0 = eng.predict(Xs)
    assert np.array_equal(m3, m0) and np.array_equal(v3, v0)
    assert np.all(v0 > 0)
    eng.close()
