"""GPU tier: every padded input width the distance kernels are instantiated or sized on — pick_dpad's 8, 16, 20, 24, 32, 48, 64
(csrc/dispatch.h) — against the oracle, each with d == width (no padding column) and d == previous width + 1 (the most), for the
three kernel families, both distance forms in one engine, one and two walkers per lane, and the fp64, seven-plane and six-plane
arithmetic of K*.  The inputs are tests/width_cases.py; tests/test_width_cases.py shows on the oracle alone that they see a dropped
last input column at more than 1e6 x every bar used here.

Every bar is one the project already asserts:
  K(X,X), K*   |.| <= 1e-13 max(c, 1)                 test_gpu_edges.py::test_length_scales_at_the_lower_bound_... (c = 1 there),
                                                       test_gpu_sliced.py (the factor max(1, c))
  L            1e-11 max|L|                            test_gpu_edges.py::test_designs_that_are_not_a_multiple_of_64_points
  LML          1e-10 |LML|, gradient 1e-9 max(|g|inf, 1), every slot      test_gpu_edges.py (all of its oracle tests)
  mean         1e-11 max|mean|, variance 1e-10 element-wise relative        test_gpu_edges.py, test_gpu_sliced.py
  K* planes    seven: ldexp(rint(ldexp(K64, 55 - e_c)), e_c - 55) bit for bit  test_gpu_predict_int8x7.py::test_kstar_planes_...
               six: |K6 - K64| <= 2^(e_c - 48), half a unit of the 47-bit fixed point the epilogue rounds to nearest (gpb_predict.hip)
  gradients    row-wise 1e-9 max(|g_ref|inf, 1)        test_gpu_gradient.py
  Sobol        sobol_reference.bar_factor x unit bounds, as test_gpu_sobol.py::test_against_model
  chain        1e-10 relative against the oracle chain  test_gpu_multi_emulator.py

Largest ratio to each bar, measured on an MI355X over all cases of this file (profiles/r14_input_widths.txt): see RATIOS below.
GPB_WIDTHS_REPORT=<file> appends one line per case with its ratios."""
import functools
import os

import numpy as np
import pytest

import width_cases as WC
from conftest import relerr

pytestmark = pytest.mark.gpu

# measured on an MI355X, the largest ratio error / bar over the cases of each part (1.0 would be the bar itself)
RATIOS = """
a. engine (42 cases x 3 GPs)   K 0.27   L 0.0023   LML 2.8e-05   LML gradient 2.6e-05 (slot d alone 1.6e-05)
     fp64 kernel               K* 0.36   mean 0.0040   variance 0.0015
     seven planes (default)    K* 0.36   mean 0.0042   variance 0.0015   the planes equal the host integer model in all 126 GPs
     six planes                K* 0.39   mean 0.0042   variance 0.050    |K6 - K64| = 2^(e_c - 48) exactly (a tie) in all 126 GPs
   K, K* and L without the four cases (d, kind) = (16, Matern25), (21, RBF), (21, Matern25), (32, Matern15): K 0.0051, K* 0.0068 (six planes 0.073),
   L 0.00054.  In those four numpy's exp and libm's exp of log l differ by one ulp on the short length scale of GP 1, x / l ~ 500
   moves by an ulp of 500 (5.7e-14) and K, K* of the difference form by up to 3.6e-14: the oracle's side of the comparison.
b. prediction gradients (18 cases)   d mean / dx 1.2e-05   d var / dx 7.4e-07
c. Sobol (6 cases)   e 0.0023   H 0.00042   V_S 0.00019   var 0.00012   mean 0.0018   first 8.1e-05   total 4.0e-05; U_S / V <= 6.3e4
d. chain (4 cases)   log-posterior against the oracle chain: fp64 2.2e-06, default arithmetic 3.9e-06
"""


def _report(line):
    print(line)
    path = os.environ.get("GPB_WIDTHS_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


class _Ledger:
    """ratios to the bars and yes/no identities of one case: all printed, then all asserted"""

    def __init__(self, name):
        self.name, self.ratios, self.bad = name, [], []

    def ratio(self, label, err, bar):
        r = float(err) / float(bar)
        self.ratios.append((label, r))
        if not r < 1.0:
            self.bad.append("%s: %.3g x its bar" % (label, r))

    def same(self, label, ok):
        if not ok:
            self.bad.append(label + ": bits differ")

    def close(self):
        _report("%s: " % self.name + "  ".join("%s %.2g" % lr for lr in self.ratios))
        assert not self.bad, "%s: %s" % (self.name, "; ".join(self.bad))


# ------------------------------------------------------------------------------------------------ a. the engine
@functools.lru_cache(maxsize=None)
def _oracle(d, kind):
    """the case and the oracle's numbers per GP, computed once (read-only)"""
    from oracle import gp_oracle as O
    kid = O.KIND_NAMES[kind]
    X, Z, th, Xs = WC.make_case(d, kind)
    per = []
    for p in range(WC.P):
        K = O.kernel_train(X, th[p], kid, WC.ALPHA)
        L = np.linalg.cholesky(K)
        _, a = O.gp_factor(X, Z[p], th[p], kid, WC.ALPHA)
        Ks = O.kernel_cross(Xs, X, th[p], kid)
        m, v = O.gp_predict(Xs, X, th[p], L, a, kid)
        val, g = O.lml(th[p], X, Z[p], kid, WC.ALPHA, eval_gradient=True)
        per.append(dict(K=K, L=L, Ks=Ks, m=m, v=v, val=val, g=g))
    return X, Z, th, Xs, per


def _plane_exponent(c):
    """e_c of the digit planes' column scale: K* in [0, c] <= 0.99 2^e_c (test_gpu_predict_int8x7.py)"""
    f, e = np.frexp(c)
    return int(e) if f <= 0.99 else int(e) + 1


SLICES = (slice(0, 1), slice(0, WC.W_ONE_PER_LANE), slice(64, WC.W))


@pytest.mark.parametrize("kind", WC.KINDS)
@pytest.mark.parametrize("d", WC.DS)
def test_engine_at_every_width(d, kind):
    """forms, K(X,X), L, LML and its gradient, then K*, mean and variance in the three arithmetics of K*, then the bit identities
    (batch cuts, walkers per lane, chunks per workgroup, a GP alone) in the fp64 and the default arithmetic"""
    from gpbayestools_hic_amd import GPEngine
    X, Z, th, Xs, per = _oracle(d, kind)
    led = _Ledger("engine d=%d dpad=%d %s" % (d, WC.dpad_of(d), kind))
    eng, single = GPEngine(0), GPEngine(0)
    arith = eng.predict_sliced
    try:
        eng.set_data(X, Z, kind, WC.ALPHA); eng.set_theta(th)
        assert eng.get("form").tolist() == WC.FORMS
        eng.fit_piece("kmat")                                       # K(X,X) alone (the factorisation overwrites it with L)
        K = eng.get("K")
        eng.factor()
        L = eng.get("L")
        val, grad = eng.lml(th)
        eng.set_theta(th); eng.factor()
        single.set_data(X, Z[1:2], kind, WC.ALPHA); single.set_theta(th[1:2]); single.factor()
        assert single.get("form").tolist() == WC.FORMS[1:2]
        amps = np.exp(th[:, 0])
        for p in range(WC.P):
            o, cb = per[p], max(float(amps[p]), 1.0)
            led.ratio("K%d" % p, np.max(np.abs(np.tril(K[p]) - np.tril(o["K"]))), 1e-13 * cb)
            led.ratio("L%d" % p, np.max(np.abs(L[p] - o["L"])), 1e-11 * np.max(np.abs(o["L"])))
            led.ratio("lml%d" % p, abs(val[p] - o["val"]), 1e-10 * abs(o["val"]))
            gbar = 1e-9 * max(np.max(np.abs(o["g"])), 1.0)
            led.ratio("grad%d" % p, np.max(np.abs(grad[p] - o["g"])), gbar)
            led.ratio("grad%d[d]" % p, abs(grad[p, d] - o["g"][d]), gbar)
        res = {}
        for code in (0, 3, 2):                                      # the fp64 kernel, seven planes (the default), six planes
            eng.tune("predict_sliced", code)
            m, v = eng.predict(Xs)
            Ks = eng.get("Kstar", WC.W)
            res[code] = (m, v, Ks)
            for p in range(WC.P):
                o, cb = per[p], max(float(amps[p]), 1.0)
                led.ratio("Ks%d/%d" % (p, code), np.max(np.abs(Ks[p] - o["Ks"])), 1e-13 * cb)
                led.ratio("mean%d/%d" % (p, code), np.max(np.abs(m[:, p] - o["m"])), 1e-11 * np.max(np.abs(o["m"])))
                led.ratio("var%d/%d" % (p, code), np.max(np.abs(v[:, p] - o["v"]) / np.abs(o["v"])), 1e-10)
        K64 = res[0][2]
        for p in range(WC.P):
            ec = _plane_exponent(float(amps[p]))
            led.same("seven planes of K* against the host integer model, GP %d" % p,
                     np.array_equal(res[3][2][p], np.ldexp(np.rint(np.ldexp(K64[p], 55 - ec)), ec - 55)))
            # (<=: the bound is the rounding's own half unit and a tie reaches it; the ledger's ratios are strict, so this one is not one)
            k6 = float(np.max(np.abs(res[2][2][p] - K64[p])) / np.ldexp(1.0, ec - 48))
            led.ratios.append(("K6-K64 %d" % p, k6))
            if not k6 <= 1.0:
                led.bad.append("six planes of K*, GP %d: %.3g x 2^(e_c - 48)" % (p, k6))
        led.same("the int8 kernels ran", not np.array_equal(res[3][1], res[0][1]) and not np.array_equal(res[2][1], res[0][1]))
        for code in (0, 3):
            eng.tune("predict_sliced", code); single.tune("predict_sliced", code)
            m, v = res[code][0], res[code][1]
            for sl in SLICES:
                ms, vs = eng.predict(Xs[sl])
                led.same("rows %d:%d alone, arithmetic %d" % (sl.start, sl.stop, code), np.array_equal(ms, m[sl]) and np.array_equal(vs, v[sl]))
            for key, value, back in (("kcross_wpl", 1, 2), ("kcross_chunks", 1, 0), ("kcross_chunks", 3, 0)):
                eng.tune(key, value)
                try:
                    mt, vt = eng.predict(Xs)
                finally:
                    eng.tune(key, back)
                led.same("%s = %d, arithmetic %d" % (key, value, code), np.array_equal(mt, m) and np.array_equal(vt, v))
            m1, v1 = single.predict(Xs)
            led.same("GP 1 alone, arithmetic %d" % code, np.array_equal(m1[:, 0], m[:, 1]) and np.array_equal(v1[:, 0], v[:, 1]))
    finally:
        eng.tune("kcross_wpl", 2); eng.tune("kcross_chunks", 0); eng.tune("predict_sliced", arith)
        eng.close(); single.close()
    led.close()


# ------------------------------------------------------------------------------------------------ b. prediction gradients
@pytest.mark.parametrize("kernel", WC.KINDS)
@pytest.mark.parametrize("d", WC.WIDE_DS)
def test_predict_grad_at_the_wide_widths(tmp_path, kernel, d):
    """k_gp_grad splits its 256 threads as G = 256 / d: 12, 10, 10, 8, 5 and 4 groups here (test_gpu_gradient.py has d = 8, 20);
    the emulator, the rows and the bar of test_gpu_gradient.py::test_predict_grad_matches_autograd, length scales 0.6 sqrt(d)"""
    import grad_reference as R
    from test_gpu_gradient import BAR, _emulator, _rowerr, _rows
    _, emu, _ = _emulator(str(tmp_path), 160, d, 6, 3, kernel, ell=0.6 * np.sqrt(d))
    eng = emu._engine_ready()
    X = _rows(d, 1)
    X[0] = emu._X_train[7]                                    # exactly on a training point
    X[1] = 0.0
    X[2] = 1.0                                                # the box corners
    X[3, ::2] = 0.0
    st = R.state_from_emulator(emu)
    dm, dv = eng.predict_grad(X)
    jm = R.jacobian_rows(lambda x: R.gp_mean_var(st, x)[0], X)
    jv = R.jacobian_rows(lambda x: R.gp_mean_var(st, x)[1], X)
    assert dm.shape == dv.shape == (len(X), 3, d)
    assert np.abs(jm[:, :, d - 1]).min() > 0.0                # (the last column does carry a slope)
    em, ev = _rowerr(dm, jm), _rowerr(dv, jv)
    _report("predict_grad d=%d %s: dmean %.2g  dvar %.2g" % (d, kernel, em.max() / BAR, ev.max() / BAR))
    assert np.all(em <= BAR), em
    assert np.all(ev <= BAR), ev
    assert np.array_equal(eng.predict_grad(X, return_var=False), dm)


# ------------------------------------------------------------------------------------------------ c. Sobol
@pytest.mark.parametrize("d", WC.WIDE_DS)
def test_sobol_at_the_wide_widths(d):
    """k_sobol_pairs<24> and <32> in one pass (d = 21, 24 / 25, 32) and <32> in two (d = 49, 64): e, H, V_S and the indices against
    the model on the device's own alpha, at the bars of test_gpu_sobol.py::test_against_model"""
    import sobol_reference as R
    from test_gpu_sobol import M_OBS, _engine, _transform
    N, _, P, seed = WC.SOBOL_CASES[d]
    X, Z, theta, lo, hi = R.make_case(N, d, P, seed)
    A, mu = _transform(P, seed)
    eng = _engine(X, Z, theta)
    eng.set_transform(0, mu, A=A, cov_trunc=np.zeros((M_OBS, M_OBS)))
    alpha = eng.get("alpha")
    e, H = eng.sobol(lo, hi)
    mean, var, first, total = eng.emu_sobol(lo, hi)
    eng.close()
    amp, ell = np.exp(theta[:, 0]), np.exp(theta[:, 1:d + 1])
    e_m, H_m, Ue, UH = R.gp_integrals(X, alpha, amp, ell, lo, hi)
    mean_m, V, UV = R.observables(e_m, H_m, Ue, UH, A, mu)
    bf = R.bar_factor(N, d)
    cap = (UV / V[:, 2 * d:]).max()
    assert np.all(V[:, 2 * d] > 0) and cap <= R.CAP
    for a in (e, H, mean, var, first, total):
        assert np.all(np.isfinite(a))
    assert np.array_equal(H, H.transpose(1, 0, 2))
    r_e = (np.abs(e - e_m) / (bf * Ue)).max()
    r_H = (np.abs(H - H_m) / (bf * UH)).max()
    _, Vd, _ = R.observables(e, H, Ue, UH, A, mu)
    BV = bf * UV
    r_V = (np.abs(Vd - V) / BV).max()
    r_var = (np.abs(var - V[:, 2 * d]) / BV[:, 2 * d]).max()
    r_mean = (np.abs(mean - mean_m) / (bf * (np.abs(mu) + np.abs(A).T @ Ue))).max()
    f_m, t_m = R.indices(V)
    bfi, bti = R.index_bars(V, BV)
    r_f, r_t = (np.abs(first - f_m) / bfi).max(), (np.abs(total - t_m) / bti).max()
    _report("sobol d=%d N=%d: U_S / V %.3g; ratios to the bar: e %.2g  H %.2g  V_S %.2g  var %.2g  mean %.2g  first %.2g  total %.2g"
            % (d, N, cap, r_e, r_H, r_V, r_var, r_mean, r_f, r_t))
    assert max(r_e, r_H, r_V, r_var, r_mean, r_f, r_t) <= 1.0


# ------------------------------------------------------------------------------------------------ d. the shared chain launch
@pytest.mark.parametrize("d", WC.CHAIN_DS)
def test_shared_chain_launch_at_the_wide_widths(tmp_path, d):
    """k_kcross_multi<24 | 32 | 64>: three emulators (one per kernel family) whose designs all pad to Np = 128 share one launch;
    W = 300 rows (Wuse = 384: two walkers per lane where dpad <= 32), a few outside the box; fp64 and the default arithmetic.
    The log-posterior is bit-equal with one launch per emulator (chain_batch 0) and within 1e-10 of the oracle chain of
    test_gpu_multi_emulator.py on 16 rows inside the box"""
    from gpbayestools_hic_amd import synth
    from gpbayestools_hic_amd.workload import build_multi_chain
    from test_gpu_multi_emulator import _oracle_chain
    chain, emus, info = build_multi_chain(WC.CHAIN_SPECS, d, workdir=str(tmp_path))
    engs = [e._engine_ready() for e in emus]
    assert all(int(g.get("form").sum()) == 0 for g in engs)   # all in the Gram form: the shared launch's condition
    X = synth.walkers(300, d, seed=d)
    X[100:108] = np.clip(info["xstar"] + 0.01 * np.random.default_rng(d).standard_normal((8, d)), 0.01, 0.99)      # near the truth
    X[5, d - 1] = 1.25                                        # outside,
    X[17, 0] = 0.0                                            # on the boundary: outside,
    X[299, d // 2] = -0.5                                     # and the last row of the batch
    inside = np.all((X > 0.0) & (X < 1.0), axis=1)
    assert inside.sum() == 297
    rows = np.r_[np.flatnonzero(inside)[:8], 100:108]         # the 16 rows held to the oracle
    ref = _oracle_chain(info)(X[rows])
    assert np.all(np.isfinite(ref))
    arith = [g.predict_sliced for g in engs]
    ratios = []
    try:
        for fp64 in (True, False):
            for g, a in zip(engs, arith):
                g.tune("predict_sliced", 0 if fp64 else a)
            one = chain.log_posterior(X)
            engs[0].tune("chain_batch", 0)
            try:
                sep = chain.log_posterior(X)
            finally:
                engs[0].tune("chain_batch", 1)
            assert np.array_equal(np.isneginf(one), ~inside)
            assert np.array_equal(sep, one), fp64
            ratios.append(relerr(one[rows], ref) / 1e-10)
    finally:
        for g, a in zip(engs, arith):
            g.tune("predict_sliced", a)
    _report("chain d=%d: log-posterior against the oracle chain, ratio to 1e-10: fp64 %.2g  default %.2g" % (d, ratios[0], ratios[1]))
    assert max(ratios) < 1.0
