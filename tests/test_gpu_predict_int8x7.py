"""
GPU tier: the default arithmetic of V = L^-1 K*^T — seven signed 8-bit digit planes per operand on v_mfma_i32_32x32x32_i8, the 28
digit products of levels 6..12 summed exactly in int32, combined in fp64 (gpb_ctx_option 51 = 3, csrc/gpb_sliced.hip).  It stands
in for the fp64 kernel everywhere, so it is held to the fp64 path's bars (sk:_gpr.py:454-460, src/emulator.py:553,573-575): mean
1e-11, variance 1e-10 relative, log-posterior 1e-10 — on the shapes of test_gpu_sliced.py, in the worst corner of the search
box, and on the likelihood cases where six planes missed the bar — and to the bit properties the fp64 kernel has.
"""
import numpy as np
import pytest

from conftest import maxrel, relerr

pytestmark = pytest.mark.gpu

D7 = 3          # option 51 values: 0 the fp64 kernel, 1 six planes by rule, 3 seven planes (the default)


def _problem(N, d, P, kind, W, seed, sn2=0.05, c=1.0):
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


def test_seven_planes_are_the_default():
    from gpbayestools_hic_amd import GPEngine
    from gpbayestools_hic_amd.engine import predict_sliced_from_env
    eng = GPEngine(0)
    assert eng.predict_sliced == (D7 if predict_sliced_from_env() is None else predict_sliced_from_env())
    eng.close()


@pytest.mark.parametrize("N,d,P,kind,W", [
    (1000, 15, 4, "RBF", 515),          # Np = 1024: padding in front and behind; ragged batch
    (320, 20, 3, "Matern15", 130),      # Np = 320: the last 128-row block is half empty
    (65, 3, 2, "Matern25", 1),          # Np = 128, one walker
    (40, 4, 2, "RBF", 70),              # Np = 64: half a row block
    (900, 12, 3, "RBF", 300),           # Np = 960: a whole 32-deep K-step of front padding skipped
    (2048, 20, 10, "RBF", 256),         # cfg 4's GPs on a rank's share of eight
    (640, 8, 9, "RBF", 1024),           # nine GPs: more than one super-block per row group
])
def test_seven_planes_against_the_oracle(N, d, P, kind, W):
    from gpbayestools_hic_amd import GPEngine
    from oracle import gp_oracle as O
    X, Z, th, Xs = _problem(N, d, P, kind, W, seed=N + W)
    eng = GPEngine(0)
    eng.set_data(X, Z, kind, alpha=0.1); eng.set_theta(th); eng.factor()
    eng.tune("predict_sliced", 0)
    m64, v64 = eng.predict(Xs)
    eng.tune("predict_sliced", D7)
    m, v = eng.predict(Xs)
    assert not np.array_equal(v, v64)                          # the int8 kernel did run ...
    assert relerr(v, v64) < 1e-11 and maxrel(m, m64) < 1e-13   # ... and stays with the fp64 kernel
    kid = O.KIND_NAMES[kind]
    rows = np.unique(np.r_[0:min(W, 12), np.random.default_rng(1).choice(W, min(W, 20), replace=False)])
    for p in range(P):
        L, a = O.gp_factor(X, Z[p], th[p], kid, 0.1)
        mo, vo = O.gp_predict(Xs[rows], X, th[p], L, a, kid)
        assert maxrel(m[rows, p], mo) < 1e-11
        assert relerr(v[rows, p], vo) < 1e-10
    assert np.all(v > 0)
    # batch cuts: integer sums are exact and the epilogue's order is the row's
    for lo, hi in ((0, W // 2), (W // 2, W), (min(3, W - 1), W)):
        if hi > lo:
            mm, vv = eng.predict(Xs[lo:hi])
            assert np.array_equal(vv, v[lo:hi]) and np.array_equal(mm, m[lo:hi])
    # every tile shape gives the same bits
    for tile in (128, 64):
        eng.force_tile(tile)
        mm, vv = eng.predict(Xs)
        assert np.array_equal(vv, v) and np.array_equal(mm, m)
    eng.force_tile(0)
    eng.close()


def test_kstar_planes_match_a_host_integer_model():
    """the digit planes of K*^T (read back by gpb_gp_get) are round(K* 2^55 / 2^e_c) 2^-55 2^e_c of the fp64 kernel's K* values,
    bit for bit: the exact split of the 55-bit integer in the cross kernel's epilogue"""
    from gpbayestools_hic_amd import GPEngine
    X, Z, th, Xs = _problem(200, 5, 2, "RBF", 70, seed=4, c=3.0)
    eng = GPEngine(0)
    eng.set_data(X, Z, "RBF", alpha=0.1); eng.set_theta(th); eng.factor()
    eng.tune("predict_sliced", 0)
    eng.predict(Xs)
    K64 = eng.get("Kstar", len(Xs))
    eng.tune("predict_sliced", D7)
    eng.predict(Xs)
    K7 = eng.get("Kstar", len(Xs))
    for p in range(2):
        c = float(np.exp(th[p, 0]))
        f, e = np.frexp(c)
        ec = int(e) if f <= 0.99 else int(e) + 1
        model = np.ldexp(np.rint(np.ldexp(K64[p], 55 - ec)), ec - 55)
        assert np.array_equal(K7[p], model)
        assert np.max(np.abs(K7[p] - K64[p])) <= np.ldexp(1.0, ec - 56)
    eng.close()


def test_the_worst_corner_of_the_search_box():
    """sigma_n^2 = 1e-2, c = e^3, l = 8 x the box: the cancellation six planes miss the bar at; seven hold it, with no rule"""
    from gpbayestools_hic_amd import GPEngine
    from oracle import gp_oracle as O
    X, Z, th, Xs = _problem(500, 5, 3, "RBF", 256, seed=9, sn2=0.05)
    th[:, 0], th[:, -1] = 3.0, np.log(1e-2)
    th[:, 1:-1] = np.log(8.0)
    Xs[:64] = X[:64] + 1e-6
    eng = GPEngine(0)
    eng.set_data(X, Z, "RBF", alpha=0.1); eng.set_theta(th); eng.factor()
    eng.tune("predict_sliced", 0)
    _, v64 = eng.predict(Xs)
    eng.tune("predict_sliced", D7)
    m7, v7 = eng.predict(Xs)
    assert not np.array_equal(v7, v64)
    for p in range(3):
        L, a = O.gp_factor(X, Z[p], th[p], O.KIND_RBF, 0.1)
        mo, vo = O.gp_predict(Xs[:64], X, th[p], L, a, O.KIND_RBF)
        assert relerr(v7[:64, p], vo) < 1e-10 and relerr(v64[:64, p], vo) < 1e-10
        assert maxrel(m7[:64, p], mo) < 1e-11
    eng.close()


@pytest.mark.parametrize("M,P", [(41, 7), (64, 10), (20, 1), (24, 17), (3, 3)])
def test_log_likelihood_where_six_planes_missed(M, P):
    """the cases of test_gpu_engine.py::test_loglike_fast_and_generic_paths that six planes failed: 1e-10 against the oracle"""
    from gpbayestools_hic_amd import GPEngine, synth
    from gpbayestools_hic_amd.engine import MODE_PCA
    from oracle import gp_oracle as O
    N, d, W = 256, 6, 203
    X = synth.lhs(N, d, seed=M)
    Y = synth.observables(X, M, seed=M + 1)
    oe = O.OracleEmulator(X, Y, np.zeros(d), np.ones(d), P).fit(synth.fixed_theta(d, P))
    eng = GPEngine(0)
    eng.tune("predict_sliced", D7)
    eng.set_data(X, oe.Z.T, "RBF", 0.1); eng.set_theta(oe.thetas); eng.factor()
    eng.set_transform(MODE_PCA, oe.mu, A=oe.A, cov_trunc=oe.cov_trunc)
    yexp = oe.predict(synth.truth_point(d)[None, :], return_cov=False)[0]
    rng = np.random.default_rng(M * P)
    Bm = rng.standard_normal((M, M)) * 0.01
    cexp = np.diag((0.05 * np.abs(yexp)) ** 2) + Bm @ Bm.T
    eng.set_likelihood(yexp, cexp)
    Xw = synth.walkers(W, d, seed=5)
    mY, mC = oe.predict(Xw, True, np.zeros(W))
    ref = np.array([O.mvn_loglike(a, c) for a, c in zip(mY - yexp, mC + cexp)])
    lowrank = eng.loglike(Xw).copy()
    assert relerr(lowrank, ref) < 1e-10
    eng.tune("lowrank", 0)
    fast = eng.loglike(Xw).copy()
    assert relerr(fast, ref) < 1e-10
    eng.close()


def test_chain_bits_with_seven_planes(tmp_path):
    """cfg 4's emulator at N = 320 through the drop-in classes, default arithmetic: compaction, the host- and C-driven loops,
    the pickled choice on a new engine"""
    import dill
    from gpbayestools_hic_amd import synth
    from gpbayestools_hic_amd.workload import build_chain
    from oracle import gp_oracle as O
    chain, emu, info = build_chain(4, workdir=str(tmp_path), N=320)
    chain.set_predict_arithmetic("fp64-int8")
    d = info["d"]
    X = synth.walkers(300, d, seed=5)
    X[::7, 3] = 1.5
    lp = chain.log_posterior(X)
    fin = np.isfinite(lp)
    oe = O.OracleEmulator(info["X"], info["Y"], info["lo"], info["hi"], info["P"], O.KIND_RBF).fit(synth.fixed_theta(d, info["P"]))
    yexp = info["yexp"]; cexp = np.diag((0.05 * np.abs(yexp)) ** 2)
    ref = O.log_prob(X, info["lo"], info["hi"], lambda x, e: oe.predict(x, True, e), yexp, cexp)
    assert np.array_equal(np.isneginf(ref), ~fin) and relerr(lp[fin], ref[fin]) < 1e-10
    assert np.array_equal(chain.log_posterior(X[fin]), lp[fin])           # compaction does not change a row's bits
    d7 = emu.state_digest()
    chain.set_predict_arithmetic("fp64")
    lp64 = chain.log_posterior(X)
    assert emu.state_digest() != d7 and not np.array_equal(lp64[fin], lp[fin]) and relerr(lp64[fin], lp[fin]) < 1e-10
    chain.set_predict_arithmetic("fp64-int8")
    assert emu.state_digest() == d7 and np.array_equal(chain.log_posterior(X), lp)
    again = dill.loads(dill.dumps(emu))
    assert again.predict_arithmetic == "fp64-int8" and again.state_digest() == d7
    m7 = emu.predict(X[fin][:32], return_cov=False)
    assert np.array_equal(np.asarray(again.predict(X[fin][:32], return_cov=False)), np.asarray(m7))
    assert again._engine_ready().predict_sliced == D7


def test_shared_multi_emulator_launch_equals_own_launches(tmp_path):
    """the emulators of a chain share one SLICE cross launch and one int8 launch (option 40): the bits of each emulator's own"""
    from gpbayestools_hic_amd.workload import build_multi_chain
    from test_gpu_multi_emulator import SPECS
    chain, emus, info = build_multi_chain(SPECS, 20, workdir=str(tmp_path))
    chain.set_predict_arithmetic("fp64-int8")
    X = np.clip(info["xstar"] + 0.05 * np.random.default_rng(3).standard_normal((300, 20)), 0.01, 0.99)
    shared = chain.log_posterior(X)
    for e in emus:
        e._engine_ready().tune("chain_batch", 0)
    chain.__dict__.pop("_digest_cache", None)
    own = chain.log_posterior(X)
    assert np.array_equal(shared, own)
    chain.set_predict_arithmetic("fp64")
    lp64 = chain.log_posterior(X)
    fin = np.isfinite(lp64)
    assert relerr(shared[fin], lp64[fin]) < 1e-10
