"""GPU tier: closed-form Sobol indices and main-effect curves on the device (gpb_gp_sobol, gpb_emu_sobol, gpb_emu_main_effect,
GPEngine.sobol / emu_sobol / emu_main_effect, Emulator.sobol_indices / main_effect, Chain.sobol_indices) against the host model
tests/sobol_reference.py evaluated on the device's own alpha, and against the existing predict path.

The bar on e, H and V_S is 2 k 2^-53 U with k = 16 (2d + 3) + 24 + T (sobol_reference.bar_factor: 16 ulp, the OpenCL bound on erf,
for each of the 2d + 3 factors of a term; 24 for the additions inside a thread and a workgroup; T = ceil(N / 64)^2 tile partials added
in sequence; the factor 2 for the model's own rounding) and U the sum of the absolute values of the same terms; the indices get
(B_S + index B_all) / V.  Every case keeps U_S / V below 1e7, so that the bar says something about the indices.
Measured on an MI355X, the largest ratio to the bar over the cases here: 0.017 (e of the "underflow" case; H 0.016, V_S 0.008, indices
0.006 there); over the other cases e 0.0018, H 0.0007, V_S 0.0004, indices 0.0001; V_j against the main-effect curve 4e-5.  Far below 1:
the bar charges every factor the 16 ulp OpenCL allows erf and the device's erf is good to about an ulp.  The formula stays as derived."""
import functools

import numpy as np
import pytest

import sobol_reference as R

pytestmark = pytest.mark.gpu

# (N, d, P, seed, small_l0): each the smallest shape that reaches its branch
CASES = {
    "one_tile": (64, 1, 1, 1, False),
    "ragged_dpad16": (65, 9, 2, 4, False),              # two row blocks, the second of one row
    "pad_front": (100, 3, 3, 11, False),                # Np = 128: 16 pad rows in front, 12 behind; p != q blocks
    "three_blocks": (150, 5, 3, 12, False),
    "width20": (100, 20, 2, 6, False),                  # cfg 4's width
    "two_pass": (64, 33, 1, 8, False),                  # dpad = 48: two passes over windows of 24 output dimensions
    "underflow": (100, 3, 2, 9, True),                  # l = 0.01 w in dimension 0
}
M_OBS = 4


def _engine(X, Z, theta):
    from gpbayestools_hic_amd import GPEngine
    eng = GPEngine(0)
    eng.set_data(X, Z, "RBF", R.ALPHA)
    eng.set_theta(theta)
    eng.factor()
    return eng


def _transform(P, seed):
    rng = np.random.default_rng(seed + 50)
    return rng.standard_normal((P, M_OBS)), rng.standard_normal(M_OBS)


@functools.lru_cache(maxsize=None)
def _case(name):
    """data, device results and the model on the device's alpha, computed once and shared (treated as read-only)"""
    N, d, P, seed, small = CASES[name]
    X, Z, theta, lo, hi = R.make_case(N, d, P, seed, small_l0=small)
    A, mu = _transform(P, seed)
    eng = _engine(X, Z, theta)
    eng.set_transform(0, mu, A=A, cov_trunc=np.zeros((M_OBS, M_OBS)))
    alpha = eng.get("alpha")
    dev = dict(gp=eng.sobol(lo, hi), emu=eng.emu_sobol(lo, hi))
    eng.close()
    amp, ell = np.exp(theta[:, 0]), np.exp(theta[:, 1:d + 1])
    e, H, Ue, UH = R.gp_integrals(X, alpha, amp, ell, lo, hi)
    mean, V, UV = R.observables(e, H, Ue, UH, A, mu)
    return dict(N=N, d=d, P=P, X=X, Z=Z, theta=theta, lo=lo, hi=hi, A=A, mu=mu, alpha=alpha, amp=amp, ell=ell, dev=dev,
                e=e, H=H, Ue=Ue, UH=UH, mean=mean, V=V, UV=UV)


@pytest.mark.parametrize("name", list(CASES))
def test_against_model(name):
    """e, H, the V_S derived from them and the indices against the model, at the bar of the module docstring (measured ratios to the
    bar: there and in DESIGN.md section 14)"""
    c = _case(name)
    N, d = c["N"], c["d"]
    bf = R.bar_factor(N, d)
    cap = (c["UV"] / c["V"][:, 2 * d:]).max()
    print("%s: U_S / V = %.3g" % (name, cap))
    assert np.all(c["V"][:, 2 * d] > 0) and cap <= R.CAP
    e, H = c["dev"]["gp"]
    mean, var, first, total = c["dev"]["emu"]
    for a in (e, H, mean, var, first, total):
        assert np.all(np.isfinite(a))
    r_e = (np.abs(e - c["e"]) / (bf * c["Ue"])).max()
    r_H = (np.abs(H - c["H"]) / (bf * c["UH"])).max()
    _, Vd, _ = R.observables(e, H, c["Ue"], c["UH"], c["A"], c["mu"])
    BV = bf * c["UV"]
    r_V = (np.abs(Vd - c["V"]) / BV).max()
    r_var = (np.abs(var - c["V"][:, 2 * d]) / BV[:, 2 * d]).max()
    r_mean = (np.abs(mean - c["mean"]) / (bf * (np.abs(c["mu"]) + np.abs(c["A"]).T @ c["Ue"]))).max()
    f_m, t_m = R.indices(c["V"])
    bfi, bti = R.index_bars(c["V"], BV)
    r_f, r_t = (np.abs(first - f_m) / bfi).max(), (np.abs(total - t_m) / bti).max()
    print("%s: ratios to the bar: e %.3g  H %.3g  V_S %.3g  var %.3g  mean %.3g  first %.3g  total %.3g"
          % (name, r_e, r_H, r_V, r_var, r_mean, r_f, r_t))
    assert max(r_e, r_H, r_V, r_var, r_mean, r_f, r_t) <= 1.0


def test_device_properties():
    """H[p][q] = H[q][p]; a P = 1 engine gives the [p, p] block of the P = 3 engine's H and its e_p bit for bit; two calls give the
    same bits; host outputs equal on_device outputs"""
    c = _case("pad_front")
    X, Z, theta, lo, hi = c["X"], c["Z"], c["theta"], c["lo"], c["hi"]
    e, H = c["dev"]["gp"]
    assert np.array_equal(H, H.transpose(1, 0, 2))
    eng = _engine(X, Z, theta)
    eng.set_transform(0, c["mu"], A=c["A"], cov_trunc=np.zeros((M_OBS, M_OBS)))
    e2, H2 = eng.sobol(lo, hi)
    assert np.array_equal(e, e2) and np.array_equal(H, H2)
    ed, Hd = eng.sobol(lo, hi, on_device=True)
    assert np.array_equal(ed.cpu().numpy(), e) and np.array_equal(Hd.cpu().numpy(), H)
    for host, dev in zip(c["dev"]["emu"], eng.emu_sobol(lo, hi, on_device=True)):
        assert np.array_equal(dev.cpu().numpy(), host)
    eng.close()
    for p in range(c["P"]):
        one = _engine(X, Z[p:p + 1], theta[p:p + 1])
        assert np.array_equal(one.get("alpha")[0], c["alpha"][p])             # (the premise: the fit's bits do not depend on P)
        e1, H1 = one.sobol(lo, hi)
        one.close()
        assert e1[0] == e[p] and np.array_equal(H1[0, 0], H[p, p])


def _gl(n, lo, hi):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (hi - lo) * x + 0.5 * (hi + lo), 0.5 * w


def test_main_effect_against_the_predict_path():
    """independent of all new arithmetic: at d = 1 the main effect IS the emulator's mean; at d = 2 it is the 64-node Gauss-Legendre
    average of emu_predict over the other input (weights that sum to 1: the predict path's own bar, 1e-11 max(|f|, 1))"""
    c = _case("one_tile")
    eng = _engine(c["X"], c["Z"], c["theta"])
    eng.set_transform(0, c["mu"], A=c["A"], cov_trunc=np.zeros((M_OBS, M_OBS)))
    t = np.linspace(R.LO, R.HI, 50)
    curve = eng.emu_main_effect(c["lo"], c["hi"], 0, t)
    f = eng.emu_predict(t[:, None], return_cov=False)
    eng.close()
    assert np.max(np.abs(curve - f)) <= 1e-11 * max(np.abs(f).max(), 1.0)
    X, Z, theta, lo, hi = R.make_case(70, 2, 2, 21)
    A, mu = _transform(2, 21)
    eng = _engine(X, Z, theta)
    eng.set_transform(0, mu, A=A, cov_trunc=np.zeros((M_OBS, M_OBS)))
    x, w = _gl(64, R.LO, R.HI)
    t = np.linspace(R.LO, R.HI, 9)
    for j in (0, 1):
        curve = eng.emu_main_effect(lo, hi, j, t)
        grid = np.empty((9, 64, 2))
        grid[:, :, j], grid[:, :, 1 - j] = t[:, None], x[None, :]
        f = eng.emu_predict(grid.reshape(-1, 2), return_cov=False).reshape(9, 64, M_OBS)
        assert np.max(np.abs(curve - np.einsum("q,gqm->gm", w, f))) <= 1e-11 * max(np.abs(f).max(), 1.0)
    eng.close()


@pytest.mark.parametrize("name", ["pad_front", "three_blocks"])
def test_first_order_is_the_variance_of_the_main_effect(name):
    """V_j from gpb_emu_sobol against the 128-node Gauss-Legendre variance of the device's own main-effect curve: the bar of the
    module docstring on V_j plus the quadrature's 1e-12 (relative to V_j)"""
    c = _case(name)
    d = c["d"]
    eng = _engine(c["X"], c["Z"], c["theta"])
    eng.set_transform(0, c["mu"], A=c["A"], cov_trunc=np.zeros((M_OBS, M_OBS)))
    x, w = _gl(128, R.LO, R.HI)
    _, var, first, _ = c["dev"]["emu"]
    BV = R.bar_factor(c["N"], d) * c["UV"]
    worst = 0.0
    for j in range(d):
        curve = eng.emu_main_effect(c["lo"], c["hi"], j, x)
        dev = curve - w @ curve
        vj = w @ dev ** 2
        worst = max(worst, (np.abs(first[:, j] * var - vj) / (BV[:, j] + 1e-12 * vj)).max())
    eng.close()
    print("%s: first-order variance against the main-effect curve, ratio to the bar %.3g" % (name, worst))
    assert worst <= 1.0


# ---------------------------------------------------------------------------- emulator and chain level
def _emulator(tmp_path, kw, kernel="RBF", N=100, nobs=6, seed=21, name=""):
    from gpbayestools_hic_amd import Emulator, synth
    d = 4
    X = synth.lhs(N, d, seed)
    Y = synth.observables(X, nobs, seed=seed + 1)
    tp, pf = str(tmp_path / ("train%s.pkl" % name)), str(tmp_path / "par.txt")
    synth.write_training_pickle(tp, X, Y, 0.02 * Y)
    synth.write_parameter_file(pf, np.full(d, -0.1), np.full(d, 1.2))
    emu = Emulator(training_set_path=tp, parameter_file=pf, npc=3, **kw)
    P = nobs if kw.get("perform_no_PCA") else 3
    emu.trainEmulator([True] * emu.nev, kernel_type=kernel, thetas=synth.fixed_theta(d, P, ell=1.3, noise=0.05))
    return emu


def _emulator_model(emu, lo, hi):
    eng = emu._engine_ready()
    X, theta, d = emu._X_train, emu.thetas_, emu._X_train.shape[1]
    amp, ell = np.exp(theta[:, 0]), np.exp(theta[:, 1:d + 1])
    e, H, Ue, UH = R.gp_integrals(X, eng.get("alpha"), amp, ell, lo, hi)
    A = np.diag(emu.scaler.scale_) if emu.perform_no_PCA_ else emu._A
    mean, V, UV = R.observables(e, H, Ue, UH, A, emu.scaler.mean_)
    return mean, V, R.bar_factor(X.shape[0], d) * UV, np.abs(emu.scaler.mean_) + np.abs(A).T @ Ue


def _check_indices(res, model, N, d):
    mean, V, BV, Umean = model
    f_m, t_m = R.indices(V)
    bfi, bti = R.index_bars(V, BV)
    assert np.all(np.abs(res.mean - mean) <= R.bar_factor(N, d) * Umean)
    assert np.all(np.abs(res.variance - V[:, 2 * d]) <= BV[:, 2 * d])
    assert np.all(np.abs(res.first_order - f_m) <= bfi) and np.all(np.abs(res.total - t_m) <= bti)


@pytest.mark.parametrize("mode", ["pca", "nopca"])
def test_emulator_sobol_indices(tmp_path, mode):
    emu = _emulator(tmp_path, dict(perform_no_PCA=True) if mode == "nopca" else {})
    d = 4
    res = emu.sobol_indices()
    assert res.first_order.shape == (emu.nobs, d) and res.names == list(emu.pardict)
    _check_indices(res, _emulator_model(emu, emu.design_min, emu.design_max), emu.nev, d)
    bounds = np.stack([np.full(d, 0.0), np.full(d, 1.0)], axis=1)
    res2 = emu.sobol_indices(bounds)
    _check_indices(res2, _emulator_model(emu, bounds[:, 0], bounds[:, 1]), emu.nev, d)
    assert not np.array_equal(res.variance, res2.variance)
    name = list(emu.pardict)[2]
    grid, curve = emu.main_effect(name)
    assert grid.shape == (101,) and curve.shape == (101, emu.nobs)
    assert grid[0] == emu.design_min[2] and grid[-1] == emu.design_max[2]
    g2, c2 = emu.main_effect(2, grid=grid[::10])
    assert np.array_equal(c2, curve[::10])
    # the curve's box average is the mean
    x, w = _gl(64, emu.design_min[2], emu.design_max[2])
    assert np.max(np.abs(w @ emu.main_effect(2, grid=x)[1] - res.mean)) <= 1e-11 * max(np.abs(res.mean).max(), 1.0)
    with pytest.raises(ValueError):
        emu.main_effect("no_such_parameter")
    with pytest.raises(ValueError):
        emu.main_effect(d)


def test_chain_sobol_indices(tmp_path):
    """two emulators with different N and M on the chain's prior box, concatenated along the observables in emuList order"""
    from gpbayestools_hic_amd import workload
    d = 3
    chain, emus, info = workload.build_multi_chain([(64, 5, 2, "RBF"), (100, 7, 3, "RBF")], d, workdir=str(tmp_path))
    res = chain.sobol_indices()
    assert res.mean.shape == (12,) and res.first_order.shape == (12, d) and res.total.shape == (12, d)
    off = 0
    for emu in emus:
        part = emu.sobol_indices(np.stack([chain.min, chain.max], axis=1))
        sl = slice(off, off + emu.nobs)
        assert all(np.array_equal(getattr(res, k)[sl], getattr(part, k)) for k in ("mean", "variance", "first_order", "total"))
        _check_indices(part, _emulator_model(emu, chain.min, chain.max), emu.nev, d)
        off += emu.nobs
    chain.emuList = [emus[0], object()]
    with pytest.raises(NotImplementedError, match="foreign"):
        chain.sobol_indices()


# ---------------------------------------------------------------------------- refusals
def test_emulator_refusals(tmp_path):
    from gpbayestools_hic_amd import workload
    from gpbayestools_hic_amd._native import GPBError
    logexp = _emulator(tmp_path, dict(logTrafo=True, exp_and_cov_diagonal=True), name="a")
    with pytest.raises(ValueError, match="log_observable"):
        logexp.sobol_indices()
    with pytest.raises(ValueError, match="log_observable"):
        logexp.main_effect(0)
    res = logexp.sobol_indices(log_observable=True)
    _check_indices(res, _emulator_model(logexp, logexp.design_min, logexp.design_max), logexp.nev, 4)
    nopca_logexp = _emulator(tmp_path, dict(perform_no_PCA=True, logTrafo=True, exp_and_cov_diagonal=True), name="b")
    with pytest.raises(ValueError, match="log_observable"):
        nopca_logexp.sobol_indices()
    assert np.all(np.isfinite(nopca_logexp.sobol_indices(log_observable=True).total))
    matern = _emulator(tmp_path, {}, kernel="Matern", name="c")
    with pytest.raises(NotImplementedError, match="Matern"):
        matern.sobol_indices()
    with pytest.raises(NotImplementedError, match="Matern"):
        matern.main_effect(0)
    (tmp_path / "mapped").mkdir()
    _, emus, _ = workload.build_multi_chain([(64, 5, 2, "RBF")], 20, workdir=str(tmp_path / "mapped"), mapped=True)
    with pytest.raises(NotImplementedError, match="parameterTrafoPCA"):
        emus[0].sobol_indices()
    eng = emus[0]._engine_ready()                       # (the engine itself refuses a context with a parameter map)
    with pytest.raises(GPBError, match="parameter map"):
        eng.sobol(np.zeros(eng.d), np.ones(eng.d))


def test_engine_refusals():
    from gpbayestools_hic_amd import GPEngine
    from gpbayestools_hic_amd._native import GPBError, ptr
    E_ARG, E_STATE = -1, -2
    N, d, P = 64, 3, 2
    X, Z, theta, lo, hi = R.make_case(N, d, P, 31)
    A, mu = _transform(P, 31)
    ns = 2 * d + 1
    e, H = np.empty(P), np.empty((P, P, ns))
    o = [np.empty(M_OBS), np.empty(M_OBS), np.empty((M_OBS, d)), np.empty((M_OBS, d))]
    t, curve = np.linspace(0.0, 1.0, 5), np.empty((5, M_OBS))

    def gp(g, lo_=lo, hi_=hi):
        return g.lib.gpb_gp_sobol(g.h, ptr(lo_), ptr(hi_), 0, ptr(e), ptr(H))

    def emu(g):
        return g.lib.gpb_emu_sobol(g.h, ptr(lo), ptr(hi), 0, *[ptr(a) for a in o])

    def main(g, j=0, G=5):
        return g.lib.gpb_emu_main_effect(g.h, ptr(lo), ptr(hi), j, ptr(t), G, 0, ptr(curve))

    eng = GPEngine(0)
    eng.set_data(X, Z, "RBF", R.ALPHA)
    eng.set_theta(theta)
    assert gp(eng) == E_STATE                            # no factorisation
    with pytest.raises(GPBError, match="gpb_gp_factor"):
        eng.sobol(lo, hi)
    eng.factor()
    assert emu(eng) == E_STATE and main(eng) == E_STATE  # no transform
    with pytest.raises(GPBError, match="gpb_emu_set_transform"):
        eng.emu_sobol(lo, hi)
    eng.set_transform(0, mu, A=A, cov_trunc=np.zeros((M_OBS, M_OBS)))
    bad = hi.copy()
    bad[1] = lo[1]
    assert gp(eng, hi_=bad) == E_ARG                     # hi <= lo
    assert main(eng, j=-1) == E_ARG and main(eng, j=d) == E_ARG and main(eng, G=0) == E_ARG
    with pytest.raises(ValueError):
        eng.sobol(lo[:2], hi[:2])
    # the context is as usable as before: the results are those of a fresh engine
    ref = _engine(X, Z, theta)
    e0, H0 = ref.sobol(lo, hi)
    ref.close()
    e1, H1 = eng.sobol(lo, hi)
    assert np.array_equal(e0, e1) and np.array_equal(H0, H1)
    assert emu(eng) == 0 and main(eng) == 0
    eng.close()
    for kernel in ("Matern", "Matern25"):
        m = GPEngine(0)
        m.set_data(X, Z, kernel, R.ALPHA)
        m.set_theta(theta)
        m.factor()
        assert gp(m) == E_ARG
        with pytest.raises(GPBError, match="Matern"):
            m.sobol(lo, hi)
        m.close()
    multi = GPEngine(0)
    multi.set_data_multi([X, X[:60]], [Z[0], Z[1][:60]], "RBF", R.ALPHA)
    multi.set_theta(theta)
    multi.factor()
    assert gp(multi) == E_STATE
    with pytest.raises(GPBError, match="fit-only"):
        multi.sobol(lo, hi)
    multi.close()
