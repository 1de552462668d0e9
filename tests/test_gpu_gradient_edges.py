"""GPU tier of the gradient path at the branches tests/test_gpu_gradient.py does not reach (csrc/gpb_grad.hip): k_like_w's
per-row slab of global memory and its largest LDS blocks, the rows whose covariance block is not positive definite, k_gp_grad's
chunk loop beyond two full chunks, k_betaT beyond its first row tile, stochastic-kriging emulators, a chain whose emulators
differ in transform mode, and empty batches.  The reference is the autograd gradient of tests/grad_reference.py, the bar the
project's own: row-wise |g - g_ref|_inf <= BAR max(|g_ref|_inf, 1), BAR = 1e-9.  Every case prints its worst ratio to the bar
(and appends it to the file GPB_GRAD_EDGES_REPORT names); the figures in the docstrings are those of an MI355X."""
import os

import numpy as np
import pytest

import grad_reference as R
from oracle import gp_oracle as O
from test_gpu_gradient import BAR, _check_chain, _emulator, _ref_logpost, _rowerr, _rows

pytestmark = pytest.mark.gpu

MODES = {"pca": (False, False), "no_pca": (True, False), "expdiag": (False, True), "no_pca_expdiag": (True, True)}


def _report(line):
    print(line)
    path = os.environ.get("GPB_GRAD_EDGES_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _ratio(name, got, ref):
    """the worst row's error over the bar: printed here, asserted by the caller"""
    r = float(np.max(_rowerr(got, ref))) / BAR
    _report("%-58s %.3g of the bar" % (name, r))
    return r


def _mode_emulator(tmp, N, d, M, P, mode, **kw):
    no_pca, expdiag = MODES[mode]
    return _emulator(tmp, N, d, M, P, no_pca=no_pca, expdiag=expdiag, **kw)


def _checked(name, chain, states, X, finite=False):
    """_check_chain, and the worst ratio of the rows inside the box reported"""
    lp, g = _check_chain(chain, states, X, finite)
    inside = np.all((X > chain.min) & (X < chain.max), axis=1)
    _, gref = R.value_and_grad(_ref_logpost(chain, states), X[inside])
    _ratio(name, g[inside], gref)
    return lp, g


def _near(xstar, n, seed, radius=0.05):
    d = len(xstar)
    return np.clip(xstar + radius * np.random.default_rng(seed).standard_normal((n, d)), 0.01, 0.99)


# ------------------------------------------------------------------ 1. either side of k_like_w's workspace switch
LIKE_W_LDS = 6144                                             # doubles (gpb_grad.hip): above it, a slab of global memory per row


def _like_w_doubles(M, P, pca):
    """like_w_doubles() of gpb_grad.hip restated: C [M][M] | B [M][ncol] | y, F, h, g2 [M] | zm, zv [P] | s, q [ncol]; the
    right-hand sides are the P rows of A (PCA) or the M unit vectors (the other three modes, where P = M without the PCA),
    and dY"""
    ncol = P + 1 if pca else M + 1
    return M * M + M * ncol + 4 * M + 2 * P + 2 * ncol


SWITCH = [("no_pca", 53, 6097), ("no_pca", 54, 6320), ("no_pca_expdiag", 54, 6320), ("expdiag", 53, 5999), ("expdiag", 54, 6220),
          ("pca", 73, 6004), ("pca", 74, 6160)]


@pytest.mark.parametrize("mode,M,doubles", SWITCH)
def test_like_w_either_side_of_the_workspace_switch(tmp_path, mode, M, doubles):
    """k_like_w with its block in dynamic LDS at the largest M that fits (NO_PCA / EXPDIAG 53, PCA 73: ~48 KiB) and in the
    per-row slab ws_g + w * ws_row of GradWs::lw at the smallest M that does not (54, 74), every mode, against autograd; d 4,
    N 64, npc 4, 24 rows.  On the slab side 130 rows too (Wld 256; more workgroups than run at once), rows 0, 63, 64, 129 held
    to autograd and lp and gradient bit-equal to each of those rows evaluated alone.
    Catches: a ws_row or a GradWs::lw carve smaller than like_w_doubles() (the slabs of neighbouring rows overlap: rows of a
    batch then differ from the same rows alone, and from autograd), a slab indexed by anything but the row, a piece of the
    block (C, B, y, F, h, g2, zm, zv, s, q) sized with the wrong one of P, M, ncol (NaN or wrong weights in one mode only), a
    dynamic-LDS size short of the block at the top of the LDS range, and a switch placed where LDS no longer holds the block.
    (Tried once: with ws_row 64 doubles short the 24 rows still pass and the 130 rows miss the bar by 1e7 - 1e9.)
    Measured, worst row's error over the bar: LDS no_pca 53 5.8e-5, expdiag 53 5.1e-5, pca 73 4.1e-5; slab (24 rows / the four
    of 130 rows) no_pca 54 3.3e-5 / 1.2e-5, no_pca_expdiag 54 4.8e-5 / 8.0e-5, expdiag 54 8.7e-5 / 6.0e-5, pca 74 4.8e-5 / 4.6e-5."""
    no_pca, _ = MODES[mode]
    P = M if no_pca else 4
    nw = _like_w_doubles(M, P, mode == "pca")
    assert nw == doubles and (nw > LIKE_W_LDS) == (M in (54, 74))
    chain, emu, xstar = _mode_emulator(str(tmp_path), 64, 4, M, 4, mode)
    st = [R.state_from_emulator(emu)]
    name = "like_w %s M %d (%d doubles, %s)" % (mode, M, nw, "slab" if nw > LIKE_W_LDS else "LDS")
    _checked(name, chain, st, _near(xstar, 24, 31))
    if nw <= LIKE_W_LDS:
        return
    X = _near(xstar, 130, 32)
    lp, g = chain.log_posterior(X, return_grad=True)
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g))
    rows = [0, 63, 64, 129]
    _, gref = R.value_and_grad(_ref_logpost(chain, st), X[rows])
    assert _ratio(name + ", 130 rows", g[rows], gref) <= 1.0
    for w in rows:
        lw, gw = chain.log_posterior(X[w:w + 1], return_grad=True)
        assert np.array_equal(lw, lp[w:w + 1]) and np.array_equal(gw, g[w:w + 1]), w


# ------------------------------------------------------------------ 2. rows whose covariance block is not positive definite
def _shift_between_rows(st, chain, X, u):
    """t in the middle of the widest gap of the sorted t*_w = 1 / (u^T C_w^-1 u) — the shift at which C_w - t u u^T turns
    singular — leaving at least four rows on either side; (t, not-PD flags, margin), all from the CPU reference"""
    import torch
    with torch.no_grad():
        C = R.emulator_mean_cov(st, R._t(X))[1].numpy() + chain.expdata_cov
    tstar = 1.0 / np.einsum("i,wi->w", u, np.linalg.solve(C, np.broadcast_to(u, (len(X), len(u)))[..., None])[..., 0])
    ts = np.sort(tstar)
    n = len(ts)
    i = 3 + int(np.argmax(ts[4:n - 3] - ts[3:n - 4]))          # gaps (ts[i], ts[i + 1]), 3 <= i <= n - 5
    t = 0.5 * (ts[i] + ts[i + 1])
    lam = np.linalg.eigvalsh(C - t * np.outer(u, u))[:, 0]
    margin = np.abs(lam) / np.abs(C).max(axis=(1, 2))
    notpd = tstar < t
    assert np.array_equal(lam < 0.0, notpd)
    return t, notpd, margin


@pytest.mark.parametrize("mode,M", [("pca", 8), ("pca", 74), ("no_pca", 54), ("expdiag", 54)])
def test_rows_not_positive_definite(tmp_path, mode, M):
    """k_like_w's `bad` flag and k_grad_finish's nanrow branch: the experiment's covariance is replaced by C_exp - t u u^T (u
    the first PCA row, normalised, or e_0) with t placed, from the CPU reference alone, between the rows' singular shifts, so
    that some of the 24 rows' blocks are positive definite and the others are not, all with |lambda_min| >= 1e-3 max|C_w|.
    PCA M 8 takes the value's NaN from the dense block kernels, PCA M 74 from the generic path with slab weights, NO_PCA and
    EXPDIAG M 54 their own forms.  Not-PD rows inside the box: lp and every gradient component NaN; a copy of such a row with
    one coordinate on the upper bound: -inf (-1e300 with finite=True) and a gradient of exactly 0.0; PD rows: within the bar
    of autograd on those rows, and bit-equal to the same rows in a batch of their own.  Chain reads last_not_pd only in
    mvn_loglike: log_posterior neither warns nor raises, as _log_prob_grad's docstring promises, and that is asserted.
    Catches: a `bad` flag read before the barrier or not reaching the weights of one mode, a NaN of one row leaking into its
    neighbours' weights (shared flag, overlapping slab), nanrow overriding the zero of a row outside the box, k_grad_finish
    missing rows, garbage instead of NaN from the square root of a negative pivot.
    Measured: not-PD rows 18, 18, 18, 16 of 24, margins 8.3e-3, 1.3e-2, 1.1e-2, 3.2e-2 (pca 8, pca 74, no_pca 54, expdiag 54);
    the PD rows' worst error over the bar 4.3e-4, 4.2e-4, 4.1e-4, 1.4e-5."""
    import warnings
    chain, emu, _ = _mode_emulator(str(tmp_path), 64, 4, M, 4, mode)
    st = R.state_from_emulator(emu)
    X = np.concatenate([emu._X_train[:8] + 1e-3, _rows(4, 41, 16)])
    assert np.all((X > chain.min) & (X < chain.max))
    if mode == "pca":
        u = emu._A[0] / np.linalg.norm(emu._A[0])
    else:
        u = np.zeros(M); u[0] = 1.0
    t, notpd, margin = _shift_between_rows(st, chain, X, u)
    _report("not-PD %s M %d: %d of %d rows not PD, margin %.3g" % (mode, M, notpd.sum(), len(X), margin.min()))
    assert 4 <= notpd.sum() <= len(X) - 4
    assert np.all(margin >= 1e-3), margin
    chain.expdata_cov = chain.expdata_cov - t * np.outer(u, u)
    xb = X[np.flatnonzero(notpd)[0]].copy()
    xb[2] = chain.max[2]                                      # on the boundary of the open box: outside
    Xall = np.concatenate([X, xb[None, :]])
    bad, pd = np.r_[notpd, False], np.r_[~notpd, False]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        lp, g = chain.log_posterior(Xall, return_grad=True)
        lpf, gf = chain.log_likelihood(Xall, finite=True, return_grad=True)
        plain = chain.log_posterior(Xall)
    assert not [w for w in caught if "definite" in str(w.message)]
    assert np.array_equal(lp, plain, equal_nan=True)
    assert np.all(np.isnan(lp[bad])) and np.all(np.isnan(g[bad]))
    assert np.all(np.isnan(lpf[bad])) and np.all(np.isnan(gf[bad]))
    assert lp[-1] == -np.inf and lpf[-1] == -1e300 and np.all(g[-1] == 0.0) and np.all(gf[-1] == 0.0)
    assert not np.any(np.signbit(g[-1]))
    assert np.array_equal(lpf[:-1], lp[:-1], equal_nan=True) and np.array_equal(gf[:-1], g[:-1], equal_nan=True)
    lp2, g2 = _checked("not-PD %s M %d, the PD rows" % (mode, M), chain, [st], Xall[pd])
    assert np.array_equal(lp2, lp[pd]) and np.array_equal(g2, g[pd])


# ------------------------------------------------------------------ 3. k_gp_grad's chunks, k_betaT's row tiles
def _corner_rows(X, Xd):
    X[0] = Xd[min(7, len(Xd) - 1)]                            # exactly on a design point
    X[1] = 0.0
    X[2] = 1.0                                                # the box corners
    X[3, ::2] = 0.0
    return X


def _predict_grad_case(name, eng, st, X, held):
    """rows `held` of dmean and dvar against autograd; every row bit-equal to predict_grad of that row alone, dmean to
    return_var=False"""
    dm, dv = eng.predict_grad(X)
    P, d = st["thetas"].shape[0], st["X"].shape[1]
    assert dm.shape == dv.shape == (len(X), P, d)
    jm = R.jacobian_rows(lambda x: R.gp_mean_var(st, x)[0], X[held])
    jv = R.jacobian_rows(lambda x: R.gp_mean_var(st, x)[1], X[held])
    rm, rv = _ratio(name + " dmean", dm[held], jm), _ratio(name + " dvar", dv[held], jv)
    assert rm <= 1.0 and rv <= 1.0, (rm, rv)
    assert np.array_equal(eng.predict_grad(X, return_var=False), dm)
    for w in range(len(X)):
        dm1, dv1 = eng.predict_grad(X[w:w + 1])
        assert np.array_equal(dm1[0], dm[w]) and np.array_equal(dv1[0], dv[w]), w


@pytest.mark.parametrize("kernel", ["RBF", "Matern15", "Matern25"])
def test_predict_grad_ragged_second_chunk(tmp_path, kernel):
    """case A: N 530, d 3, P 2 (Np 576).  k_gp_grad stages 512 + 18 design points: the last chunk is shorter than the 256
    threads of phase 1 and than the G = 85 groups of phase 2, and wa / wb keep the first chunk's entries 18 .. 511.  8 rows
    (one on a design point, the box corners), then 130 rows: Wld 256, k_betaT's second row tile (blockIdx.y = 1) feeds dvar of
    rows 128, 129; rows 0, 127, 128, 129 against autograd.
    Catches: a phase-2 bound of GG_CHUNK or G instead of n (stale weights of the previous chunk enter the sum), c0 missing
    from an index, the pad_front offset of alpha or beta^T, beta^T rows of the second tile stored with the wrong stride
    or not computed (tried once: k_betaT launched over its first row tile only puts dvar of the 130 rows at 1e7 of the bar).
    Measured, worst error over the bar, all three kernels, 8 and 130 rows: dmean <= 3.7e-6, dvar <= 2.2e-6."""
    _, emu, _ = _emulator(str(tmp_path), 530, 3, 4, 2, kernel)
    eng, st = emu._engine_ready(), R.state_from_emulator(emu)
    X = _corner_rows(_rows(3, 51, 8), emu._X_train)
    _predict_grad_case("predict_grad A %s N 530, 8 rows" % kernel, eng, st, X, list(range(8)))
    X = _corner_rows(_rows(3, 52, 130), emu._X_train)
    _predict_grad_case("predict_grad A %s N 530, 130 rows" % kernel, eng, st, X, [0, 127, 128, 129])


def test_predict_grad_three_chunks(tmp_path):
    """case B: N 1100, d 7, P 2, Matern-5/2: chunks 512 + 512 + 76, G = 36 (252 of the 256 threads active in phase 2).
    Catches: the accumulators sa / sb reset per chunk, a chunk offset that is right only for c0 in {0, 512}, the four idle
    threads' partials entering the final sum.
    Measured, worst error over the bar: dmean 4.3e-6, dvar 2.2e-6."""
    _, emu, _ = _emulator(str(tmp_path), 1100, 7, 4, 2, "Matern25")
    X = _corner_rows(_rows(7, 53, 8), emu._X_train)
    _predict_grad_case("predict_grad B Matern25 N 1100", emu._engine_ready(), R.state_from_emulator(emu), X, list(range(8)))


def _bare_engine(N, d, P, kernel, seed):
    """GPs straight on a GPEngine (an Emulator cannot be trained on one event: its scaler and PCA divide by N - 1), and the
    reference's state for them, factored by the oracle"""
    from gpbayestools_hic_amd import synth
    from gpbayestools_hic_amd.engine import GPEngine
    rng = np.random.default_rng(seed)
    X, Z = rng.uniform(0.0, 1.0, (N, d)), rng.standard_normal((P, N))
    th = synth.fixed_theta(d, P, ell=0.6)
    eng = GPEngine(0)
    eng.set_data(X, Z, kernel, 0.1)
    eng.set_theta(th)
    eng.factor()
    kind = O.KIND_NAMES[kernel]
    fac = [O.gp_factor(X, Z[p], th[p], kind, 0.1) for p in range(P)]
    st = dict(X=R._t(X), thetas=R._t(th), L=[R._t(L) for L, _ in fac], a=[R._t(a) for _, a in fac], kind=kind)
    return eng, st, X


@pytest.mark.parametrize("N,kernel", [(1, "RBF"), (2, "Matern15")])
def test_predict_grad_one_and_two_design_points(N, kernel):
    """cases C and D: d 1, P 1, N 1 (RBF) and N 2 (Matern-3/2): G = 256 groups for one or two design points, Np 64 with 63 or
    62 padded rows in front of the design.
    Catches: padded design rows or padded alpha / beta^T entries entering the sum, G or j computed wrongly at d = 1, a
    reduction over the 256 partials that assumes G d < 256.
    Measured, worst error over the bar: N 1 dmean 5.6e-8, dvar 2.2e-7; N 2 dmean 2.2e-7, dvar 6.4e-7."""
    eng, st, Xd = _bare_engine(N, 1, 1, kernel, 60 + N)
    X = _rows(1, 54, 8)
    X[0], X[1], X[2] = Xd[N - 1], 0.0, 1.0
    _predict_grad_case("predict_grad %s N %d d 1" % (kernel, N), eng, st, X, list(range(8)))
    eng.close()


# ------------------------------------------------------------------ 4. stochastic kriging
def _sk_errors(Y):
    return np.abs(Y) * np.random.default_rng(300).uniform(0.005, 0.08, size=Y.shape)


@pytest.mark.parametrize("mode", ["pca", "no_pca"])
def test_stochastic_kriging_gradients(tmp_path, mode):
    """Emulator(simulation_error=True): 96 events, d 3, 6 observables, statistical errors of 0.5 - 8 % on the GPs' training
    diagonals.  The reference factors GP p with emu.alpha + point_noise_[p] (grad_reference.state_from_emulator).
    predict_grad and the chain's gradient at the bar; both move by more than 1e-6 relative against the same emulator without
    simulation_error, so the noise is known to reach alpha, L^-1 and with them the gradient.
    Catches: a gradient path that refactors or reads alpha / L^-1 without the per-point noise.
    Measured, worst error over the bar: pca dmean 2.6e-6, dvar 7.5e-7, chain 1.1e-4; no_pca 2.7e-6, 7.6e-7, 5.2e-5."""
    kw = dict(yerr=_sk_errors, seed=3)
    chain, emu, xstar = _mode_emulator(str(tmp_path / "sk"), 96, 3, 6, 3, mode, simulation_error=True, **kw)
    pchain, plain, _ = _mode_emulator(str(tmp_path / "plain"), 96, 3, 6, 3, mode, **kw)
    assert emu.nev == 96 and plain.point_noise_ is None
    assert emu.point_noise_.shape == (emu._ngp, 96) and emu.point_noise_.max() / emu.point_noise_.min() > 10.0
    eng, st = emu._engine_ready(), R.state_from_emulator(emu)
    X = _corner_rows(_rows(3, 55, 8), emu._X_train)
    name = "stochastic kriging %s" % mode
    _predict_grad_case(name, eng, st, X, list(range(8)))
    Xc = _near(xstar, 24, 56)
    lp, g = _checked(name + " chain", chain, [st], Xc)
    dm, dv = eng.predict_grad(X)
    dmp, dvp = plain._engine_ready().predict_grad(X)
    assert _rowerr(dmp, dm).min() > 1e-6 and _rowerr(dvp, dv).min() > 1e-6
    pchain.expdata, pchain.expdata_cov = chain.expdata, chain.expdata_cov       # the same experiment for both
    _, gp = pchain.log_posterior(Xc, return_grad=True)
    assert _rowerr(gp, g).min() > 1e-6


# ------------------------------------------------------------------ 5. one chain, four transform modes
FOUR = [("pca", 64, 8, 4, "RBF"), ("no_pca", 80, 54, 4, "Matern25"), ("expdiag", 96, 10, 3, "RBF"),
        ("no_pca_expdiag", 72, 6, 4, "Matern15")]


def _four_mode_chain(tmp, d, mapped_first):
    """the four emulators, each with a chain of its own, and one Chain over all four; the experiment's covariance is block-
    diagonal with correlated observables inside every block (correlation 0.2)"""
    from gpbayestools_hic_amd import synth
    from gpbayestools_hic_amd.mcmc import Chain
    singles = []
    for i, (mode, N, M, P, kernel) in enumerate(FOUR):
        c, e, xstar = _mode_emulator(os.path.join(tmp, "e%d" % i), N, d, M, P, mode, kernel=kernel, seed=10 * (i + 1),
                                     mapped=mapped_first and i == 0)
        err = np.sqrt(np.diag(c.expdata_cov))
        c.expdata_cov = np.outer(err, err) * (0.8 * np.eye(M) + 0.2)
        singles.append((c, e))
    yexp = np.concatenate([c.expdata[0] for c, _ in singles])
    nobs = len(yexp)
    cov = np.zeros((nobs, nobs))
    i0 = 0
    for c, e in singles:
        cov[i0:i0 + e.nobs, i0:i0 + e.nobs] = c.expdata_cov
        i0 += e.nobs
    pf, ep = os.path.join(tmp, "par.txt"), os.path.join(tmp, "exp.pkl")
    synth.write_parameter_file(pf, np.zeros(d), np.ones(d))
    synth.write_experiment_pickle(ep, yexp, np.sqrt(np.diag(cov)))
    chain = Chain(mcmc_path=os.path.join(tmp, "mcmc", "chain.pkl"), expdata_path=ep, model_parafile=pf, device=0)
    assert np.array_equal(chain.expdata[0], yexp)
    chain.expdata_cov = cov
    chain.emuList = [e for _, e in singles]
    return chain, singles, xstar


def _sum_of_singles(singles, X):
    lp, g = 0.0, 0.0
    for c, _ in singles:                                      # emuList order, as k_grad_fold accumulates
        l1, g1 = c.log_likelihood(X, return_grad=True)
        lp, g = lp + (l1 - O.EXTRA_STD_CONST), g + g1
    return lp + O.EXTRA_STD_CONST, g


def test_chain_of_four_modes(tmp_path):
    """one Chain over PCA (M 8, P 4), NO_PCA (M 54: slab weights), EXPDIAG (M 10, P 3) and NO_PCA_EXPDIAG (M 6) emulators, d
    6, N 64 - 96, three kernel kinds: k_grad_fold(accumulate = 1) adds blocks of other modes and other P onto the first, one
    call carries LDS and slab blocks.  32 rows near the truth point, two outside the box; against autograd over the four
    states, and against the sum of the four single-emulator chains' gradients (1e-12 relative to max(|g|_inf, 1): the same
    terms, added in the same order).
    Catches: a fold that overwrites instead of adding (or adds onto an uninitialised first block), weights or workspaces of
    one context used for the next, the LDS / slab decision taken once per chain instead of per emulator (tried once: a fold
    that does not accumulate fails both comparisons).
    Measured, worst error over the bar: 3.1e-5."""
    chain, singles, xstar = _four_mode_chain(str(tmp_path), 6, False)
    X = _near(xstar, 32, 57, radius=0.03)
    X[5, 1] = 1.1
    X[17, 4] = 0.0
    lp, g = _checked("four modes in one chain", chain, [R.state_from_emulator(e) for _, e in singles], X)
    inside = np.all((X > chain.min) & (X < chain.max), axis=1)
    assert inside.sum() == 30
    lps, gs = _sum_of_singles(singles, X[inside])
    assert np.all(_rowerr(g[inside], gs) <= 1e-12), _rowerr(g[inside], gs)
    assert np.all(np.abs(lp[inside] - lps) <= 1e-12 * np.abs(lps))


def test_chain_of_four_modes_first_mapped(tmp_path):
    """the same four modes over d = 20 with the first emulator parameterTrafoPCA-mapped: the map's Jacobian J is present on
    the first block of the accumulation and absent on the next three.  Against central differences of the log-posterior with
    the step (1e-6) and the bar (1e-5 relative to max(|g|_inf, 1)) of test_log_posterior_grad_nine_mapped_emulators, whose
    docstring derives them; and against the sum of the single-emulator chains at 1e-12.
    Catches: J of one emulator applied to the blocks that have none, nd and d exchanged in the fold.
    Measured: 1.4e-4 of the 1e-5 bar."""
    chain, singles, xstar = _four_mode_chain(str(tmp_path), 20, True)
    X = _near(xstar, 4, 58, radius=0.02)
    lp, g = chain.log_posterior(X, return_grad=True)
    assert np.array_equal(lp, chain.log_posterior(X))
    h = 1e-6
    fd = np.empty_like(g)
    for q in range(20):
        e = np.zeros(20); e[q] = h
        fd[:, q] = (chain.log_posterior(X + e) - chain.log_posterior(X - e)) / (2 * h)
    r = _rowerr(g, fd)
    _report("%-58s %.3g of the bar (1e-5, central differences)" % ("four modes, first mapped", r.max() / 1e-5))
    assert np.all(r <= 1e-5), r
    _, gs = _sum_of_singles(singles, X)
    assert np.all(_rowerr(g, gs) <= 1e-12), _rowerr(g, gs)


# ------------------------------------------------------------------ 6. empty and single batches
def test_empty_and_single_batches(tmp_path):
    """W = 0 through the three gradient entry points: shapes (0,), (0, d), (0, P, d), (0, nobs, d), no device call refused, and
    the next ordinary batch unaffected; one row alone equals that row of a batch."""
    chain, emu, _ = _emulator(str(tmp_path), 96, 5, 4, 3)
    eng = emu._engine_ready()
    X = _rows(5, 59, 7)
    lp, g = chain.log_posterior(X, return_grad=True)
    dm, dv = eng.predict_grad(X)
    J = emu.predict_jacobian(X)
    E = np.zeros((0, 5))
    lp0, g0 = chain.log_posterior(E, return_grad=True)
    assert lp0.shape == (0,) and g0.shape == (0, 5)
    lp0, g0 = chain.log_likelihood(E, finite=True, return_grad=True)
    assert lp0.shape == (0,) and g0.shape == (0, 5)
    dm0, dv0 = eng.predict_grad(E)
    assert dm0.shape == dv0.shape == (0, 3, 5) and eng.predict_grad(E, return_var=False).shape == (0, 3, 5)
    assert emu.predict_jacobian(E).shape == (0, 4, 5)
    lp1, g1 = chain.log_posterior(X[3:4], return_grad=True)
    assert lp1.shape == (1,) and g1.shape == (1, 5) and np.array_equal(lp1, lp[3:4]) and np.array_equal(g1, g[3:4])
    dm1, dv1 = eng.predict_grad(X[3:4])
    assert np.array_equal(dm1, dm[3:4]) and np.array_equal(dv1, dv[3:4])
    assert np.array_equal(emu.predict_jacobian(X[3:4]), J[3:4])
