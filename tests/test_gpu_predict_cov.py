"""
GPU tier: the joint predictive covariance gpb_gp_predict_cov (csrc/gpb_cov.hip: k_vmat, k_kss, k_cov_update, k_cov_pack — what
Emulator.sample_y, FittedGP.predict(return_cov=True) and FittedGP.sample_y draw from; sk:_gpr.py:441-469) at the shapes of
tests/cov_reference.py: one, two and three 128-wide tiles a side, padded batch columns (the covariance is computed at
Wc = round_up(W, 128) and packed to W), a half-empty last 128-row block of V and its clipped K range, all three kernels, query
rows that are design points and a repeated query row.
  * against the independent oracle (gp_oracle.gp_predict_cov) at the package's fp64 bars: covariance 1e-10, mean 1e-11;
  * against the long-double evaluation of Kss - V^T V from the device's OWN L^-1 and K* (get("Linv"), get("Kstar", W) right after
    the call: the accessor describes the predict_cov batch, which always leaves the cross kernel as fp64 values), elementwise
    inside the forward rounding bound B of cov_reference.joint_cov_bound;
  * structure (symmetry, the diagonal against predict's variance, the noise on the diagonal only, an isolated row), batch
    independence bit for bit, the on_device branch of the C entry point, the limits, and FittedGP.predict(return_cov=True).
"""
import numpy as np
import pytest

import cov_reference as R
from conftest import golden, maxrel

pytestmark = pytest.mark.gpu

ISOLATED_SHAPE = (200, 20, "Matern25", 128)        # the shape that also takes an isolated query row (W = 129 with it)
SPLIT_SHAPE = (448, 5, "RBF", 257)                 # the shape of the batch-independence and on_device tests


class Case:
    """one shape: the engine (factored), the batch, the device's results and operands, the references — computed once"""

    def __init__(self, shape):
        from gpbayestools_hic_amd import GPEngine
        from oracle import gp_oracle as O
        self.shape = shape
        self.N, self.d, self.kernel, self.W = shape
        self.kind = O.KIND_NAMES[self.kernel]
        self.X, self.Z, self.theta, self.Xs = R.problem(self.N, self.d, self.W)
        self.eng = eng = GPEngine(0)
        eng.set_data(self.X, self.Z, self.kernel, alpha=R.ALPHA)
        eng.set_theta(self.theta)
        eng.factor()
        self.mean, cov = eng.predict_cov(self.Xs)
        self.Kstar = eng.get("Kstar", self.W)       # K(X*, X) of THIS batch, fp64 (the covariance path takes no digit planes)
        self.cov = np.array(cov)
        self.Linv = eng.get("Linv")
        self.prior = np.array([O.prior_var(th, self.d) for th in self.theta])
        self.noise = np.exp(self.theta[:, -1])
        self.ref, self.B, self.oracle = [], [], []
        for p in range(R.P):
            self.ref.append(R.joint_cov_ld(self.Linv[p], self.Kstar[p], self.Xs, self.theta[p], self.kind))
            self.B.append(R.joint_cov_bound(self.Linv[p], self.Kstar[p], self.Xs, self.theta[p], self.kind))
            L, a = O.gp_factor(self.X, self.Z[p], self.theta[p], self.kind, R.ALPHA)
            self.oracle.append(O.gp_predict_cov(self.Xs, self.X, self.theta[p], L, a, self.kind))


_CASES = {}


def _case(shape):
    """the module's one Case (and engine) per shape, built on first use"""
    if shape not in _CASES:
        _CASES[shape] = Case(shape)
    return _CASES[shape]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for c in _CASES.values():
        c.eng.close()
    _CASES.clear()


@pytest.fixture(params=R.SHAPES, ids=lambda s: "N%d-d%d-%s-W%d" % s)
def case(request):
    return _case(request.param)


@pytest.fixture
def split_case():
    return _case(SPLIT_SHAPE)


def test_against_the_oracle(case):
    from oracle import gp_oracle as O
    assert case.mean.shape == (case.W, R.P) and case.cov.shape == (R.P, case.W, case.W)
    for p in range(R.P):
        mo, co = case.oracle[p]
        assert maxrel(case.cov[p], co) < 1e-10
        assert maxrel(case.mean[:, p], mo) < 1e-11
        # the accessor does describe this batch: K(X*, X) in fp64, at the bar test_gpu_sliced.py reads it back with
        c = float(np.exp(case.theta[p, 0]))
        assert np.max(np.abs(case.Kstar[p] - O.kernel_cross(case.Xs, case.X, case.theta[p], case.kind))) < 1e-13 * max(1.0, c)


def test_inside_the_rounding_bound_of_the_long_double_evaluation(case):
    """|cov - ref| <= B elementwise, ref and B from the device's own L^-1 and K*.  Largest |cov - ref| / B measured on an MI355X
    (product and debug library alike), over both GPs:
        N = 130, d = 3, RBF, W = 1:           9.1e-4
        N = 320, d = 6, Matern-3/2, W = 129:  2.5e-3
        N = 200, d = 20, Matern-5/2, W = 128: 2.7e-3
        N = 448, d = 5, RBF, W = 257:         2.4e-3
    (numpy's own fp64 evaluation of the formula: 0.9e-3 to 2.8e-3 of B, tests/test_cov_reference.py) — B is a worst-case bound
    over Np terms, the device's errors are those of a sum whose roundings mostly cancel."""
    worst = 0.0
    for p in range(R.P):
        err = np.abs(case.cov[p] - case.ref[p]).astype(float)
        worst = max(worst, float(np.max(err / case.B[p])))
    print("RATIO N%d-d%d-%s-W%d max |cov - ref| / B = %.4g" % (case.shape + (worst,)))
    for p in range(R.P):
        err = np.abs(case.cov[p] - case.ref[p]).astype(float)
        assert np.max(case.B[p]) <= 1e-11 * case.prior[p]
        assert np.all(err <= case.B[p]), (p, float(np.max(err / case.B[p])), np.unravel_index(np.argmax(err / case.B[p]), err.shape))


def test_structure(case):
    eng, W = case.eng, case.W
    before = eng.predict_sliced
    eng.tune("predict_sliced", 0)
    try:
        _, var = eng.predict(case.Xs)                                   # the fp64 predict kernel's own sum of squares
    finally:
        eng.tune("predict_sliced", before)
    for p in range(R.P):
        cov, B = case.cov[p], case.B[p]
        asym = float(np.max(np.abs(cov - cov.T)))
        print("ASYM N%d-d%d-%s-W%d gp %d: max |cov - cov^T| = %.3g" % (case.shape + (p, asym)))
        assert asym <= 1e-15 * case.prior[p]
        # bit-equal on the device: V_i . V_j and V_j . V_i are the same products added in the same order (k ascending), and the
        # scaled differences of k_kss change sign exactly
        assert np.array_equal(cov, cov.T)
        assert np.all(np.abs(np.diag(cov) - var[:, p]) <= 2 * np.diag(B))
        assert np.all(np.diag(cov) > 0) and np.all(np.diag(cov) <= case.prior[p])
        if W >= 2:                                                      # rows W - 2 and W - 1 are the same point
            i, j = W - 2, W - 1
            assert abs((cov[i, i] - cov[i, j]) - case.noise[p]) <= B[i, i] + B[i, j]
            assert abs((cov[j, j] - cov[j, i]) - case.noise[p]) <= B[j, j] + B[j, i]
            assert np.array_equal(cov[i, :i], cov[j, :i])               # ... and see every other row alike


def test_an_isolated_query_row_keeps_the_prior_and_no_covariance():
    """x = 1e3 in every coordinate: K* underflows to exactly 0 for all three kernels, so V's column is 0, the row's variance is
    the prior c + sigma_n^2 and its covariance with every other row exactly 0.  Appended to the W = 128 batch it is the only
    live row of a second tile row and column; the 128 rows in front of it keep their bits."""
    c = _case(ISOLATED_SHAPE)
    W = c.W
    Xs = np.vstack([c.Xs, np.full((1, c.d), 1e3)])
    mean, cov = c.eng.predict_cov(Xs)
    Ks = c.eng.get("Kstar", W + 1)
    cov = np.array(cov)
    assert np.all(Ks[:, W, :] == 0.0)
    for p in range(R.P):
        assert abs(cov[p, W, W] - c.prior[p]) <= 2 * np.spacing(c.prior[p])
        assert np.all(cov[p, W, :W] == 0.0) and np.all(cov[p, :W, W] == 0.0)
        assert mean[W, p] == 0.0
    assert np.array_equal(cov[:, :W, :W], c.cov) and np.array_equal(mean[:W], c.mean)


@pytest.mark.parametrize("k", [1, 128, 129])
def test_a_rows_numbers_do_not_depend_on_the_batch(split_case, k):
    c = split_case
    mean, cov = c.eng.predict_cov(c.Xs[:k])
    assert np.array_equal(np.asarray(cov), c.cov[:, :k, :k]) and np.array_equal(mean, c.mean[:k])


def test_the_result_survives_an_intervening_predict_of_another_size(split_case):
    """predict reuses the K*^T workspace with another leading dimension (the padded batch: 768 here, 384 for the covariance)"""
    c = split_case
    rng = np.random.default_rng(7)
    c.eng.predict(rng.random((700, c.d)))
    mean, cov = c.eng.predict_cov(c.Xs)
    assert np.array_equal(np.asarray(cov), c.cov) and np.array_equal(mean, c.mean)
    c.eng.predict(rng.random((3, c.d)))
    mean, cov = c.eng.predict_cov(c.Xs[:129])
    assert np.array_equal(np.asarray(cov), c.cov[:, :129, :129]) and np.array_equal(mean, c.mean[:129])


def test_the_on_device_branch_gives_the_host_paths_bits(split_case):
    """gpb_gp_predict_cov(on_device = 1): input and both outputs are device pointers, nothing is staged or copied back"""
    import torch
    from gpbayestools_hic_amd import _native as nat
    c, eng = split_case, split_case.eng
    for W in (c.W, 129, 1):
        Xs = torch.as_tensor(np.ascontiguousarray(c.Xs[:W]), device="cuda")
        mean = torch.full((W, R.P), float("nan"), dtype=torch.float64, device="cuda")
        cov = torch.full((R.P, W, W), float("nan"), dtype=torch.float64, device="cuda")
        eng._track_stream()
        eng._ck(eng.lib.gpb_gp_predict_cov(eng.h, nat.ptr(Xs), W, 1, nat.ptr(mean), nat.ptr(cov)))
        assert np.array_equal(cov.cpu().numpy(), c.cov[:, :W, :W]) and np.array_equal(mean.cpu().numpy(), c.mean[:W])


def test_limits(split_case):
    """W > 8192 is refused by the entry point before anything is staged, launched or allocated for it (the call is handed
    one-row buffers: it must not touch them); the Python wrapper refuses before it allocates the result; W = 0 is empty"""
    from gpbayestools_hic_amd import _native as nat
    c, eng = split_case, split_case.eng
    one, m1, c1 = np.zeros((1, c.d)), np.full((1, R.P), 7.0), np.full((R.P, 1, 1), 7.0)
    too_many = eng.PREDICT_COV_MAX_W + 1
    assert too_many == 8193
    rc = eng.lib.gpb_gp_predict_cov(eng.h, nat.ptr(one), too_many, 0, nat.ptr(m1), nat.ptr(c1))
    assert rc < 0 and b"8192" in eng.lib.gpb_last_error(eng.h)
    assert np.all(m1 == 7.0) and np.all(c1 == 7.0)
    with pytest.raises(nat.GPBError, match="8192"):
        eng.predict_cov(np.zeros((too_many, c.d)))
    mean, cov = eng.predict_cov(np.zeros((0, c.d)))
    assert mean.shape == (0, R.P) and cov.shape == (R.P, 0, 0)
    mean, cov = eng.predict_cov(c.Xs[:1])                                 # the context is as it was
    assert np.array_equal(np.asarray(cov), c.cov[:, :1, :1]) and np.array_equal(mean, c.mean[:1])


def test_fitted_gp_predict_return_cov(tmp_path):
    """FittedGP.predict(X, return_cov=True) on a trained emulator (the Matern golden's design and hyper-parameters), W = 5"""
    from gpbayestools_hic_amd import Emulator, synth
    from oracle import gp_oracle as O
    g = golden("g3_emulator_pca_matern.npz")
    tp, pf = str(tmp_path / "train.pkl"), str(tmp_path / "par.txt")
    synth.write_training_pickle(tp, g["X"], g["Y"], g["Yerr"])
    synth.write_parameter_file(pf, g["lo"], g["hi"])
    emu = Emulator(training_set_path=tp, parameter_file=pf, npc=int(g["npc"]))
    emu.trainEmulator([True] * emu.nev, kernel_type="Matern", thetas=g["thetas"])
    Xq = np.ascontiguousarray(g["Xs"][:5])
    Xq[4] = Xq[3]
    for i, gp in enumerate(emu.gps):
        mean, cov = gp.predict(Xq, return_cov=True)
        L, a = O.gp_factor(gp.X_train_, gp.y_train_, gp.kernel_theta, O.KIND_MATERN15, emu.alpha)
        mo, co = O.gp_predict_cov(Xq, gp.X_train_, gp.kernel_theta, L, a, O.KIND_MATERN15)
        assert mean.shape == (5,) and cov.shape == (5, 5)
        assert maxrel(cov, co) < 1e-10 and maxrel(mean, mo) < 1e-11
        assert np.array_equal(cov, cov.T)
        noise = np.exp(gp.kernel_theta[-1])
        assert abs((cov[3, 3] - cov[3, 4]) - noise) < 1e-10 * (np.exp(gp.kernel_theta[0]) + noise)   # rows 3 and 4: one point
