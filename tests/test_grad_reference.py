"""CPU tier of the gradient work: the torch restatement in tests/grad_reference.py reproduces the oracle's log-posterior, and its
autograd gradient agrees with central differences of that log-posterior — so that the GPU tier can hold the device gradient
against it."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import grad_reference as R  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402

N, D, M, P = 48, 4, 6, 3
KINDS = [O.KIND_RBF, O.KIND_MATERN15, O.KIND_MATERN25]
MODES = [O.MODE_PCA, O.MODE_NO_PCA, O.MODE_EXPDIAG, O.MODE_NO_PCA_EXPDIAG]


def _case(kind, mode, seed=0):
    rng = np.random.default_rng(100 + 10 * kind + mode + seed)
    X = rng.uniform(0.0, 1.0, (N, D))
    W1, W2 = rng.standard_normal((D, M)), rng.standard_normal((D, M))
    Y = 2.0 + np.sin(X @ W1) + 0.5 * np.cos(X @ W2) + 0.01 * rng.standard_normal((N, M))
    emu = O.OracleEmulator(X, Y, np.zeros(D), np.ones(D), P, kind=kind, mode=mode)
    npc = emu.npc
    theta = np.tile(np.concatenate([[0.0], np.log(np.full(D, 0.6)), [np.log(0.05)]]), (npc, 1))
    emu.fit(theta)
    xstar = np.full(D, 0.45)
    yexp = emu.predict(xstar[None, :], return_cov=False)[0]
    cexp = np.diag((0.05 * np.abs(yexp)) ** 2)
    Xw = rng.uniform(0.2, 0.8, (6, D))
    return emu, yexp, cexp, Xw


def _oracle_lp(emu, X, yexp, cexp):
    return O.log_prob(X, np.zeros(D), np.ones(D), lambda x, e: emu.predict(x, True, e), yexp, cexp)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_matches_oracle_value(kind, mode):
    emu, yexp, cexp, Xw = _case(kind, mode)
    Xw[0] = emu.X[5]                                          # a query row on a training point
    ref = _oracle_lp(emu, Xw, yexp, cexp)
    st = R.state_from_oracle(emu)
    got = R.log_posterior([st], R._t(Xw), np.zeros(D), np.ones(D), yexp, cexp).numpy()
    assert np.all(np.isfinite(ref))
    assert np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)) < 1e-12


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_gradient_matches_central_differences(kind, mode):
    emu, yexp, cexp, Xw = _case(kind, mode)
    st = R.state_from_oracle(emu)
    _, g = R.value_and_grad(lambda x: R.log_posterior([st], x, np.zeros(D), np.ones(D), yexp, cexp), Xw)
    h = 1e-5
    fd = np.empty_like(g)
    for j in range(D):
        e = np.zeros(D); e[j] = h
        fd[:, j] = (_oracle_lp(emu, Xw + e, yexp, cexp) - _oracle_lp(emu, Xw - e, yexp, cexp)) / (2 * h)
    scale = np.maximum(np.abs(g).max(1), 1.0)
    assert np.all(np.abs(g - fd).max(1) / scale < 1e-6), np.abs(g - fd).max(1) / scale


def test_outside_rows_have_zero_gradient_and_two_emulators_add():
    e1, y1, c1, Xw = _case(O.KIND_RBF, O.MODE_PCA)
    e2, y2, c2, _ = _case(O.KIND_MATERN25, O.MODE_EXPDIAG, seed=1)
    yexp = np.concatenate([y1, y2])
    cexp = np.zeros((2 * M, 2 * M)); cexp[:M, :M] = c1; cexp[M:, M:] = c2
    Xw[1, 2] = 1.3
    sts = [R.state_from_oracle(e1), R.state_from_oracle(e2)]
    v, g = R.value_and_grad(lambda x: R.log_posterior(sts, x, np.zeros(D), np.ones(D), yexp, cexp, outside=-1e300), Xw)
    assert v[1] == -1e300 and np.all(g[1] == 0.0)
    ref = O.log_prob(Xw, np.zeros(D), np.ones(D), lambda x, e: O.chain_predict([e1, e2], x, e), yexp, cexp, finite=True,
                     posterior=False)
    ok = np.arange(6) != 1
    assert np.max(np.abs(v[ok] - ref[ok]) / np.abs(ref[ok])) < 1e-12


@pytest.mark.parametrize("mode", [O.MODE_PCA, O.MODE_NO_PCA])
def test_vector_alpha_state_matches_oracle_and_central_differences(mode):
    """stochastic kriging: every GP factored with its own vector alpha + s_p on the training diagonal.  state_from_emulator
    reads the vector from point_noise_ (here off a stand-in carrying the attributes it reads of an Emulator); the value agrees
    with the oracle's own vector-alpha emulator at 1e-12, autograd with central differences of the oracle at 1e-6, and the
    noise reaches the factors (the scalar-alpha state gives another value)."""
    import types
    emu, yexp, cexp, Xw = _case(O.KIND_RBF, mode)
    rng = np.random.default_rng(7)
    s = rng.uniform(0.002, 0.2, (emu.npc, N))                 # a factor 100 across the points, another row per GP
    emu.L, emu.a = [], []
    for p in range(emu.npc):
        L, a = O.gp_factor(emu.X, np.ascontiguousarray(emu.Z[:, p]), emu.thetas[p], emu.kind, emu.alpha_reg + s[p])
        emu.L.append(L); emu.a.append(a)
    no_pca = mode == O.MODE_NO_PCA
    ns = types.SimpleNamespace
    stand_in = ns(_X_train=emu.X, _Z_train=np.ascontiguousarray(emu.Z.T), kernel_type_="RBF", thetas_=emu.thetas,
                  alpha=emu.alpha_reg, point_noise_=s, perform_no_PCA_=no_pca, _mode=mode, _A=emu.A, _cov_trunc=emu.cov_trunc,
                  scaler=ns(mean_=emu.mu, scale_=emu.scale))
    st = R.state_from_emulator(stand_in)
    lo, hi = np.zeros(D), np.ones(D)
    ref = _oracle_lp(emu, Xw, yexp, cexp)
    got, g = R.value_and_grad(lambda x: R.log_posterior([st], x, lo, hi, yexp, cexp), Xw)
    assert np.all(np.isfinite(ref))
    assert np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)) < 1e-12
    stand_in.point_noise_ = None
    plain = R.log_posterior([R.state_from_emulator(stand_in)], R._t(Xw), lo, hi, yexp, cexp).numpy()
    assert np.min(np.abs(plain - ref) / np.maximum(np.abs(ref), 1.0)) > 1e-6
    h = 1e-5
    fd = np.empty_like(g)
    for j in range(D):
        e = np.zeros(D); e[j] = h
        fd[:, j] = (_oracle_lp(emu, Xw + e, yexp, cexp) - _oracle_lp(emu, Xw - e, yexp, cexp)) / (2 * h)
    scale = np.maximum(np.abs(g).max(1), 1.0)
    assert np.all(np.abs(g - fd).max(1) / scale < 1e-6), np.abs(g - fd).max(1) / scale
