"""CPU tier of the PTLMC sampler: the restatement of tests/ptlmc_reference.py against the reference's own runs
(tests/golden/g12_ptlmc.npz, tools/make_ptlmc_goldens.py), Chain.tempexchange against the reference's recorded orders, and the
restated Philox / Box-Muller draws against known counters."""
import numpy as np
import pytest

import ptlmc_reference as R
from conftest import golden


def _ladder(g):
    from gpbayestools_hic_amd.ptlmc import ladder
    return ladder(int(g["numtemps"]), int(g["numchain"]), float(g["maxtemp"]))


@pytest.mark.parametrize("branch", ["plain", "grad"])
def test_restatement_reproduces_reference_samples(branch):
    """fed the reference's draws from its start state, the restated step loop saves the reference's samples — to 1e-12: the
    reference forms rvalo @ hc and dfval @ covmat0 with BLAS, the restatement (as the device) sums in index order, and the two
    differ in the last bit (4.4e-16 at most over these 36 steps); every accept and exchange decision is the same"""
    from gpbayestools_hic_amd.ptlmc import proposal_factor, TARACC_GRAD, TARACC_PLAIN
    g = golden("g12_ptlmc.npz")
    p = branch + "_"
    gradient = branch == "grad"
    temps = _ladder(g)
    start = g[p + "start"]
    covmat0, hc = proposal_factor(start)
    steps = [dict(normals=n, logu_accept=np.log(ua), picks=pk, logu_swap=np.log(us))
             for n, ua, pk, us in zip(g[p + "normals"], g[p + "u_accept"], g[p + "picks"], g[p + "u_swap"])]
    spc = int(g["sampperchain"])
    save = R.replay(start, steps, R.gaussian_target(g[p + "mean"], g[p + "prec"], gradient), temps, hc, covmat0,
                    int(g["numtemps"]), 2 * spc, spc, TARACC_GRAD if gradient else TARACC_PLAIN, gradient)
    ref = g[p + "theta"]
    assert save.shape == ref.shape
    assert np.max(np.abs(save - ref)) <= 1e-12 * np.max(np.abs(ref)), np.max(np.abs(save - ref))
    assert len(np.unique(ref[:, :, 0])) > 4                     # the chains moved


def test_tempexchange_reproduces_reference_orders():
    from gpbayestools_hic_amd.mcmc import Chain
    g = golden("g12_ptlmc.npz")
    ch = Chain.__new__(Chain)
    state = np.random.get_state()
    try:
        for i in range(3):
            np.random.seed(int(g["tx%d_seed" % i]))
            got = ch.tempexchange(g["tx%d_lpostf" % i], g["tx%d_temps" % i], iters=int(g["tx%d_iters" % i]))
            assert np.array_equal(got, g["tx%d_order" % i]), i
    finally:
        np.random.set_state(state)


def test_exchange_rule_matches_tempexchange():
    """the restatement's exchange (the device's rule) with the picks and uniforms tempexchange draws gives its order"""
    from gpbayestools_hic_amd.mcmc import Chain
    g = golden("g12_ptlmc.npz")
    ch = Chain.__new__(Chain)
    state = np.random.get_state()
    try:
        lp, temps, iters = g["tx1_lpostf"][:, 0], g["tx1_temps"][:, 0], int(g["tx1_iters"])
        T = len(lp)
        np.random.seed(int(g["tx1_seed"]))
        picks, lus = [], []
        for _ in range(iters):
            rtv = np.random.choice(range(1, T), T)
            for rt in rtv:
                picks.append(rt)
                lus.append(np.log(np.random.uniform(size=1))[0])
        assert np.array_equal(R.exchange_order(lp, temps, picks, lus), g["tx1_order"])
        np.random.seed(int(g["tx1_seed"]))
        assert np.array_equal(ch.tempexchange(g["tx1_lpostf"], g["tx1_temps"], iters=iters), g["tx1_order"])
    finally:
        np.random.set_state(state)


def test_device_draws_layout():
    """the restated draws on known counters: pair j of rung c from philox(seed, c, k, j, 2) by Box-Muller, the accept draw
    from philox(seed, c, k, 0, 3), pick i from philox(seed, i, k, 0, 4); the stream depends on (seed, k) only"""
    from oracle.stretch_oracle import philox4x32_10, u01
    seed, k, T, d = 0x123456789ABCDEF, 17, 7, 5
    dr = R.device_draws(seed, k, T, d)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    x, y, z, w = (int(v) for v in philox4x32_10(key, (3, k, 1, 2)))
    u1, u2 = u01(x, y), u01(z, w)
    r = np.sqrt(-2.0 * np.log(1.0 - u1))
    assert dr["normals"][3, 2] == r * np.cos((2.0 * np.pi) * u2)
    assert dr["normals"][3, 3] == r * np.sin((2.0 * np.pi) * u2)
    x, y, z, w = (int(v) for v in philox4x32_10(key, (6, k, 2, 2)))
    assert dr["normals"][6, 4] == np.sqrt(-2.0 * np.log(1.0 - u01(x, y))) * np.cos((2.0 * np.pi) * u01(z, w))
    x, y, _, _ = (int(v) for v in philox4x32_10(key, (5, k, 0, 3)))
    assert dr["logu_accept"][5] == np.log(u01(x, y))
    x, y, z, _ = (int(v) for v in philox4x32_10(key, (11, k, 0, 4)))
    assert dr["picks"][11] == 1 + ((x * (T - 1)) >> 32)
    assert dr["logu_swap"][11] == np.log(u01(y, z))
    assert dr["normals"].shape == (T, d) and dr["picks"].shape == (5 * T,)
    assert np.all((dr["picks"] >= 1) & (dr["picks"] < T))
    again = R.device_draws(seed, k, T, d)
    assert all(np.array_equal(again[n], dr[n]) for n in dr)
    other = R.device_draws(seed, k + 1, T, d)
    assert not np.array_equal(other["normals"], dr["normals"])
    # the stretch move's tags (0, 1, 7) never meet PTLMC's: the same (c0, c1, c2) under tag 2 gives other words
    assert philox4x32_10(key, (3, k, 1, 0))[0] != philox4x32_10(key, (3, k, 1, 2))[0]


@pytest.mark.parametrize("threads", [False, True])
def test_batched_lbfgsb_returns_scipys_inverse_hessian(threads, monkeypatch):
    """the pre-optimizer's eigen-moves need each search's hess_inv: the lock-step driver's operator is scipy.optimize.minimize's,
    and its callers without the flag still get (x, f)"""
    import scipy.optimize
    from gpbayestools_hic_amd import emulator as E
    rng = np.random.default_rng(3)
    A = rng.standard_normal((4, 4))
    H = A @ A.T + 4 * np.eye(4)
    c = rng.uniform(-0.5, 0.5, 4)

    def fg(x):
        r = x - c
        return 0.5 * r @ H @ r + np.sum(np.cosh(0.3 * x)), H @ r + 0.3 * np.sinh(0.3 * x)

    class Obj:
        @staticmethod
        def lml(X, eval_gradient=True):
            out = [fg(x) for x in X]
            return -np.array([o[0] for o in out]), -np.array([o[1] for o in out])

    starts = rng.uniform(-2, 2, (3, 4))
    bounds = np.tile([[-2.5, 2.5]], (4, 1))
    if threads:
        monkeypatch.setattr(E, "_setulb_usable", lambda: False)
    x, f, hinv = E._batched_lbfgsb(Obj, starts, bounds, return_hess_inv=True)
    assert len(E._batched_lbfgsb(Obj, starts, bounds)) == 2
    for p in range(3):
        ref = scipy.optimize.minimize(fg, starts[p], method="L-BFGS-B", jac=True, bounds=bounds)
        assert np.array_equal(x[p], ref.x)
        assert np.array_equal(hinv[p] @ np.eye(4), ref.hess_inv @ np.eye(4))
