"""GPU tier: the expected information gain on the device — gpb_eig_simulate, gpb_eig_lse (GPEngine.eig_simulate / eig_lse),
eig.expected_information_gain and Chain.expected_information_gain — against the numpy model of tests/eig_reference.py fed the
device's own simulated data.

Bars (computed by every test from its own inputs, eig_reference.lse_bound / self_bound).  With a_ik, b_jk the centred operands of
the matrix product and b_gj the bias, |lse_excl - model| <= (2 M_g + 64) 2^-52 (max_j (sum_k |a_ik b_jk| + |b_gj|) + |model| + 1):
the forward error of a dot product of 2 M_g terms plus a few ulps for exp and log.  self: (M_g + 8) 2^-52 (sum |terms| + 1).
The kernel's tile is 64 outer rows x 64 inner samples with a K step of 16 (8 observables); the shapes sit below, at and past
one and two tiles and K steps.  Repeated calls, on_device 0 / 1: bit equality."""
import functools
import math

import numpy as np
import pytest

import eig_reference as R

pytestmark = pytest.mark.gpu

E_ARG = -1
SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 257, 1000]
MGS = [1, 2, 7, 8, 9, 17, 64]


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _eng():
    from gpbayestools_hic_amd import GPEngine
    return GPEngine(0)


def _dev(a):
    torch, dev = _torch()
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev)


class Case:
    """an inner set [S_in, M] (sample-major on the host), an outer index list and the pieces that may be absent"""

    def __init__(self, S_in, S_out, M, seed, spread=1.0, var=True, vadd=True, logw=True, oidx=None):
        rng = np.random.default_rng(seed)
        self.S_in, self.S_out, self.M = S_in, S_out, M
        self.var = rng.uniform(0.2, 2.0, size=(S_in, M)) if var else None
        self.vadd = rng.uniform(0.1, 1.0, size=M) if vadd else None
        self.s = (np.zeros((S_in, M)) if self.var is None else self.var) + (np.zeros(M) if self.vadd is None else self.vadd)[None, :]
        self.mu = spread * np.sqrt(self.s) * rng.normal(size=(S_in, M)) + 3.0
        self.logw = np.log(rng.uniform(0.5, 4.0, size=S_in)) if logw else None
        self.oidx = (rng.integers(0, S_in, size=S_out) if oidx is None else np.asarray(oidx)).astype(np.int32)
        self.seed = 1000 + seed


def _simulate(c, pad_in=0, pad_out=0, seed=None):
    """the device's y and z (sample-major numpy) and the device tensors; pads: ld_in = S_in + pad_in with NaN behind the samples,
    ld_out = S_out + pad_out with a canary behind the rows"""
    torch, dev = _torch()
    mu_full = torch.full((c.M, c.S_in + pad_in), float("nan"), dtype=torch.float64, device=dev)
    mu_full[:, :c.S_in] = _dev(c.mu.T)
    mu_T = mu_full[:, :c.S_in]
    var_T = None
    if c.var is not None:
        var_full = torch.full((c.M, c.S_in + pad_in), float("nan"), dtype=torch.float64, device=dev)
        var_full[:, :c.S_in] = _dev(c.var.T)
        var_T = var_full[:, :c.S_in]
    y_full = torch.full((c.M, c.S_out + pad_out), 777.0, dtype=torch.float64, device=dev)
    y_full, z_full = _eng().eig_simulate(mu_T, var_T, c.vadd, c.oidx, c.seed if seed is None else seed, out=y_full, return_z=True)
    assert bool((y_full[:, c.S_out:] == 777.0).all()) and bool((z_full[:, c.S_out:] == 0.0).all())      # the canaries
    y = y_full[:, :c.S_out].cpu().numpy().T.copy()
    z = z_full[:, :c.S_out].cpu().numpy().T.copy()
    return mu_T, var_T, y_full, y, z


def _lse(c, mu_T, var_T, y_full, ranges, splits=0, on_device=False):
    lse, slf = _eng().eig_lse(mu_T, var_T, c.vadd, c.logw, y_full, c.oidx, ranges, splits=splits, on_device=on_device)
    if on_device:
        lse, slf = lse.cpu().numpy(), slf.cpu().numpy()
    return lse, slf


def _model(c, y, ranges):
    lse, slf = R.direct(c.mu, c.s, c.logw, y, c.oidx, ranges)
    _, mag = R.gemm_form(c.mu, c.s, c.logw, y, c.oidx, ranges)
    return lse, slf, R.lse_bound(mag, lse, ranges), R.self_bound(c.mu, c.s, c.logw, y, c.oidx, ranges)


def _assert_close(got, model, what=""):
    lse, slf = got
    mlse, mslf, blse, bslf = model
    inf = np.isneginf(mlse)
    assert np.array_equal(np.isneginf(lse), inf), what
    fin = ~inf
    assert np.all(np.isfinite(lse[fin])) and np.all(np.isfinite(slf)), what
    r1 = (np.abs(lse - mlse)[fin] / blse[fin]).max() if fin.any() else 0.0
    r2 = (np.abs(slf - mslf) / bslf).max()
    print("%s: lse_excl error / bound %.3g, self error / bound %.3g" % (what, r1, r2))
    assert r1 <= 1.0 and r2 <= 1.0, what


def _check(c, ranges, pad_in=0, pad_out=0, splits=0, what=""):
    mu_T, var_T, y_full, y, z = _simulate(c, pad_in, pad_out)
    assert np.array_equal(y, R.simulate(c.mu, c.s, c.oidx, z))                     # y - (mu + sqrt(s) z) == 0 exactly
    got = _lse(c, mu_T, var_T, y_full, ranges, splits)
    _assert_close(got, _model(c, y, ranges), what)
    return got


# ------------------------------------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("k", range(len(SIZES)))
def test_sample_counts_around_the_tiles(k):
    """S_in and S_out each below, at and past one and two tiles of 64, and 1000; every size meets a different partner"""
    S_in, S_out = SIZES[k], SIZES[(3 * k + 4) % len(SIZES)]
    M = MGS[k % len(MGS)]
    _check(Case(S_in, S_out, M, 10 + k), [(0, M)], what="S_in %d S_out %d M %d" % (S_in, S_out, M))
    _check(Case(S_out, S_in, M, 40 + k), [(0, M)], what="S_in %d S_out %d M %d" % (S_out, S_in, M))


@pytest.mark.parametrize("M", MGS)
def test_group_sizes_around_the_k_step(M):
    """2 M_g below, at and past the K step of 16, multiples of 4 and not; more than one tile either way"""
    _check(Case(129, 65, M, 70 + M), [(0, M)], what="M %d" % M)


def test_several_groups_in_one_call():
    """adjacent, overlapping, a single observable at either end, one spanning all of M = 91 — with leading dimensions past the
    sample counts: NaN behind the inner samples (read, they would poison every sum), canaries behind the outer rows"""
    M = 91
    ranges = [(0, 30), (30, 61), (20, 50), (0, 91), (90, 91), (0, 1), (61, 91)]
    _check(Case(257, 129, M, 5), ranges, pad_in=5, pad_out=7, what="groups")
    _check(Case(257, 129, M, 6), ranges[::-1], pad_in=1, pad_out=64, what="groups reversed")


@pytest.mark.parametrize("absent", ["var", "vadd", "logw"])
def test_optional_inputs_absent(absent):
    c = Case(130, 70, 9, 3, **{absent: False})
    _check(c, [(0, 9), (2, 5)], what="no " + absent)


# ------------------------------------------------------------------------------------------------ 2. self-exclusion
def test_repeated_outer_indices():
    """one index 50 times, others twice: every position gets its own noise and leaves out the same sample"""
    oidx = np.concatenate([np.full(50, 7), np.arange(20), np.arange(20), [99, 99, 0]])
    c = Case(100, len(oidx), 6, 8, oidx=oidx)
    mu_T, var_T, y_full, y, z = _simulate(c)
    assert len({tuple(r) for r in z[:50]}) == 50                                   # the same index, different noise
    _assert_close(_lse(c, mu_T, var_T, y_full, [(0, 6)]), _model(c, y, [(0, 6)]), "repeated")


def test_two_inner_samples_and_one():
    """S_in = 2: lse_excl is the other sample's single term; S_in = 1: -inf, self finite"""
    c = Case(2, 66, 5, 12)
    lse, slf = _check(c, [(0, 5)], what="S_in 2")
    mu_T, var_T, y_full, y, z = _simulate(c)                                      # (the same seed: the same data)
    other = 1 - c.oidx
    d = y - c.mu[other]
    term = c.logw[other] - 0.5 * np.sum(d * d / c.s[other] + np.log(c.s[other]), axis=1)
    assert np.all(np.abs(lse[0] - term) <= _model(c, y, [(0, 5)])[2][0])
    c1 = Case(1, 65, 5, 13)
    lse, slf = _check(c1, [(0, 5), (1, 2)], what="S_in 1")
    assert np.all(np.isneginf(lse)) and np.all(np.isfinite(slf))


def test_own_sample_dominates():
    """means 40 sigma apart: the row's own sample carries the whole sum — the excluded sum is more than 10^3 times smaller than
    the included one, and still within its bound"""
    c = Case(200, 70, 4, 14, spread=40.0)
    lse, slf = _check(c, [(0, 4)], what="dominant")
    assert np.all(np.logaddexp(lse, slf) - lse > math.log(1e3))


# ------------------------------------------------------------------------------------------------ 3. the running maximum
def test_a_row_far_from_every_sample():
    """one outer row 500 sigma from every inner sample: logits near -10^5, a finite result within the bound"""
    torch, dev = _torch()
    c = Case(150, 65, 3, 15)
    mu_T, var_T, y_full, y, z = _simulate(c)
    far = c.mu.max(axis=0) + 500.0 * np.sqrt(c.s.max(axis=0))
    y[17] = far
    y_full[:, 17] = _dev(far)
    got = _lse(c, mu_T, var_T, y_full, [(0, 3)])
    model = _model(c, y, [(0, 3)])
    assert model[0][0, 17] < -1e5 and np.isfinite(got[0][0, 17])
    _assert_close(got, model, "far row")


def test_log_weights_of_700():
    """one inner sample with a log-weight of +700, the rest at -700: no overflow, no underflow to -inf"""
    c = Case(130, 70, 4, 16)
    c.logw = np.full(130, -700.0)
    c.logw[5] = 700.0
    c.oidx[:3] = 5                                     # rows that leave the heavy sample out
    lse, slf = _check(c, [(0, 4)], what="weights of +-700")
    assert np.all(lse[0, :3] < -600.0) and np.all(lse[0, 3:][c.oidx[3:] != 5] > 600.0)


# ------------------------------------------------------------------------------------------------ 4. splits, repeatability
def test_splits_and_repeatability():
    c = Case(1000, 129, 10, 17)
    ranges = [(0, 10), (3, 4)]
    mu_T, var_T, y_full, y, z = _simulate(c)
    model = _model(c, y, ranges)
    outs = {}
    for splits in (1, 3, 64, 0):
        outs[splits] = _lse(c, mu_T, var_T, y_full, ranges, splits)
        _assert_close(outs[splits], model, "splits %d" % splits)
    for splits in (1, 3, 0):
        again = _lse(c, mu_T, var_T, y_full, ranges, splits)
        assert np.array_equal(again[0], outs[splits][0]) and np.array_equal(again[1], outs[splits][1])
        dev_out = _lse(c, mu_T, var_T, y_full, ranges, splits, on_device=True)
        assert np.array_equal(dev_out[0], outs[splits][0]) and np.array_equal(dev_out[1], outs[splits][1])


# ------------------------------------------------------------------------------------------------ 5. gpb_eig_simulate
def test_simulate():
    c = Case(40, 300, 7, 18, oidx=np.concatenate([np.full(100, 3), np.arange(200) % 40]))
    _, _, _, y, z = _simulate(c, seed=99)
    _, _, _, y2, z2 = _simulate(c, seed=99)
    _, _, _, y3, z3 = _simulate(c, seed=100)
    assert np.array_equal(y, y2) and np.array_equal(z, z2)
    assert not np.array_equal(z, z3) and not np.any(z == z3)
    assert np.all(z[0] != z[1])                                                      # positions 0 and 1 share index 3
    assert np.array_equal(y, R.simulate(c.mu, c.s, c.oidx, z))
    ref = R.device_z(99, 300, 7)
    assert np.max(np.abs(z - ref)) <= 1e-15 * max(1.0, np.abs(ref).max())         # the bar of tests/test_gpu_smc.py for such draws
    # var_T and vadd absent in turn: s is the other one
    for absent in ("var", "vadd"):
        c2 = Case(40, 70, 3, 19, **{absent: False})
        _, _, _, ya, za = _simulate(c2)
        assert np.array_equal(ya, R.simulate(c2.mu, c2.s, c2.oidx, za))


def test_simulate_moments():
    """mean and variance of 10^5 draws within 5 standard errors"""
    c = Case(10, 50000, 2, 20)
    _, _, _, _, z = _simulate(c)
    n = z.size
    assert n == 100000
    assert abs(z.mean()) <= 5.0 / math.sqrt(n)
    assert abs(z.var() - 1.0) <= 5.0 * math.sqrt(2.0 / n)


# ------------------------------------------------------------------------------------------------ 6. error codes
def test_argument_errors():
    from gpbayestools_hic_amd import _native as nat
    torch, dev = _torch()
    eng = _eng()
    M, S_in, S_out = 6, 50, 40
    mu = torch.ones((M, S_in), dtype=torch.float64, device=dev)
    var = torch.ones((M, S_in), dtype=torch.float64, device=dev)
    y = torch.zeros((M, S_out), dtype=torch.float64, device=dev)
    good_idx = torch.zeros(S_out, dtype=torch.int32, device=dev)
    lse = torch.full((65, S_out), 5.0, dtype=torch.float64, device=dev)
    slf = torch.full((65, S_out), 5.0, dtype=torch.float64, device=dev)
    ranges = np.zeros((65, 2), dtype=np.int32)
    ranges[:, 1] = M

    def lse_call(M=M, S_in=S_in, ld_in=S_in, S_out=S_out, ld_out=S_out, G=1, splits=0, on_device=1, idx=good_idx, rg=ranges):
        return eng.lib.gpb_eig_lse(eng.h, nat.ptr(mu), nat.ptr(var), None, None, M, S_in, ld_in, nat.ptr(y), nat.ptr(idx), S_out,
                                   ld_out, nat.ptr(np.ascontiguousarray(rg)), G, splits, on_device, nat.ptr(lse), nat.ptr(slf))

    def sim_call(M=M, S_in=S_in, ld_in=S_in, S_out=S_out, ld_out=S_out, idx=good_idx):
        return eng.lib.gpb_eig_simulate(eng.h, nat.ptr(mu), nat.ptr(var), None, M, S_in, ld_in, nat.ptr(idx), S_out, 1, nat.ptr(y),
                                        None, ld_out)

    assert lse_call() == 0 and sim_call() == 0
    empty, outside, negative = ranges.copy(), ranges.copy(), ranges.copy()
    empty[0] = (3, 3)
    outside[0] = (2, M + 1)
    negative[0] = (-1, 2)
    low = good_idx.clone()
    low[7] = -1
    high = good_idx.clone()
    high[S_out - 1] = S_in
    lse.fill_(5.0)
    slf.fill_(5.0)
    bad = [dict(ld_in=S_in - 1), dict(ld_out=S_out - 1), dict(M=0), dict(M=4097), dict(G=0), dict(G=65), dict(rg=empty),
           dict(rg=outside), dict(rg=negative), dict(S_out=0), dict(S_in=0), dict(idx=low), dict(idx=high), dict(splits=-1),
           dict(splits=65), dict(on_device=2)]
    for kw in bad:
        assert lse_call(**kw) == E_ARG, kw
    assert bool((lse == 5.0).all()) and bool((slf == 5.0).all())                   # a refused call writes nothing
    assert lse_call(splits=64) == 0 and lse_call(G=64, on_device=1) == 0
    for kw in (dict(ld_in=S_in - 1), dict(ld_out=S_out - 1), dict(M=0), dict(M=4097), dict(S_out=0), dict(S_in=0), dict(idx=low),
               dict(idx=high)):
        assert sim_call(**kw) == E_ARG, kw
    # the Python layer: non-finite inputs and s <= 0 are ValueError before any launch
    from gpbayestools_hic_amd.eig import expected_information_gain
    m = np.ones((20, 3))
    for kw in (dict(mean=np.where(np.arange(60).reshape(20, 3) == 7, np.nan, 1.0), var=None, planned_var=1.0),
               dict(mean=m, var=np.zeros((20, 3)), planned_var=0.0), dict(mean=m, var=None, planned_var=[1.0, -1.0, 1.0]),
               dict(mean=m[:1], var=None, planned_var=1.0), dict(mean=m, var=None, planned_var=1.0, weights=np.zeros(20)),
               dict(mean=m, var=None, planned_var=1.0, groups=[(0, 4)])):
        with pytest.raises(ValueError):
            expected_information_gain(**kw)


# ------------------------------------------------------------------------------------------------ 7. the public interface
def test_plain_arrays_against_the_model():
    """eig.expected_information_gain on a linear-Gaussian set: the estimates are the model's within the propagated bounds and
    bracket the closed form; the result's table names every group"""
    from gpbayestools_hic_amd.eig import estimates, expected_information_gain
    mu, s, _, _, exact = R.linear_gaussian(4000, 8, 3)
    res = expected_information_gain(mu, None, s[0], groups={"first": (0, 3), "all": (0, 6)}, n_outer=1024, seed=4)
    assert res.names == ["first", "all"] and res.n_inner == 4000 and res.n_outer == 1024
    assert abs(res.ln_n_inner - math.log(4000)) < 1e-12 and res.per_row[0].shape == (2, 1024)
    print(res.table())
    assert "first" in res.table() and "all" in res.table()
    assert res.lower[1] - 4 * res.stderr[1] <= exact <= res.upper[1] + 4 * res.stderr[1]
    assert res.lower[0] < res.lower[1]                                               # fewer observables teach less
    assert np.all(res.per_row[0] <= math.log(4000) + 1e-12)


SPECS = [(100, 5, 3, "RBF"), (130, 4, 2, "Matern25"), (90, 6, 3, "RBF")]


@functools.lru_cache(maxsize=None)
def _chain():
    import tempfile
    from gpbayestools_hic_amd import synth, workload
    chain, emus, info = workload.build_multi_chain(SPECS, 20, workdir=tempfile.mkdtemp(prefix="gpb_eig_"))
    X = synth.walkers(512, 20, seed=31)
    X[100], X[101], X[300] = X[3], X[3], X[4]                                        # repeated rows: 509 distinct samples
    return chain, X


def test_chain_expected_information_gain():
    from gpbayestools_hic_amd.eig import estimates
    chain, X = _chain()
    res = chain.expected_information_gain(X, n_outer=128, seed=11)
    assert res.names == ["emulator0", "emulator1", "emulator2", "all"]
    assert res.ranges.tolist() == [[0, 5], [5, 9], [9, 15], [0, 15]]
    # the collapse of repeated rows: the weights of np.unique
    ux, counts = np.unique(X, axis=0, return_counts=True)
    assert res.n_inner == 509 and res.n_outer == 128 and np.array_equal(res.weights, counts.astype(np.float64))
    assert sorted(counts.tolist())[-2:] == [2, 3]
    # the draws, restated
    w = counts.astype(np.float64)
    rng = np.random.default_rng(11)
    oidx = rng.choice(509, 128, p=w / w.sum()).astype(np.int32)
    sim_seed = int(rng.integers(0, 2 ** 63))
    assert np.array_equal(res.outer_idx, oidx)
    # the model on the emulators' own predictions and the device's own simulated data
    engs, mu_T, var_T = chain._ppd_arrays(np.ascontiguousarray(ux))
    pv = np.diag(chain.expdata_cov).copy()
    y_T = engs[0].eig_simulate(mu_T, var_T, pv, oidx, sim_seed)
    mu, s, y = mu_T.cpu().numpy().T.copy(), var_T.cpu().numpy().T + pv[None, :], y_T.cpu().numpy().T.copy()
    logw = np.log(w)
    mlse, mslf = R.direct(mu, s, logw, y, oidx, res.ranges)
    _, mag = R.gemm_form(mu, s, logw, y, oidx, res.ranges)
    row_tol = 2.0 * R.lse_bound(mag, mlse, res.ranges) + 2.0 * R.self_bound(mu, s, logw, y, oidx, res.ranges)
    L, U, lower, upper, stderr = estimates(mlse, mslf, w, oidx)
    for g in range(4):
        print("%s: lower %.6f (model %.6f) upper %.6f (model %.6f) stderr %.4f" % (res.names[g], res.lower[g], lower[g], res.upper[g],
                                                                                 upper[g], res.stderr[g]))
    assert np.all(np.abs(res.per_row[0] - L) <= row_tol) and np.all(np.abs(res.per_row[1] - U) <= row_tol)
    assert np.all(np.abs(res.lower - lower) <= row_tol.mean(axis=1) + 4 * R.EPS * np.abs(lower))
    assert np.all(np.abs(res.upper - upper) <= row_tol.mean(axis=1) + 4 * R.EPS * np.abs(upper))
    assert np.all(np.abs(res.stderr - stderr) <= 2.0 * row_tol.max(axis=1) + 4 * R.EPS * stderr)
    assert np.all(res.per_row[0] <= np.log(w.sum() / w[oidx])[None, :] + 1e-12)
    assert np.all(res.lower <= res.upper)
    # the same call twice: the same bits; a planned error ten times smaller teaches more; own groups
    again = chain.expected_information_gain(X, n_outer=128, seed=11)
    assert np.array_equal(again.lower, res.lower) and np.array_equal(again.upper, res.upper)
    fine = chain.expected_information_gain(X, n_outer=128, seed=11, planned_error=0.1 * np.sqrt(pv))
    assert fine.upper[3] > res.upper[3]
    own = chain.expected_information_gain(X, n_outer=128, seed=11, groups={"a": (0, 5), "b": (3, 12)})
    assert own.names == ["a", "b"] and np.array_equal(own.lower[0], res.lower[0])
    # a stored [nwalkers, nsteps, ndim] array is flattened after discard and thin
    st = chain.expected_information_gain(X.reshape(8, 64, 20), discard=32, thin=2, n_outer=64, seed=2)
    fl = chain.expected_information_gain(X.reshape(8, 64, 20)[:, 32::2].reshape(-1, 20), n_outer=64, seed=2)
    assert np.array_equal(st.lower, fl.lower) and st.n_inner == fl.n_inner


def test_saturation_warning(caplog):
    """means 30 sigma apart with 50 samples: every row identifies its sample, lower sits at ln 50 and a warning says so"""
    import logging
    from gpbayestools_hic_amd.eig import expected_information_gain
    c = Case(50, 64, 3, 23, spread=30.0)
    with caplog.at_level(logging.WARNING, logger="gpbayestools_hic_amd.eig"):
        res = expected_information_gain(c.mu, c.var, c.vadd, n_outer=64, seed=1)
    assert res.saturated[0] and res.lower[0] > math.log(50) - 1.0 and res.lower[0] <= math.log(50) + 1e-12
    assert any("saturates" in r.getMessage() for r in caplog.records)


def test_chain_refusals():
    chain, X = _chain()

    class Foreign:
        nobs = 4

        def predict(self, X, return_cov=True, extra_std=0):
            return np.zeros((X.shape[0], 4)), np.zeros((X.shape[0], 4, 4))

    class TwoRanks:
        world, rank = 2, 0

    keep = list(chain.emuList)
    try:
        chain.emuList = [keep[0], Foreign()]
        with pytest.raises(NotImplementedError, match="foreign"):
            chain.expected_information_gain(X)
        chain.emuList = keep
        chain.sharding = TwoRanks()
        with pytest.raises(NotImplementedError, match="sharded"):
            chain.expected_information_gain(X)
    finally:
        chain.emuList, chain.sharding = keep, None
    for bad in (X[:, :19], X.reshape(2, 4, 64, 20), np.repeat(X[:1], 10, axis=0)):
        with pytest.raises(ValueError):
            chain.expected_information_gain(bad, n_outer=16)
    Xn = X.copy()
    Xn[5, 2] = np.inf
    with pytest.raises(ValueError):
        chain.expected_information_gain(Xn, n_outer=16)
    for kw in (dict(weights=-np.ones(512)), dict(weights=np.ones(511)), dict(planned_error=np.ones(14)), dict(n_outer=0),
               dict(groups=[(0, 16)])):
        with pytest.raises(ValueError):
            chain.expected_information_gain(X, **dict(dict(n_outer=16), **kw))
    with pytest.raises(ValueError):
        chain.expected_information_gain(X.reshape(8, 64, 20), weights=np.ones(512))


def test_sampler_method_is_the_chains_on_the_stored_rows():
    from gpbayestools_hic_amd import StretchSampler, synth
    chain, _ = _chain()
    s = StretchSampler(chain, 40, seed=5)
    s.run(synth.walkers_ball(40, np.full(20, 0.5), 0.02, seed=6), 12)
    a = s.expected_information_gain(discard=3, thin=2, n_outer=64, seed=1)
    rows = s._chain_dev[3::2].reshape(-1, 20).cpu().numpy()
    b = chain.expected_information_gain(rows, n_outer=64, seed=1)
    assert a.n_inner == b.n_inner == np.unique(rows, axis=0).shape[0] and a.n_inner <= rows.shape[0]     # (rejected moves repeat rows)
    assert np.array_equal(a.lower, b.lower) and np.array_equal(a.upper, b.upper) and np.array_equal(a.stderr, b.stderr)
    assert np.all(np.isfinite(a.lower)) and np.all(np.isfinite(a.upper))
    with pytest.raises(ValueError):
        s.expected_information_gain(thin=0)
