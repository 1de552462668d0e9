"""CPU tier: the inputs of tests/test_gpu_input_widths.py (tests/width_cases.py) held to the conditions under which that file's
bars say something — on the oracle alone, no device.

  * the width list is the one pick_dpad and every launch's with_dpad take their widths from (csrc/dispatch.h), read from the
    source text: a width added there fails here until it gets cases;
  * every GP is in the distance form the cases intend, by the engine's rule S = sum (ptp / l)^2 > 1024 (gpb_internal.h
    gram_limit; restated as tests/test_gpu_edges.py does);
  * the inputs can see a wrong kernel: every query has max_i K*(x, x_i) > 0.05 for each GP, the oracle's variance is >= 1e-3 c,
    and the oracle with input column d - 1 left out differs from the full one by more than 1e6 x the bar the GPU test applies —
    for K, K*, the mean and slot d of the LML gradient (a dropped or mis-padded last column is the defect these cases exist for);
  * the Sobol cases keep every U_S / V below sobol_reference.CAP, the condition tests/test_gpu_sobol.py states for its bar."""
import functools
import os
import re

import numpy as np
import pytest

import sobol_reference as SR
import width_cases as WC
from conftest import REPO
from oracle import gp_oracle as O

# the bars of tests/test_gpu_input_widths.py part a (each the project's own: see that file), and the factor by which a dropped
# column has to exceed them
BAR_K, BAR_MEAN, BAR_GRAD = 1e-13, 1e-11, 1e-9
SEEN = 1e6


def test_the_width_list_is_pick_dpads():
    src = open(os.path.join(REPO, "gpbayestools_hic_amd", "csrc", "dispatch.h")).read()
    m = re.search(r"using\s+Widths\s*=\s*std::integer_sequence\s*<\s*int\s*,([^>]*)>", src)
    assert m, "the list of widths (Widths) not found in dispatch.h"
    assert tuple(int(v) for v in m.group(1).split(",")) == WC.WIDTHS


def test_two_input_counts_per_width():
    assert WC.DS == (1, 8, 9, 16, 17, 20, 21, 24, 25, 32, 33, 48, 49, 64)
    for i, w in enumerate(WC.WIDTHS):
        lo = (WC.WIDTHS[i - 1] if i else 0) + 1
        assert w in WC.DS and lo in WC.DS and WC.dpad_of(w) == w and WC.dpad_of(lo) == w
    for d in WC.WIDE_DS + WC.CHAIN_DS:
        assert d in WC.DS
    assert {WC.dpad_of(d) for d in WC.WIDE_DS} == {24, 32, 64} and {WC.dpad_of(d) for d in WC.CHAIN_DS} == {24, 32, 64}
    assert all((N + 63) // 64 * 64 == 128 for N, _, _, _ in WC.CHAIN_SPECS)           # one shared launch: the same Np


def test_batch_geometry():
    """N = 130 pads to 192 rows with padding in front and behind; 130 queries pad to 256 walkers, 70 to 128"""
    Np = (WC.N + 63) // 64 * 64
    front = (Np - WC.N) // 16 * 16
    assert Np == 192 and front == 48 and Np - WC.N - front == 14
    assert (WC.W + 127) // 128 * 128 == 256 and (WC.W_ONE_PER_LANE + 127) // 128 * 128 == 128


@functools.lru_cache(maxsize=None)
def _oracle(d, kind):
    """the oracle on the case and on the case without its last column: K, K*, mean, variance, LML gradient per GP"""
    kid = O.KIND_NAMES[kind]
    X, Z, th, Xs = WC.make_case(d, kind)
    out = []
    for Xa, Xsa in ((X, Xs), (WC.without_last_column(X), WC.without_last_column(Xs))):
        per = []
        for p in range(WC.P):
            K = O.kernel_train(Xa, th[p], kid, WC.ALPHA)
            L, a = O.gp_factor(Xa, Z[p], th[p], kid, WC.ALPHA)
            Ks = O.kernel_cross(Xsa, Xa, th[p], kid)
            m, v = O.gp_predict(Xsa, Xa, th[p], L, a, kid)
            _, g = O.lml(th[p], Xa, Z[p], kid, WC.ALPHA, eval_gradient=True)
            per.append(dict(K=K, Ks=Ks, m=m, v=v, g=g))
        out.append(per)
    return X, Z, th, Xs, out[0], out[1]


@pytest.mark.parametrize("kind", WC.KINDS)
@pytest.mark.parametrize("d", WC.DS)
def test_the_case_can_see_a_wrong_kernel(d, kind):
    X, Z, th, Xs, full, drop = _oracle(d, kind)
    assert X.shape == (WC.N, d) and Z.shape == (WC.P, WC.N) and th.shape == (WC.P, d + 2) and Xs.shape == (WC.W, d)
    # the forms, by the engine's rule
    S = WC.form_sums(X, th)
    assert [int(s > WC.GRAM_LIMIT) for s in S] == WC.FORMS, S
    # queries within 1e-3 of design points, a few exactly on them
    near = np.abs(Xs[:, None, :] - X[None, :, :]).max(axis=2).min(axis=1)
    assert near.max() <= 1e-3 and np.count_nonzero(near == 0.0) >= WC.ON_DESIGN
    for p in range(WC.P):
        c = float(np.exp(th[p, 0]))
        f, o = full[p], drop[p]
        assert f["Ks"].max(axis=1).min() > 0.05, (p, f["Ks"].max(axis=1).min())
        assert f["v"].min() >= 1e-3 * c, (p, f["v"].min())
        dK = np.max(np.abs(np.tril(f["K"]) - np.tril(o["K"])))
        dKs = np.max(np.abs(f["Ks"] - o["Ks"]))
        dm = np.max(np.abs(f["m"] - o["m"]))
        dg = abs(f["g"][d] - o["g"][d])
        assert o["g"][d] == 0.0                                       # (a kernel that never sees the column has no slope along it)
        assert dK > SEEN * BAR_K * max(c, 1.0), (p, dK)
        assert dKs > SEEN * BAR_K * max(c, 1.0), (p, dKs)
        assert dm > SEEN * BAR_MEAN * np.max(np.abs(f["m"])), (p, dm)
        assert dg > SEEN * BAR_GRAD * max(np.max(np.abs(f["g"])), 1.0), (p, dg, np.max(np.abs(f["g"])))


@pytest.mark.parametrize("d", WC.WIDE_DS)
def test_sobol_cases_keep_the_bar_meaningful(d):
    """U_S / V < CAP for every observable and subset, on the host's own alpha (the GPU test repeats it on the device's)"""
    N, d_, P, seed = WC.SOBOL_CASES[d]
    assert d_ == d and N in (64, 65) and P == 2
    X, Z, theta, lo, hi = SR.make_case(N, d, P, seed)
    alpha = SR.host_alpha(X, Z, theta)
    e, H, Ue, UH = SR.gp_integrals(X, alpha, np.exp(theta[:, 0]), np.exp(theta[:, 1:d + 1]), lo, hi)
    rng = np.random.default_rng(seed + 50)                            # the transform of tests/test_gpu_sobol.py::_transform
    A, mu = rng.standard_normal((P, 4)), rng.standard_normal(4)
    _, V, UV = SR.observables(e, H, Ue, UH, A, mu)
    assert np.all(V[:, 2 * d] > 0) and (UV / V[:, 2 * d:]).max() < SR.CAP
