"""Joint predictive covariance reference for the tests (a helper module, not a test file): cov = k(X*, X*) - V^T V with
V = L^-1 K(X*, X)^T (oracle.gp_oracle.gp_predict_cov, sk:_gpr.py:441-469) evaluated in long double from a GIVEN L^-1 and K*, and
a forward rounding bound for any fp64 evaluation of that formula from the same two operands.  Handed the device's own read-back
L^-1 and K* they hold csrc/gpb_cov.hip's kernels (k_vmat, k_kss, k_cov_update, k_cov_pack) alone to account, not the
factorisation or the cross kernel in front of them.  Also here: the shapes and inputs the CPU and the GPU tests share."""
import numpy as np

from gpbayestools_hic_amd import synth
from oracle import gp_oracle as O

ALPHA = 0.1
P = 2
U = 2.0 ** -53                                                    # unit roundoff of fp64
# (N, d, kernel, W): Np = 192 / 320 / 256 / 448 — a half-empty last 128-row block of V (Np % 128 == 64) in three of the four;
# W = 1 (one tile, 127 padded columns), 128 (no padding), 129 (two tiles a side, 127 padded), 257 (three a side)
SHAPES = [(130, 3, "RBF", 1), (320, 6, "Matern15", 129), (200, 20, "Matern25", 128), (448, 5, "RBF", 257)]


def padded(N):
    """Np: the design padded to whole 64-row blocks (gp_set_impl), the length of the device's sums over the design"""
    return (N + 63) // 64 * 64


def kss(Xs, theta, kind):
    """k(X*, X*) as gp_predict_cov builds it: the diagonal forced to c, the noise added on the diagonal only"""
    d = Xs.shape[1]
    K = O.kernel_cross(Xs, Xs, theta, kind)
    np.fill_diagonal(K, np.exp(theta[0]))
    K[np.diag_indices_from(K)] += np.exp(theta[d + 1])
    return K


def joint_cov_ld(Linv, Kstar, Xs, theta, kind):
    """cov [W, W] in long double: V = Linv @ Kstar^T (Linv [N, N] lower triangular, Kstar [W, N]), cov = Kss - V^T V.  The
    products and the difference carry 64-bit significands: against the 53-bit evaluations held to joint_cov_bound this is exact
    to 2^-11 of the bound.  Kss's entries are the oracle's fp64 ones (kernel_cross), exactly converted."""
    ld = np.longdouble
    V = np.asarray(Linv, ld) @ np.asarray(Kstar, ld).T
    return kss(Xs, theta, kind).astype(ld) - V.T @ V


def joint_cov_f64(Linv, Kstar, Xs, theta, kind):
    """the same formula in numpy's plain fp64 (BLAS order of summation)"""
    V = Linv @ Kstar.T
    return kss(Xs, theta, kind) - V.T @ V


def kss_rounding_factor(Xs, theta):
    """G [W, W]: an entry of k(X*, X*) evaluated in fp64 by two different programs (the oracle's and the one under test) differs
    by at most u G |Kss|.  Per evaluation, against exact arithmetic on the fp64 inputs x, log l, log c, with q = x / l:
      * l = exp(log l) to 1 ulp (2 u) and the quotient's rounding: q within 3 u |q|; the difference df = q_i - q_j within
        3 u (|q_i| + |q_j|) + u |df| — NOT relative to df: two programs need not share the bits of l;
      * r^2 = sum_k df_k^2 over d terms, products rounded or fused: within 6 u S + (d + 3) u r^2, S = sum_k |df_k| (|q_ik| + |q_jk|);
      * the shape functions: |d f / d r^2| <= 1.5 f for all three (RBF 1/2, Matern-5/2 5/6, Matern-3/2 3/2 at r = 0); their own
        roundings — sqrt, the constant, the polynomial (up to 8 u) and exp to 1 ulp of an argument t <= sqrt(5 r^2) that carries
        3 u itself (3 t u) — and c = exp(log c) with its product (3 u): 11 u + 3 sqrt(5 r^2) u.
    One evaluation: (1.5 (6 S + (d + 3) r^2) + 11 + 3 sqrt(5 r^2)) u |k|; two of them against each other twice that:
        G = 18 S + 3 (d + 3) r^2 + 22 + 6 sqrt(5 r^2)           off the diagonal,
        G = 8 on it (c + sigma_n^2: two exps, one sum, each side)."""
    d = Xs.shape[1]
    Q = Xs / np.exp(theta[1:1 + d])
    adf = np.abs(Q[:, None, :] - Q[None, :, :])
    S = np.einsum("ijk,ijk->ij", adf, np.abs(Q)[:, None, :] + np.abs(Q)[None, :, :])
    r2 = np.einsum("ijk,ijk->ij", adf, adf)
    G = 18.0 * S + 3.0 * (d + 3) * r2 + 22.0 + 6.0 * np.sqrt(5.0 * r2)
    G = np.maximum(G, G.T)
    np.fill_diagonal(G, 8.0)
    return G


def joint_cov_bound(Linv, Kstar, Xs, theta, kind, Np=None):
    """B [W, W] >= |cov_fp64 - cov_exact| for an fp64 evaluation, in ANY order of summation, with or without fused
    multiply-adds, of cov = Kss - V^T V, V = Linv Kstar^T, over Np terms per sum (Np = the padded design; default padded(N)):

        B = u ((Np + 4) |V|^T |V| + G |Kss|) + E^T |V| + |V|^T E,        E = Np u |Linv| |Kstar|^T,   u = 2^-53

      * E bounds the computed V: a dot product of n terms in fp64 is within gamma_n sum |a_k b_k| of the exact one whatever its
        order (Higham, Accuracy and Stability, 3.1), gamma_n = n u / (1 - n u); a row of the triangular Linv has at most Np
        nonzero terms.  E^T |V| + |V|^T E is that error carried to first order through V^T V (the E^T E term is O(u^2) and sits
        in the + 4 below with room to spare: E <= Np u |Linv| |Kstar|^T is itself some 1e-13 of |V| here).
      * u Np |V|^T |V|: the length-Np dot products of V^T V, by the same lemma.
      * u 4 |V|^T |V|: + 1 for the final subtraction Kss - (V^T V), one rounding of a result no larger than |Kss| + |V|^T |V|
        (its |Kss| share: + 1 on G), + 1 for gamma_n against n u, + 2 for the second-order terms.
      * u G |Kss| (elementwise): the entry of k(X*, X*) against the oracle's fp64 evaluation of it, kss_rounding_factor — a
        count per entry from the rows' own coordinates (22 to about 400 here) in place of a constant per dimension, which the
        difference of two separately rounded quotients does not admit.  It alone covers an entry whose V columns vanish.
    Derived from the formula and the number format alone — nothing here is fitted to what a device returns.  tests/
    test_cov_reference.py checks that numpy's own fp64 evaluation stays inside B and that B itself stays below 1e-11 of the prior
    variance at the tests' shapes, so that the bound can never hide an error the 1e-10 bar would have caught."""
    N = Linv.shape[0]
    Np = padded(N) if Np is None else int(Np)
    aV = np.abs(Linv @ Kstar.T)
    E = Np * U * (np.abs(Linv) @ np.abs(Kstar).T)
    EV, VV, aK = E.T @ aV, aV.T @ aV, np.abs(kss(Xs, theta, kind))
    VV, aK = np.maximum(VV, VV.T), np.maximum(aK, aK.T)            # (BLAS's own rounding: B[i, j] == B[j, i] exactly)
    return U * ((Np + 4) * VV + (kss_rounding_factor(Xs, theta) + 1.0) * aK) + (EV + EV.T)


# ---------------------------------------------------------------------------- data and hyper-parameters of the tests
def problem(N, d, W):
    """X = lhs(N, d, seed=N), Z [P, N] = sin(X w_p) + 0.05 eps, theta = fixed_theta + 0.1 eps (c ~ 1, l ~ 1.5, sigma_n^2 ~ 0.05
    per GP and dimension), W queries uniform in the unit box of which the first min(W // 3, 20) ARE design points (spread over
    the design, both ends included: the heaviest cancellation in Kss - V^T V) and the last is a copy of the one before it (two
    rows of the covariance that differ by the noise on the diagonal alone)"""
    rng = np.random.default_rng(N + 1000)
    X = synth.lhs(N, d, seed=N)
    Z = np.sin(X @ rng.standard_normal((d, P))).T + 0.05 * rng.standard_normal((P, N))
    theta = synth.fixed_theta(d, P) + 0.1 * rng.standard_normal((P, d + 2))
    Xs = rng.random((W, d))
    k = min(W // 3, 20)
    if k:
        Xs[:k] = X[np.linspace(0, N - 1, k).astype(int)]
    if W >= 2:
        Xs[-1] = Xs[-2]
    return X, Z, theta, Xs


def n_design_rows(W):
    return min(W // 3, 20)


def host_operands(X, theta, kind, Xs):
    """(Linv [N, N], Kstar [W, N]) of one GP from the oracle: the CPU tests' stand-in for the device's read-back"""
    from scipy.linalg import solve_triangular
    L = np.linalg.cholesky(O.kernel_train(X, theta, kind, ALPHA))
    Linv = solve_triangular(L, np.eye(L.shape[0]), lower=True, check_finite=False)
    return np.tril(Linv), O.kernel_cross(Xs, X, theta, kind)
