"""Host model of the closed-form Sobol indices (a helper module, not a test file): numpy + scipy.special.erf.

RBF kernel, uniform box [lo, hi], widths w = hi - lo (Oakley & O'Hagan 2004).  GP p has the posterior mean
m_p(x) = c_p sum_i alpha_pi prod_l exp(-(x_l - x_il)^2 / 2 l_pl^2); observable m is f_m = mu_m + sum_p A_pm m_p.  With a = x_il,
b = x_i'l, l = l_pl, l' = l_ql:
    I^p_l(a)     = l sqrt(pi/2) / w_l [erf((hi_l - a) / (sqrt2 l)) - erf((lo_l - a) / (sqrt2 l))]
    Q^pq_l(a, b) = exp(-(a - b)^2 / 2(l^2 + l'^2)) sqrt(pi / 2s) / w_l [erf((hi_l - c) sqrt(s/2)) - erf((lo_l - c) sqrt(s/2))],
                   s = 1/l^2 + 1/l'^2, c = (a/l^2 + b/l'^2) / s
    e_p    = c_p sum_i alpha_pi prod_l I^p_l(x_il)
    H^pq_S = c_p c_q sum_ii' alpha_pi alpha_qi' prod_{l in S} Q^pq_l(x_il, x_i'l) prod_{l not in S} I^p_l(x_il) I^q_l(x_i'l)
for the 2d + 1 subsets S = {j} (slot j), all \\ {j} (slot d + j), all (slot 2d);
    E[f_m] = mu_m + sum_p A_pm e_p,  V_S(m) = sum_pq A_pm A_qm (H^pq_S - e_p e_q),  V = V_all,
    first-order S_j = V_{j} / V,  total T_j = 1 - V_{all \\ j} / V,
    main effect E[f_m | x_j = t] = mu_m + sum_p A_pm c_p sum_i alpha_pi exp(-(t - x_ij)^2 / 2 l_pj^2) prod_{l != j} I^p_l(x_il).
Every factor is positive, so the sum of the absolute values of the terms of an e or an H (the unit bound U the tests' bar is
built on) is the same expression with |alpha| in the place of alpha.

The order the device adds in (restated here for the bar, the model itself sums with numpy): a workgroup takes one 64 x 64 tile of
(i, i') — design points in blocks of 64 from i = 0, the last block ragged — and one GP pair; within it every thread adds 16 rows,
a wave reduces its 64 lanes, four waves are added.  The tile partials of one output are then added in sequence, row block by row
block: nB^2 of them for p != q and nB (nB + 1) / 2 for p = q (the lower block triangle, off-diagonal tiles doubled), with
nB = ceil(N / 64).  T below is the larger count."""
import numpy as np
from scipy.special import erf

from gpbayestools_hic_amd import synth


def tile_partials(N):
    """T: tile partials added in sequence per output"""
    nB = (N + 63) // 64
    return nB * nB


def bar_factor(N, d):
    """2 k 2^-53 with k = 16 (2d + 3) + 24 + T: 16 ulp (the OpenCL bound on erf) for every one of the 2d + 3 factors of a term, 24 for
    the additions inside a thread and a workgroup, T tile partials added in sequence; the factor 2 is the model's own rounding"""
    k = 16 * (2 * d + 3) + 24 + tile_partials(N)
    return 2.0 * k * 2.0 ** -53


def I1(a, ell, lo, hi):
    r = 1.0 / (np.sqrt(2.0) * ell)
    return ell * np.sqrt(np.pi / 2.0) / (hi - lo) * (erf((hi - a) * r) - erf((lo - a) * r))


def Q1(a, b, ell, ellp, lo, hi):
    s = 1.0 / ell ** 2 + 1.0 / ellp ** 2
    c = (a / ell ** 2 + b / ellp ** 2) / s
    rs = np.sqrt(0.5 * s)
    return (np.exp(-(a - b) ** 2 / (2.0 * (ell ** 2 + ellp ** 2))) * np.sqrt(np.pi / (2.0 * s)) / (hi - lo)
            * (erf((hi - c) * rs) - erf((lo - c) * rs)))


def itable(X, ell, lo, hi):
    """I [P, N, d]"""
    return I1(X[None, :, :], ell[:, None, :], lo[None, None, :], hi[None, None, :])


def gp_integrals(X, alpha, amp, ell, lo, hi):
    """e [P], H [P, P, 2d + 1] and their unit bounds Ue, UH (the same sums over the absolute values of the terms) for the design
    X [N, d], alpha [P, N], amplitudes amp [P], length scales ell [P, d] and the box lo, hi [d]"""
    X, alpha, amp, ell, lo, hi = (np.asarray(v, dtype=np.float64) for v in (X, alpha, amp, ell, lo, hi))
    N, d = X.shape
    P = alpha.shape[0]
    It = itable(X, ell, lo, hi)
    prodI = It.prod(axis=2)                                      # [P, N]
    e = amp * (alpha * prodI).sum(axis=1)
    Ue = amp * (np.abs(alpha) * prodI).sum(axis=1)
    H = np.empty((P, P, 2 * d + 1))
    UH = np.empty_like(H)
    for p in range(P):
        for q in range(p, P):
            Q = Q1(X[:, None, :], X[None, :, :], ell[p][None, None, :], ell[q][None, None, :], lo, hi)      # [N, N, d]
            U = It[p][:, None, :] * It[q][None, :, :]
            Wt = amp[p] * amp[q] * alpha[p][:, None] * alpha[q][None, :]
            for S in range(2 * d + 1):
                if S < d:                                        # {j}: Q in dimension j, u elsewhere
                    F = U.copy()
                    F[:, :, S] = Q[:, :, S]
                elif S < 2 * d:                                  # all \ {j}: u in dimension j, Q elsewhere
                    F = Q.copy()
                    F[:, :, S - d] = U[:, :, S - d]
                else:
                    F = Q
                t = F.prod(axis=2)
                H[p, q, S] = H[q, p, S] = (Wt * t).sum()
                UH[p, q, S] = UH[q, p, S] = (np.abs(Wt) * t).sum()
    return e, H, Ue, UH


def observables(e, H, Ue, UH, A, mu):
    """mean [M], V [M, 2d + 1] (V_S in the slots of H) and its unit bound UV through f_m = mu_m + sum_p A_pm m_p"""
    A = np.asarray(A, dtype=np.float64)
    mean = mu + A.T @ e
    V = np.einsum("pm,qm,pqs->ms", A, A, H - (e[:, None] * e[None, :])[:, :, None])
    UV = np.einsum("pm,qm,pqs->ms", np.abs(A), np.abs(A), UH + (Ue[:, None] * Ue[None, :])[:, :, None])
    return mean, V, UV


def indices(V):
    """first [M, d], total [M, d] from V [M, 2d + 1]"""
    d = (V.shape[1] - 1) // 2
    return V[:, :d] / V[:, 2 * d:], 1.0 - V[:, d:2 * d] / V[:, 2 * d:]


def index_bars(V, BV):
    """the bar BV [M, 2d + 1] on V_S propagated to the indices: (B_S + index B_all) / V; for the total index, whose V-ratio is
    1 - T_j, that ratio takes the place of the index"""
    d = (V.shape[1] - 1) // 2
    Vall, Ball = V[:, 2 * d:], BV[:, 2 * d:]
    return (BV[:, :d] + np.abs(V[:, :d] / Vall) * Ball) / Vall, (BV[:, d:2 * d] + np.abs(V[:, d:2 * d] / Vall) * Ball) / Vall


def main_effect(X, alpha, amp, ell, lo, hi, j, t, A, mu):
    """curve [G, M] = E[f_m | x_j = t_g]"""
    X, alpha, amp, ell, lo, hi, t = (np.asarray(v, dtype=np.float64) for v in (X, alpha, amp, ell, lo, hi, t))
    It = itable(X, ell, lo, hi)
    It[:, :, j] = 1.0
    Ej = It.prod(axis=2)                                         # [P, N]
    k = np.exp(-(t[None, :, None] - X[None, None, :, j]) ** 2 / (2.0 * ell[:, None, None, j] ** 2))          # [P, G, N]
    z = amp[:, None] * np.einsum("pgn,pn->pg", k, alpha * Ej)
    return mu[None, :] + z.T @ np.asarray(A, dtype=np.float64)


def gp_mean(Xs, X, alpha, amp, ell):
    """m_p(x) at the rows Xs: [W, P]"""
    out = np.empty((Xs.shape[0], alpha.shape[0]))
    for p in range(alpha.shape[0]):
        r2 = (((Xs[:, None, :] - X[None, :, :]) / ell[p]) ** 2).sum(axis=2)
        out[:, p] = amp[p] * np.exp(-0.5 * r2) @ alpha[p]
    return out


# ---------------------------------------------------------------------------- data and hyper-parameters of the tests
LO, HI = -0.05, 1.1             # the box per dimension: not the unit cube, wider than the design
ALPHA = 0.1                     # GPR's alpha
CAP = 1e7                       # every case keeps U_S / V below this, so that the bar is a statement about the indices


def make_case(N, d, P, seed, small_l0=False):
    """X = lhs(N, d, seed), z_p = sin(X w_p) + 0.1 eps; theta [P, d + 2] with l in [0.5, 3] w, c in [0.5, 2], sigma_n^2 = 0.05
    (small_l0: l = 0.01 w in dimension 0, where the Q factors of distant pairs underflow); the box lo, hi [d]"""
    X = synth.lhs(N, d, seed)
    rng = np.random.default_rng(seed + 1000)
    Z = np.sin(X @ rng.standard_normal((d, P))) + 0.1 * rng.standard_normal((N, P))
    w = HI - LO
    ell = rng.uniform(0.5, 3.0, size=(P, d)) * w
    if small_l0:
        ell[:, 0] = 0.01 * w
    amp = rng.uniform(0.5, 2.0, size=P)
    theta = np.concatenate([np.log(amp)[:, None], np.log(ell), np.full((P, 1), np.log(0.05))], axis=1)
    return X, np.ascontiguousarray(Z.T), theta, np.full(d, LO), np.full(d, HI)


def host_alpha(X, Z, theta, alpha_reg=ALPHA):
    """alpha [P, N] = (K + (sigma_n^2 + alpha_reg) I)^-1 z on the host (the CPU tests; the GPU tests take the device's own)"""
    N, d = X.shape
    out = np.empty_like(Z)
    for p in range(Z.shape[0]):
        amp, ell, nz = np.exp(theta[p, 0]), np.exp(theta[p, 1:d + 1]), np.exp(theta[p, d + 1])
        r2 = (((X[:, None, :] - X[None, :, :]) / ell) ** 2).sum(axis=2)
        K = amp * np.exp(-0.5 * r2) + (nz + alpha_reg) * np.eye(N)
        out[p] = np.linalg.solve(K, Z[p])
    return out
