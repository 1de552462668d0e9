"""Host model of the variance-reduction sequential design (a helper module, not a test file): numpy + scipy.

For GP p with amplitude c, kernel k (RBF, Matern-3/2, Matern-5/2 over the scaled distance), tau = sigma_n^2 + alpha and
Ky = c k(X, X) + tau I = L L^T:
    v(a)    = L^-1 c k(X, a)
    s(a, b) = c k(a, b) - v(a)^T v(b)                      posterior covariance of the latent function (no White term)
A run at x, observed with noise tau, gives  s'(a, b) = s(a, b) - s(a, x) s(x, b) / (s(x, x) + tau), and lowers the averaged
variance  sum_p g_p sum_r w_r s_p(r, r)  by
    J(x) = sum_p g_p [sum_r w_r s_p(r, x)^2] / (s_p(x, x) + tau_p).
greedy() runs the loop by these rank-one formulas on the full matrices (S_rc and S_cc: the host can afford [C, C]);
refit_scores() is the brute force: append the candidate to the design, take a fresh Cholesky, difference the averaged variance."""
import numpy as np
from scipy.linalg import cholesky, solve_triangular

KINDS = ("RBF", "Matern", "Matern25")       # the engine's kernel names: Matern = nu 3/2
ALPHA = 0.01                                # GPR's alpha


def shape(r2, kind):
    if kind == "RBF":
        return np.exp(-0.5 * r2)
    r = np.sqrt(r2)
    if kind == "Matern":
        t = np.sqrt(3.0) * r
        return (1.0 + t) * np.exp(-t)
    t = np.sqrt(5.0) * r
    return (1.0 + t + t * t / 3.0) * np.exp(-t)


def kern(A, B, ell, kind):
    """k(A, B) [len(A), len(B)] in the difference form"""
    df = A[:, None, :] / ell - B[None, :, :] / ell
    return shape((df * df).sum(axis=2), kind)


def unpack(theta_p, d):
    """(c, l [d], sigma_n^2) of one row of theta = [log c, log l_1..l_d, log sigma_n^2]"""
    return np.exp(theta_p[0]), np.exp(theta_p[1:d + 1]), np.exp(theta_p[d + 1])


def posterior_cov(X, theta_p, kind, A, B, alpha_reg=ALPHA):
    """s(A, B) [len(A), len(B)] of one GP and its tau"""
    c, ell, nz = unpack(theta_p, X.shape[1])
    tau = nz + alpha_reg
    L = cholesky(c * kern(X, X, ell, kind) + tau * np.eye(X.shape[0]), lower=True)
    vA = solve_triangular(L, c * kern(X, A, ell, kind), lower=True)
    vB = vA if B is A else solve_triangular(L, c * kern(X, B, ell, kind), lower=True)
    return c * kern(A, B, ell, kind) - vA.T @ vB, tau


def averaged_variance(X, theta, kind, Xr, w, g, alpha_reg=ALPHA):
    """sum_p g_p sum_r w_r s_p(r, r)"""
    return float(sum(g[p] * (w @ np.diag(posterior_cov(X, theta[p], kind, Xr, Xr, alpha_reg)[0])) for p in range(theta.shape[0])))


def scores_of(S_rc, s_cc, tau, w, g):
    """J [C] from the per-GP lists S_rc [R, C], s_cc [C]"""
    J = np.zeros(S_rc[0].shape[1])
    for p in range(len(S_rc)):
        J += g[p] * ((w @ S_rc[p] ** 2) / (s_cc[p] + tau[p]))
    return J


def greedy(X, theta, kind, Xc, Xr, w, g, T, eligible=None, alpha_reg=ALPHA):
    """The greedy loop by the rank-one formulas.  Returns dict(picks [T], gain [T], scores [T, C] (-inf where ineligible),
    gaps [T] = (best - second best) / best over the eligible candidates of each step (inf with one left), variance0)."""
    P, C = theta.shape[0], Xc.shape[0]
    S_rc, S_cc, tau = [], [], []
    for p in range(P):
        s, t = posterior_cov(X, theta[p], kind, Xr, Xc, alpha_reg)
        S_rc.append(s)
        S_cc.append(posterior_cov(X, theta[p], kind, Xc, Xc, alpha_reg)[0])
        tau.append(t)
    el = np.ones(C, dtype=bool) if eligible is None else np.asarray(eligible, dtype=bool).copy()
    picks, gain, scores, gaps = np.empty(T, dtype=np.int64), np.empty(T), np.empty((T, C)), np.empty(T)
    for t in range(T):
        J = scores_of(S_rc, [np.diag(s).copy() for s in S_cc], tau, w, g)
        row = np.where(el, J, -np.inf)
        scores[t] = row
        order = np.sort(row[el])[::-1]
        gaps[t] = (order[0] - order[1]) / order[0] if order.shape[0] > 1 else np.inf
        b = int(np.argmax(row))
        picks[t], gain[t] = b, row[b]
        el[b] = False
        for p in range(P):
            den = S_cc[p][b, b] + tau[p]
            S_rc[p] = S_rc[p] - np.outer(S_rc[p][:, b], S_cc[p][b, :]) / den
            S_cc[p] = S_cc[p] - np.outer(S_cc[p][:, b], S_cc[p][b, :]) / den
    return dict(picks=picks, gain=gain, scores=scores, gaps=gaps, variance0=averaged_variance(X, theta, kind, Xr, w, g, alpha_reg))


def refit_scores(X, theta, kind, Xc, Xr, w, g, chosen, alpha_reg=ALPHA):
    """Brute force: (J [C], base) with base the averaged variance of the design X + Xc[chosen] and J[c] = base - that of the
    design with candidate c appended as well, by a fresh Cholesky each (every candidate, chosen ones included)."""
    Xd = np.concatenate([X, Xc[list(chosen)]], axis=0) if len(chosen) else X
    base = averaged_variance(Xd, theta, kind, Xr, w, g, alpha_reg)
    J = np.array([base - averaged_variance(np.concatenate([Xd, Xc[c:c + 1]], axis=0), theta, kind, Xr, w, g, alpha_reg)
                  for c in range(Xc.shape[0])])
    return J, base


def make_case(N, d, P, C, R, seed, kernel="RBF", ell0=0.6):
    """Uniform-random design, candidates and reference points in the unit cube; theta [P, d + 2] with l = ell0 e^(+-0.4), c in
    [0.5, 2], sigma_n^2 = 0.05; weights w [R] (sum 1) and g [P] in [0.5, 2]; Z [P, N] only so that an engine can be fitted (the
    design never reads it).  Returns dict(X, Z, theta, Xc, Xr, w, g, kernel)."""
    assert kernel in KINDS
    rng = np.random.default_rng(seed)
    X, Xc, Xr = rng.uniform(size=(N, d)), rng.uniform(size=(C, d)), rng.uniform(size=(R, d))
    ell = ell0 * np.exp(rng.uniform(-0.4, 0.4, size=(P, d)))
    amp = rng.uniform(0.5, 2.0, size=P)
    theta = np.concatenate([np.log(amp)[:, None], np.log(ell), np.full((P, 1), np.log(0.05))], axis=1)
    w = rng.uniform(0.2, 1.0, size=R)
    Z = np.sin(X @ rng.standard_normal((d, P))).T + 0.1 * rng.standard_normal((P, N))
    return dict(X=X, Z=np.ascontiguousarray(Z), theta=theta, Xc=Xc, Xr=Xr, w=w / w.sum(), g=rng.uniform(0.5, 2.0, size=P),
                kernel=kernel)
