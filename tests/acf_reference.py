"""Host model of the chain diagnostics (a helper module, not a test file): a numpy restatement of emcee's autocorr.function_1d,
auto_window and integrated_time (emcee 3.1: the FFT zero-padded to 2 next_pow_two(n), the walker average of acf / acf[0],
taus = 2 cumsum(f) - 1, the first m with m >= c taus[m]) with the library's two deviations as switches, split-R-hat in
long double, a long-double direct-sum autocorrelation function, and the AR(1) chains the tests run on."""
import functools

import numpy as np

NO_WINDOW = 1 << 30

# (nsteps, nwalkers, ndim) of the GPU tests: exactly one 64 x 64 tile and one K-step of 16 walkers; one past both; two walkers;
# a few blocks; an 11-block band
SHAPES = ((64, 16, 1), (65, 17, 2), (130, 2, 3), (300, 6, 3), (700, 34, 3))
PHIS = (0.5, 0.8, 0.3)                     # AR(1) coefficient of parameter j: tau = (1 + phi) / (1 - phi) = 3, 9, 1.86
BAND_LAGS = (0, 63, 64, 65, 127, 699)      # max_lag at the band's edges for the last shape
C = 5.0


def next_pow_two(n):
    i = 1
    while i < n:
        i = i << 1
    return i


def function_1d(x):
    """emcee.autocorr.function_1d: the normalised autocorrelation function of a 1-D series, raw lag sums by FFT"""
    x = np.atleast_1d(x)
    if len(x.shape) != 1:
        raise ValueError("invalid dimensions for 1D autocorrelation function")
    n = next_pow_two(len(x))
    f = np.fft.fft(x - np.mean(x), n=2 * n)
    acf = np.fft.ifft(f * np.conjugate(f))[: len(x)].real
    acf /= acf[0]
    return acf


def function_1d_direct(x):
    """the same by direct sums in long double"""
    y = np.asarray(x, dtype=np.longdouble)
    y = y - y.sum() / len(y)
    acf = np.array([np.sum(y[: len(y) - k] * y[k:]) for k in range(len(y))], dtype=np.longdouble)
    return acf / acf[0]


def auto_window(taus, c, emcee_argmin_quirk=False):
    """emcee.autocorr.auto_window.  The quirk: when every m is still inside (m < c taus[m] throughout) emcee's np.argmin over the
    all-True mask returns 0; the library (quirk off) returns the last index, as emcee does when NO m is inside."""
    m = np.arange(len(taus)) < c * taus
    if np.any(m):
        if not emcee_argmin_quirk and np.all(m):
            return len(taus) - 1
        return int(np.argmin(m))
    return len(taus) - 1


def walker_mean_acf(x, skip_constant=True, acf=function_1d):
    """f [n_t, n_d]: the mean over the walkers of their normalised autocorrelation functions, x [n_t, n_w, n_d].
    skip_constant (the library's deviation): walkers that never moved are left out (emcee: 0 / 0 = NaN for the parameter);
    n_const [n_d] counts them."""
    n_t, n_w, n_d = x.shape
    f = np.zeros((n_t, n_d))
    n_const = np.zeros(n_d, dtype=np.int64)
    for d in range(n_d):
        used = 0
        for k in range(n_w):
            s = x[:, k, d]
            if skip_constant and np.all(s == s[0]):
                n_const[d] += 1
                continue
            with np.errstate(invalid="ignore", divide="ignore"):
                f[:, d] += np.asarray(acf(s), dtype=np.float64)
            used += 1
        f[:, d] = f[:, d] / used if used else np.nan
    return f, n_const


def integrated_time(x, c=5, skip_constant=True, emcee_argmin_quirk=False, max_lag=None):
    """emcee.autocorr.integrated_time on x [n_t, n_w, n_d] without its tol check -> dict(rho [n_d, L + 1], tau, window, taus,
    nconst).  max_lag = L (default n_t - 1) restricts the window search to lags <= L as gpb_mcmc_diag does: no window inside
    gives window = L with bit 30 set (emcee, quirk aside: L) and tau = taus[L]."""
    x = np.asarray(x, dtype=np.float64)
    n_t, n_w, n_d = x.shape
    L = n_t - 1 if max_lag is None else int(max_lag)
    f, n_const = walker_mean_acf(x, skip_constant)
    tau, window, taus_all = np.empty(n_d), np.empty(n_d, dtype=np.int64), []
    for d in range(n_d):
        taus = 2.0 * np.cumsum(f[: L + 1, d]) - 1.0
        taus_all.append(taus)
        if n_const[d] == n_w:
            tau[d], window[d] = np.nan, -1
            continue
        inside = np.arange(len(taus)) < c * taus
        if np.all(inside):
            window[d] = L | NO_WINDOW
            tau[d] = taus[L]
        else:
            w = auto_window(taus, c, emcee_argmin_quirk)
            window[d], tau[d] = w, taus[w]
    return dict(rho=np.ascontiguousarray(f[: L + 1].T), tau=tau, window=window, taus=taus_all, nconst=n_const)


def window_margin(taus, window, c):
    """the least |m - c taus[m]| over m <= window + 2: how far every decision of the window search is from flipping"""
    m = np.arange(min(int(window) + 3, len(taus)))
    return float(np.min(np.abs(m - c * taus[: len(m)])))


def split_rhat(x):
    """x [n_t, n_w, n_d] -> (moments [n_d, 3] = grand mean | W | B, rhat [n_d]) in long double: halves of h = n_t // 2 draws (the
    middle draw of an odd n_t dropped), W the mean of the 2 n_w sample variances, B = h var(means, ddof=1) — BDA3 (11.1)-(11.4)"""
    x = np.asarray(x, dtype=np.longdouble)
    n_t = x.shape[0]
    h = n_t // 2
    halves = np.concatenate([x[:h], x[n_t - h:]], axis=1)              # [h, 2 n_w, n_d]
    means = halves.mean(axis=0)
    W = halves.var(axis=0, ddof=1).mean(axis=0)
    B = h * means.var(axis=0, ddof=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        rhat = np.sqrt(((h - 1) / np.longdouble(h) * W + B / h) / W)
    return np.stack([x.mean(axis=(0, 1)), W, B], axis=1), rhat


@functools.lru_cache(maxsize=None)
def ar1_chain(n_t, n_w, n_d, seed=0, phis=PHIS):
    """[n_t, n_w, n_d] stationary AR(1) series of unit variance, parameter j with coefficient phis[j % len]; parameter 1 carries
    an offset of 1e3 and a per-walker shift (standard normal): centring has something to remove.  Read-only (shared)."""
    rng = np.random.default_rng([seed, n_t, n_w, n_d])
    x = np.empty((n_t, n_w, n_d))
    for j in range(n_d):
        phi = phis[j % len(phis)]
        e = rng.standard_normal((n_t, n_w))
        x[0, :, j] = e[0]
        for t in range(1, n_t):
            x[t, :, j] = phi * x[t - 1, :, j] + np.sqrt(1.0 - phi * phi) * e[t]
    if n_d > 1:
        x[:, :, 1] += 1e3 + rng.standard_normal(n_w)[None, :]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(n_t, n_w, n_d, max_lag=None, c=C):
    """the model's answer for ar1_chain(n_t, n_w, n_d), computed once"""
    x = ar1_chain(n_t, n_w, n_d)
    out = integrated_time(x, c, max_lag=max_lag)
    out["moments"], out["rhat"] = split_rhat(x)
    return out


def gpu_inputs():
    """every (shape, max_lag) the GPU tests compare against the model"""
    cases = [(s, None) for s in SHAPES]
    cases += [(SHAPES[-1], L) for L in BAND_LAGS]
    return cases
