"""Inputs for the tests of the padded input widths (a helper module, not a test file; host only: numpy and synth).

Every kernel that forms a scaled distance is instantiated or sized on the padded input width dpad that pick_dpad
(csrc/dispatch.h) takes from WIDTHS.  DS holds two input counts per width: d == width (no padding column; k_lml_grad's noise
slot tid == DPAD + 1 is then d + 1) and d == previous width + 1 (the most padding columns).

make_case(d, kind, seed) is one emulator of three GPs over N = 130 design points (Np = 192: 48 padding rows in front, 14 behind)
whose GPs 0 and 2 have length scales proportional to sqrt(d) — r^2 of order 1 at every width, S = sum (ptp / l)^2 of order 1: the
Gram form — and whose GP 1 has, in the LAST real input column d - 1, a length scale of 2e-3 x the extent (S ~ 2.5e5 > 1024: the
difference form, as in test_gpu_edges.py::test_gps_of_one_emulator_in_different_distance_forms), so that every engine call launches
both instantiations of its width and a dropped or mis-padded last column is seen by all of K, K*, the mean and the LML gradient.
The W = 130 queries (Wuse = 256: two walkers per lane where dpad <= 32; the first 70 alone: Wuse = 128, one per lane) sit within
1e-3 of design points, the first eight exactly on them."""
import numpy as np

from gpbayestools_hic_amd import synth

WIDTHS = (8, 16, 20, 24, 32, 48, 64)
DS = tuple(sorted({w for w in WIDTHS} | {p + 1 for p in (0,) + WIDTHS[:-1]}))
KINDS = ("RBF", "Matern15", "Matern25")

N, P, W = 130, 3, 130
W_ONE_PER_LANE = 70                 # rows 0:70 alone pad to 128 walkers
NOISE = 0.05
ALPHA = 0.1                         # GPR's alpha
AMPS = (0.8, 1.0, 1.3)              # near 1, in two binades (the column scale of the int8 planes: e_c = 0, 1, 1)
ELL = (0.6, 0.6, 0.9)               # x sqrt(d) x extent
SHORT = 2e-3                        # x extent, GP 1, column d - 1
GRAM_LIMIT = 1024.0                 # S above this: the difference form (gpb_internal.h gram_limit)
ON_DESIGN = 8                       # queries exactly on design points
FORMS = [0, 1, 0]


# the widths no test ran before (24, 32) and the widest (48, 64), with and without padding columns: prediction gradients and Sobol
WIDE_DS = (21, 24, 25, 32, 49, 64)
# Sobol (RBF only): d -> (N, d, P, seed) of sobol_reference.make_case with its own length scales (0.5 to 3 box widths), for which
# U_S / V stays below sobol_reference.CAP at every d here (test_width_cases.py); N = 65: a second row block of one row
SOBOL_CASES = {d: (64 + (i % 2), d, 2, d) for i, d in enumerate(WIDE_DS)}
# the shared chain launch: three emulators whose designs all pad to Np = 128
CHAIN_DS = (21, 24, 32, 64)
CHAIN_SPECS = [(72, 10, 3, "RBF"), (100, 6, 2, "Matern25"), (120, 5, 2, "Matern15")]


def dpad_of(d):
    return next(w for w in WIDTHS if d <= w)


def length_scales(d, ptp):
    ls = np.array([e * np.sqrt(d) * ptp for e in ELL])
    ls[1, d - 1] = SHORT * ptp[d - 1]
    return ls


def form_sums(X, theta):
    """S_p = sum_k (ptp_k / l_pk)^2: the quantity the engine's rule compares with GRAM_LIMIT"""
    d = X.shape[1]
    ptp = X.max(0) - X.min(0)
    return np.sum((ptp[None, :] / np.exp(theta[:, 1:1 + d])) ** 2, axis=1)


def make_case(d, kind="RBF", seed=0):
    """X [N, d], Z [P, N], theta [P, d + 2], Xs [W, d].  `kind` only enters the seed: every kernel family gets its own draw."""
    s = 1000 * d + 10 * KINDS.index(kind) + seed
    rng = np.random.default_rng(s)
    X = synth.lhs(N, d, seed=s + 1)
    ptp = X.max(0) - X.min(0)
    ls = length_scales(d, ptp)
    # targets that vary along every input, the last column included, at about the GPs' own length scale
    w = rng.standard_normal((d, P)) * (2.0 / np.sqrt(d))
    w[d - 1] = (3.0, 3.0, -3.0)
    Z = (np.sin(X @ w) + 0.1 * rng.standard_normal((N, P))).T
    theta = np.concatenate([np.log(AMPS)[:, None], np.log(ls), np.full((P, 1), np.log(NOISE))], axis=1)
    idx = rng.permutation(N)[:W] if W <= N else rng.integers(0, N, W)
    Xs = np.clip(X[idx] + rng.uniform(-1e-3, 1e-3, (W, d)), 0.0, 1.0)
    Xs[:ON_DESIGN] = X[idx[:ON_DESIGN]]
    return X, np.ascontiguousarray(Z), theta, Xs


def without_last_column(A):
    """the same rows with input column d - 1 held at zero: to every distance what leaving the column out is"""
    B = np.array(A, dtype=np.float64, copy=True)
    B[:, -1] = 0.0
    return B
