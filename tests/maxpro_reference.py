"""Host model of the MaxPro Latin-hypercube generator (gpb_maxpro_lhd, gpb_maxpro_criterion, gpb_maxpro_run_order; DESIGN.md
section 24) in numpy, fp64.  It restates csrc/maxpro_index.h (the scale of a pair term, ln psi, the decoding of a proposal) and
follows csrc/gpb_maxpro.hip decision for decision: the pair matrix holds the same bits as the device's (every entry is a chain of
IEEE multiplications and divisions), only the order of the sums differs.  For every decision it records the margin by which it
was taken, so that a test can show its cases to be far from rounding before it compares them with the device."""
import math

import numpy as np

from oracle.stretch_oracle import philox4x32_10

E15 = 4.4816890703380645           # e^1.5 (MP_E15)
TAG = 11                           # MP_TAG
BEST_EPS = 1e-10                   # MP_BEST_EPS
MIN_N, MAX_N, MIN_D, MAX_D, MAX_R, MAX_BLOCK = 4, 4096, 2, 64, 16, 64


def scale(n):
    return E15 / float(n)


def lnpsi_from_f(f, n, d):
    """mp_lnpsi: ln psi = (f + 3 d - ln(n (n - 1) / 2)) / d"""
    pairs = 0.5 * float(n) * float(n - 1)
    return (f + 3.0 * float(d) - math.log(pairs)) / float(d)


def pair_matrix(cols, s):
    """T [n, n] of the columns `cols` [n, d] (integer levels or reals): t_ij = 1 / prod_c (s (c_i - c_j))^2 in column order, 0 on
    the diagonal — k_mp_build's arithmetic"""
    cols = np.asarray(cols)
    n, d = cols.shape
    p = np.ones((n, n))
    for c in range(d):
        q = s * (cols[:, None, c] - cols[None, :, c]).astype(np.float64)
        p = p * (q * q)
    np.fill_diagonal(p, 1.0)
    with np.errstate(divide="ignore", over="ignore"):
        T = 1.0 / p
    np.fill_diagonal(T, 0.0)
    return T


def pair_sum(T):
    """sum over i < j, exactly rounded (math.fsum): the yardstick of the device's sums"""
    return math.fsum(T[np.triu_indices(T.shape[0], 1)])


def levels_sum(levels):
    levels = np.asarray(levels, dtype=np.int64)
    return pair_sum(pair_matrix(levels, scale(levels.shape[0])))


def design_of(levels):
    levels = np.asarray(levels)
    return (levels + 0.5) / levels.shape[0]


def design_sum(X):
    """the sum of the pair terms prod_c (e^1.5 (x_ic - x_jc))^-2 of a real design (inf when two rows share a coordinate)"""
    return pair_sum(pair_matrix(np.asarray(X, dtype=np.float64), E15))


def lnpsi(X):
    X = np.asarray(X, dtype=np.float64)
    s = design_sum(X)
    return lnpsi_from_f(math.log(s) if np.isfinite(s) else np.inf, *X.shape)


def lnpsi_bruteforce(X):
    """the criterion as the paper writes it, with no scale: ln of (mean_{i<j} prod_c (x_ic - x_jc)^-2)^(1/d)"""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    iu = np.triu_indices(n, 1)
    logs = -2.0 * np.log(np.abs(X[iu[0]] - X[iu[1]])).sum(axis=1)
    m = logs.max()
    return (m + math.log(math.fsum(np.exp(logs - m))) - math.log(len(iu[0]))) / d


def decode(x, y, z, w, n, d):
    """mp_decode on arrays of the four Philox words: (column, a, b != a, u in (0, 1))"""
    x, y, z, w = (np.asarray(v, dtype=np.uint64) for v in (x, y, z, w))
    c = (x * np.uint64(d)) >> np.uint64(32)
    a = (y * np.uint64(n)) >> np.uint64(32)
    b0 = (z * np.uint64(n - 1)) >> np.uint64(32)
    b = b0 + (b0 >= a).astype(np.uint64)
    u = (w.astype(np.float64) + 0.5) * (1.0 / 4294967296.0)
    return c.astype(np.int64), a.astype(np.int64), b.astype(np.int64), u


def proposals(seed, gblock, restart, B, n, d):
    """the B proposals of a block: the counter (global block index, restart, slot, TAG)"""
    seed = int(seed)
    w = philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), (gblock, restart, np.arange(B), TAG))
    return decode(*w, n, d)


def random_starts(seed, R, n, d):
    """the starts of the Python layer: np.random.default_rng(seed), one permutation per column per restart"""
    rng = np.random.default_rng(seed)
    out = np.empty((R, n, d), dtype=np.int32)
    for r in range(R):
        for c in range(d):
            out[r, :, c] = rng.permutation(n)
    return out


def _ratios(la, lb, lj):
    qa, qb = (la - lj).astype(np.float64), (lb - lj).astype(np.float64)
    fa, fb = qa / qb, qb / qa
    return fa * fa, fb * fb


def anneal(levels, seed, restart, n_stages, blocks_per_stage, B, temp0, cool, check=None):
    """One restart of gpb_maxpro_lhd from `levels` [n, d].  Returns a dict: levels (the best seen), f_start, f_best (recomputed
    from them), accepted, consumed, trace [n_stages blocks_per_stage], margin (the smallest acceptance margin
    |ln u + df / temp| / max(1, |ln u|, |df / temp|) over every decision taken), best_margin (how near the
    relative gain (S_best - S) / S_best of an accepted state came to BEST_EPS, the gain that makes it the new best).  check(T, S, lev): called
    after every accepted swap (the self-tests compare the ratio update with a recomputation there)."""
    lev = np.array(levels, dtype=np.int64)
    n, d = lev.shape
    s = scale(n)
    T = pair_matrix(lev, s)
    S = pair_sum(T)
    if not (np.isfinite(S) and S > 0.0):
        raise ValueError("the objective of the start is not finite")
    S_start = S_best = S
    best = lev.copy()
    trace = np.full(n_stages * blocks_per_stage, -1, dtype=np.int32)
    accepted = consumed = 0
    margin = best_margin = np.inf
    others = np.ones(n, dtype=bool)
    for k in range(n_stages):
        temp = temp0 * math.pow(cool, float(k))
        if k > 0:
            T = pair_matrix(lev, s)
            S = pair_sum(T)
        for kb in range(blocks_per_stage):
            gb = k * blocks_per_stage + kb
            pc, pa, pb, pu = proposals(seed, gb, restart, B, n, d)
            pick = -1
            for slot in range(B):
                c, a, b = int(pc[slot]), int(pa[slot]), int(pb[slot])
                others[:] = True
                others[[a, b]] = False
                ra, rb = _ratios(lev[a, c], lev[b, c], lev[others, c])
                delta = math.fsum(T[a, others] * (ra - 1.0) + T[b, others] * (rb - 1.0))
                with np.errstate(invalid="ignore", divide="ignore"):
                    df = float(np.log1p(np.float64(delta) / S))
                lnu = math.log(pu[slot])
                rhs = -df / temp
                margin = min(margin, abs(lnu - rhs) / max(1.0, abs(lnu), abs(rhs)))
                if lnu < rhs:
                    pick = slot
                    break
            trace[gb] = pick
            if pick < 0:
                consumed += B
                continue
            accepted += 1
            consumed += pick + 1
            ta, tb = T[a, others] * ra, T[b, others] * rb
            T[a, others] = T[others, a] = ta
            T[b, others] = T[others, b] = tb
            lev[a, c], lev[b, c] = lev[b, c], lev[a, c]
            S = S + delta
            best_margin = min(best_margin, abs((S_best - S) / S_best - BEST_EPS))
            if S < S_best * (1.0 - BEST_EPS):
                S_best = S
                best = lev.copy()
            if check is not None:
                check(T, S, lev)
    return dict(levels=best.astype(np.int32), f_start=math.log(S_start), f_best=math.log(levels_sum(best)), accepted=accepted,
                consumed=consumed, trace=trace, margin=margin, best_margin=best_margin)


def sequential_anneal(levels, seed, restart, n_steps, temp, tag_block=lambda t: t):
    """textbook sequential annealing at one temperature on the draws of slot 0 of the blocks 0 .. n_steps - 1, every proposal
    evaluated by recomputing the whole objective: what anneal(B = 1) must equal.  Returns (levels, accept flags)."""
    lev = np.array(levels, dtype=np.int64)
    n, d = lev.shape
    S = levels_sum(lev)
    flags = np.zeros(n_steps, dtype=bool)
    for t in range(n_steps):
        pc, pa, pb, pu = proposals(seed, tag_block(t), restart, 1, n, d)
        c, a, b = int(pc[0]), int(pa[0]), int(pb[0])
        new = lev.copy()
        new[a, c], new[b, c] = lev[b, c], lev[a, c]
        S_new = levels_sum(new)
        if math.log(pu[0]) < -(math.log(S_new) - math.log(S)) / temp:
            lev, S, flags[t] = new, S_new, True
    return lev, flags


def centre_row(X):
    """the row nearest the cube's centre, the lowest index at a tie; the squared distance summed in column order"""
    X = np.asarray(X, dtype=np.float64)
    a = np.zeros(X.shape[0])
    for c in range(X.shape[1]):
        v = X[:, c] - 0.5
        a = a + v * v
    return int(np.argmin(a))


def run_order(X, first=-1):
    """gpb_maxpro_run_order: (order [n], margin) — row `first` (-1: centre_row), then again and again the row with the smallest sum
    of its pair terms with the rows chosen so far, the lowest index at a tie; margin: the smallest relative gap between the best
    and the second-best score over all steps (0 at an exact tie)."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    T = pair_matrix(X, E15)
    pick = centre_row(X) if first < 0 else int(first)
    order = [pick]
    used = np.zeros(n, dtype=bool)
    score = np.zeros(n)
    margin = np.inf
    for _ in range(n - 1):
        used[pick] = True
        score = score + T[pick]
        sc = np.where(used, np.inf, score)
        pick = int(np.argmin(sc))
        if n - len(order) >= 2:
            two = np.partition(sc, 1)[:2]
            if np.isfinite(two[1]):
                margin = min(margin, (two[1] - two[0]) / two[1])
            else:
                margin = min(margin, 0.0 if not np.isfinite(two[0]) else np.inf)
        order.append(pick)
    return np.array(order, dtype=np.int32), margin


# ---------------------------------------------------------------------------------------------------------------- shared cases
# The trajectory cases of tests/test_gpu_maxpro.py: name -> (n, d, R, B, n_stages, blocks_per_stage, temp0, cool, seed).  The seeds
# were searched on the host so that the smallest acceptance margin of every restart is >= MIN_MARGIN and (for the first five) the
# trace holds a wholly rejected block, an accept in the last slot and an accept in slot 0; tests/test_maxpro_reference.py and
# the GPU test both assert that before anything is compared.
MIN_MARGIN = 1e-8
MIN_BEST_MARGIN = 1e-11            # the device's sums carry about 1e-13
CASES = {
    "n7_d2_B1": (7, 2, 1, 1, 3, 40, 0.1, 0.5, 1),
    "n65_d3_R2_B5": (65, 3, 2, 5, 4, 33, 0.1, 0.5, 1),
    "n130_d20_R3_B32": (130, 20, 3, 32, 3, 50, 0.003, 0.5, 1),
    "n20_d64_B64": (20, 64, 1, 64, 2, 20, 0.003, 0.5, 6),
    "n1100_d4_B32": (1100, 4, 1, 32, 2, 25, 0.003, 0.5, 3),
    "hot": (33, 5, 2, 8, 2, 30, 1e6, 0.5, 1),
    "cold": (33, 5, 2, 8, 2, 30, 1e-9, 0.5, 1),
}
PATH_CASES = ("n7_d2_B1", "n65_d3_R2_B5", "n130_d20_R3_B32", "n20_d64_B64", "n1100_d4_B32")
GOLDEN_STARTS = ("n130_d20_R3_B32", "n20_d64_B64", "n1100_d4_B32")
_case_cache = {}


def case_starts(name):
    """random hypercubes; for the three large cases the pre-annealed ones of tests/golden/g14_maxpro_starts.npz
    (tools/make_maxpro_starts.py): from a random start nearly every proposal is accepted, and no block is ever rejected"""
    n, d, R = CASES[name][:3]
    if name in GOLDEN_STARTS:
        import os
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_maxpro_starts.npz")) as z:
            return z[name].astype(np.int32)
    return random_starts(CASES[name][8] + 1000, R, n, d)


def case_reference(name):
    """the host model's result for every restart of a case (computed once, shared, not to be changed by a test)"""
    if name not in _case_cache:
        n, d, R, B, ns, bps, temp0, cool, seed = CASES[name]
        init = case_starts(name)
        _case_cache[name] = [anneal(init[r], seed, r, ns, bps, B, temp0, cool) for r in range(R)]
    return _case_cache[name]


def trace_paths(name):
    """(a wholly rejected block, an accept in the last slot, an accept in slot 0) over the restarts of a case"""
    B = CASES[name][3]
    tr = np.concatenate([m["trace"] for m in case_reference(name)])
    return bool(np.any(tr == -1)), bool(np.any(tr == B - 1)), bool(np.any(tr == 0))


# rows 0 / 2, 3 / 4 and 5 / 6 mirror one another about row 1, the centre; sixteenths, so every difference is exact and the mirror
# rows tie exactly in the run order from row 1
TIE_DESIGN = np.array([[3, 6], [8, 8], [13, 10], [5, 2], [11, 14], [1, 13], [15, 3]]) / 16.0
