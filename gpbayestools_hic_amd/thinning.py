"""
Stein thinning and the kernel Stein discrepancy of a chain, on the device (gpb_stein_thin, gpb_stein_ksd).

Two questions the chain's own diagnostics cannot answer.  How well does a point set represent the posterior — R-hat and ESS
compare a chain with itself and say nothing when every walker is wrong in the same way; the kernel Stein discrepancy (Gorham &
Mackey 2017) needs only the points and the score grad log p at them and is positive for a set that does not represent the
posterior, whatever produced it.  And which few parameter sets should the full model be run at again — the reference picks
k-means centres of the most likely rows (clusters.py), which are not posterior samples; Stein thinning (Riabiz, Chen, Cockayne,
Swietach, Niederer, Mackey & Oates 2022) picks, greedily, the m rows of the chain whose empirical measure has the smallest
discrepancy: it drops burn-in by itself, corrects a biased sample (SMC particles need no weights) and returns rows of the chain.

The kernel is the inverse multiquadric k(x, y) = (1 + (x - y)^T Gamma^-1 (x - y))^(-1/2) with a preconditioner Gamma:
    "id"      the identity                       "med"     l^2 I, l the median pairwise distance of the first <= 1000 valid rows
    "sclmed"  l^2 / ln n  (n the valid rows)     "smpcov"  the sample covariance of the valid rows       "diag"  its diagonal
or an explicit symmetric positive definite [ndim, ndim] matrix.

The posterior of a calibration lives in a box with hard walls, where the Langevin Stein operator is not valid: the density does
not vanish on the boundary, so the discrepancy of a perfect sample would not be zero.  transform="logit" (the default when lo and
hi are given) therefore maps every row to z = ln((x - lo) / (hi - x)), where the density p_z(z) = p_x(x) (x - lo)(hi - x) / (hi - lo)
does vanish at infinity, with the score g_z = g_x (x - lo)(hi - x) / (hi - lo) + (hi + lo - 2 x) / (hi - lo); the preconditioner
is computed in z.  A row on a wall (or outside) becomes non-finite and is skipped and counted.  transform=None takes x as it is:
right for a density on all of R^d, and acceptable for a boxed posterior whose mass near the walls is negligible.
"""
import numpy as np

PRECONDITIONERS = ("id", "med", "sclmed", "smpcov", "diag")
MED_ROWS = 1000


def _is_torch(a):
    return hasattr(a, "data_ptr")


def logit_transform(x, g, lo, hi):
    """(z, g_z) of rows x [n, d] with scores g [n, d] in the box lo < x < hi: z = ln((x - lo) / (hi - x)), g_z = g (x - lo)
    (hi - x) / (hi - lo) + (hi + lo - 2 x) / (hi - lo) — the score of the density of z, the Jacobian included.  numpy arrays
    or torch tensors (lo, hi are brought to x's kind); a row on or outside a wall comes out non-finite."""
    if _is_torch(x):
        import torch
        lo = torch.as_tensor(np.asarray(lo, dtype=np.float64), device=x.device)
        hi = torch.as_tensor(np.asarray(hi, dtype=np.float64), device=x.device)
        log = torch.log
    else:
        x, g = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
        lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
        log = np.log
    if lo.shape != (x.shape[-1],) or hi.shape != lo.shape:
        raise ValueError("lo, hi: expected [%d]" % x.shape[-1])
    a, b, w = x - lo, hi - x, hi - lo
    if _is_torch(x):
        z = log(a / b)
    else:
        with np.errstate(all="ignore"):
            z = log(a / b)
    return z, g * a * b / w + (hi + lo - 2.0 * x) / w


def median_distance(z):
    """the median of the pairwise Euclidean distances (i < j) of the rows z [k, d] (numpy)"""
    z = np.asarray(z, dtype=np.float64)
    k = z.shape[0]
    if k < 2:
        raise ValueError("the median pairwise distance needs at least two valid rows")
    d2 = np.zeros((k, k))
    for l in range(z.shape[1]):
        t = z[:, l][:, None] - z[:, l][None, :]
        d2 += t * t
    return float(np.median(np.sqrt(d2[np.triu_indices(k, 1)])))


def preconditioner_matrix(z, kind="sclmed"):
    """Gamma [d, d] of the rows z [n, d] (numpy, the space the kernel works in); kind one of PRECONDITIONERS or an explicit
    symmetric positive definite matrix.  Rows with a non-finite entry are left out."""
    z = np.asarray(z, dtype=np.float64)
    d = z.shape[1]
    if not isinstance(kind, str):
        gam = np.array(kind, dtype=np.float64)
        if gam.shape != (d, d) or not np.all(np.isfinite(gam)) or not np.array_equal(gam, gam.T):
            raise ValueError("preconditioner: a finite symmetric [%d, %d] matrix" % (d, d))
        try:
            np.linalg.cholesky(gam)
        except np.linalg.LinAlgError:
            raise ValueError("preconditioner: the matrix is not positive definite") from None
        return gam
    if kind not in PRECONDITIONERS:
        raise ValueError("preconditioner: one of %s or a [%d, %d] matrix" % (PRECONDITIONERS, d, d))
    if kind == "id":
        return np.eye(d)
    zv = z[np.all(np.isfinite(z), axis=1)]
    n = zv.shape[0]
    if n < 2:
        raise ValueError("preconditioner %r needs at least two valid rows" % kind)
    if kind in ("med", "sclmed"):
        l2 = median_distance(zv[:MED_ROWS]) ** 2
        if kind == "sclmed":
            l2 = l2 / np.log(n)
        if not (l2 > 0.0 and np.isfinite(l2)):
            raise ValueError("preconditioner %r: the median pairwise distance is 0 (repeated rows only)" % kind)
        return l2 * np.eye(d)
    cov = np.atleast_2d(np.cov(zv, rowvar=False))
    if kind == "diag":
        cov = np.diag(np.diag(cov))
    if not np.all(np.diag(cov) > 0.0):
        raise ValueError("preconditioner %r: a parameter does not vary" % kind)
    return cov


def _gamma_inverse(gam):
    """Gamma^-1, exactly symmetric; a diagonal Gamma is inverted entry by entry"""
    if np.array_equal(gam, np.diag(np.diag(gam))):
        return np.diag(1.0 / np.diag(gam))
    inv = np.linalg.inv(gam)
    return 0.5 * (inv + inv.T)


class SteinThinning:
    """idx [m] (int32: the picked rows, numbered in the memory order of the input, outer axis first; rows may repeat; -1: no row
    could be picked), points [m, ndim] (those rows, in the chain's own units), ksd [m] (ksd[t - 1]: the kernel Stein discrepancy
    of the first t picks, in the transformed space), n_samples, n_skipped (rows that are not finite after the transform: never
    picked), gamma [ndim, ndim] (the preconditioner), transform ("logit" or None), names."""

    def __init__(self, idx, points, ksd, n_samples, n_skipped, gamma, transform=None, names=None):
        self.idx, self.points, self.ksd = idx, points, ksd
        self.n_samples, self.n_skipped = int(n_samples), int(n_skipped)
        self.gamma, self.transform = gamma, transform
        self.names = None if names is None else list(names)

    def savetxt(self, path="cluster_centers.txt"):
        """the format of the reference's cluster_centers.txt: one row per parameter, one column per point, '%.6f'"""
        np.savetxt(path, self.points.T, fmt="%.6f")

    def __repr__(self):
        m, d = self.points.shape
        names = self.names or ["p%d" % j for j in range(d)]
        wid = max([9] + [len(str(s)) for s in names])
        show = min(m, 8)
        lines = ["SteinThinning(n_samples=%d, ndim=%d, m=%d, distinct=%d, ksd=%.6g, transform=%s%s)"
                 % (self.n_samples, d, m, len(np.unique(self.idx)), self.ksd[-1] if m else float("nan"), self.transform,
                    ", skipped=%d" % self.n_skipped if self.n_skipped else ""),
                 "  %-*s %s%s" % (wid, "parameter", " ".join("%12s" % ("pick%d" % c) for c in range(show)), " ..." if m > show else ""),
                 "  %-*s %s" % (wid, "row", " ".join("%12d" % i for i in self.idx[:show]))]
        for j, nm in enumerate(names):
            lines.append("  %-*s %s" % (wid, nm, " ".join("%12.5g" % v for v in self.points[:show, j])))
        return "\n".join(lines)


class SteinDiscrepancy:
    """ksd (the kernel Stein discrepancy of all valid rows, in the transformed space), ksd2 (its square: sum_ij kp(i, j) /
    n_valid^2), row_sum [n_samples] (sum_j kp(i, j): a row's share, NaN for a skipped row; None unless asked for), n_samples,
    n_valid, n_skipped, gamma, transform."""

    def __init__(self, ksd2, row_sum, n_samples, n_skipped, gamma, transform=None):
        self.ksd2 = float(ksd2)
        self.ksd = float(np.sqrt(self.ksd2)) if self.ksd2 >= 0.0 else float("nan")
        self.row_sum = row_sum
        self.n_samples, self.n_skipped = int(n_samples), int(n_skipped)
        self.n_valid = self.n_samples - self.n_skipped
        self.gamma, self.transform = gamma, transform

    def __repr__(self):
        return "SteinDiscrepancy(ksd=%.6g, n_samples=%d, n_valid=%d, transform=%s)" % (self.ksd, self.n_samples, self.n_valid, self.transform)


def prepare(x, grad, preconditioner="sclmed", lo=None, hi=None, transform="logit", layout="steps", device=0):
    """What both entry points do first.  x, grad: numpy or torch cuda, [S, ndim] or a three-dimensional chain ([nsteps, nwalkers,
    ndim] with layout "steps", [nwalkers, nsteps, ndim] with "walkers"; either way the rows are taken in memory order, outer
    axis first).  Returns (rows, z, g_z, gamma, ginv, transform): rows [S, ndim] as given, z and g_z the float64 cuda tensors the
    kernels read, gamma and ginv numpy [ndim, ndim]."""
    import torch
    if layout not in ("steps", "walkers"):
        raise ValueError("layout: 'steps' ([nsteps, nwalkers, ndim]) or 'walkers' ([nwalkers, nsteps, ndim])")
    dev = x.device if _is_torch(x) and x.is_cuda else grad.device if _is_torch(grad) and grad.is_cuda else torch.device("cuda", device)

    def up(a, name):
        if _is_torch(a):
            a = a.to(device=dev, dtype=torch.float64)
        else:
            a = torch.as_tensor(np.require(np.asarray(a, dtype=np.float64), requirements=["C"]), device=dev)
        if a.dim() not in (2, 3):
            raise ValueError("%s: [S, ndim] or a three-dimensional chain" % name)
        return a.reshape(-1, a.shape[-1])
    rows, g = up(x, "x"), up(grad, "grad")
    if g.shape != rows.shape:
        raise ValueError("grad: expected the shape of x")
    n, d = int(rows.shape[0]), int(rows.shape[1])
    if n < 1 or d < 1:
        raise ValueError("x: no samples")
    if d > 64:
        raise ValueError("x: %d parameters, at most 64" % d)
    if (lo is None) != (hi is None):
        raise ValueError("lo and hi go together")
    if transform == "logit" and lo is None:
        transform = None
    if transform not in ("logit", None):
        raise ValueError("transform: 'logit' or None")
    z, gz = logit_transform(rows, g, lo, hi) if transform == "logit" else (rows, g)
    kind = preconditioner
    need_rows = isinstance(kind, str) and kind != "id"
    gamma = preconditioner_matrix(z.cpu().numpy() if need_rows else np.empty((0, d)), kind)
    return rows, z, gz, gamma, _gamma_inverse(gamma), transform


def stein_thin(x, grad, m, preconditioner="sclmed", lo=None, hi=None, transform="logit", layout="steps", names=None, eng=None,
               device=0):
    """SteinThinning: the m rows of x whose empirical measure has the smallest kernel Stein discrepancy, picked greedily on
    the device (gpb_stein_thin: m dependent passes over the rows, enqueued in one call).  grad: the score grad log p at every
    row, in x's units (Chain.log_posterior(x, return_grad=True)[1]).  lo, hi [ndim]: the prior box, for transform="logit" (the
    module's docstring says why).  ndim <= 64, m <= 2^20."""
    from .diagnostics import _engine
    rows, z, gz, gamma, ginv, transform = prepare(x, grad, preconditioner, lo, hi, transform, layout, device)
    eng = eng or _engine(z.device.index or 0)
    out = eng.stein_thin(z, gz, ginv, int(m))
    idx = out["idx"]
    import torch
    pts = rows.index_select(0, torch.as_tensor(np.maximum(idx, 0).astype(np.int64), device=rows.device)).cpu().numpy()
    pts[idx < 0] = np.nan
    return SteinThinning(idx, pts, out["ksd"], rows.shape[0], out["n_skipped"], gamma, transform, names)


def ksd(x, grad, preconditioner="sclmed", lo=None, hi=None, transform="logit", layout="steps", splits=0, return_rows=True, eng=None,
        device=0):
    """SteinDiscrepancy of ALL rows of x with scores grad (as stein_thin takes them): n^2 pair evaluations in fp64 on the device
    (gpb_stein_ksd).  To compare point sets — a chain, its thinned picks, cluster centres — give every call the SAME explicit
    preconditioner matrix (a SteinThinning's or SteinDiscrepancy's .gamma): the data-driven ones depend on the set."""
    from .diagnostics import _engine
    rows, z, gz, gamma, ginv, transform = prepare(x, grad, preconditioner, lo, hi, transform, layout, device)
    eng = eng or _engine(z.device.index or 0)
    out = eng.stein_ksd(z, gz, ginv, splits=splits, return_rows=return_rows)
    return SteinDiscrepancy(out["ksd2"], out.get("row_sum"), rows.shape[0], out["n_skipped"], gamma, transform)
