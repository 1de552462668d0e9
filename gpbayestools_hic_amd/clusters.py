"""
Posterior clusters of a chain, on the device: what examples/generate_posterior_clusters.py does with a finished pocoMC chain —
sort it by log-likelihood and keep the `num_samples` most likely rows, `StandardScaler().fit_transform`, `KMeans(n_clusters,
n_init=10)`, `inverse_transform` of the cluster centres, written to cluster_centers.txt — for a chain that lies in device
memory (gpb_chain_kmeans): the sampler's [nsteps, nwalkers, ndim] store, a pickle's [nwalkers, nsteps,
ndim], a thinned view of either or a flat particle set is read through its strides; all restarts share every pass.

The Lloyd iteration is sklearn's (its loop, its stopping rule, its n_iter_); started from the same centres (`init`) it reaches
the same labels.  Two things differ on purpose.  The seeding is the published k-means++ driven by uniforms from
np.random.default_rng(seed), not sklearn's greedy variant on a Mersenne stream: the same seed gives other (equally good)
starting centres than sklearn's random_state.  A cluster that loses all its rows keeps its centre and reports size 0; sklearn
moves it to a far row.

Importance weights (the `weights` of a pocoMC / run_SMC pickle) are honoured; the reference's script drops them.
"""
import pickle

import numpy as np


class PosteriorClusters:
    """centers [k, ndim] of the best restart (the lowest inertia), in the chain's own units; sizes [k] (rows, int64) and
    weight_share [k] (the clusters' share of the total weight); inertia, n_iter, converged of the best restart, best (its
    index); all_centers [n_init, k, ndim], all_inertia [n_init]; mean, scale [ndim] the rows were standardised with;
    n_samples (rows clustered), n_skipped (rows with a non-finite coordinate, left out); labels [n_samples] (int32 numpy,
    in the row order of the memory layout, -1 a skipped row) or None; names."""

    def __init__(self, centers, sizes, weight_share, inertia, n_iter, converged, best, all_centers, all_inertia, mean, scale,
                 n_samples, n_skipped, labels=None, names=None):
        self.centers, self.sizes, self.weight_share = centers, sizes, weight_share
        self.inertia, self.n_iter, self.converged, self.best = float(inertia), int(n_iter), bool(converged), int(best)
        self.all_centers, self.all_inertia = all_centers, all_inertia
        self.mean, self.scale = mean, scale
        self.n_samples, self.n_skipped = int(n_samples), int(n_skipped)
        self.labels = labels
        self.names = None if names is None else list(names)

    def savetxt(self, path="cluster_centers.txt"):
        """the reference's file: one row per parameter, one column per cluster, '%.6f'"""
        np.savetxt(path, self.centers.T, fmt="%.6f")

    def __repr__(self):
        k, d = self.centers.shape
        names = self.names or ["p%d" % j for j in range(d)]
        wid = max([9] + [len(str(s)) for s in names])
        lines = ["PosteriorClusters(n_samples=%d, ndim=%d, k=%d, n_init=%d, best=%d, inertia=%.6g, n_iter=%d%s%s)"
                 % (self.n_samples, d, k, len(self.all_inertia), self.best, self.inertia, self.n_iter,
                    "" if self.converged else ", not converged", ", skipped=%d" % self.n_skipped if self.n_skipped else ""),
                 "  %-*s %s" % (wid, "parameter", " ".join("%12s" % ("c%d" % c) for c in range(k))),
                 "  %-*s %s" % (wid, "rows", " ".join("%12d" % n for n in self.sizes)),
                 "  %-*s %s" % (wid, "share", " ".join("%12.4f" % s for s in self.weight_share))]
        for j, nm in enumerate(names):
            lines.append("  %-*s %s" % (wid, nm, " ".join("%12.5g" % v for v in self.centers[:, j])))
        return "\n".join(lines)


def top_by_logl(logl, num_samples):
    """indices of the num_samples rows of largest logl, in descending order of logl: `np.argsort(logl)[::-1][:num_samples]`,
    the reference's sort_chain_likelihood followed by [:num_samples].  Ties go to the higher index (the reversed ascending
    sort).  logl a torch tensor: sorted on the device (a stable sort)."""
    import torch
    n = int(logl.shape[0])
    order = torch.sort(logl, stable=True).indices
    return torch.flip(order, dims=(0,))[:max(0, min(int(num_samples), n))]


def posterior_clusters(x, n_clusters=10, n_init=10, *, logl=None, num_samples=None, weights=None, init=None, seed=42,
                       max_iter=300, tol=1e-4, standardize=True, layout="steps", return_labels=False, names=None, device=0,
                       eng=None):
    """PosteriorClusters of a chain: x numpy or a torch cuda tensor / view, [nsteps, nwalkers, ndim] (layout "steps"),
    [nwalkers, nsteps, ndim] ("walkers") or a flat [S, ndim]; ndim <= 64, n_clusters <= 32, n_init <= 16.
    logl [S] with num_samples (a flat x only): the num_samples rows of largest logl are clustered — the reference's
    sort_chain_likelihood followed by [:num_samples], taken on the device (a sort and a gather); ties at the cut go to the
    HIGHER index, as in np.argsort(logl)[::-1].  The rows, weights and labels are then in that descending order.
    weights [S] with a flat x only (non-negative).  init [n_init, n_clusters, ndim] (or [n_clusters, ndim] with n_init=1):
    the starting centres in the chain's units — sklearn's KMeans(init=...) reaches the same labels from them; otherwise
    k-means++ seeding driven by np.random.default_rng(seed).random((n_init, n_clusters)).  max_iter, tol, as sklearn's;
    standardize=False clusters the rows as they are.  return_labels: the best restart's label per row."""
    import torch
    from .diagnostics import _engine
    if hasattr(x, "data_ptr"):
        x = x if x.dtype == torch.float64 else x.to(torch.float64)
    else:                                   # (non-finite rows are the library's to skip: no check here)
        x = torch.as_tensor(np.require(np.asarray(x, dtype=np.float64), requirements=["C"]), device=torch.device("cuda", device))
    flat = x.dim() == 2
    if x.dim() not in (2, 3):
        raise ValueError("x: [nsteps, nwalkers, ndim], [nwalkers, nsteps, ndim] or [S, ndim]")
    if not flat and (weights is not None or logl is not None or num_samples is not None):
        raise ValueError("weights, logl and num_samples go with a flat [S, ndim] sample set")
    if (logl is None) != (num_samples is None):
        raise ValueError("logl and num_samples go together")
    dev = x.device
    if weights is not None:
        w = np.asarray(weights.cpu().numpy() if hasattr(weights, "data_ptr") else weights, dtype=np.float64).reshape(-1)
        if w.shape[0] != x.shape[0] or not np.all(np.isfinite(w)) or np.any(w < 0.0) or not w.max() > 0.0:
            raise ValueError("weights: [%d] finite, non-negative, not all zero" % x.shape[0])
        weights = torch.as_tensor(w, device=dev)
    if logl is not None:
        ll = logl if hasattr(logl, "data_ptr") else torch.as_tensor(np.asarray(logl, dtype=np.float64).reshape(-1))
        ll = ll.to(dev).reshape(-1)
        if ll.shape[0] != x.shape[0]:
            raise ValueError("logl: expected [%d]" % x.shape[0])
        if int(num_samples) < 1:
            raise ValueError("num_samples: at least one")
        keep = top_by_logl(ll, num_samples)
        x = x.index_select(0, keep)
        if weights is not None:
            weights = weights.index_select(0, keep)
    x3 = x[:, None, :] if flat else x
    if flat:
        layout = "steps"
    d = int(x3.shape[2])
    S = int(x3.shape[0]) * int(x3.shape[1])
    if S < 1 or d < 1:
        raise ValueError("x: no samples")
    k, R = int(n_clusters), int(n_init)
    u = None
    if init is not None:
        init = np.asarray(init, dtype=np.float64)
        if init.ndim == 2 and R == 1:
            init = init[None]
        if init.shape != (R, k, d):
            raise ValueError("init: [%d, %d, %d]" % (R, k, d))
    else:
        u = np.random.default_rng(seed).random((R, k))
    eng = eng or _engine(dev.index or 0)
    out = eng.chain_kmeans(x3, layout, k, R, init=init, u=u, weights=weights, max_iter=max_iter, tol=tol, standardize=standardize,
                           return_labels=return_labels)
    b = out["best"]
    wsum = out["wsum"][b]
    labels = out["labels"].cpu().numpy() if return_labels else None
    return PosteriorClusters(out["centers"][b].copy(), out["size"][b].copy(), wsum / wsum.sum(), out["inertia"][b], out["n_iter"][b],
                             out["converged"][b], b, out["centers"], out["inertia"], out["mean"], out["scale"], S, out["n_skipped"],
                             labels=labels, names=names)


def sort_chain_likelihood(path):
    """examples/generate_posterior_clusters.py's sort_chain_likelihood as a drop-in: reads the six-key pickle of a pocoMC run
    (chain, weights, logl, logp, logz, logz_err — also what this package's run_pocoMC / run_SMC write), sorts chain, weights,
    logl and logp by descending logl (`np.argsort(logl)[::-1]`) and writes the six keys to path with '.pkl' replaced by
    '_sorted.pkl'.  Returns that path."""
    with open(path, "rb") as f:
        run = pickle.load(f)
    logl = np.asarray(run["logl"])
    order = np.argsort(logl)[::-1]
    data = {"chain": np.asarray(run["chain"])[order], "weights": np.asarray(run["weights"])[order], "logl": logl[order],
            "logp": np.asarray(run["logp"])[order], "logz": run["logz"], "logz_err": run["logz_err"]}
    out = path.replace(".pkl", "_sorted.pkl")
    with open(out, "wb") as f:
        pickle.dump(data, f)
    return out
