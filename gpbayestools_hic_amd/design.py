"""
Maximum-projection Latin-hypercube designs: the reference's src/design.py (`Design`, `generate_lhs`) as a drop-in, with the
generator on the device instead of R.

The reference shells out to R, `MaxProRunOrder(MaxProLHD(npoints, ndim)$Design)`: a Latin hypercube that minimises the MaxPro
criterion of Joseph, Gul and Ba (2015) by simulated annealing over column-wise swaps, then put into a greedy run order.  Here
the annealing runs on the GPU (gpb_maxpro_lhd, csrc/gpb_maxpro.hip): independent restarts from random
hypercubes, each proposal a pass over two rows of the restart's pair matrix; the best restart is put into run order
(gpb_maxpro_run_order).  The array has the shape the reference gets from R — column 0 the run order 1 .. n, then the design —
and the same cache file, so a cache written by either side serves the other.

The random streams differ from R's, so a seed does not give R's design, only one of the same kind; and R's package is not
available to compare with, so MaxProRunOrder's starting row and tie-breaking are this module's choice (the row nearest the
cube's centre; the lowest index), not a restatement of the package's.
"""
import logging
import os
from collections import namedtuple
from datetime import datetime
from pathlib import Path

import numpy as np

from .preprocess import parse_model_parameter_file

__all__ = ["Design", "generate_lhs", "maxpro_design", "maxpro_criterion", "run_order", "MaxProDesign", "DEFAULTS"]

# The default schedule (DESIGN.md section 24 has what it was chosen on): temperatures temp0 cool^k, k < n_stages, on f = ln sum
# of the pair terms; blocks of `block` proposals, `proposals_per_cell` n ndim of them in all (a block that accepts early consumes
# fewer than it draws).
DEFAULTS = dict(n_restarts=4, n_stages=16, temp0=0.001, cool=0.75, block=32, proposals_per_cell=160)

MaxProDesign = namedtuple("MaxProDesign", ["levels", "design", "order", "lnpsi", "lnpsi_start", "best", "accepted", "consumed",
                                           "all_levels"])
MaxProDesign.__doc__ = """What maxpro_design found: levels [n, ndim] (int32) and design [n, ndim] = (levels + 0.5) / n of the
best restart, in run order; order [n] the rows of the best restart's hypercube in that order (0-based); lnpsi, lnpsi_start
[n_restarts] ln of the MaxPro criterion of every restart's result and start; best the restart with the lowest criterion;
accepted, consumed [n_restarts] proposals; all_levels [n_restarts, n, ndim] every restart's levels as annealed."""


def _int_seed(seed):
    """the 64-bit key of the draws: an integral seed as it is, any other number (the reference's default is a time stamp) by its
    microseconds"""
    s = float(seed)
    return (int(s) if s == int(s) else int(round(s * 1e6))) & 0xFFFFFFFFFFFFFFFF


def _engine(device):
    from .diagnostics import _engine as lend
    return lend(device)


def maxpro_design(npoints, ndim, seed, *, n_restarts=None, n_stages=None, blocks_per_stage=None, block=None, temp0=None, cool=None,
                  init=None, first=-1, device=0, eng=None):
    """A MaxPro Latin hypercube of npoints x ndim (4 <= npoints <= 4096, 2 <= ndim <= 64) as a MaxProDesign.  The starts are drawn
    from np.random.default_rng(seed), one permutation per column per restart, or given as init [n_restarts, npoints, ndim]
    (integer levels, every column a permutation of 0 .. npoints - 1); the annealing's draws are keyed by the seed as well.
    Schedule arguments left None take DEFAULTS; blocks_per_stage then follows from proposals_per_cell."""
    n, d = int(npoints), int(ndim)
    R = int(DEFAULTS["n_restarts"] if n_restarts is None else n_restarts)
    n_stages = int(DEFAULTS["n_stages"] if n_stages is None else n_stages)
    block = int(DEFAULTS["block"] if block is None else block)
    temp0 = float(DEFAULTS["temp0"] if temp0 is None else temp0)
    cool = float(DEFAULTS["cool"] if cool is None else cool)
    key = _int_seed(seed)
    if init is None:
        if n < 1 or d < 1 or R < 1:
            raise ValueError("npoints, ndim and n_restarts must be positive")
        rng = np.random.default_rng(key)
        init = np.empty((R, n, d), dtype=np.int32)
        for r in range(R):
            for c in range(d):
                init[r, :, c] = rng.permutation(n)
    else:
        init = np.asarray(init)
        if init.shape != (R, n, d):
            raise ValueError("init: expected [%d, %d, %d]" % (R, n, d))
    if blocks_per_stage is None:
        blocks_per_stage = max(1, -(-DEFAULTS["proposals_per_cell"] * n * d // (max(block, 1) * max(n_stages, 1))))
    eng = eng or _engine(device)
    out = eng.maxpro_lhd(init, key, n_stages, int(blocks_per_stage), block, temp0, cool)
    best = int(np.argmin(out["f_best"]))
    levels = out["levels"][best]
    order = eng.maxpro_run_order((levels + 0.5) / n, first)
    levels = np.ascontiguousarray(levels[order])
    return MaxProDesign(levels, (levels + 0.5) / n, order, out["lnpsi"], out["lnpsi_start"], best, out["accepted"], out["consumed"],
                        out["levels"])


def maxpro_criterion(X, device=0, eng=None):
    """ln of the MaxPro criterion psi = (mean over pairs of 1 / prod_c (x_ic - x_jc)^2)^(1/ndim) of a design X [n, ndim] in the
    unit cube, on the device (gpb_maxpro_criterion); +inf when two rows share a coordinate."""
    return (eng or _engine(device)).maxpro_criterion(X)


def run_order(X, first=-1, device=0, eng=None):
    """The greedy run order of a design X [n, ndim], after MaxProRunOrder's documented method: from one row (first; -1: the row
    nearest the cube's centre) append again and again the row with the smallest sum, over the rows already chosen, of
    1 / prod_c (x_ic - x_jc)^2; the lowest index wins a tie.  Returns 0-based row indices [n] (int32).  The R package's own
    starting row and tie-breaking could not be looked up and are not claimed to match."""
    return (eng or _engine(device)).maxpro_run_order(X, first)


def _cachedir(cache_dir):
    return Path(cache_dir) if cache_dir is not None else Path(os.getenv("WORKDIR", ".")) / "cache" / "lhs"


def generate_lhs(npoints, ndim, seed, *, cache_dir=None, device=0, **schedule):
    """src/design.py's generate_lhs: float64 [npoints, ndim + 1], column 0 the run order 1 .. npoints, the others the MaxPro
    Latin hypercube in that order (the reference slices it with [:, 1:]).  Like the reference it first looks for
    npoints{}_ndim{}_seed{}.npy under <$WORKDIR or .>/cache/lhs (or cache_dir), loads it if present and writes it otherwise;
    the directory is created when a file is written, not before.  schedule: maxpro_design's keyword arguments."""
    logging.debug("generating MaxPro LHS: npoints = %d, ndim = %d, seed = %s", npoints, ndim, seed)
    cachefile = _cachedir(cache_dir) / "npoints{}_ndim{}_seed{}.npy".format(npoints, ndim, seed)
    if cachefile.exists():
        logging.debug("loading from cache")
        return np.load(cachefile)
    logging.debug("not found in cache, generating on the device")
    res = maxpro_design(npoints, ndim, seed, device=device, **schedule)
    lhs = np.concatenate([np.arange(1, int(npoints) + 1, dtype=np.float64)[:, None], res.design], axis=1)
    cachefile.parent.mkdir(parents=True, exist_ok=True)
    np.save(cachefile, lhs)
    return lhs


class Design:
    """
    Latin-hypercube model design: src/design.py's class as a drop-in.

    Creates a design for the parameter set of `parfile` (`name: label, min, max` lines) with `npoints` points; the main
    (training) design if `validation` is false, the validation design if it is true.  With seed=None a time-based seed is
    taken and printed, as the reference does.  cache_dir, device and schedule go to generate_lhs.

    Public attributes: ``type`` ('main' or 'validation'), ``pardict``, ``min``, ``max`` (numpy arrays), ``ndim``, ``points``
    (design point names, zero-padded numbers), ``array`` (the design, scaled into [min, max]).  Converts to a numpy array.
    """

    def __init__(self, parfile, npoints=500, validation=False, seed=None, *, cache_dir=None, device=0, **schedule):
        self.pardict = parse_model_parameter_file(parfile)
        self.type = "validation" if validation else "main"
        self.ndim = len(self.pardict.keys())
        fmt = "parameter_{:0" + str(len(str(npoints - 1))) + "d}"
        self.points = [fmt.format(i) for i in range(npoints)]
        if seed is None:
            seed = datetime.now().timestamp()
            print("seed = {}".format(seed))
        self.min = np.array([val[1] for val in self.pardict.values()])
        self.max = np.array([val[2] for val in self.pardict.values()])
        array_tmp = generate_lhs(npoints, self.ndim, seed, cache_dir=cache_dir, device=device, **schedule)
        self.array = self.min + (self.max - self.min) * array_tmp[:, 1:]

    def __array__(self, dtype=None, copy=None):
        return self.array if dtype is None else self.array.astype(dtype)

    def write_files(self, basedir):
        """Write one input file per design point, `name value` lines, to basedir/<type>/parameter_XXX."""
        outdir = Path(basedir) / self.type
        outdir.mkdir(parents=True, exist_ok=True)
        for point, row in zip(self.points, self.array):
            filepath = outdir / point
            with filepath.open("w") as f:
                for idx, ikey in enumerate(self.pardict.keys()):
                    f.write("{} {}\n".format(ikey, row[idx]))
            logging.debug("wrote %s", filepath)
