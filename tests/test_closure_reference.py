"""CPU tier: the host code of closure.ClosureResult — the truth's rank counted with numpy, coverage and the rank histogram
decided from the rank alone, the pickles of save / write_chain — against the element-by-element restatement of
tests/closure_reference.py on seeded arrays, with ties and truths outside all samples."""
import pickle

import numpy as np
import pytest

import closure_reference as CR
from gpbayestools_hic_amd.closure import ClosureResult, truth_rank

K, NW, NS, D = 7, 6, 9, 4


def _arrays(seed=3):
    rng = np.random.default_rng(seed)
    chain = rng.uniform(0.0, 1.0, (K, NW, NS, D))
    chain = np.round(chain, 2)                                 # two decimals: ties among the samples
    truths = rng.uniform(0.2, 0.8, (K, D))
    truths[0] = chain[0, 2, 3]                                 # a truth that IS a sample (strictly below: not counted)
    truths[1, 0] = -1.0                                        # below every sample: rank 0
    truths[1, 1] = 2.0                                         # above every sample: rank n
    truths[2, 2] = np.median(chain[2, :, :, 2])
    return chain, truths


def test_rank_coverage_and_histogram_against_the_restatement():
    chain, truths = _arrays()
    n = NW * NS
    ref = CR.rank(chain, truths)
    assert np.array_equal(truth_rank(chain, truths), ref)
    res = ClosureResult(chain, None, None, None, truths=truths)
    assert res.n_samples == n and res.rank.dtype == np.int64 and np.array_equal(res.rank, ref)
    assert ref[1, 0] == 0 and ref[1, 1] == n                   # outside all samples, on either side
    assert ref[0, 0] == int((chain[0, :, :, 0] < chain[0, 2, 3, 0]).sum()) < n
    for level in (0.1, 0.5, 0.68, 0.9, 0.95, 1.0):
        assert np.array_equal(res.coverage(level), CR.coverage(ref, n, level)), level
    assert np.all(res.coverage(1.0) == 1.0)                    # every rank lies in [0, n]
    cov = res.coverage(0.9)
    assert cov[0] <= (K - 1) / K and cov[1] <= (K - 1) / K     # set 1's truths lie outside every sample
    for bins in (1, 4, 10, n, n + 5):
        h = res.rank_histogram(bins)
        assert h.shape == (D, bins) and h.dtype == np.int64
        assert np.array_equal(h, CR.histogram(ref, n, bins)), bins
        assert np.all(h.sum(axis=1) == K)
    assert res.rank_histogram(10)[0, 0] >= 1 and res.rank_histogram(10)[1, 9] >= 1      # rank 0 and rank n: the end bins


def test_rank_passed_in_is_kept_and_shapes_are_checked():
    chain, truths = _arrays(5)
    rk = CR.rank(chain, truths)
    res = ClosureResult(chain, None, None, None, truths=truths, rank=rk)
    assert np.array_equal(res.rank, rk)
    with pytest.raises(ValueError):
        ClosureResult(chain, None, None, None, truths=truths[:, :3])
    with pytest.raises(ValueError):
        ClosureResult(chain[0], None, None, None)
    with pytest.raises(ValueError):
        ClosureResult(chain, None, None, None).coverage(0.9)   # no truths
    with pytest.raises(ValueError):
        res.coverage(0.0)
    with pytest.raises(ValueError):
        res.rank_histogram(0)
    with pytest.raises(ValueError):
        res.write_chain(K, "nowhere.pkl")


def test_pickles_round_trip(tmp_path):
    chain, truths = _arrays(7)
    rng = np.random.default_rng(1)
    lnp = rng.standard_normal((K, NW, NS))
    acc = rng.uniform(size=(K, NW))
    data = rng.standard_normal((K, 11))
    pr = np.stack([np.zeros(D), np.ones(D)], axis=1)
    seeds = np.arange(K, dtype=np.uint64) + np.uint64(2 ** 63)
    res = ClosureResult(chain, lnp, acc, data, truths=truths, prior_ranges=pr, names=list("abcd"), seeds=seeds)
    p = tmp_path / "closure.pkl"
    res.save(p)
    with open(p, "rb") as f:
        raw = pickle.load(f)
    assert isinstance(raw, dict) and np.array_equal(raw["chain"], chain)
    back = ClosureResult.load(p)
    for name in ("chain", "lnprobability", "acceptance", "data", "truths", "prior_ranges", "rank", "seeds"):
        assert np.array_equal(getattr(back, name), getattr(res, name)), name
    assert back.names == list("abcd") and back.n_samples == res.n_samples
    assert np.array_equal(back.coverage(0.68), res.coverage(0.68))
    for k in (0, K - 1):
        q = tmp_path / ("chain%d.pkl" % k)
        res.write_chain(k, q)
        with open(q, "rb") as f:                               # the reference's reader: pickle.load(f)["chain"]
            got = pickle.load(f)
        assert list(got) == ["chain"] and got["chain"].shape == (NW, NS, D) and np.array_equal(got["chain"], chain[k])
