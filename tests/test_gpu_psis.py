"""GPU tier: Pareto-smoothed importance sampling on the device — gpb_psis and gpb_psis_loo (GPEngine.psis / psis_loo, loo.psis) —
against the numpy model of tests/psis_reference.py on the input sets that tests/test_psis_reference.py vouches for.

Bars.  n_tail and the set of smoothed samples: exact.  khat: 1e-12 absolute (MOM_BAR of tests/test_gpu_diag.py); the log weights
and elpd_loo: 1e-11 absolute — more than 100 times the model's own float64-against-longdouble spread (khat 2.9e-15, lw 5.8e-14),
which leaves room for the device's log1p / exp / expm1.  ess, lppd, p_waic and loo_pit, which the issue leaves open: 1e-12
relative — each is a ratio or a logarithm of sums of S <= 20000 non-negative terms added in a tree of depth <= 24, about 30 roundings
of 1.1e-16 each, with a margin of 300.  Rows against themselves under another R, row stride, row order, on_device, set of outputs
and in a second call: bit equality.
Measured on an MI355X (the maxima over all cases; each is printed with -s): see the docstrings of the tests."""
import functools

import numpy as np
import pytest

import psis_reference as R

pytestmark = pytest.mark.gpu

KHAT_BAR, LW_BAR, REL_BAR = 1e-12, 1e-11, 1e-12
E_ARG = -1


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _eng():
    from gpbayestools_hic_amd import GPEngine
    return GPEngine(0)


@functools.lru_cache(maxsize=None)
def _sets():
    return R.named_sets()


@functools.lru_cache(maxsize=None)
def _model(name):
    d = {}
    lw, khat, n, ess = R.psis_row(_sets()[name], details=d)
    return lw, khat, n, ess, d


def _dev(a):
    torch, dev = _torch()
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _compare(name, lr, got_lw, got_khat, got_ntail, got_ess):
    lw, khat, n, ess, d = _model(name)
    assert int(got_ntail) == n, (name, got_ntail, n)
    # the samples smoothing moved: the model's tail (but for a largest value truncated back to 0), exactly
    want_set = R.changed_set(lr, lw)
    assert np.array_equal(R.changed_set(lr, got_lw), want_set), name
    if d["smoothed"]:
        assert set(want_set) <= set(d["tail"]) and len(want_set) >= n - 1
    else:
        assert len(want_set) == 0
    if np.isfinite(khat):
        dk = abs(got_khat - khat)
    else:
        assert got_khat == np.inf
        dk = 0.0
    dl = float(np.abs(got_lw - lw).max())
    de = abs(got_ess - ess) / ess
    print("psis %-22s S=%5d n_tail=%4d khat=%8.4f: khat %.1e  lw %.1e  ess %.1e relative" % (name, lr.shape[0], n, khat, dk, dl, de))
    assert dk <= KHAT_BAR and dl <= LW_BAR and de <= REL_BAR, name
    return dk, dl, de


@pytest.mark.parametrize("name", sorted(R.named_sets()))
def test_psis_against_the_model(name):
    """every input set, one row per call: S in {20 (M = 4, no fit), 25, 26 (n = 5), 225, 226 (S // 5 meets 3 sqrt S), 4096, 4097
    (the ceil), 20000 (twenty strides of the workgroup, M = 425)}, lr = a z^2 / 2 with khat in all four classes, the tied set, the
    all-equal row, the row whose range exceeds 745 and the row with values on the cutoff.
    Measured: khat within 3.1e-15 (a = 1.3, S = 4096), lw within 1.1e-14 and ess within 1.3e-14 relative (both a = 0.9, S = 20000) —
    all below 1/16 of their bars, which therefore stay."""
    lr = _sets()[name]
    out = _eng().psis(_dev(lr[None, :]))
    _compare(name, lr, out["log_weights"].cpu().numpy()[0], float(out["khat"][0]), int(out["n_tail"][0]), float(out["ess"][0]))
    assert abs(float(np.logaddexp.reduce(out["log_weights"].cpu().numpy()[0]))) <= 1e-12


@functools.lru_cache(maxsize=None)
def _rows(n_rows, S=640):
    return R.row_block(n_rows, S)


@pytest.mark.parametrize("n_rows", [1, 3, 65])
def test_rows_and_bit_equality(n_rows):
    """R in {1, 3, 65} rows of S = 640 against the model (measured: khat 2.9e-15, lw 6.2e-15, ess 8.7e-15 relative), then the same
    rows with a row stride above S, in reversed order, from host memory, with subsets of the outputs, alone, and in a second call:
    the same bits"""
    torch, dev = _torch()
    eng = _eng()
    lr = _rows(n_rows)
    S = lr.shape[1]
    want = R.psis(lr)
    a = eng.psis(_dev(lr))
    got = {k: v.cpu().numpy() for k, v in a.items()}
    assert np.array_equal(got["n_tail"], want["n_tail"])
    dk, dl = np.abs(got["khat"] - want["khat"]).max(), np.abs(got["log_weights"] - want["lw"]).max()
    de = (np.abs(got["ess"] - want["ess"]) / want["ess"]).max()
    print("psis R=%d: khat %.1e  lw %.1e  ess %.1e relative" % (n_rows, dk, dl, de))
    assert dk <= KHAT_BAR and dl <= LW_BAR and de <= REL_BAR

    def same(b, rows=slice(None), keys=("khat", "n_tail", "ess", "log_weights")):
        for k in keys:
            v = b[k].cpu().numpy() if hasattr(b[k], "cpu") else b[k]
            assert np.array_equal(v, got[k][rows]), k
    wide = torch.full((n_rows, S + 37), float("nan"), dtype=torch.float64, device=dev)
    wide[:, :S] = _dev(lr)
    b = eng.psis(wide[:, :S])
    assert n_rows == 1 or b["log_weights"].stride(0) == S + 37
    same(b)
    same(eng.psis(_dev(np.array(lr[::-1]))), rows=slice(None, None, -1))
    same(eng.psis(lr))                                           # host memory
    same(eng.psis(_dev(lr), outputs=("khat",)), keys=("khat",))
    same(eng.psis(_dev(lr), outputs=("ess", "log_weights")), keys=("ess", "log_weights"))
    same(eng.psis(_dev(lr[n_rows // 2:n_rows // 2 + 1])), rows=slice(n_rows // 2, n_rows // 2 + 1))
    same(eng.psis(_dev(lr)))


def test_loo_psis_helper_and_refusals():
    from gpbayestools_hic_amd import loo
    lr = _sets()["chi2_a0.6_S640"]
    one = loo.psis(lr)
    two = loo.psis(np.stack([lr, lr]))
    assert isinstance(one.khat, float) and one.log_weights.shape == (640,) and two.khat.shape == (2,)
    assert one.khat == two.khat[0] == two.khat[1] and np.array_equal(one.log_weights, two.log_weights[1])
    assert one.n_tail == _model("chi2_a0.6_S640")[2] and "khat" in repr(one)
    bad = lr.copy()
    bad[3] = np.nan
    for arg in (bad, np.zeros((2, 3, 4)), np.zeros((0, 5))):
        with pytest.raises(ValueError):
            loo.psis(arg)


LOO_CASES = [("edge_S20",), ("edge_S26",), ("edge_S226",), ("chi2_a0.9_S640", "chi2_a0.1_S640", "cutoff_ties"), ("edge_S4097",),
             ("chi2_a0.3_S20000", "edge_S20000"), ("wide_range",), ("tied", "chi2_a1.3_S4096"), ("all_equal",)]


@pytest.mark.parametrize("names", LOO_CASES, ids=lambda n: n[0])
def test_psis_loo_against_the_model(names):
    """gpb_psis_loo on ll = -lr of the shared sets (sets of one size as the rows of one call) with random standardised residuals:
    elpd_loo within 1e-11 absolute, khat within 1e-12, n_tail and min ll exact, lppd, p_waic, ess and loo_pit within 1e-12
    relative; khat, ess and n_tail carry the bits gpb_psis gives for lr = -ll; without zc the PIT is NaN and nothing else moves; host
    memory gives the same bits.
    Measured: elpd_loo within 1.5e-14 (the wide-range set), khat 3.1e-15, lppd 0, p_waic 2.7e-16, ess 4.9e-15, loo_pit 9.1e-16
    relative — all below 1/16 of their bars."""
    eng = _eng()
    name, n_rows = names[0], len(names)
    ll = np.stack([-_sets()[nm] for nm in names])
    zc = np.random.default_rng(5).standard_normal(ll.shape)
    want = R.psis_loo(ll, zc)
    got = eng.psis_loo(_dev(ll), _dev(zc)).cpu().numpy()
    assert got.shape == (n_rows, 8) and eng.LOO_COLUMNS == R.LOO_COLS
    d_elpd = np.abs(got[:, 0] - want[:, 0]).max()
    fin = np.isfinite(want[:, 3])
    assert np.all(got[~fin, 3] == np.inf)
    d_khat = np.abs(got[fin, 3] - want[fin, 3]).max() if fin.any() else 0.0
    rel = {}
    for c, nm in ((1, "lppd"), (2, "p_waic"), (4, "ess"), (6, "loo_pit")):
        den = np.abs(want[:, c])
        rel[nm] = float((np.abs(got[:, c] - want[:, c]) / np.where(den > 0, den, 1.0)).max())
    print("psis_loo %-18s R=%d: elpd %.1e  khat %.1e  %s" % (name, n_rows, d_elpd, d_khat,
                                                            "  ".join("%s %.1e" % kv for kv in rel.items())))
    assert d_elpd <= LW_BAR and d_khat <= KHAT_BAR
    assert np.array_equal(got[:, 5], want[:, 5]) and np.array_equal(got[:, 7], ll.min(axis=1))
    for nm, v in rel.items():
        if nm == "p_waic" and name == "all_equal":
            assert np.all(got[:, 2] == 0.0)
            continue
        assert v <= REL_BAR, nm
    p = eng.psis(_dev(-ll), outputs=("khat", "n_tail", "ess"))
    assert np.array_equal(p["khat"].cpu().numpy(), got[:, 3]) and np.array_equal(p["ess"].cpu().numpy(), got[:, 4])
    assert np.array_equal(p["n_tail"].cpu().numpy(), got[:, 5].astype(np.int64))
    nz = eng.psis_loo(_dev(ll)).cpu().numpy()
    assert np.isnan(nz[:, 6]).all() and np.array_equal(np.delete(nz, 6, axis=1), np.delete(got, 6, axis=1))
    assert np.array_equal(eng.psis_loo(ll, zc), got)


def test_argument_errors_allocate_nothing():
    """S above 2^24 is refused from the arguments alone (the row handed over has 8 values: nothing of that size is allocated or
    read), as are ld < S, R < 1 and null pointers"""
    torch, dev = _torch()
    eng = _eng()
    from gpbayestools_hic_amd import _native as nat
    x = torch.zeros((1, 8), dtype=torch.float64, device=dev)
    k = torch.zeros(1, dtype=torch.float64, device=dev)
    big = (1 << 24) + 1
    assert eng.lib.gpb_psis(eng.h, nat.ptr(x), 1, big, big, 1, nat.ptr(k), None, None, None) == E_ARG
    assert b"2^24" in eng.lib.gpb_last_error(eng.h)
    assert eng.lib.gpb_psis_loo(eng.h, nat.ptr(x), None, 1, big, big, 1, nat.ptr(x)) == E_ARG
    assert eng.lib.gpb_psis(eng.h, nat.ptr(x), 1, 8, 7, 1, nat.ptr(k), None, None, None) == E_ARG
    assert eng.lib.gpb_psis(eng.h, nat.ptr(x), 0, 8, 8, 1, nat.ptr(k), None, None, None) == E_ARG
    assert eng.lib.gpb_psis(eng.h, None, 1, 8, 8, 1, nat.ptr(k), None, None, None) == E_ARG
    assert eng.lib.gpb_psis_loo(eng.h, nat.ptr(x), None, 1, 8, 8, 1, None) == E_ARG
    assert float(k[0]) == 0.0
    with pytest.raises(ValueError):
        eng.psis(x, S=9)
    with pytest.raises(ValueError):
        eng.psis(x.cpu())
    with pytest.raises(ValueError):
        eng.psis(x, outputs=("khat", "nope"))
    with pytest.raises(ValueError):
        eng.psis_loo(x, np.zeros((1, 8)))
    assert 1 << 24 == eng.PSIS_MAX_S
