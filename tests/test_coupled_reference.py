"""CPU tier of the coupled chain likelihood: the torch restatement in tests/coupled_reference.py reproduces the oracle's
log-posterior under a FULL experimental covariance (oracle.log_prob with chain_predict) and, for a block-diagonal one, the
block restatement of tests/grad_reference.py — so that the GPU tier can hold the device values and gradients against it."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import coupled_reference as CR  # noqa: E402
import grad_reference as R  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402
from test_grad_reference import D, M, _case  # noqa: E402


def _two():
    e1, y1, c1, Xw = _case(O.KIND_RBF, O.MODE_PCA)
    e2, y2, c2, _ = _case(O.KIND_MATERN25, O.MODE_PCA, seed=1)
    yexp = np.concatenate([y1, y2])
    sigma = 0.05 * np.abs(yexp)
    Xw[1, 2] = 1.3                                            # one row outside the box
    return [e1, e2], yexp, sigma, Xw


@pytest.mark.parametrize("which", ["a", "b"])
def test_restatement_matches_the_oracle_under_a_full_covariance(which):
    emus, yexp, sigma, Xw = _two()
    cexp = CR.cov_a(yexp, sigma) if which == "a" else CR.cov_b(sigma)
    assert np.any(cexp[:M, M:] != 0.0)                        # it does couple the two emulators
    ref = O.log_prob(Xw, np.zeros(D), np.ones(D), lambda x, e: O.chain_predict(emus, x, e), yexp, cexp)
    sts = [R.state_from_oracle(e) for e in emus]
    got = CR.log_posterior(sts, R._t(Xw), np.zeros(D), np.ones(D), yexp, cexp).numpy()
    ins = np.isfinite(ref)
    assert ins.sum() == len(Xw) - 1 and np.array_equal(np.isneginf(got), ~ins)
    assert np.max(np.abs(got[ins] - ref[ins]) / np.maximum(np.abs(ref[ins]), 1.0)) < 1e-12
    # the coupling matters: the block-diagonal part alone gives another number
    blocks = np.zeros_like(cexp); blocks[:M, :M] = cexp[:M, :M]; blocks[M:, M:] = cexp[M:, M:]
    other = R.log_posterior(sts, R._t(Xw), np.zeros(D), np.ones(D), yexp, blocks).numpy()
    assert np.min(np.abs(other[ins] - ref[ins])) > 1e-3


def test_block_diagonal_covariance_gives_the_block_restatement_and_its_gradient():
    emus, yexp, sigma, Xw = _two()
    cexp = np.diag(sigma ** 2)
    cexp[:M, :M] += np.outer(0.03 * yexp[:M], 0.03 * yexp[:M])        # correlated inside the first block only
    sts = [R.state_from_oracle(e) for e in emus]
    box = (np.zeros(D), np.ones(D))
    v1, g1 = R.value_and_grad(lambda x: CR.log_posterior(sts, x, *box, yexp, cexp), Xw)
    v2, g2 = R.value_and_grad(lambda x: R.log_posterior(sts, x, *box, yexp, cexp), Xw)
    ins = np.isfinite(v2)
    assert np.array_equal(np.isfinite(v1), ins)
    assert np.max(np.abs(v1[ins] - v2[ins]) / np.maximum(np.abs(v2[ins]), 1.0)) < 1e-12
    assert np.max(np.abs(g1 - g2)) / max(np.max(np.abs(g2)), 1.0) < 1e-10
    assert np.all(g1[~ins] == 0.0)
