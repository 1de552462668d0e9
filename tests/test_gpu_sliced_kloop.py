"""
GPU tier: the K loop of the int8 predict kernel (csrc/gpb_sliced.hip) at the smallest shapes where its index arithmetic
(csrc/sl_index.h) can go wrong — the DMA sources a wave sets once per tile and moves by a stride, from a K range that may begin
behind the design's front padding and end at a ragged row block — against the exact host integer model of
tests/int8_reference.py, BIT FOR BIT (np.array_equal, no tolerance), as check_against_model of tests/test_gpu_int8_exact.py does.
A source one stride off reads another K-step's digits and changes integer level sums, and so bits
(tests/test_int8_reference.py: a zeroed K range is resolved).  tests/host/sl_index_check.cpp proves the same arithmetic on the host
for every geometry; this file holds the compiled kernels to it.
"""
import numpy as np
import pytest

import int8_reference as R
from test_gpu_int8_exact import check_against_model, _engine

pytestmark = pytest.mark.gpu

CASES = [                       # (N, d, P, kernel, W)
    (97, 3, 2, "RBF", 65),      # Np = 128, front padding 16: one row block, every step lies in the diagonal block
    (128, 4, 1, "RBF", 1),      # one walker
    (150, 4, 2, "Matern25", 33),    # Np = 192, front padding 32: the second row block starts at k_begin = 32 and is ragged
    (230, 5, 2, "RBF", 130),    # Np = 256, front padding 16 rounds to no skipped K-step
    (256, 4, 3, "RBF", 64),
    (384, 6, 2, "RBF", 70),     # three row blocks: steps in front of the diagonal block and inside it
]
SIX_PLANE_CASES = [CASES[0], CASES[2], CASES[5]]
_ids = lambda s: "N%d-P%d-%s-W%d" % (s[0], s[2], s[3], s[4])


def _problem(case):
    N, d, P, kind, W = case
    return R.problem(N, d, P, kind, W, seed=N + W)


def test_the_cases_have_the_geometry_they_are_named_for():
    geo = [(R.padded_size(c[0]), R.pad_front(R.padded_size(c[0]), c[0])) for c in CASES]
    assert geo == [(128, 16), (128, 0), (192, 32), (256, 16), (256, 0), (384, 0)]


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_seven_planes_bit_for_bit(case):
    X, Z, th, Xs = _problem(case)
    eng = _engine(X, Z, th, case[3])
    check_against_model(eng, "K loop, seven planes N=%d d=%d P=%d %s W=%d" % case, th, Xs, 3)
    eng.close()


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("case", SIX_PLANE_CASES, ids=_ids)
def test_six_planes_bit_for_bit_on_both_tiles(case, tile):
    """option value 2 with the walker tile forced: 64 (one 32-walker n-tile per wave) and 128 (two)"""
    X, Z, th, Xs = _problem(case)
    eng = _engine(X, Z, th, case[3])
    eng.force_tile(tile)
    check_against_model(eng, "K loop, six planes, tile %d N=%d d=%d P=%d %s W=%d" % ((tile,) + case), th, Xs, 2)
    eng.force_tile(0)
    eng.close()


def test_two_emulators_in_one_launch_equal_their_own_launches(tmp_path):
    """two emulators of N = 150 (Np = 192, front padding 32) with 2 and 3 GPs in one chain: the shared launch over the five GPs
    (k_predict_sliced_multi) gives the log-posterior of one launch per emulator, bit for bit; rows outside the box make the batch
    a compacted one (the live walker tiles come from the device's row count)"""
    import ctypes
    from gpbayestools_hic_amd import synth
    from gpbayestools_hic_amd.workload import build_multi_chain
    d = 4
    chain, emus, info = build_multi_chain([(150, 12, 2, "RBF"), (150, 10, 3, "Matern25")], d, workdir=str(tmp_path))
    chain.set_predict_arithmetic("fp64-int8")
    engs = [e._engine_ready() for e in emus]
    assert all(g.predict_sliced == 3 for g in engs)
    X = synth.walkers(200, d, seed=11)
    X[::9, 2] = 1.5                                              # outside the box
    X[5, 0] = 0.0                                                # on the boundary: outside
    for g in engs:
        g.tune("chain_batch", 1)
    shared = chain.log_posterior(X)
    assert engs[0].lib.gpb_chain_supported((ctypes.c_void_p * 2)(*[g.h for g in engs]), 2) == 1      # one call of the C ABI took it
    fin = np.isfinite(shared)
    assert 0 < fin.sum() < len(X) and not fin[0] and not fin[5]
    for g in engs:
        g.tune("chain_batch", 0)
    chain.__dict__.pop("_digest_cache", None)
    own = chain.log_posterior(X)
    assert np.array_equal(shared, own)
    assert np.array_equal(chain.log_posterior(X[fin]), own[fin])  # compaction does not change a row's bits
