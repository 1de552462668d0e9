"""
GPU tier: the fit's 128-wide tile instantiations — k_trtri_level<1|2, 128> and k_syrk<128> (csrc/gpb_fit.hip) — which a fill
rule selects from the number of 128-wide tiles x the GPs of the launch (launch_trtri, launch_syrk_range: at least 16 per CU)
and which two or three GPs at test sizes therefore never reach.  Forced here through their option keys (trtri_tile = 12,
syrk_tile = 14: 0 by rule, 64, 128) at sizes with ragged last groups at every doubling level and a 64-row partial tile of 128:
the source's "same bits either way" is asserted, because the rule reads the GP count of the launch — if the two tiles ever
differed in a bit a GP's factor would depend on its neighbours, which the batched hyper-parameter searches rely on it not
doing (launch_potrf_fused).  Also the panel schedule with a ragged last panel and lookahead (chol_outer not dividing Np, more
than two panels), otherwise only run from N = 1024 up.  Bars: those of test_g1_kernel_matrix_via_factor and
test_cholesky_schedules_agree.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P, D, KERNEL = 3, 4, "Matern25"
TUNED = (("trtri_tile", 0), ("syrk_tile", 0), ("chol_outer", 0), ("chol_lookahead", 1))


def _data(N, seed):
    from gpbayestools_hic_amd import synth
    rng = np.random.default_rng(seed)
    X = synth.lhs(N, D, seed=seed)
    Z = np.sin(X @ rng.standard_normal((D, P))).T + 0.05 * rng.standard_normal((P, N))
    th = synth.fixed_theta(D, P) + 0.1 * rng.standard_normal((P, D + 2))
    return X, Z, th


def _engine(N, alpha=0.1):
    from gpbayestools_hic_amd import GPEngine
    X, Z, th = _data(N, seed=N)
    eng = GPEngine(0)
    eng.set_data(X, Z, KERNEL, alpha=alpha)
    eng.set_theta(th)
    return eng, X, Z, th


def _restore(eng):
    for key, value in TUNED:
        eng.tune(key, value)


def _oracle_factors(X, th, alpha=0.1):
    from oracle import gp_oracle as O
    return [np.linalg.cholesky(O.kernel_train(X, th[p], O.KIND_MATERN25, alpha)) for p in range(P)]


@pytest.mark.parametrize("N", [130, 320, 704])
def test_triangular_inverse_tiles_give_the_same_bits(N):
    """Np = 192, 320, 704: the last group of every doubling level is ragged (n2 < hs) or absent, and 128-wide tiles end in a
    64-row partial one.  L^-1 by 64-wide tiles, by 128-wide tiles and by the rule: bit-equal; L is not touched; L^-1 L = I"""
    eng, X, Z, th = _engine(N)
    try:
        got = {}
        for tile in (64, 128, 0):
            eng.tune("trtri_tile", tile)
            eng.factor()
            got[tile] = (eng.get("L"), eng.get("Linv"))
        for tile in (128, 0):
            assert np.array_equal(got[tile][1], got[64][1]), tile
            assert np.array_equal(got[tile][0], got[64][0]), tile
        Lo = _oracle_factors(X, th)
        for p in range(P):
            L, Linv = got[128][0][p], got[128][1][p]
            assert np.max(np.abs(L - Lo[p])) < 1e-11 * np.max(np.abs(Lo[p]))
            assert np.max(np.abs(Linv @ Lo[p] - np.eye(N))) < 1e-11
            assert np.all(np.triu(Linv, 1) == 0.0) and np.all(np.triu(L, 1) == 0.0)
            assert np.all(np.diag(Linv) > 0)
    finally:
        _restore(eng)
        eng.close()


def test_panel_updates_give_the_same_bits_whatever_the_tile_and_the_stream():
    """N = Np = 704, eleven block columns: outer panels of 64, 128, 192 and 256 columns are 11, 6, 4 and 3 panels (so the
    lookahead side stream has a far part in all four), the last one ragged for 128 (64 columns), 192 (128) and 256 (192); the
    trailing updates start at rows that are odd multiples of 64, so 128-wide tiles end in a partial one.  At equal panel width
    the factor does not depend on the tile of the panel update nor on the stream it runs on, bit for bit; across widths and
    against the one-panel default it agrees to rounding; and it is LAPACK's factor."""
    N = 704
    eng, X, Z, th = _engine(N)
    try:
        eng.factor()
        auto_L, auto_X = eng.get("L"), eng.get("Linv")
        first = {}
        for outer in (64, 128, 192, 256):
            eng.tune("chol_outer", outer)
            for look in (0, 1):
                for tile in (64, 128):
                    eng.tune("chol_lookahead", look); eng.tune("syrk_tile", tile)
                    eng.factor()
                    L, Xi = eng.get("L"), eng.get("Linv")
                    if outer not in first:
                        first[outer] = (L, Xi)
                    else:
                        assert np.array_equal(L, first[outer][0]), (outer, look, tile)
                        assert np.array_equal(Xi, first[outer][1]), (outer, look, tile)
        Lo = _oracle_factors(X, th)
        for outer, (L, Xi) in first.items():
            for other_L, other_X in ((auto_L, auto_X), first[64]):
                assert np.max(np.abs(L - other_L)) < 1e-12 * np.max(np.abs(other_L)), outer
                assert np.max(np.abs(Xi - other_X)) < 1e-11 * np.max(np.abs(other_X)), outer
            for p in range(P):
                assert np.max(np.abs(L[p] - Lo[p])) < 1e-11 * np.max(np.abs(Lo[p])), (outer, p)
        # the panel update did change the schedule's rounding somewhere: the widths are not all the one-panel default's bits
        assert any(not np.array_equal(first[o][0], auto_L) for o in first)
    finally:
        _restore(eng)
        eng.close()


@pytest.mark.parametrize("late", [False, True])
def test_an_indefinite_matrix_is_reported_with_lapacks_info_under_the_wide_panel_update(late):
    """panels of 192 columns with the 128-wide panel update; info is LAPACK dpotrf's, per GP.
    alpha = -1.2: K's diagonal c + sigma_n^2 + alpha is negative for these GPs, the first pivot fails.
    late: alpha = -(sigma_n^2 of the last GP) - 1e-6, so that GP's matrix is c k(X, X) - 1e-6 I and its first non-positive pivot
    (about -1e-6, seven decades above the rounding of the updates) falls in the SECOND panel, behind a panel update, while the
    other two GPs of the launch stay positive definite (info 0)"""
    from oracle import gp_oracle as O
    from scipy.linalg import lapack
    N = 704
    _, _, th = _data(N, seed=N)
    alpha = -(np.exp(th[P - 1, -1]) + 1e-6) if late else -1.2
    eng, X, Z, th = _engine(N, alpha=alpha)
    try:
        eng.tune("chol_outer", 192); eng.tune("syrk_tile", 128)
        info = eng.factor(raise_on_fail=False)
        ref = np.array([lapack.dpotrf(O.kernel_train(X, th[p], O.KIND_MATERN25, alpha), lower=1)[1] for p in range(P)])
        if late:
            assert ref[P - 1] > 192 and np.all(ref[:P - 1] == 0)
        else:
            assert np.all(ref > 0)
        assert np.array_equal(info, ref), (info, ref)
        eng.tune("syrk_tile", 64)
        assert np.array_equal(eng.factor(raise_on_fail=False), info)
    finally:
        _restore(eng)
        eng.close()


def test_lml_and_gradient_do_not_depend_on_the_tiles():
    """what the batched searches rely on: eng.lml(theta), value and gradient, bit-equal between trtri_tile 64 / 128 and
    syrk_tile 64 / 128 — with the one-panel default (no panel update: the triangular inverse's tiles alone) and with panels of
    192 columns (both)"""
    from oracle import gp_oracle as O
    N = 704
    eng, X, Z, th = _engine(N)
    try:
        for outer in (0, 192):
            eng.tune("chol_outer", outer)
            ref = None
            for ttile in (64, 128):
                for stile in (64, 128):
                    eng.tune("trtri_tile", ttile); eng.tune("syrk_tile", stile)
                    val, grad = eng.lml(th)
                    if ref is None:
                        ref = (val.copy(), grad.copy())
                    assert np.array_equal(val, ref[0]) and np.array_equal(grad, ref[1]), (outer, ttile, stile)
            for p in range(P):
                vo, go = O.lml(th[p], X, Z[p], O.KIND_MATERN25, 0.1, eval_gradient=True)
                assert abs(ref[0][p] - vo) < 1e-10 * abs(vo)
                assert np.max(np.abs(ref[1][p] - go)) < 1e-9 * np.max(np.abs(go))
    finally:
        _restore(eng)
        eng.close()
