"""CPU tier: the host model of the sequential design (tests/design_reference.py) against itself by brute force — the rank-one
score J(c) must be the drop of the averaged posterior variance when candidate c joins the design and the GPs are refitted (a
fresh Cholesky per candidate), at every step of the greedy loop."""
import numpy as np
import pytest

import design_reference as R

# (N, d, P, C, R, T, seed, kernel)
CASES = [
    (30, 1, 1, 16, 15, 4, 1, "RBF"),
    (40, 3, 2, 20, 25, 4, 2, "RBF"),
    (35, 4, 3, 16, 16, 3, 3, "RBF"),
    (40, 3, 2, 20, 25, 3, 4, "Matern"),
    (40, 3, 2, 20, 25, 3, 5, "Matern25"),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-N%d-d%d-P%d" % (c[7], c[0], c[1], c[2]))
def test_rank_one_scores_are_the_refit_drop(case):
    N, d, P, C, Rn, T, seed, kernel = case
    c = R.make_case(N, d, P, C, Rn, seed, kernel)
    args = (c["X"], c["theta"], kernel, c["Xc"], c["Xr"], c["w"], c["g"])
    m = R.greedy(*args, T)
    assert np.all(m["gain"] >= 0.0)
    chosen, el, worst = [], np.ones(C, dtype=bool), 0.0
    for t in range(T):
        J, base = R.refit_scores(*args, chosen)
        if t == 0:
            assert abs(base - m["variance0"]) <= 1e-12 * m["variance0"]
        top = J[el].max()
        worst = max(worst, np.abs(m["scores"][t][el] - J[el]).max() / top)
        assert np.all(np.abs(m["scores"][t][el] - J[el]) <= 1e-11 * top)
        assert np.all(np.isneginf(m["scores"][t][~el]))
        b = int(np.argmax(np.where(el, J, -np.inf)))
        assert b == m["picks"][t] and m["gain"][t] == m["scores"][t][b]
        chosen.append(b)
        el[b] = False
    final = R.refit_scores(*args, chosen)[1]
    print("rank-one against refit: largest gap %.3g max J" % worst)
    assert abs((m["variance0"] - m["gain"].sum()) - final) <= 1e-11 * m["variance0"]


def test_eligibility_and_gaps():
    c = R.make_case(30, 2, 2, 20, 10, 7)
    args = (c["X"], c["theta"], "RBF", c["Xc"], c["Xr"], c["w"], c["g"])
    free = R.greedy(*args, 3)
    el = np.ones(20, dtype=bool)
    el[free["picks"][0]] = False
    masked = R.greedy(*args, 3, eligible=el)
    assert free["picks"][0] not in masked["picks"] and len(set(masked["picks"])) == 3
    assert np.array_equal(masked["scores"][0][el], free["scores"][0][el])            # step 0 differs in the mask alone
    assert np.all(free["gaps"] > 0.0) and np.all(np.isfinite(free["gaps"]))
    order = np.sort(free["scores"][0])[::-1]
    assert free["gaps"][0] == (order[0] - order[1]) / order[0]
    assert np.isinf(R.greedy(*args, 20)["gaps"][-1])                                  # one candidate left
