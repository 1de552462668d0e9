"""Writes tests/golden/g14_maxpro_starts.npz: the starts of the three large trajectory cases of tests/test_gpu_maxpro.py.  A
random hypercube accepts almost every proposal, so a short run from one never rejects a whole block nor accepts in a late slot.
These starts are random hypercubes (np.random.default_rng(4242)) after a pure descent of the host model
(tests/maxpro_reference.py: seed 777, blocks of 32, temperature 1e-9), long enough that about half of the blocks are rejected.

    python tools/make_maxpro_starts.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import maxpro_reference as M  # noqa: E402

DESCENT_BLOCKS = {"n130_d20_R3_B32": 1500, "n20_d64_B64": 600, "n1100_d4_B32": 3000}


def main():
    out = {}
    for name, K in DESCENT_BLOCKS.items():
        n, d, R = M.CASES[name][:3]
        init = M.random_starts(4242, R, n, d)
        res = [M.anneal(init[r], 777, r, 1, K, 32, 1e-9, 1.0) for r in range(R)]
        out[name] = np.array([m["levels"] for m in res], dtype=np.int16)
        print(name, [(m["accepted"], m["consumed"]) for m in res])
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "g14_maxpro_starts.npz"), **out)


if __name__ == "__main__":
    main()
