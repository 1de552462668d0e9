"""What setting a context up costs: GPEngine() + set_data + close over and over (the buffer cache of csrc/gpb_pool.hip exists for
this: trainings create and destroy contexts all the time), and set_data on a context that already holds GPs of another shape.
Prints one JSON line of median / min / max milliseconds per case:  python tools/micro/setup_cost.py [repetitions]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def _ms(fn, reps, warm=3):
    import torch
    t = []
    for _ in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    t = np.array(t[warm:])
    return dict(median=round(float(np.median(t)), 4), min=round(float(t.min()), 4), max=round(float(t.max()), 4))


def main(reps=30):
    from gpbayestools_hic_amd import GPEngine, synth
    d = 12
    out = {}
    for P in (63, 7):
        data = {N: (synth.lhs(N, d), np.ascontiguousarray(synth.observables(synth.lhs(N, d), P).T)) for N in (1000, 900)}

        def fresh():
            eng = GPEngine(0)
            eng.set_data(*data[1000])
            eng.sync()
            eng.close()

        out["create_set_close_ms_P%d" % P] = _ms(fresh, reps)
        eng = GPEngine(0)
        flip = [0]

        def reset():
            flip[0] ^= 1
            eng.set_data(*data[900 if flip[0] else 1000])
            eng.sync()

        out["reset_ms_P%d" % P] = _ms(reset, reps)
        eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 30)
