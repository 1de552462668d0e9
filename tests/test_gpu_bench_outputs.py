"""GPU tier: a plain bench.py run (no --full) times the headline alone and, with --dump-outputs DIR, writes what the timed steps
computed — the final ensemble a caller of StretchSampler.run receives — as float64 .npy files that hash to the line's
ensemble_checksum."""
import hashlib
import os
import sys

import numpy as np
import pytest

from conftest import REPO
from test_gpu_bench_ranks import _run

pytestmark = pytest.mark.gpu


def test_plain_bench_dumps_the_timed_ensemble(tmp_path):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "GPB_BENCH_ONE_RANK_SHARDED"):
        env.pop(k, None)
    out = str(tmp_path / "out")
    line = _run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                 "--dump-outputs", out], env, "plain_dump")
    assert line["steps"] == 3 and line["warmup"] == 2 and line["dtype"] == "f64" and line["higher_is_better"] is True
    assert "extras" not in line and "cpu_baseline" not in line                  # --full only
    assert line["rows_inside_box_fraction"] >= 0.95
    nw = line["config"]["walkers"]
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 / nw - 1.0) < 1e-9    # value = walkers x steps / timed seconds
    assert sorted(os.listdir(out)) == ["acceptance_fraction.npy", "log_prob.npy", "positions.npy"]
    pos, lp, acc = (np.load(os.path.join(out, n + ".npy")) for n in ("positions", "log_prob", "acceptance_fraction"))
    assert pos.dtype == lp.dtype == acc.dtype == np.float64
    assert pos.shape == (nw, 20) and lp.shape == (nw,) and acc.shape == (nw,)
    assert np.all(np.isfinite(pos)) and np.all(np.isfinite(lp)) and np.all((acc >= 0) & (acc <= 1))
    assert hashlib.sha256(pos.tobytes() + lp.tobytes()).hexdigest()[:16] == line["ensemble_checksum"]
    assert float(acc.mean()) == line["acceptance_fraction"]
