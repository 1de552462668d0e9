"""CPU tier: design.Design against the reference's own Design (src/design.py) on the same cache file — tests/golden/g13_design.npz
(tools/make_goldens.py) holds the seeded 12 x 4 cache array, a three-parameter file and what the reference made of them: arrays bit
for bit, written files byte for byte.  With the cache file present no design is generated, so this needs no GPU."""
import os

import numpy as np
import pytest

from conftest import REPO
from gpbayestools_hic_amd import design as D


@pytest.fixture(scope="module")
def g13():
    with np.load(os.path.join(REPO, "tests", "golden", "g13_design.npz")) as z:
        return {k: z[k] for k in z.files}


def _seeded(g13, root):
    n, seed = int(g13["npoints"]), int(g13["seed"])
    cache = root / "cache" / "lhs"
    cache.mkdir(parents=True)
    np.save(cache / "npoints{}_ndim3_seed{}.npy".format(n, seed), g13["cache"])
    par = root / "pars.txt"
    par.write_text(str(g13["parfile"]))
    return n, seed, cache, par


@pytest.mark.parametrize("validation", [False, True])
def test_design_matches_the_reference_bit_for_bit(g13, tmp_path, validation):
    n, seed, cache, par = _seeded(g13, tmp_path)
    des = D.Design(str(par), npoints=n, validation=validation, seed=seed, cache_dir=cache)
    k = "val_" if validation else "main_"
    assert des.type == str(g13[k + "type"]) and des.ndim == int(g13[k + "ndim"])
    assert list(des.pardict.keys()) == list(g13[k + "keys"]) and des.points == list(g13[k + "points"])
    assert np.array_equal(des.min, g13[k + "min"]) and np.array_equal(des.max, g13[k + "max"])
    assert des.array.dtype == np.float64 and np.array_equal(des.array, g13[k + "array"])
    assert np.array_equal(np.asarray(des), g13[k + "asarray"])
    des.write_files(tmp_path / "out")
    written = sorted(os.listdir(tmp_path / "out" / des.type))
    assert written == des.points
    for name in (des.points[0], des.points[-1]):
        assert (tmp_path / "out" / des.type / name).read_text() == str(g13[k + "file_" + name])


def test_generate_lhs_reads_the_cache_under_workdir(g13, tmp_path, monkeypatch):
    n, seed, cache, _ = _seeded(g13, tmp_path)
    monkeypatch.setenv("WORKDIR", str(tmp_path))
    assert np.array_equal(D.generate_lhs(n, 3, seed), g13["cache"])                # <$WORKDIR>/cache/lhs, as the reference
    assert np.array_equal(D.generate_lhs(n, 3, seed, cache_dir=cache), g13["cache"])
    monkeypatch.setenv("WORKDIR", str(tmp_path / "elsewhere"))
    import gpbayestools_hic_amd  # noqa: F401
    assert not (tmp_path / "elsewhere").exists()                                    # nothing is created at import or by a look-up


def test_time_based_seed_is_printed(g13, tmp_path, capsys, monkeypatch):
    n, seed, cache, par = _seeded(g13, tmp_path)

    class Clock:
        @staticmethod
        def now():
            class T:
                @staticmethod
                def timestamp():
                    return seed
            return T
    monkeypatch.setattr(D, "datetime", Clock)
    des = D.Design(str(par), npoints=n, cache_dir=cache)
    assert "seed = %d" % seed in capsys.readouterr().out and np.array_equal(des.array, g13["main_array"])


def test_exports():
    import gpbayestools_hic_amd as pkg
    assert pkg.Design is D.Design and pkg.generate_lhs is D.generate_lhs and pkg.MaxProDesign is D.MaxProDesign
    assert {"Design", "generate_lhs"} <= set(pkg.__all__)
