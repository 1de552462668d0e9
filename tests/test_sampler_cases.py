"""CPU tier of tests/sampler_cases.py: the torch restatement of the parameter map, whose autograd gradient the GPU tier holds
the device to, against the numpy map the emulators use (param_pca.ParameterPCA.transform)."""
import numpy as np
import torch

from conftest import golden
from sampler_cases import _torch_param_map


def test_torch_parameter_map_is_the_numpy_map():
    from gpbayestools_hic_amd import synth
    from gpbayestools_hic_amd.param_pca import ParameterPCA
    g = golden("g7_param_pca.npz")
    for d in (20, 71):
        lo, hi = np.concatenate([g["lo"], np.zeros(d - 20)]), np.concatenate([g["hi"], np.ones(d - 20)])
        X = synth.lhs(80, d, seed=5, lo=lo, hi=hi)
        ppca = ParameterPCA(X, lo, hi)
        Q = lo + (hi - lo) * np.random.default_rng(2).uniform(0.02, 0.98, (16, d))
        ref = ppca.transform(Q)
        got = _torch_param_map(ppca, torch.as_tensor(Q)).numpy()
        assert got.shape == ref.shape == (16, d - 10 + sum(ppca.n_components))
        assert np.max(np.abs(got - ref)) <= 1e-13 * max(1.0, np.abs(ref).max())
