"""Chains the sampler tests (tests/test_gpu_smc.py, tests/test_gpu_ptlmc.py) share — a helper module, not a test file: a chain
of more parameters than its GPs have inputs (wide_chain), a real parameterTrafoPCA emulator over d > 64 parameters
(mapped_chain) and the float64 torch restatement of that emulator's log-posterior, parameter map included
(mapped_log_posterior), whose gradient comes from autograd through tests/grad_reference.py."""
import numpy as np


def wide_chain(tmp, D):
    """a chain of D parameters: one parameterTrafoPCA emulator trained over 20 of them whose device map (gpb_param_map_set)
    is told that the rows have D columns.  The GPs take at most 64 inputs and the map drops only a few columns, so an
    Emulator trained over D > ~70 parameters does not exist; the C ABI's map reads any columns of a wider row, which is how
    a chain gets more parameters than its GPs have inputs.  The likelihood is flat in columns 20 .. D - 1, the box is not."""
    from gpbayestools_hic_amd import _native as nat
    from gpbayestools_hic_amd import param_pca as pp
    from gpbayestools_hic_amd.workload import build_multi_chain
    chain, emus, info = build_multi_chain([(128, 12, 3, "RBF")], 20, workdir=tmp, mapped=True)
    emu = emus[0]
    eng = emu._engine_ready()
    groups = emu._ppca.groups
    G, maxpc = len(groups), int(max(g.pca.n_components_ for g in groups))
    cols = np.arange(20, dtype=np.int64)          # the column bookkeeping of GPEngine.set_param_map over the trained 20
    desc = np.full((G, 6), -1, dtype=np.int32)
    tab = np.zeros((G, 4 + maxpc, 100))
    for gi, (g, idx, grid) in enumerate(zip(groups, (pp.IDX_BULK, pp.IDX_SHEAR, pp.IDX_YLOSS),
                                            (pp.T_GRID, pp.MUB_GRID, pp.YINIT_GRID))):
        k = int(g.pca.n_components_)
        cols = np.concatenate((np.delete(cols, idx), -1 - (gi * maxpc + np.arange(k))))
        desc[gi, 0], desc[gi, 1:1 + len(idx)], desc[gi, 5] = gi, idx, k
        tab[gi, 0], tab[gi, 1], tab[gi, 2], tab[gi, 3] = grid, g.scaler.mean_, g.scaler.scale_, g.pca.mean_
        tab[gi, 4:4 + k] = g.pca.components_
    col_src = np.ascontiguousarray(cols, dtype=np.int32)
    assert col_src.shape[0] == eng.pmap_d_out
    eng._ck(eng.lib.gpb_param_map_set(eng.h, D, eng.pmap_d_out, nat.ptr(col_src), G, nat.ptr(np.ascontiguousarray(desc)),
                                      nat.ptr(np.ascontiguousarray(tab)), maxpc))
    eng.pmap_d_in = D
    chain.ndim = D
    chain.min, chain.max = np.zeros(D), np.ones(D)
    chain.prior_volume_ = 1.0
    return chain


def wide_start(D):
    """the truth point of wide_chain's 20 trained parameters, 0.5 in the columns the likelihood is flat in"""
    from gpbayestools_hic_amd import synth
    return np.concatenate((synth.truth_point(20), np.full(D - 20, 0.5)))


def mapped_chain(tmp_path, d):
    """a real parameterTrafoPCA emulator over d >= 20 parameters (the construction of
    test_gpu_multi_emulator.test_chain_with_more_than_64_parameters): one varying parameter per mapped group, so one principal
    component each and d - 7 GP inputs; the experiment is the prediction at the box's centre -> (chain, emu, centre)"""
    from conftest import golden
    from gpbayestools_hic_amd import Chain, Emulator, synth
    g = golden("g7_param_pca.npz")
    lo, hi = np.concatenate([g["lo"], np.zeros(d - 20)]), np.concatenate([g["hi"], np.ones(d - 20)])
    X = synth.lhs(80, d, seed=5, lo=lo, hi=hi)
    mid = 0.5 * (lo + hi)
    for group in ([15, 16, 17, 18], [12, 13, 14], [2, 3, 4]):
        X[:, group[1:]] = mid[group[1:]]
    Y = synth.observables((X - lo) / (hi - lo), 6, seed=11)
    tp, pf, ep = str(tmp_path / "t.pkl"), str(tmp_path / "p.txt"), str(tmp_path / "e.pkl")
    synth.write_training_pickle(tp, X, Y, 0.01)
    synth.write_parameter_file(pf, lo, hi)
    emu = Emulator(training_set_path=tp, parameter_file=pf, npc=3, parameterTrafoPCA=True)
    assert emu.PCA_new_design_points.shape == (80, d - 7)
    emu.trainEmulator([True] * emu.nev, thetas=synth.fixed_theta(d - 7, 3, ell=3.0))
    yexp = emu.predict(mid[None], return_cov=False)[0]
    synth.write_experiment_pickle(ep, yexp, 0.05 * np.abs(yexp))
    chain = Chain(mcmc_path=str(tmp_path / "mcmc" / "c.pkl"), expdata_path=ep, model_parafile=pf)
    chain.emuList = [emu]
    return chain, emu, mid


def _torch_param_map(ppca, X):
    """param_pca.ParameterPCA.transform on a torch tensor [W, d]: the three parametrised functions on their 100-point grids,
    standardised and projected on the fitted components; each group's columns deleted, its components appended"""
    import torch
    from gpbayestools_hic_amd import param_pca as pp
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64)       # noqa: E731

    def bulk(p):
        zmax, T0, sp, sm = (p[:, i:i + 1] for i in range(4))
        T = t(pp.T_GRID)[None, :]
        sig = torch.where(T < T0, sm, sp)
        return zmax * torch.exp(-(T - T0) ** 2.0 / (2.0 * sig ** 2.0))

    def shear(p):
        e0, e2, e4 = (p[:, i:i + 1] for i in range(3))
        m = t(pp.MUB_GRID)[None, :]
        return torch.where((0.0 < m) & (m <= 0.2), e0 + (e2 - e0) * (m / 0.2),
                           torch.where((0.2 < m) & (m < 0.4), e2 + (e4 - e2) * ((m - 0.2) / 0.2), e4 + 0.0 * m))

    def yloss(p):
        y2, y4, y6 = (p[:, i:i + 1] for i in range(3))
        y = t(pp.YINIT_GRID)[None, :]
        return torch.where((0.0 < y) & (y <= 2.0), y2 * (y / 2.0),
                           torch.where((2.0 < y) & (y < 4.0), y2 + (y4 - y2) * ((y - 2.0) / 2.0),
                                       y4 + (y6 - y4) * ((y - 4.0) / 2.0)))

    new = X
    for g, fn in zip(ppca.groups, (bulk, shear, yloss)):
        z = (fn(X[:, g.idx]) - t(g.scaler.mean_)) / t(g.scaler.scale_)
        pcs = (z - t(g.pca.mean_)) @ t(g.pca.components_).T
        keep = [c for c in range(new.shape[1]) if c not in g.idx]
        new = torch.cat((new[:, keep], pcs), dim=1)
    return new


def mapped_log_posterior(chain, emu):
    """torch X [W, d] -> the log-posterior of a one-emulator chain whose emulator maps its parameters: the box in the chain's
    parameters, grad_reference.block_loglike on the mapped rows (the GP factors are the oracle's own, nothing is read back
    from the device)"""
    import torch
    import grad_reference as G
    from oracle import gp_oracle as O
    st = G.state_from_emulator(emu)
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64)       # noqa: E731
    lo, hi, yexp, cexp = t(chain.min), t(chain.max), t(chain.expdata).reshape(-1), t(chain.expdata_cov)

    def f(X):
        inside = ((X > lo) & (X < hi)).all(1)
        ll = G.block_loglike(st, _torch_param_map(emu._ppca, X), yexp, cexp) + O.EXTRA_STD_CONST
        return torch.where(inside, ll, torch.full_like(ll, -np.inf))
    return f
