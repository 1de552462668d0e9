"""
gpbayestools_hic_amd — MI355X-native GP-emulator + MCMC log-posterior engine.

Drop-in for the hot path of Hendrik1704/GPBayesTools-HIC (src/emulator.py fit()/predict() and the
src/mcmc.py log-posterior loop): hand-written HIP kernels for gfx950 behind a C ABI
(include/gpbayes.h, ctypes), Python only for orchestration.  No CPU fallback.
"""
__version__ = "0.1.0"

__all__ = ["Emulator", "Chain", "mvn_loglike", "GPEngine", "StretchSampler", "LoggingEnsembleSampler",
           "WalkerSharding", "rms_relative_error", "honesty", "DesignProposal", "PosteriorMarginals", "PosteriorClusters",
           "posterior_clusters", "Design", "generate_lhs", "MaxProDesign", "maxpro_design", "GoodnessOfFit", "posterior_gof",
           "InformationGain", "PosteriorComparison", "information_gain", "posterior_divergence", "knn_distances",
           "HMCSampler", "EIGResult", "expected_information_gain", "LooResult", "PsisResult", "posterior_loo", "psis",
           "HistoryMatch", "implausibility", "implausibility_maps", "SteinThinning", "SteinDiscrepancy", "stein_thin", "ksd"]


def __getattr__(name):   # lazy: importing the package must not need torch / the built library
    if name == "Emulator":
        from .emulator import Emulator
        return Emulator
    if name in ("rms_relative_error", "honesty", "DesignProposal"):
        from . import emulator
        return getattr(emulator, name)
    if name in ("Chain", "mvn_loglike"):
        from . import mcmc
        return getattr(mcmc, name)
    if name == "GPEngine":
        from .engine import GPEngine
        return GPEngine
    if name in ("StretchSampler", "LoggingEnsembleSampler"):
        from . import sampler
        return getattr(sampler, name)
    if name == "HMCSampler":
        from .hmc import HMCSampler
        return HMCSampler
    if name in ("PosteriorMarginals", "marginals"):       # (`marginals` is the submodule; the function is marginals.marginals)
        import importlib
        mod = importlib.import_module(".marginals", __name__)
        return mod if name == "marginals" else mod.PosteriorMarginals
    if name in ("PosteriorClusters", "posterior_clusters"):
        from . import clusters
        return getattr(clusters, name)
    if name in ("GoodnessOfFit", "posterior_gof"):
        from . import gof
        return getattr(gof, name)
    if name in ("InformationGain", "PosteriorComparison", "information_gain", "posterior_divergence", "knn_distances"):
        from . import divergence
        return getattr(divergence, name)
    if name in ("LooResult", "PsisResult", "posterior_loo", "psis"):
        from . import loo
        return getattr(loo, name)
    if name in ("HistoryMatch", "implausibility", "implausibility_maps"):
        from . import history
        return getattr(history, name)
    if name in ("SteinThinning", "SteinDiscrepancy", "stein_thin", "ksd"):
        from . import thinning
        return getattr(thinning, name)
    if name in ("EIGResult", "expected_information_gain"):
        from . import eig
        return getattr(eig, name)
    if name in ("Design", "generate_lhs", "MaxProDesign", "maxpro_design"):
        import importlib
        return getattr(importlib.import_module(".design", __name__), name)
    if name == "WalkerSharding":
        from .dist import WalkerSharding
        return WalkerSharding
    raise AttributeError(name)
