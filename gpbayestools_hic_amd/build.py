"""Build the HIP extension in-tree: gpbayestools_hic_amd/libgpbayes.so (gfx950 only)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libgpbayes.so")
LIB_DEBUG = os.path.join(HERE, "libgpbayes_debug.so")
SOURCES = ["gpb_api.hip", "gpb_fit.hip", "gpb_chol.hip", "gpb_predict.hip", "gpb_sliced.hip", "gpb_like.hip", "gpb_coupled.hip", "gpb_chain.hip", "gpb_stretch.hip", "gpb_sets.hip", "gpb_cov.hip", "gpb_pmap.hip", "gpb_pool.hip",
           "gpb_grad.hip", "gpb_ptlmc.hip", "gpb_smc.hip", "gpb_cv.hip", "gpb_sobol.hip", "gpb_design.hip", "gpb_ppd.hip", "gpb_diag.hip", "gpb_rank.hip", "gpb_marg.hip", "gpb_kmeans.hip", "gpb_maxpro.hip", "gpb_curves.hip", "gpb_sens.hip", "gpb_gof.hip", "gpb_knn.hip", "gpb_hmc.hip", "gpb_eig.hip", "gpb_loo.hip", "gpb_psis.hip", "gpb_hm.hip", "gpb_stein.hip"]
# per-source compiler flags.  gpb_sens.hip: its two-double dot products and its bit-for-bit R / I formulas hold only if no product
# is fused into a sum (hipcc's default -ffp-contract=fast fuses in the backend, past pragmas and the __d*_rn intrinsics);
# gpb_gof.hip carries the same two-double dot products; gpb_knn.hip's squared distance is acc = acc + t * t, two roundings, which
# a numpy model reproduces bit for bit; gpb_hmc.hip: the kick, the drift and the kinetic energy of hmc_step.h, restated bit for bit;
# gpb_eig.hip: the simulated data y = mu + sqrt(s) z, two roundings, which numpy reproduces from the returned z;
# gpb_rank.hip: np.quantile's interpolation lo + (hi - lo) g, two roundings; gpb_loo.hip carries gpb_gof.hip's two-double dot
# products; gpb_psis.hip: the fit of psis_fit.h, whose host check runs the same operations in the same order; gpb_hm.hip: the candidate
# rows x = lo + (hi - lo) u, two roundings after the subtraction, and I = |y - mu| / sqrt(var + vadd), which numpy reproduces bit for bit;
# gpb_stein.hip: the four sums of a pair, q = q + r * h and its like, and kp's polynomial in 1 / sqrt(q), one rounding per operation
SOURCE_FLAGS = {"gpb_sens.hip": ["-ffp-contract=off"], "gpb_gof.hip": ["-ffp-contract=off"], "gpb_knn.hip": ["-ffp-contract=off"],
                "gpb_hmc.hip": ["-ffp-contract=off"], "gpb_eig.hip": ["-ffp-contract=off"], "gpb_rank.hip": ["-ffp-contract=off"],
                "gpb_loo.hip": ["-ffp-contract=off"], "gpb_psis.hip": ["-ffp-contract=off"], "gpb_hm.hip": ["-ffp-contract=off"], "gpb_stein.hip": ["-ffp-contract=off"]}
HEADERS = ["gpb_internal.h", "dispatch.h", "dev_buf.h", "ws_carve.h", "ws_layout.h", "coupled_setup.h", "lowrank_setup.h", "stretch_move.h", "sl_index.h", "gemm_tile.h", "block_reduce.h", "chol_block.h", "fast_math.h", "philox.h", "maxpro_index.h", "curve_fn.h", "order_key.h", "diag_gram.h", "ndtri.h", "chi2_sf.h", "knn_plan.h", "hmc_step.h", "eig_plan.h", "psis_fit.h", "stein_plan.h", os.path.join("..", "..", "include", "gpbayes.h"),
           os.path.join("..", "..", "include", "gpbayes_debug.h")]


def _stale(lib=LIB):
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    return any(os.path.getmtime(os.path.join(CSRC, f)) > t for f in SOURCES + HEADERS)


def build_native(force=False, verbose=False, debug_variants=False):
    """libgpbayes.so: the product library (the kernels its own rules select).  debug_variants=True: libgpbayes_debug.so,
    the same sources with -DGPB_DEBUG_VARIANTS — every measured-and-rejected kernel variant behind its gpb_ctx_option key and
    the test hooks of include/gpbayes_debug.h, for the sweeps in tools/ and the tests that need them (GPB_DEBUG_LIB=1, or
    _native.debug_library() for one test)."""
    lib = LIB_DEBUG if debug_variants else LIB
    if not force and not _stale(lib):
        return lib
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    procs = []
    bdir = os.path.join(HERE, "build", "debug" if debug_variants else "product")
    os.makedirs(bdir, exist_ok=True)
    for src in SOURCES:
        obj = os.path.join(bdir, src.replace(".hip", ".o"))
        # -fvisibility=hidden: the library exports the entry points of include/gpbayes.h (GPB_API) and, in the debug build,
        # include/gpbayes_debug.h — nothing of the C++ inside
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-c",
               os.path.join(CSRC, src), "-o", obj] + SOURCE_FLAGS.get(src, []) + (["-DGPB_DEBUG_VARIANTS"] if debug_variants else [])
        if debug_variants:
            cmd += os.environ.get("GPB_DEBUG_EXTRA_DEFINES", "").split()      # A/B builds of the debug library only
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
        objs.append(obj)
    for cmd, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError("hipcc failed: %s\n%s" % (" ".join(cmd), out.decode()))
    # -Bsymbolic: the entry points call each other inside their own library, so that the product and the debug build can be
    # loaded into one process side by side (tests that need the debug hooks, _native.debug_library())
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,-Bsymbolic", "-o", lib] + objs + ["-ldl"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError("link failed: %s\n%s" % (" ".join(cmd), r.stdout.decode()))
    return lib


if __name__ == "__main__":
    print(build_native(force="--force" in sys.argv, verbose=True))
    if "--debug-variants" in sys.argv:
        print(build_native(force="--force" in sys.argv, verbose=True, debug_variants=True))
