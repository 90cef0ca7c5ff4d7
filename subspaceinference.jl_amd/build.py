"""Build libsubspace_hip.so (gfx950) in-tree with hipcc.  Used by __graft_entry__.build() and the tests.

The library is plain HIP + C++ (no torch, no Triton, no hipify); it is built next to its sources so that it
travels to the GPU box with the repository snapshot.
"""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libsubspace_hip.so")
ARCH = "gfx950"

# (source, extra flags).  kernels_stream.hip must not contract a*b+c: K1 is bit-exact against the reference's
# three rounded operations.
SOURCES = [
    ("capi.hip", []),
    ("capi_infer.hip", []),
    ("capi_sample.hip", []),
    ("capi_mala.hip", []),
    ("capi_advi.hip", []),
    ("capi_hmc.hip", []),
    ("capi_nuts.hip", []),
    ("capi_ess.hip", []),
    ("capi_train.hip", []),
    ("capi_diffmap.hip", []),
    ("capi_node.hip", []),
    ("capi_ae_train.hip", []),
    ("comm.hip", []),
    ("host_copy.cpp", []),
    ("kernels_stream.hip", ["-ffp-contract=off"]),
    ("kernels_chain.hip", ["-ffp-contract=off"]),
    ("kernels_mala.hip", ["-ffp-contract=off"]),   # (the transition's sums and products are rounded one by one, as the audit forms them)
    ("kernels_hmc.hip", ["-ffp-contract=off"]),    # (likewise: the leapfrog step, the energies and the adaptor's recursions)
    ("kernels_nuts.hip", ["-ffp-contract=off"]),   # (likewise: the leaves, the energies, the U-turn sums and the tree's weights)
    ("kernels_advi.hip", ["-ffp-contract=off"]),   # (likewise: the update's sums, products and quotients, for the bit-for-bit test)
    ("kernels_ess.hip", ["-ffp-contract=off"]),    # (likewise: the bracket's angles and the ellipse's two products and sum)
    # (-amdgpu-mfma-vgpr-form: accumulators stay in VGPRs; the default moved them between the two register files at every
    #  block boundary of the layer loops, 32 copies + a pipeline drain per 16 MFMAs)
    ("kernels_chain_grid.hip", ["-ffp-contract=off", "-mllvm", "-amdgpu-mfma-vgpr-form=1"]),
    ("kernels_chain_grad.hip", ["-ffp-contract=off", "-mllvm", "-amdgpu-mfma-vgpr-form=1"]),
    ("kernels_diffmap.hip", ["-ffp-contract=off"]),   # (Xr = (x - min) * (1 / (max - min)) in three rounded operations: bit-equal to diffmap.py)
    ("kernels_decoder.hip", ["-ffp-contract=off"]),   # (every product and sum rounded as autoencoder.py forms them; W_D = P gives K4's bits)
    ("kernels_node.hip", ["-ffp-contract=off"]),      # (every product and sum rounded as node.py forms them: Tsit5, its interpolant, the controller)
    ("kernels_node_train.hip", ["-ffp-contract=off"]),   # (the training step's tail: the slice sum and the penalty as node.py rounds them; the update is optimiser_update.h's, which carries its own pragma)
    ("kernels_ae_train.hip", ["-ffp-contract=off"]),     # (every product and sum rounded as autoencoder.py: train_step forms them)
    ("kernels_gemm.hip", []),
    ("kernels_gemm_small.hip", []),
    ("kernels_gemm_panel.hip", []),
    ("kernels_gemm_f32.hip", []),
    ("kernels_gram.hip", []),
    ("kernels_gram_wave.hip", ["-DSI_GW_PART=0"], "kernels_gram_wave0"),   # same source, three slices of the tile counts
    ("kernels_gram_wave.hip", ["-DSI_GW_PART=1"], "kernels_gram_wave1"),
    ("kernels_gram_wave.hip", ["-DSI_GW_PART=2"], "kernels_gram_wave2"),
    ("kernels_project.hip", []),
    ("kernels_bwd.hip", []),
    ("kernels_bwd_f32.hip", []),
    ("kernels_cost.hip", ["-ffp-contract=off"]),   # (the costs' summands and derivatives rounded as costs.py forms them)
    ("kernels_lik.hip", ["-ffp-contract=off"]),    # (the likelihoods' summands rounded as costs.py forms them, and as kernels_cost.hip does)
    ("kernels_conv.hip", []),
    ("kernels_conv.hip", ["-DSI_CONV_F32"], "kernels_conv_f32"),   # same source on fp32 operands (forward kernels only)
    ("capi_net.hip", []),
    ("eig.cpp", ["-DSI_EIG_NS=base"]),
    ("eig.cpp", ["-DSI_EIG_NS=avx2", "-mavx2", "-mfma"], "eig_avx2"),   # same source, other ISAs (eig_dispatch.cpp chooses)
    ("eig.cpp", ["-DSI_EIG_NS=avx512", "-mavx512f", "-mavx512vl", "-mavx512dq", "-mfma"], "eig_avx512"),
    ("eig_dispatch.cpp", []),
    ("chain_spec_rtc.cpp", []),   # hiprtc front end of chain_spec.inc (the kernel text is embedded: _embed_spec_source)
]
HEADERS = ["si_internal.h", "dev_buf.h", "philox.h", "kernels_gemm.h", "gemm_pipeline.h", "chain_common.h", "sampler_device.h", "capi_common.h", "node_tableau.h", "optimiser_update.h", "cost_reduce.h", "chain_spec.inc", "chain_spec_args.h",
           "chain_spec_rtc.h", os.path.join("..", "..", "include", "subspace_hip.h")]
# the kernel text that chain_spec_rtc.cpp hands to hiprtc at run time, in this order
SPEC_SOURCES = [("SI_SPEC_SRC_COMMON", "chain_common.h"), ("SI_SPEC_SRC_PHILOX", "philox.h"), ("SI_SPEC_SRC_ARGS", "chain_spec_args.h"),
                ("SI_SPEC_SRC_KERNELS", "chain_spec.inc")]


def _embed_spec_source(objdir):
    """csrc/build*/chain_spec_src.h: the four files above as raw string literals (split at 12 KB: a literal has a length limit)"""
    out = os.path.join(objdir, "chain_spec_src.h")
    parts = ["// generated by build.py from " + ", ".join(f for _, f in SPEC_SOURCES) + " -- do not edit\n"]
    for name, f in SPEC_SOURCES:
        text = open(os.path.join(CSRC, f)).read().replace("#pragma once", "")
        assert ')SISPEC"' not in text
        chunks, cur = [], ""
        for line in text.splitlines(keepends=True):
            if len(cur) + len(line) > 12000:
                chunks.append(cur)
                cur = ""
            cur += line
        chunks.append(cur)
        parts.append("static const char %s[] =\n%s;\n" % (name, "\n".join('R"SISPEC(' + c + ')SISPEC"' for c in chunks)))
    new = "".join(parts)
    if not os.path.exists(out) or open(out).read() != new:
        with open(out, "w") as fh:
            fh.write(new)
    return out


def _hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: cannot build libsubspace_hip.so")
    return exe


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


DEV_LIB = os.path.join(os.path.dirname(HERE), "tools", "bin", "libsubspace_hip_dev.so")


def build(force=False, verbose=False, dev=False):
    """dev=True: the DEVELOPMENT build (-DSI_DEV_KNOBS: the alternative kernels and SI_* environment knobs behind the
    measurements quoted in DESIGN.md) into tools/bin/libsubspace_hip_dev.so -- never loaded by the package."""
    hipcc = _hipcc()
    objdir = os.path.join(CSRC, "build_dev" if dev else "build")
    os.makedirs(objdir, exist_ok=True)
    lib = DEV_LIB if dev else LIB
    os.makedirs(os.path.dirname(lib), exist_ok=True)
    hdrs = [os.path.join(CSRC, h) for h in HEADERS] + [os.path.abspath(__file__)]
    _embed_spec_source(objdir)
    objs, jobs = [], []
    for entry in SOURCES + ([("guard_alloc.hip", [])] if dev else []):   # (guard-page allocator: development build only)
        src, extra = entry[0], entry[1]
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, (entry[2] if len(entry) > 2 else os.path.splitext(src)[0]) + ".o")
        objs.append(o)
        if force or _stale(o, [s] + hdrs):
            jobs.append([hipcc, "--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function",
                         "-I", objdir, "-c", s, "-o", o] + extra + (["-DSI_DEV_KNOBS"] if dev else []))

    def run(cmd):
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
    if jobs:  # the translation units are independent: compile them side by side (the fully unrolled Gram kernels take minutes)
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(len(jobs), max(1, (os.cpu_count() or 2) - 1), 8)) as ex:
            list(ex.map(run, jobs))
    if force or _stale(lib, objs):
        cmd = [hipcc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", lib] + objs + ["-lhiprtc"]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
    return lib


if __name__ == "__main__":
    import sys
    print(build(verbose=True, dev="--dev" in sys.argv))
