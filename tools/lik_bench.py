"""Times the launch-per-step RWMH transition at tools/cost_bench.py's classifier -- Dense 784-256-10 (relu, identity), B = 4096 --
with the Gaussian likelihood and with the categorical one (si_infer_set_likelihood), in Float64 and with compute_dtype = SI_F32, for
C = 1 and C = 8 chains, on one GPU:

    python tools/lik_bench.py [--itr 200] [--out profiles/lik_bench.log]
    python tools/lik_bench.py --lib OTHER/libsubspace_hip.so     # another build, e.g. the parent commit's: a build without
                                                                  # si_infer_set_likelihood is timed with the Gaussian alone

Modes: set_chain_loop(0) is one launch per layer and per step of the tail, the same launches for both likelihoods but the new
kernel; set_chain_loop(2) is what a user gets without the device-resident loops (Gaussian: the one-launch narrow-chain density and
the fused tail; categorical: the per-layer launches and the fused tail).  A call of `itr` transitions is timed by the host clock
around si_sample_rwmh (which ends with its synchronisation and read-back); five timed calls behind a warm-up call, the two
likelihoods alternating; printed: the mean over the calls of the time per transition, and their range.

The new kernel's own time: the library's event pairs around the SSE class alone (si_set_profiling_classes) in mode 0, categorical
minus Gaussian, per transition -- lik_logitce_kernel plus the sse_final_kernel launch behind it.  Its traffic is 8 out B (C + 1)
bytes (the outputs of every slot once, the labels once per launch if the cache holds them).  Needs a GPU (there is no fallback)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CALLS = 5
DIMS, BATCH, M = [784, 256, 10], 4096, 20


def run(args, say):
    from subspaceinference_jl_amd import _capi
    if args.lib:
        _capi.LIB_PATH = os.path.abspath(args.lib)
    with open(_capi.LIB_PATH, "rb") as fh:   # (looked up in the file: the library is loaded once, by the package)
        has_lik = b"si_infer_set_likelihood" in fh.read()
    if not has_lik:   # a build from before the switch: the Gaussian alone, through the calls it has
        for name in ("si_infer_set_likelihood", "si_infer_likelihood_info"):
            _capi.SIGNATURES.pop(name, None)
    import subspaceinference_jl_amd as si
    from oracle import subspace_oracle as so

    kinds = [("gaussian", 0), ("categorical", 1)] if has_lik else [("gaussian", 0)]
    table, n = so.layer_table(DIMS, [so.ACT_RELU, so.ACT_IDENTITY])
    rng = np.random.default_rng(0)
    x = np.asfortranarray(rng.standard_normal((DIMS[0], BATCH)))
    y = np.zeros((DIMS[-1], BATCH), order="F")
    y[rng.integers(0, DIMS[-1], BATCH), np.arange(BATCH)] = 1.0
    w = rng.standard_normal(n) * np.sqrt(2.0 / 256)
    p = np.asfortranarray(0.01 * rng.standard_normal((n, M)))
    result = {"lib": _capi.LIB_PATH, "itr": args.itr, "rows": []}
    with si.Context(0) as ctx:
        say("device: %s   library: %s   %d calls of %d transitions per row" % (ctx.device_name(), _capi.LIB_PATH, CALLS, args.itr))
        for dname, cdt in (("f64", _capi.SI_F64), ("f32", _capi.SI_F32)):
            ctx.infer_setup(table, n, M, w, p, x, y, 1.0, compute_dtype=cdt)
            for nch in (1, 8):
                for mode in (0, 2):
                    ctx.set_chain_loop(mode)
                    us = {k: [] for k, _ in kinds}
                    for call in range(CALLS + 1):      # call 0 warms up and is dropped
                        for k, code in kinds:
                            if has_lik:
                                ctx.infer_set_likelihood(code)
                            ctx.synchronize()
                            t0 = time.perf_counter()
                            ctx.sample_rwmh(args.itr, 0.01, seed=1, nchains=nch)
                            if call:
                                us[k].append((time.perf_counter() - t0) * 1e6 / args.itr)
                    for k, _ in kinds:
                        t = np.array(us[k])
                        say("%s C=%d mode %d %-12s %9.1f us per transition  (calls %.1f .. %.1f)" % (dname, nch, mode, k, t.mean(), t.min(), t.max()))
                        result["rows"].append({"dtype": dname, "chains": nch, "mode": mode, "likelihood": k, "us_mean": t.mean(),
                                               "us_min": t.min(), "us_max": t.max()})
                if has_lik:   # the kernel's own time: the SSE class's event pairs, categorical minus Gaussian, mode 0
                    ctx.set_chain_loop(0)
                    ms = {}
                    for k, code in kinds:
                        ctx.infer_set_likelihood(code)
                        ctx.set_profiling(True, ["sse"])
                        ctx.reset_stats()
                        ctx.sample_rwmh(args.itr, 0.01, seed=1, nchains=nch)
                        ms[k] = ctx.stats()["sse"]["ms"]
                        ctx.set_profiling(False)
                    own = (ms["categorical"] - ms["gaussian"]) * 1e3 / args.itr
                    byts = 8.0 * DIMS[-1] * BATCH * (nch + 1)
                    say("%s C=%d  SSE class per transition: gaussian %.2f us, categorical %.2f us; the likelihood kernel and its final stage: "
                        "%.2f us, %.0f bytes, %.1f GB/s" % (dname, nch, ms["gaussian"] * 1e3 / args.itr, ms["categorical"] * 1e3 / args.itr, own, byts,
                                                          byts / (own * 1e-6) / 1e9 if own > 0 else float("nan")))
                    result["rows"].append({"dtype": dname, "chains": nch, "kernel_us": own, "kernel_bytes": byts})
                    ctx.infer_set_likelihood(0)
            ctx.set_chain_loop(1)
    say("JSON " + json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--itr", type=int, default=200)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lik_bench.log"))
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    run(args, say)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
