"""si_sample_ess (elliptical slice sampling, state on the device) against the launch-per-step RWMH transition, on one GPU:

  * the tutorial chain (docs/src/nn_example.md:112-118: 2-200-50-50-50-1, relu, 1000 observations), M = 20, at 1 and 512 chains;
  * tools/cost_bench.py's classifier -- Dense 784-256-10 (relu, identity), B = 4096 -- under the categorical likelihood, M = 20, at
    1 and 8 chains.

A ROUND of si_sample_ess is one evaluation of the density at the chains' pending points (eval_density_all: the launches of an RWMH
transition's evaluation), one memset of the open word, ess_round_kernel, one 4-byte read-back and one synchronisation.  Per row the
tool prints

    time per round          (t(itr) - t(1)) / (rounds(itr) - rounds(1)): ess_begin_kernel, once per transition, is inside
    evaluations and rounds per transition, and the lock-step waste 1 - evals / (rounds C)   (si_ess_kernel_info)
    RWMH transition         (t(itr) - t(1)) / (itr - 1) of si_sample_rwmh with set_chain_loop(0) -- one launch per layer and per step of
                            the tail, the path this sampler's evaluation shares -- in the same process, the two alternating
    empty round             memset of 4 bytes, read-back of 4 bytes and a synchronisation on an idle stream (the HIP runtime through
                            ctypes: the library has no entry point that does nothing)

and whether round <= RWMH transition + empty round holds within the run-to-run spread (max - min over the repeats) of the RWMH
figure.  Five repeats after a warm-up; a call's time is a host clock around work that ends in a synchronise; median [min - max].

    python tools/ess_bench.py [--repeats 5] [--out profiles/ess_bench.log]

Needs a GPU (there is no fallback)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NN_DIMS, NN_B = [2, 200, 50, 50, 50, 1], 1000
CLS_DIMS, CLS_B = [784, 256, 10], 4096
M = 20
# sigma_z: the prior's standard deviation on z for si_sample_ess; a step size for si_sample_rwmh (its value does not enter the time)
ROWS = [("nn_example", 1, 101, 1.0), ("nn_example", 512, 11, 1.0), ("classifier", 1, 51, 1.0), ("classifier", 8, 26, 1.0)]


def empty_round(repeats, n=200):
    """microseconds per (memset 4 bytes, read back 4 bytes, synchronise) on the idle null stream, `repeats` figures"""
    hip = ctypes.CDLL("libamdhip64.so")
    dev = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(dev), ctypes.c_size_t(4)) == 0
    host = ctypes.c_int32(0)
    out = []
    try:
        for rep in range(repeats + 1):       # (0 warms up)
            assert hip.hipDeviceSynchronize() == 0
            t0 = time.perf_counter()
            for _ in range(n):
                hip.hipMemsetAsync(dev, 0, ctypes.c_size_t(4), None)
                hip.hipMemcpyAsync(ctypes.byref(host), dev, ctypes.c_size_t(4), 2, None)   # hipMemcpyDeviceToHost
                hip.hipStreamSynchronize(None)
            if rep:
                out.append((time.perf_counter() - t0) * 1e6 / n)
    finally:
        hip.hipFree(dev)
    return np.array(out)


def timed(ctx, fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e6


def run(args, say):
    import subspaceinference_jl_amd as si
    from oracle import subspace_oracle as so
    from subspaceinference_jl_amd import _capi
    rng = np.random.default_rng(0)
    result = {"lib": _capi.LIB_PATH, "rows": []}
    with si.Context(0) as ctx:
        say("device: %s   library: %s   %d repeats" % (ctx.device_name(), _capi.LIB_PATH, args.repeats))
        empty = empty_round(args.repeats)
        say("empty round (memset, 4-byte read-back, synchronise): median %.2f us [%.2f - %.2f]" % (np.median(empty), empty.min(), empty.max()))
        result["empty_round_us"] = float(np.median(empty))
        current = None
        for model, c, itr, sigma_z in ROWS:
            if model != current:
                current = model
                if model == "nn_example":
                    table, n = so.layer_table(NN_DIMS, [so.ACT_RELU] * 4 + [so.ACT_IDENTITY])
                    x, y = rng.standard_normal((NN_DIMS[0], NN_B)), rng.standard_normal((NN_DIMS[-1], NN_B))
                    w, p = 0.3 * rng.standard_normal(n), np.asfortranarray(0.05 * rng.standard_normal((n, M)))
                    ctx.infer_setup(table, n, M, w, p, x, y, 1.0)
                else:
                    table, n = so.layer_table(CLS_DIMS, [so.ACT_RELU, so.ACT_IDENTITY])
                    x = np.asfortranarray(rng.standard_normal((CLS_DIMS[0], CLS_B)))
                    y = np.zeros((CLS_DIMS[-1], CLS_B), order="F")
                    y[rng.integers(0, CLS_DIMS[-1], CLS_B), np.arange(CLS_B)] = 1.0
                    w, p = rng.standard_normal(n) * np.sqrt(2.0 / 256), np.asfortranarray(0.01 * rng.standard_normal((n, M)))
                    ctx.infer_setup(table, n, M, w, p, x, y, 1.0)
                    ctx.infer_set_likelihood(_capi.LIKELIHOODS["categorical"])
            ctx.set_chain_loop(0)
            ess = {1: [], itr: []}
            rw = {1: [], itr: []}
            info = {}
            for rep in range(args.repeats + 1):      # (0 warms up: workspace, code objects)
                for k in (1, itr):                    # the two samplers alternating
                    t = timed(ctx, lambda: ctx.sample_ess(k, sigma_z, seed=1, nchains=c))
                    info[k] = ctx.ess_kernel_info()
                    u = timed(ctx, lambda: ctx.sample_rwmh(k, 0.005, seed=1, nchains=c))
                    if rep:
                        ess[k].append(t)
                        rw[k].append(u)
            ctx.set_chain_loop(1)
            passes, rounds, evals = info[itr]
            dr = rounds - info[1][1]
            per_round = (np.array(ess[itr]) - np.array(ess[1])) / dr
            per_rwmh = (np.array(rw[itr]) - np.array(rw[1])) / (itr - 1)
            spread = float(per_rwmh.max() - per_rwmh.min())
            gap = float(np.median(per_round) - np.median(per_rwmh) - np.median(empty))
            waste = 1.0 - evals / (rounds * c)
            say("%-10s C = %3d  passes %d  transitions %3d  rounds / transition %5.2f  evals / transition and chain %5.2f  lock-step waste %.3f"
                % (model, c, passes, itr - 1, rounds / (itr - 1), evals / ((itr - 1) * c), waste))
            say("%-10s C = %3d  us / round: median %9.2f [%9.2f - %9.2f]   us / RWMH transition (set_chain_loop(0)): median %9.2f [%9.2f - %9.2f], "
                "spread %.2f   round - (RWMH + empty round) = %+.2f us: %s"
                % (model, c, np.median(per_round), per_round.min(), per_round.max(), np.median(per_rwmh), per_rwmh.min(), per_rwmh.max(), spread,
                   gap, "within the expectation" if gap <= spread else "ABOVE the expectation by more than the spread"))
            result["rows"].append({"model": model, "chains": c, "passes": passes, "transitions": itr - 1, "rounds": rounds, "evals": evals,
                                   "waste": waste, "round_us": float(np.median(per_round)), "rwmh_us": float(np.median(per_rwmh)),
                                   "rwmh_spread_us": spread, "gap_us": gap})
    say("JSON " + json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ess_bench.log"))
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
