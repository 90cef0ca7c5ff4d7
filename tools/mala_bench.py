"""MALA on the nn_example chain (docs/src/nn_example.md:112-118: 2-200-50-50-50-1, relu, 1000 observations): microseconds per
transition at M = 3 and 20, C = 1, 8 and 64 chains, itr = 200, for

  * the host loop: samplers.mala_chains over Context.logdensity_grad_batch (one stacked gradient call, two downloads and a host
    synchronisation per transition, the sampler's arithmetic in NumPy), and
  * si_sample_mala: the same transition queued on the stream, the chain state on the device, one synchronisation per call.

Five repeats after a warm-up, the two legs alternating; a call's time is a host clock around work that ends in a synchronise,
divided by itr (the itr value + gradient evaluations of a call).  min / median / max are printed.

    python tools/mala_bench.py                             # both legs, on the library of this tree
    python tools/mala_bench.py --lib PATH --host-only      # the host loop on another build (the tree before si_sample_mala)
    python tools/mala_bench.py --trace-run                 # si_sample_mala alone, 50 transitions at C = 1 and 8 (for rocprofv3
                                                           #   --kernel-trace --stats: the launches per transition)
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DIMS, B = [2, 200, 50, 50, 50, 1], 1000
MS, CS, ITR, SIGMA_Z = (3, 20), (1, 8, 64), 200, 0.005
REPEATS = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libsubspace_hip.so")
    ap.add_argument("--host-only", action="store_true", help="the library has no si_sample_mala (a tree before it)")
    ap.add_argument("--trace-run", action="store_true", help="si_sample_mala alone, short: the target of a kernel trace")
    args = ap.parse_args()
    import subspaceinference_jl_amd as si
    from subspaceinference_jl_amd import _capi, flux, samplers
    if args.lib:
        _capi.LIB_PATH = os.path.abspath(args.lib)
    if args.host_only:
        for name in ("si_sample_mala", "si_mala_kernel_info"):
            _capi.SIGNATURES.pop(name, None)
    rng = np.random.default_rng(0)
    layers = [flux.Dense(DIMS[i], DIMS[i + 1], "relu" if i + 2 < len(DIMS) else "identity", rng=rng) for i in range(len(DIMS) - 1)]
    table, n = flux.layer_table(flux.Chain(*layers))
    x, y = rng.standard_normal((DIMS[0], B)), rng.standard_normal((DIMS[-1], B))
    w_swa = 0.3 * rng.standard_normal(n)
    print("library: %s" % _capi.LIB_PATH)
    with si.Context(0) as ctx:
        print("device: %s   chain %s   B = %d   N = %d   itr = %d   sigma_z = %g" % (ctx.device_name(), "-".join(map(str, DIMS)), B, n, ITR, SIGMA_Z))
        for m in MS:
            p = np.asfortranarray(0.05 * rng.standard_normal((n, m)))
            ctx.infer_setup(table, n, m, w_swa, p, x, y, 1.0)
            if args.trace_run:
                for c in (1, 8):
                    _, _, acc = ctx.sample_mala(50, SIGMA_Z, seed=1, nchains=c)
                    print("M = %2d  C = %2d  50 samples, accept rates %s, (fused, passes) = %s" % (m, c, np.round(acc, 2), ctx.mala_kernel_info()))
                continue
            for c in CS:
                legs = [("host loop over si_logdensity_grad_batch",
                         lambda: samplers.mala_chains(ctx.logdensity_grad_batch, m, ITR, SIGMA_Z, [np.random.default_rng([1, j]) for j in range(c)]))]
                if not args.host_only:
                    legs.append(("si_sample_mala", lambda: ctx.sample_mala(ITR, SIGMA_Z, seed=1, nchains=c)))
                times = {name: [] for name, _ in legs}
                for name, fn in legs:
                    fn()   # warm-up (workspace, code objects)
                for _ in range(REPEATS):
                    for name, fn in legs:   # alternating
                        ctx.lib.si_synchronize(ctx.h)
                        t0 = time.perf_counter()
                        out = fn()
                        ctx.lib.si_synchronize(ctx.h)
                        times[name].append(time.perf_counter() - t0)
                        acc = out[2]
                for name, _ in legs:
                    us = 1e6 * np.array(times[name]) / ITR
                    print("M = %2d  C = %2d  %-40s us / transition: min %9.2f  median %9.2f  max %9.2f   (per chain: median %8.2f)%s"
                          % (m, c, name, us.min(), np.median(us), us.max(), np.median(us) / c,
                             "  (fused, passes) = %s  accept %.2f" % (ctx.mala_kernel_info(), float(np.mean(acc))) if name == "si_sample_mala" else ""))


if __name__ == "__main__":
    main()
