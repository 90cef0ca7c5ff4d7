"""One-step HMC on the nn_example chain (docs/src/nn_example.md:112-118: 2-200-50-50-50-1, relu, 1000 observations): microseconds
per transition at M = 3 and 20, itr = 200, for

  * the host loop: samplers.hmc over Context.logdensity_grad at C = 1 (per transition an upload, the gradient, two downloads, a
    host synchronisation and the sampler's arithmetic in NumPy on PCG64 draws), and
  * si_sample_hmc at C = 1, 8 and 64: the same transition queued on the stream, position, momentum, step size, metric and adaptor
    state on the device, one synchronisation per call after the search.

Both legs start with the step-size search, which is data dependent and synchronises on both.  It is timed separately: a call with
itr = 1 is the search plus one transition, so  preamble = t(itr = 1)  and  per transition = (t(itr = 200) - t(itr = 1)) / 199.
Five repeats after a warm-up, the legs alternating; a call's time is a host clock around work that ends in a synchronise.
min / median / max are printed, and the search's rounds (si_hmc_kernel_info) or evaluations (host loop).

    python tools/hmc_bench.py                              # both legs, on the library of this tree
    python tools/hmc_bench.py --lib PATH --host-only       # the host loop on another build (the tree before si_sample_hmc)
    python tools/hmc_bench.py --trace-run                  # si_sample_hmc alone, 20 transitions at C = 1 and 8 (for a kernel trace)
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
    ap.add_argument("--host-only", action="store_true", help="the library has no si_sample_hmc (a tree before it)")
    ap.add_argument("--trace-run", action="store_true", help="si_sample_hmc alone, short: the target of a kernel trace")
    args = ap.parse_args()
    import subspaceinference_jl_amd as si
    from subspaceinference_jl_amd import _capi, flux, samplers
    if args.lib:
        _capi.LIB_PATH = os.path.abspath(args.lib)
    if args.host_only:
        for name in ("si_sample_hmc", "si_hmc_kernel_info", "si_host_hmc_windows"):
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
                    out = ctx.sample_hmc(20, SIGMA_Z, seed=1, nchains=c)
                    print("M = %2d  C = %2d  20 transitions, mean alpha %s, eps_0 %s, (fused, passes, search rounds) = %s"
                          % (m, c, np.round(out[2][1:].mean(axis=0), 2), out[3][0], ctx.hmc_kernel_info()))
                continue
            evals = [0]

            def counted(z):
                evals[0] += 1
                return ctx.logdensity_grad(z)
            legs = [("host loop: samplers.hmc", 1, lambda itr: samplers.hmc(counted, m, itr, SIGMA_Z, np.random.default_rng([1, 0])))]
            if not args.host_only:
                for c in CS:
                    legs.append(("si_sample_hmc", c, lambda itr, c=c: ctx.sample_hmc(itr, SIGMA_Z, seed=1, nchains=c)))
            times = {(name, c, itr): [] for name, c, _ in legs for itr in (1, ITR)}
            info = {}
            for name, c, fn in legs:
                fn(ITR)   # warm-up (workspace, code objects)
            for _ in range(REPEATS):
                for name, c, fn in legs:   # alternating
                    for itr in (1, ITR):
                        ctx.lib.si_synchronize(ctx.h)
                        evals[0] = 0
                        t0 = time.perf_counter()
                        out = fn(itr)
                        ctx.lib.si_synchronize(ctx.h)
                        times[(name, c, itr)].append(time.perf_counter() - t0)
                        if itr == 1:
                            info[(name, c)] = ("search evaluations %d" % (evals[0] - 2) if name.startswith("host") else
                                               "(fused, passes, search rounds) = %s" % (ctx.hmc_kernel_info(),))
                        else:
                            info[(name, c)] += "  mean alpha %.2f" % (out[2] if name.startswith("host") else float(out[2][1:].mean()))
            for name, c, _ in legs:
                pre = 1e6 * np.array(times[(name, c, 1)])
                us = (1e6 * np.array(times[(name, c, ITR)]) - pre) / (ITR - 1)
                print("M = %2d  C = %2d  %-24s us / transition: min %8.2f  median %8.2f  max %8.2f  (per chain: median %7.2f)   "
                      "preamble (search + 1 transition) us: min %9.1f  median %9.1f   %s"
                      % (m, c, name, us.min(), np.median(us), us.max(), np.median(us) / c, pre.min(), np.median(pre), info[(name, c)]))


if __name__ == "__main__":
    main()
