"""NUTS on the nn_example chain (docs/src/nn_example.md:112-118: 2-200-50-50-50-1, relu, 1000 observations): microseconds per
leapfrog step and chain at M = 3 and 20, itr = 200, for

  * the host loop: samplers.nuts over Context.logdensity_grad at C = 1 (per leapfrog step an upload, the per-layer reverse sweep, two
    downloads, a host synchronisation and the tree's arithmetic in NumPy on PCG64 draws), and
  * si_sample_nuts at C = 1, 8 and 64: the same tree built leaf by leaf on the device, one stacked value-and-gradient evaluation, one
    kernel and one 4-byte read-back per round, the chains of a call in lock-step within a transition.

Both legs start with the step-size search.  A call with itr = 1 is the search plus one transition, so with L(itr) the leapfrog steps
of a call (gradient evaluations of the host loop after the search; si_nuts_kernel_info's leaves)

    per leapfrog step and chain = (t(itr = 200) - t(itr = 1)) / (L(200) - L(1))

and the lock-step waste of the device leg is 1 - leaves / (rounds C).  Five repeats after a warm-up, the legs alternating in one
process; a call's time is a host clock around work that ends in a synchronise.  median [min - max] are printed.

    python tools/nuts_bench.py                 # both legs, on the library of this tree
    python tools/nuts_bench.py --trace-run     # si_sample_nuts alone, 10 transitions at C = 1 and 8 (the target of a kernel trace)
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
    ap.add_argument("--trace-run", action="store_true", help="si_sample_nuts alone, short: the target of a kernel trace")
    ap.add_argument("--itr", type=int, default=ITR)
    ap.add_argument("--repeats", type=int, default=REPEATS)
    ap.add_argument("--ms", type=int, nargs="+", default=list(MS), help="the subspace dimensions to run")
    args = ap.parse_args()
    import subspaceinference_jl_amd as si
    from subspaceinference_jl_amd import _capi, flux, samplers
    if args.lib:
        _capi.LIB_PATH = os.path.abspath(args.lib)
    itr_n = args.itr
    rng = np.random.default_rng(0)
    layers = [flux.Dense(DIMS[i], DIMS[i + 1], "relu" if i + 2 < len(DIMS) else "identity", rng=rng) for i in range(len(DIMS) - 1)]
    table, n = flux.layer_table(flux.Chain(*layers))
    x, y = rng.standard_normal((DIMS[0], B)), rng.standard_normal((DIMS[-1], B))
    w_swa = 0.3 * rng.standard_normal(n)
    print("library: %s" % _capi.LIB_PATH)
    with si.Context(0) as ctx:
        print("device: %s   chain %s   B = %d   N = %d   itr = %d   sigma_z = %g" % (ctx.device_name(), "-".join(map(str, DIMS)), B, n, itr_n, SIGMA_Z))
        for m in args.ms:
            p = np.asfortranarray(0.05 * rng.standard_normal((n, m)))
            ctx.infer_setup(table, n, m, w_swa, p, x, y, 1.0)
            if args.trace_run:
                for c in (1, 8):
                    out = ctx.sample_nuts(10, SIGMA_Z, seed=1, nchains=c)
                    print("M = %2d  C = %2d  10 transitions, leaves per transition %s, (fused, passes, search rounds, rounds, leaves) = %s"
                          % (m, c, np.round(out[5][1:].mean(axis=0), 1), ctx.nuts_kernel_info()))
                continue
            evals = [0]

            def counted(z):
                evals[0] += 1
                return ctx.logdensity_grad(z)
            legs = [("host loop: samplers.nuts", 1, lambda itr: samplers.nuts(counted, m, itr, SIGMA_Z, np.random.default_rng([1, 0])))]
            for c in CS:
                legs.append(("si_sample_nuts", c, lambda itr, c=c: ctx.sample_nuts(itr, SIGMA_Z, seed=1, nchains=c)))
            times = {(name, c, itr): [] for name, c, _ in legs for itr in (1, itr_n)}
            steps, info = {}, {}
            for name, c, fn in legs:
                fn(itr_n)   # warm-up (workspace, code objects)
            for _ in range(args.repeats):
                for name, c, fn in legs:   # alternating
                    for itr in (1, itr_n):
                        ctx.lib.si_synchronize(ctx.h)
                        evals[0] = 0
                        t0 = time.perf_counter()
                        out = fn(itr)
                        ctx.lib.si_synchronize(ctx.h)
                        times[(name, c, itr)].append(time.perf_counter() - t0)
                        if name.startswith("host"):
                            steps[(name, c, itr)] = evals[0]   # (the search's evaluations are in both and cancel)
                            info[(name, c)] = "mean alpha %.2f" % out[2]
                        else:
                            fused, passes, search, rounds, leaves = ctx.nuts_kernel_info()
                            steps[(name, c, itr)] = leaves
                            info[(name, c)] = ("(fused, passes, search rounds) = (%d, %d, %d)  rounds %d  leaves %d  lock-step waste %.3f  "
                                               "mean alpha %.2f  mean depth %.2f" % (fused, passes, search, rounds, leaves,
                                                                                   1.0 - leaves / (rounds * c), float(out[2][1:].mean()),
                                                                                   float(out[4][1:].mean())))
            for name, c, _ in legs:
                pre = 1e6 * np.array(times[(name, c, 1)])
                dl = steps[(name, c, itr_n)] - steps[(name, c, 1)]
                us = (1e6 * np.array(times[(name, c, itr_n)]) - pre) / dl   # (per leapfrog step, the chains' steps added up: per step AND chain)
                print("M = %2d  C = %2d  %-25s us / leapfrog step and chain: median %8.2f [%8.2f - %8.2f]   leapfrog steps %7d   "
                      "preamble (search + 1 transition) us: median %9.1f   %s"
                      % (m, c, name, np.median(us), us.min(), us.max(), dl, np.median(pre), info[(name, c)]))


if __name__ == "__main__":
    main()
