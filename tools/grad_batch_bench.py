"""Value + gradient of the nn_example chain (docs/src/nn_example.md:112-118: 2-200-50-50-50-1, relu, 1000 observations) at
M = 3 and M = 20: microseconds per point for

  * C sequential si_logdensity_grad calls (what a caller can do without the batch entry), and
  * one si_logdensity_grad_batch call,

at C = 1, 8, 64, 512.  Five repeats after a warm-up, si_synchronize around every timed region; min / median / max are printed.

    python tools/grad_batch_bench.py                       # both, on the library of this tree
    python tools/grad_batch_bench.py --lib PATH --sequential-only   # the sequential figure on another build (the tree before the change)
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DIMS, B = [2, 200, 50, 50, 50, 1], 1000
CS = (1, 8, 64, 512)
REPEATS = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libsubspace_hip.so")
    ap.add_argument("--sequential-only", action="store_true", help="the library has no batch entry (a tree before it)")
    ap.add_argument("--seq-max", type=int, default=512, help="largest C timed with sequential calls")
    args = ap.parse_args()
    import subspaceinference_jl_amd as si
    from subspaceinference_jl_amd import _capi, flux
    if args.lib:
        _capi.LIB_PATH = os.path.abspath(args.lib)
    if args.sequential_only:
        for name in ("si_logdensity_grad_batch", "si_grad_kernel_info"):
            _capi.SIGNATURES.pop(name, None)
    rng = np.random.default_rng(0)
    layers = [flux.Dense(DIMS[i], DIMS[i + 1], "relu" if i + 2 < len(DIMS) else "identity", rng=rng) for i in range(len(DIMS) - 1)]
    model = flux.Chain(*layers)
    table, n = flux.layer_table(model)
    x, y = rng.standard_normal((DIMS[0], B)), rng.standard_normal((DIMS[-1], B))
    w_swa = 0.3 * rng.standard_normal(n)
    print("library: %s" % _capi.LIB_PATH)
    with si.Context(0) as ctx:
        print("device: %s   chain %s   B = %d   N = %d" % (ctx.device_name(), "-".join(map(str, DIMS)), B, n))

        def timed(fn):
            fn()   # warm-up (workspace, code objects)
            out = []
            for _ in range(REPEATS):
                ctx.lib.si_synchronize(ctx.h)
                t0 = time.perf_counter()
                fn()
                ctx.lib.si_synchronize(ctx.h)
                out.append(time.perf_counter() - t0)
            return np.array(out)

        for m in (3, 20):
            p = np.asfortranarray(0.05 * rng.standard_normal((n, m)))
            ctx.infer_setup(table, n, m, w_swa, p, x, y, 1.0)
            for c in CS:
                z = np.asfortranarray(0.3 * rng.standard_normal((m, c)))
                cols = [np.ascontiguousarray(z[:, j]) for j in range(c)]
                rows = []
                if c <= args.seq_max:
                    rows.append(("sequential si_logdensity_grad", timed(lambda: [ctx.logdensity_grad(v) for v in cols])))
                if not args.sequential_only:
                    rows.append(("one si_logdensity_grad_batch", timed(lambda: ctx.logdensity_grad_batch(z))))
                    fused = ctx.grad_kernel_info()
                for name, t in rows:
                    us = 1e6 * t / c
                    print("M = %2d  C = %3d  %-30s  us / point: min %9.2f  median %9.2f  max %9.2f   (call: median %9.1f us)%s"
                          % (m, c, name, us.min(), np.median(us), us.max(), 1e6 * np.median(t),
                             "  fused = %d" % fused if name.startswith("one") else ""))


if __name__ == "__main__":
    main()
