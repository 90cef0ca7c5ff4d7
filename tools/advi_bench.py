"""ADVI on the nn_example chain (docs/src/nn_example.md:112-118: 2-200-50-50-50-1, relu, 1000 observations): microseconds per
step of ADVI(10, T) at M = 3 and 20, T = 1000, for

  * the host loop: the step of si_fit_advi in NumPy (PCG64 draws) around Context.logdensity_grad_batch -- one stacked value +
    gradient call for the S = 10 points, two downloads and a host synchronisation per step, and
  * si_fit_advi: the same step queued on the stream, the state on the device, one synchronisation per call (D = 0: the fit alone).

Five repeats after a warm-up, the two legs alternating in one process; a call's time is a host clock around work that ends in a
synchronise, divided by T.  min / median / max are printed.

    python tools/advi_bench.py
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DIMS, B = [2, 200, 50, 50, 50, 1], 1000
MS, T, S, W, ETA, TAU, SIGMA_Z = (3, 20), 1000, 10, 100, 0.1, 1.0, 0.005
REPEATS = 5


def host_advi(grad_batch, m, rng):
    """the definition in the header comment of si_fit_advi, on NumPy's generator"""
    theta = SIGMA_Z * rng.standard_normal(2 * m)
    ring = np.zeros((W, 2 * m))
    for t in range(T):
        mu, sig = theta[:m], np.exp(theta[m:])
        eta = rng.standard_normal((m, S))
        _, g = grad_batch(np.asfortranarray(mu[:, None] + sig[:, None] * eta))
        d = np.concatenate([-np.sum(g, axis=1) / S, -np.sum(g * eta, axis=1) * sig / S - 1.0])
        ring[t % W] = d * d
        theta = theta - d * (ETA / (TAU + np.sqrt(np.sum(ring, axis=0))))
    return theta


def main():
    import subspaceinference_jl_amd as si
    from subspaceinference_jl_amd import _capi, flux
    rng = np.random.default_rng(0)
    layers = [flux.Dense(DIMS[i], DIMS[i + 1], "relu" if i + 2 < len(DIMS) else "identity", rng=rng) for i in range(len(DIMS) - 1)]
    table, n = flux.layer_table(flux.Chain(*layers))
    x, y = rng.standard_normal((DIMS[0], B)), rng.standard_normal((DIMS[-1], B))
    w_swa = 0.3 * rng.standard_normal(n)
    print("library: %s" % _capi.LIB_PATH)
    with si.Context(0) as ctx:
        print("device: %s   chain %s   B = %d   N = %d   T = %d   S = %d   sigma_z = %g" % (
            ctx.device_name(), "-".join(map(str, DIMS)), B, n, T, S, SIGMA_Z))
        for m in MS:
            p = np.asfortranarray(0.05 * rng.standard_normal((n, m)))
            ctx.infer_setup(table, n, m, w_swa, p, x, y, 1.0)
            legs = [("host loop over si_logdensity_grad_batch", lambda: host_advi(ctx.logdensity_grad_batch, m, np.random.default_rng(1))),
                    ("si_fit_advi", lambda: ctx.fit_advi(T, SIGMA_Z, 1, samples_per_step=S, eta=ETA, tau=TAU, window=W, ndraws=0)[0])]
            times = {name: [] for name, _ in legs}
            for name, fn in legs:
                theta = fn()   # warm-up (workspace, code objects)
                print("M = %2d  %-40s warm-up: theta finite %s, max |theta| %.3g" % (m, name, bool(np.all(np.isfinite(theta))), float(np.max(np.abs(theta)))))
            for _ in range(REPEATS):
                for name, fn in legs:   # alternating
                    ctx.lib.si_synchronize(ctx.h)
                    t0 = time.perf_counter()
                    fn()
                    ctx.lib.si_synchronize(ctx.h)
                    times[name].append(time.perf_counter() - t0)
            for name, _ in legs:
                us = 1e6 * np.array(times[name]) / T
                print("M = %2d  %-40s us / step: min %9.2f  median %9.2f  max %9.2f%s" % (
                    m, name, us.min(), np.median(us), us.max(),
                    "   (fused, passes) = %s" % (ctx.advi_kernel_info(),) if name == "si_fit_advi" else ""))


if __name__ == "__main__":
    main()
