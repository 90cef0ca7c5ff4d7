"""Times the NeuralODE density (csrc/kernels_node.hip) at the tutorial's shape (docs/src/node_example.md): x.^3 -> Dense(2, 15, tanh)
-> Dense(15, 2), 100 trajectories, 30 save points over [0, 1.5], Tsit5 at reltol 1e-7 / abstol 1e-9, M = 5.

    python tools/node_bench.py [--reps 50] [--out profiles/node_bench.log]

Reports, for C = 1 chain and C = 512 stacked chains:
  kernel time per density evaluation (the library's event pairs around the integration launches, class "dense") and per chain;
  wall time per si_logdensity call (a host clock around a call that ends in a synchronise);
  RWMH transitions per second (si_sample_rwmh: the launch-per-step loop), wall clock over the whole call;
  mean accepted and rejected steps per trajectory (si_node_solve);
  achieved right-hand-side evaluations per second: trajectories * (2 + 6 * (accepted + rejected)) / kernel time -- a step costs six
  new evaluations (k_1 is the last step's k_7), the first one and the starting-step rule two more;
  the same with `identity` in place of tanh and without the cube (a linear problem, which cannot blow up, with its own step counts):
  the kernel time per evaluation with and without the 15 fp64 tanh shows what they cost on this part.
Every figure is the mean of five blocks after a warm-up block; the spread is the range of the block means.  Needs a GPU."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M, F, S = 5, 100, 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--itr", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "node_bench.log"))
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    import subspaceinference_jl_amd as si
    from subspaceinference_jl_amd import flux, node

    rng = np.random.default_rng(0)
    n = 2 * 15 + 15 + 15 * 2 + 2
    w_swa = np.concatenate([0.8 / np.sqrt(2) * rng.standard_normal(30), 0.1 * rng.standard_normal(15),
                            0.8 / np.sqrt(15) * rng.standard_normal(30), 0.1 * rng.standard_normal(2)])
    p = np.asfortranarray(0.05 * rng.standard_normal((n, M)))
    u0 = np.asfortranarray(rng.uniform(-1.0, 1.0, (2, F)))
    ts = np.linspace(0.0, 1.5, S)
    kw = dict(t0=0.0, reltol=1e-7, abstol=1e-9, pre_power=3)
    with si.Context(0) as ctx:
        say("device: %s   2 -> 15 -> 2 behind the cube, f = %d, S = %d, reltol 1e-7, abstol 1e-9, M = %d, reps = %d" % (ctx.device_name(), F, S, M, args.reps))
        for act_name, act in (("tanh", flux.tanh), ("identity", flux.identity)):
            table = [(2, 15, act, 0, 30), (15, 2, flux.identity, 45, 75)]
            kwa = dict(kw, pre_power=3 if act == flux.tanh else 1)
            y = node.solve(table, w_swa, u0, ts, node.Opts(**kwa)).U + 0.05 * rng.standard_normal((2 * S, F))
            ctx.infer_setup_node(table, n, M, w_swa, p, u0, np.asfortranarray(y), ts, **kwa)
            g = ctx.node_info()[4]
            for c in (1, 512):
                z = np.asfortranarray(0.3 * rng.standard_normal((M, c)))
                _, _, na, nr, st = ctx.node_solve(z, want_u=False)
                if st.any():
                    say("%-8s C = %3d: %d of %d trajectories did not finish (status != 0); their steps are counted as taken" % (act_name, c, int((st != 0).sum()), st.size))
                evals = float(np.sum(2 + 6 * (na.astype(np.int64) + nr)))
                kern, wall = [], []
                r = max(1, args.reps // 5)
                for blk in range(6):          # block 0 warms the shape up and is dropped
                    ctx.set_profiling(True, ["dense"])
                    ctx.reset_stats()
                    t0 = time.perf_counter()
                    for _ in range(r):
                        lp = ctx.logdensity(z)
                    t1 = time.perf_counter()
                    st_ms = ctx.stats()["dense"]["ms"]
                    ctx.set_profiling(False)
                    if blk:
                        kern.append(st_ms * 1e3 / r)
                        wall.append((t1 - t0) * 1e6 / r)
                kern, wall = np.array(kern), np.array(wall)
                say("%-8s G = %2d  C = %3d  integration %9.1f us per evaluation (blocks %.1f .. %.1f), %8.2f us per chain; si_logdensity call %9.1f us "
                    "(%.1f .. %.1f)" % (act_name, g, c, kern.mean(), kern.min(), kern.max(), kern.mean() / c, wall.mean(), wall.min(), wall.max()))
                say("%-8s          C = %3d  accepted %.2f, rejected %.2f steps per trajectory; %.3e RHS evaluations per density, %.3e per second, "
                    "%.3f ns of kernel time per evaluation" % (act_name, c, na.mean(), nr.mean(), evals, evals / (kern.mean() * 1e-6),
                                                                   kern.mean() * 1e3 / evals))
                # RWMH through the launch-per-step loop: wall clock over the whole call, profiling off
                ctx.sample_rwmh(5, 0.05, 1, 0, c)
                rates = []
                for blk in range(3):
                    t0 = time.perf_counter()
                    ctx.sample_rwmh(args.itr, 0.05, 1, 0, c)
                    rates.append(args.itr / (time.perf_counter() - t0))
                rates = np.array(rates)
                say("%-8s          C = %3d  RWMH %9.1f transitions/s per call of %d chains (%.1f .. %.1f), %.1f chain-transitions/s" % (
                    act_name, c, rates.mean(), c, rates.min(), rates.max(), rates.mean() * c))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
