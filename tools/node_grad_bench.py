"""Times the gradient through the NeuralODE solver (si_node_set_grad; csrc/kernels_node.hip: the forward with record and the reverse
kernel) at the tutorial's shape (docs/src/node_example.md): x.^3 -> Dense(2, 15, tanh) -> Dense(15, 2), 100 trajectories, 30 save
points over [0, 1.5], Tsit5 at reltol 1e-7 / abstol 1e-9, M = 5 -- tools/node_bench.py's problem.

    python tools/node_grad_bench.py [--reps 50] [--itr 30] [--out profiles/node_grad_bench.log]

Reports, for C = 1 point and C = 512 stacked points:
  the forward integration alone (si_logdensity: kernel time of class "dense", and the call's wall time), measured in this run;
  value and gradient (si_logdensity_grad_batch): kernel time of the forward with record (class "dense") and of the reverse kernel
  with its sum (class "backward"), the call's wall time, and the ratio of the value-and-gradient call to the forward call;
  si_sample_hmc and si_sample_nuts transitions per second per call of C chains (wall clock over the whole call);
and, once, the frozen-step gradient against central differences of the ADAPTIVE density along three directions in z -- reported,
not a test: step decisions make that function piecewise.
Every timing is the mean of five blocks after a warm-up block; the spread is the range of the block means.  Needs a GPU."""
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
    ap.add_argument("--itr", type=int, default=30)
    ap.add_argument("--max-steps", type=int, default=2000, help="the record is sized by it: 100 x 2000 x 4 doubles per chain")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "node_grad_bench.log"))
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
    kw = dict(t0=0.0, reltol=1e-7, abstol=1e-9, pre_power=3, max_steps=args.max_steps)
    table = [(2, 15, flux.tanh, 0, 30), (15, 2, flux.identity, 45, 75)]
    y = node.solve(table, w_swa, u0, ts, node.Opts(**kw)).U + 0.05 * rng.standard_normal((2 * S, F))

    def blocks(ctx, classes, call, r):
        kern, wall = {c: [] for c in classes}, []
        for blk in range(6):          # block 0 warms the shape up and is dropped
            ctx.set_profiling(True, classes)
            ctx.reset_stats()
            t0 = time.perf_counter()
            for _ in range(r):
                call()
            t1 = time.perf_counter()
            st = ctx.stats()
            ctx.set_profiling(False)
            if blk:
                for c in classes:
                    kern[c].append(st[c]["ms"] * 1e3 / r)
                wall.append((t1 - t0) * 1e6 / r)
        return {c: np.array(v) for c, v in kern.items()}, np.array(wall)

    with si.Context(0) as ctx:
        ctx.infer_setup_node(table, n, M, w_swa, p, u0, np.asfortranarray(y), ts, **kw)
        ctx.node_set_grad(True)
        say("device: %s   2 -> 15 -> 2 behind the cube, f = %d, S = %d, reltol 1e-7, abstol 1e-9, M = %d, max_steps = %d, reps = %d; "
            "G = %d, %d chains per pass" % (ctx.device_name(), F, S, M, args.max_steps, args.reps, ctx.node_info()[4], ctx.node_grad_info()[1]))
        r = max(1, args.reps // 5)
        for c in (1, 512):
            z = np.asfortranarray(0.3 * rng.standard_normal((M, c)))
            _, _, na, nr, st = ctx.node_solve(z, want_u=False)
            say("C = %3d  accepted %.2f, rejected %.2f steps per trajectory, %d of %d trajectories unfinished" % (c, na.mean(), nr.mean(), int((st != 0).sum()), st.size))
            kf, wf = blocks(ctx, ["dense"], lambda: ctx.logdensity(z), r)
            say("C = %3d  forward alone          integration %9.1f us (blocks %.1f .. %.1f); si_logdensity call %9.1f us (%.1f .. %.1f)" % (
                c, kf["dense"].mean(), kf["dense"].min(), kf["dense"].max(), wf.mean(), wf.min(), wf.max()))
            kg, wg = blocks(ctx, ["dense", "backward"], lambda: ctx.logdensity_grad_batch(z), r)
            say("C = %3d  value and gradient     forward with record %9.1f us (%.1f .. %.1f), reverse + sum %9.1f us (%.1f .. %.1f); "
                "si_logdensity_grad_batch call %9.1f us (%.1f .. %.1f)" % (c, kg["dense"].mean(), kg["dense"].min(), kg["dense"].max(), kg["backward"].mean(),
                                                                          kg["backward"].min(), kg["backward"].max(), wg.mean(), wg.min(), wg.max()))
            say("C = %3d  ratios: kernels (record + reverse) / forward %.2f, reverse / forward %.2f, call / call %.2f" % (
                c, (kg["dense"].mean() + kg["backward"].mean()) / kf["dense"].mean(), kg["backward"].mean() / kf["dense"].mean(), wg.mean() / wf.mean()))
            for name, fn in (("HMC", ctx.sample_hmc), ("NUTS", ctx.sample_nuts)):
                fn(4, 0.05, 1, 0, c)
                rates = []
                for blk in range(3):
                    t0 = time.perf_counter()
                    fn(args.itr, 0.05, 1, 0, c)
                    rates.append(args.itr / (time.perf_counter() - t0))
                rates = np.array(rates)
                say("C = %3d  %-4s %9.1f transitions/s per call of %d chains (%.1f .. %.1f), %.1f chain-transitions/s" % (
                    c, name, rates.mean(), c, rates.min(), rates.max(), rates.mean() * c))
        # the frozen-step gradient against central differences of the adaptive density (steps free to move): reported only
        z0 = np.asfortranarray(0.3 * rng.standard_normal((M, 1)))
        _, g = ctx.logdensity_grad_batch(z0)
        for k in range(3):
            v = rng.standard_normal(M)
            v /= np.sqrt(v @ v)
            gv = float(g[:, 0] @ v)
            for h in (1e-3, 1e-4, 1e-5):
                zz = np.asfortranarray(np.stack([z0[:, 0] + h * v, z0[:, 0] - h * v], axis=1))
                lp = ctx.logdensity(zz)
                fd = (lp[0] - lp[1]) / (2.0 * h)
                say("direction %d  h = %.0e  frozen-step g.v %+.10e   central difference of the adaptive lp %+.10e   relative difference %.2e" % (
                    k, h, gv, fd, abs(gv - fd) / abs(fd)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
