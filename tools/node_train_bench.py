"""Times the NeuralODE training step (si_train_setup_node; csrc/kernels_node.hip: the forward with record and the reverse kernel,
csrc/kernels_node_train.hip: the tail) at the tutorial's shape (docs/src/node_example.md): x.^3 -> Dense(2, 15, tanh) -> Dense(15, 2),
f = 100 trajectories, S = 30 save points over [0, 1.5], Tsit5 at reltol 1e-7 / abstol 1e-9, ADAM(0.1), max_steps = 2000,
cost flux.node_sse.

    python tools/node_train_bench.py [--reps 100] [--out profiles/node_train_bench.log]

Reports
  the queued step (si_train_step without loss_out, one synchronisation per block) at batch 1 and at batch 100: microseconds per step
  on the host clock, and the kernel split from the library's event pairs in a run of its own (classes "sse": batch gather, ||W||^2 and
  the zeroing of the slices; "dense": the forward with record; "backward": the reverse kernel; "reconstruct": the tail kernel);
  one T = 1 epoch of subspace_construction with its pushes, end to end, on the device step and, for scale, on the host step.
The weights are put back before every block, so that every block times the same steps.  Every timing is the mean of five blocks
after a warm-up block; the spread is the range of the block means.  Nothing is asserted.  Needs a GPU."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F, S = 100, 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100, help="steps per block at batch 1 (a quarter of it at batch 100)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "node_train_bench.log"))
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    import subspaceinference_jl_amd as si
    from subspaceinference_jl_amd import flux

    rng = np.random.default_rng(0)
    ts = np.linspace(0.0, 1.5, S)

    def model(seed):
        return flux.NeuralODE(flux.Chain(flux.cube, flux.Dense(2, 15, "tanh", rng=np.random.default_rng(seed)),
                                         flux.Dense(15, 2, rng=np.random.default_rng(seed + 1))),
                              (0.0, 1.5), ts, reltol=1e-7, abstol=1e-9, max_steps=2000, sensealg="discrete_adjoint")
    u0 = np.asfortranarray(rng.uniform(-1.0, 1.0, (2, F)))
    y = np.asfortranarray(model(11)(u0) + 0.05 * rng.standard_normal((2 * S, F)))
    m0 = model(21)
    table, n = flux.layer_table(m0.chain)
    w0 = flux.extract_params(flux.params(m0))
    classes = ["sse", "dense", "backward", "reconstruct"]

    with si.Context(0) as ctx:
        say("device: %s   2 -> 15 tanh -> 2 behind the cube, f = %d, S = %d, reltol 1e-7, abstol 1e-9, ADAM(0.1), max_steps = 2000, N = %d" % (
            ctx.device_name(), F, S, n))
        for bs in (1, F):
            reps = args.reps if bs == 1 else max(8, args.reps // 4)
            batches = [np.arange(i, i + bs, dtype=np.int64) % F for i in range(0, reps * bs, bs)]
            # (batch 1 walks through the data: the index path but for observation 0; batch 100 is 0 .. 99 in order: used in place)

            def block(profile):
                ctx.train_setup_node(table, n, w0, u0, y, ts, bs, 2, 0.1, 0.9, 0.999, 100.0, **m0.options())
                ctx.train_step(batches[0], want_loss=True)          # (code objects, the pinned buffers)
                ctx.synchronize()
                if profile:
                    ctx.set_profiling(True, classes)
                    ctx.reset_stats()
                t0 = time.perf_counter()
                for b in batches:
                    ctx.train_step(b, want_loss=False)
                ctx.synchronize()
                t1 = time.perf_counter()
                st = ctx.stats() if profile else None
                if profile:
                    ctx.set_profiling(False)
                return (t1 - t0) * 1e6 / len(batches), st
            wall = np.array([block(False)[0] for _ in range(6)][1:])
            say("batch %3d  queued step %9.1f us (blocks %.1f .. %.1f), %d steps per block; failed step: %d" % (
                bs, wall.mean(), wall.min(), wall.max(), len(batches), ctx.train_node_info()[2]))
            prof = [block(True) for _ in range(6)][1:]
            kern = {c: np.array([st[c]["ms"] * 1e3 / len(batches) for _, st in prof]) for c in classes}
            pw = np.array([w for w, _ in prof])
            say("batch %3d  kernels per step (event pairs, a run of its own: %9.1f us per step on the host clock): " % (bs, pw.mean()) + "; ".join(
                "%s %.1f us (%.1f .. %.1f)" % (c, kern[c].mean(), kern[c].min(), kern[c].max()) for c in classes) +
                "; sum %.1f us" % sum(kern[c].mean() for c in classes))
        for dev in (True, False):
            times = []
            for blk in range(3 if dev else 2):          # (the host step integrates in NumPy: one block after its warm-up)
                mdl = model(21)
                data = flux.DataLoader(u0, y) if dev else flux.DataLoader(u0[:, :10], y[:, :10])
                t0 = time.perf_counter()
                si.subspace_construction(mdl, flux.node_sse, data, flux.ADAM(0.1), T=1, M=3, ctx=ctx, verbose=False, device_training=dev)
                times.append(time.perf_counter() - t0)
            t = np.array(times[1:])
            if dev:
                say("one T = 1 epoch, batchsize 1, 100 steps with their pushes and the finish, device step: %.1f ms (blocks %.1f .. %.1f)" % (
                    t.mean() * 1e3, t.min() * 1e3, t.max() * 1e3))
            else:
                say("the same through the host step (node.py in NumPy), 10 of the 100 observations: %.1f ms, i.e. %.1f ms per step" % (
                    t.mean() * 1e3, t.mean() * 1e2))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
