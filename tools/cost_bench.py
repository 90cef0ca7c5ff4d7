"""Times a queued training step (si_train_step without the loss read-back) for every cost of si_train_set_cost, and for mse, on
one GPU:

    dense10    a 10-class Dense classifier 784-256-10 (relu, identity), batch 4096        (Float64 and Float32 data)
    head1000   a 1000-wide head 64-128-1000 (relu, identity), batch 512                   (Float64 and Float32 data)
    cnn        a small CNN in BASELINE cfg4's style on 32 x 32 x 3 images, batch 256: conv3x3 3->16 + MaxPool 2, conv3x3 16->32 +
               MaxPool 2, flatten, Dense 2048->64 (relu), Dense 64->10

    python tools/cost_bench.py [--reps 200] [--out profiles/cost_bench.log]
    python tools/cost_bench.py --lib OTHER/libsubspace_hip.so       # another build of the library, e.g. the parent commit's: a
                                                                    # build without si_train_set_cost is timed with mse alone

One context and one set-up per shape; the optimiser is Descent with eta = 0, so every step does the same work on the same weights.
The costs alternate block by block (si_train_set_cost between two blocks), five timed blocks of `reps` queued steps each behind a
warm-up block of every cost; a block is timed by the host clock around its steps and the synchronisation that ends it.  Printed per
cost: the mean over the five blocks of the time per step, and their range (the run-to-run spread the comparison has to exceed).
Needs a GPU (there is no fallback)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BLOCKS = 5


def shapes(so):
    r, i = so.ACT_RELU, so.ACT_IDENTITY
    cnn = [("conv", (3, 3), 16, r, (1, 1), (1, 1)), ("maxpool", (2, 2)), ("conv", (3, 3), 32, r, (1, 1), (1, 1)), ("maxpool", (2, 2)),
           ("flatten",), ("dense", 64, r), ("dense", 10, i)]
    out = []
    for name, dims, batch in (("dense10", [784, 256, 10], 4096), ("head1000", [64, 128, 1000], 512)):
        table, n = so.layer_table(dims, [r, i])
        for dt in (np.float64, np.float32):
            out.append(("%s/%s" % (name, "f64" if dt == np.float64 else "f32"), table, n, dims[0], dims[-1], batch, dt))
    table, n = so.conv_table(cnn, (32, 32, 3))
    out.append(("cnn/f64", table, n, 32 * 32 * 3, 10, 256, np.float64))
    return out


def run(args, say):
    from subspaceinference_jl_amd import _capi, costs
    if args.lib:
        _capi.LIB_PATH = os.path.abspath(args.lib)
    with open(_capi.LIB_PATH, "rb") as fh:   # (looked up in the file: the library is loaded once, by the package, behind torch)
        has_costs = b"si_train_set_cost" in fh.read()
    if not has_costs:   # a build from before the costs: mse alone, through the calls it has
        for name in ("si_train_set_cost", "si_train_cost_info"):
            _capi.SIGNATURES.pop(name, None)
    import subspaceinference_jl_amd as si
    from oracle import subspace_oracle as so

    kinds = list(costs.KINDS) if has_costs else [costs.MSE]
    result = {"lib": _capi.LIB_PATH, "reps": args.reps, "rows": []}
    with si.Context(0) as ctx:
        say("device: %s   library: %s   %d blocks of %d queued steps per cost" % (ctx.device_name(), _capi.LIB_PATH, BLOCKS, args.reps))
        for name, table, n, fin, fout, batch, dt in shapes(so):
            rng = np.random.default_rng(0)
            x = np.asfortranarray(rng.standard_normal((fin, batch)).astype(dt))
            y = np.zeros((fout, batch), dtype=dt, order="F")
            y[rng.integers(0, fout, batch), np.arange(batch)] = 1.0
            w0 = (rng.standard_normal(n) * np.sqrt(2.0 / 256)).astype(np.float32)
            ctx.train_setup(table, n, w0, x, y, batch, 0, 0.0)
            ids = np.arange(batch, dtype=np.int64)
            us = {k: [] for k in kinds}
            for blk in range(BLOCKS + 1):      # block 0 warms every cost up and is dropped
                for k in kinds:
                    if has_costs:
                        ctx.train_set_cost(k, 1.0 if k == costs.HUBER else 0.0)
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.reps):
                        ctx.train_step(ids, want_loss=False)
                    ctx.synchronize()
                    if blk:
                        us[k].append((time.perf_counter() - t0) * 1e6 / args.reps)
            for k in kinds:
                t = np.array(us[k])
                say("%-14s %-24s %9.1f us per step  (blocks %.1f .. %.1f)" % (name, costs.NAMES[k], t.mean(), t.min(), t.max()))
                result["rows"].append({"shape": name, "cost": costs.NAMES[k], "us_mean": t.mean(), "us_min": t.min(), "us_max": t.max()})
    say("JSON " + json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cost_bench.log"))
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
