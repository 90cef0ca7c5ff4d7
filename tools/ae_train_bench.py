"""Times the autoencoder training step on the device (si_ae_train_step; csrc/kernels_ae_train.hip) at BASELINE cfg2's
N = 1 047 361 with K = 100 columns, encoder N -> 20, decoder 20 -> N, ADAM, batches of 5, with Float32 and with Float64 parameters,
next to the host step it replaces (the loop body of api.auto_encoder_subspace: flux.gradient + flux.update, and the read-back of A
that the device route drops) and to K4 (reconstruct_kernel) on the same context.

    python tools/ae_train_bench.py [--reps 100] [--host-steps 3] [--out profiles/ae_train_bench.log]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ae_train_bench.py --reps 20 --host-steps 0 --out DIR/run.log
    python tools/ae_train_bench.py --parse DIR [--out profiles/ae_train_bench_kernels.log]

Device: the library's event pairs per class of a step (SI_K_DENSE: first layer forward + head; SI_K_DENSE_MAIN: the pass over W_D with
its fused update; SI_K_BACKWARD: head reverse, loss, the updates of the small arrays and of W_1), `reps` queued steps per variant in
five blocks, the two variants alternating block by block; the spread is the range of the per-step means over the five blocks (a
warm-up block in front is dropped).  The kernels by name (and ptg_partial_kernel, which has no event class) come from the kernel
trace of a run of its own (`--parse`).  Needs a GPU (there is no fallback).

Algorithmic bytes per step, e = bytes per parameter, a = 8 (fp64 A), ADAM (w, m, v read and written: 5 e with the forward's read
counted once):   first forward  N (e e_1 + a nb);   last pass  N (5 e (H + 1) + a nb);   first update  N e_1 (5 e) + N a nb."""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_CFG2, K, E1, H, NB = 1047361, 100, 20, 20, 5
DIMS, ACTS = [128, 960, 960, 1], [1, 1, 0]
CLASSES = ("dense", "dense_main", "backward")


def step_bytes(n, e):
    return {"dense": n * (e * E1 + 8.0 * NB), "dense_main": n * (5.0 * e * (H + 1) + 8.0 * NB), "backward": n * E1 * 5.0 * e + n * 8.0 * NB}


def parse(dirname, say):
    rows = {}
    for path in glob.glob(os.path.join(dirname, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            name = r.get("Name") or r.get("KernelName") or ""
            if any(k in name for k in ("ae_", "reconstruct_kernel", "ptg_partial")):
                c0, t0 = rows.get(name, (0, 0.0))
                rows[name] = (c0 + int(r["Calls"]), t0 + float(r["TotalDurationNs"]))
    if not rows:
        raise SystemExit("no kernel_stats.csv with the kernels of interest under " + dirname)
    for name, (calls, tot) in sorted(rows.items()):
        us = tot / calls / 1e3
        e = 4.0 if "<float" in name else 8.0
        by = None
        if "ae_first_fwd" in name:
            by = step_bytes(N_CFG2, e)["dense"]
        elif "ae_last_kernel" in name and "true>" in name.replace(" ", ""):
            by = step_bytes(N_CFG2, e)["dense_main"]
        elif "ae_first_update" in name:
            by = step_bytes(N_CFG2, e)["backward"]
        elif "reconstruct_kernel<1>" in name:
            by = 8.0 * N_CFG2 * (H + 1) + 8.0 * N_CFG2
        elif "ptg_partial" in name:
            by = 8.0 * N_CFG2 * (H + 1)
        note = "  %7.1f MB  %.2f TB/s" % (by / 1e6, by / us / 1e6) if by else ""
        say("%-84s calls %5d  mean %9.2f us%s" % (name[:84], calls, us, note))


def host_step(say, steps, n_threads):
    """the parent's loop body at the same shape: flux.gradient(flux.mse, sae, xb, xb) and flux.update on Float32 parameters"""
    from subspaceinference_jl_amd import flux
    rng = np.random.default_rng(0)
    sae = flux.Chain(flux.Dense(N_CFG2, E1, flux.tanh, rng=rng), flux.Dense(E1, N_CFG2, rng=rng))
    ps, opt = flux.params(sae), flux.ADAM()
    xb = 0.01 * rng.standard_normal((N_CFG2, NB))
    times = []
    for _ in range(steps + 1):            # the first step allocates the optimiser's state and is dropped
        t0 = time.perf_counter()
        _, gs = flux.gradient(flux.mse, sae, xb, xb)
        flux.update(opt, ps, gs)
        times.append(time.perf_counter() - t0)
    t = np.array(times[1:]) * 1e3
    say("host step (flux.gradient + flux.update, Float32 parameters, %d CPUs): %8.1f ms (steps %.1f .. %.1f)" % (n_threads, t.mean(), t.min(), t.max()))
    return t.mean()


def run(args, say):
    import subspaceinference_jl_amd as si
    from oracle import subspace_oracle as so

    rng = np.random.default_rng(0)
    table = [(N_CFG2, E1, 2, 0, N_CFG2 * E1), (E1, N_CFG2, 0, N_CFG2 * E1 + E1, N_CFG2 * E1 + E1 + E1 * N_CFG2)]
    npar = N_CFG2 * E1 + E1 + E1 * N_CFG2 + N_CFG2
    w = (0.01 * rng.standard_normal(npar))
    batches = [np.asarray(b, dtype=np.int64) for b in np.split(rng.permutation(K), K // NB)]
    ctxs = {}
    for name, dtype in (("Float32", np.float32), ("Float64", np.float64)):
        ctx = si.Context(0)
        ctxs[name] = ctx
    ctx = ctxs["Float32"]
    say("device: %s   N = %d, K = %d, e_1 = H = %d, batch %d, ADAM, reps = %d" % (ctx.device_name(), N_CFG2, K, E1, NB, args.reps))
    # the deviation matrix through a construction, as the API leaves it: both variants read it in place; the read-back is timed once
    snaps = 0.01 * rng.standard_normal((K, N_CFG2)).astype(np.float32)
    readback = None
    for name, c in ctxs.items():
        c.construct_begin(N_CFG2, K, 0)
        for i in range(K):
            c.construct_push(snaps[i], float(1 + i // 4))
        if readback is None:
            t0 = time.perf_counter()
            a = c.construct_get_A(0, K)
            readback = time.perf_counter() - t0
            say("construct_get_A(0, %d): %.1f MB read back in %.1f ms (the device route drops it)" % (K, a.nbytes / 1e6, readback * 1e3))
            del a
        c.ae_train_setup(table, w.astype(np.float32 if name == "Float32" else np.float64), None, N_CFG2, NB, 2, 0.001, 0.9, 0.999)
    del snaps
    blocks = {name: {k: [] for k in CLASSES + ("wall",)} for name in ctxs}
    r = max(1, args.reps // 5)
    for blk in range(6):                  # block 0 warms up and is dropped
        for name, c in ctxs.items():
            c.set_profiling(True, list(CLASSES))
            c.reset_stats()
            t0 = time.perf_counter()
            for i in range(r):
                c.ae_train_step(batches[i % len(batches)], want_loss=False)
            c.synchronize()
            wall = time.perf_counter() - t0
            st = c.stats()
            c.set_profiling(False)
            if blk:
                for k in CLASSES:
                    blocks[name][k].append(st[k]["ms"] * 1e3 / r)
                blocks[name]["wall"].append(wall * 1e6 / r)
    dev_ms = {}
    for name in ctxs:
        e = 4.0 if name == "Float32" else 8.0
        tot = np.sum([blocks[name][k] for k in CLASSES], axis=0)
        dev_ms[name] = tot.mean() / 1e3
        say("%s parameters: step %8.1f us by the event pairs (blocks %.1f .. %.1f), %8.1f us wall per queued step (blocks %.1f .. %.1f)"
            % (name, tot.mean(), tot.min(), tot.max(), np.mean(blocks[name]["wall"]), np.min(blocks[name]["wall"]), np.max(blocks[name]["wall"])))
        for k, what in zip(CLASSES, ("first forward + head", "pass over W_D, fused update", "head reverse, loss, small arrays, W_1 update")):
            us = np.array(blocks[name][k])
            by = step_bytes(N_CFG2, e)[k]
            say("    %-46s %8.1f us (blocks %.1f .. %.1f)  %7.1f MB  %5.2f TB/s" % (what, us.mean(), us.min(), us.max(), by / 1e6, by / us.mean() / 1e6))
        say("    loss over all %d columns (si_ae_train_loss): %.6e" % (K, ctxs[name].ae_train_loss()))
    # K4 on the same context at the same N with M = H, for the rate of a plain stream (and ptg_partial_kernel for the kernel trace)
    tab, n = so.layer_table(DIMS, ACTS)
    x, y = rng.standard_normal((DIMS[0], 16)), rng.standard_normal((1, 16))
    p = np.asfortranarray(0.01 * rng.standard_normal((n, H)))
    ctx.infer_setup(tab, n, H, 0.05 * rng.standard_normal(n), p, x, y, 1.0)
    ctx.set_chain_loop(0)
    z = np.asfortranarray(0.1 * rng.standard_normal((H, 1)))
    ctx.logdensity(z)
    ctx.set_profiling(True, ["reconstruct"])
    ctx.reset_stats()
    for _ in range(r):
        ctx.logdensity(z)
    us = ctx.stats()["reconstruct"]["ms"] * 1e3 / r
    ctx.set_profiling(False)
    by = 8.0 * n * (H + 1) + 8.0 * n
    say("K4 reconstruct_kernel, 1 point, same context:          %8.1f us  %7.1f MB  %5.2f TB/s" % (us, by / 1e6, by / us / 1e6))
    for _ in range(3):
        ctx.logdensity_grad(z[:, 0])      # (ptg_partial_kernel for the kernel trace)
    for c in ctxs.values():
        c.close()
    if args.host_steps > 0:
        host = host_step(say, args.host_steps, int(os.environ.get("OMP_NUM_THREADS", len(os.sched_getaffinity(0)))))
        for name, ms in dev_ms.items():
            say("host step / device step (%s): %.0f x; with the read-back spread over the %d steps of a pass: %.0f x"
                % (name, host / ms, K // NB, (host + readback * 1e3 / (K // NB)) / ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ae_train_bench.log"))
    ap.add_argument("--parse", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if args.parse:
        parse(args.parse, say)
    else:
        run(args, say)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
