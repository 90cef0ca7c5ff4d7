"""Times si_construct_finish_diffmap at the size of the reference's tutorial model (docs/src/nn_example.md:112-118: N = 15 801
weights; K = 200 snapshots, M = 20) and writes profiles/diffmap_nn_example.log.

    python tools/diffmap_bench.py [--n 15801] [--k 200] [--m 20] [--reps 3] [--out profiles/diffmap_nn_example.log]

The deviation matrix is synthetic (clustered weights, seeded): the time of the call depends on N, K, M and on how many iterations
the spectrum takes, not on where the numbers came from.  Needs a GPU (there is no fallback).  One warm-up call, then `reps` calls
timed with a host clock around the synchronous call (wall) and, in a run of their own, with the library's event pairs per kernel
class (profiling on serialises nothing but adds events, so the wall time is taken with it off).
Peaks used for the shares: fp64 matrix 78.6 TFLOP/s, HBM 8 TB/s spec (about 6.3 achievable), DESIGN section 2."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_F64_MATRIX, PEAK_HBM = 78.6e12, 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=15801)
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--m", type=int, default=20)
    ap.add_argument("--clusters", type=int, default=48)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tol", type=float, default=0.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diffmap_nn_example.log"))
    args = ap.parse_args()
    import subspaceinference_jl_amd as si

    n, k, m = args.n, args.k, args.m
    rng = np.random.default_rng(0)
    cen = rng.random((args.clusters, k))
    lab = rng.integers(0, args.clusters, n)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with si.Context(0) as ctx:
        say("device: %s   N = %d, K = %d, M = %d, block = %d" % (ctx.device_name(), n, k, m, min(n - 1, 2 * m + 16)))
        ctx.construct_begin(n, k)
        s = np.zeros(n)
        for j in range(k):   # (snapshots whose deviation columns are the clustered columns: tests/diffmap_cases.py push_columns)
            col = cen[lab, j] * (1.0 + j / max(k - 1, 1)) + 0.05 * rng.standard_normal(n)
            ctx.construct_push(s + 2.0 * col, 1.0)
            s = s + col

        def call():
            t0 = time.perf_counter()
            err = None
            try:
                ctx.construct_finish_diffmap(m, tol=args.tol, want_swa=False, want_p=False)
            except si.SubspaceError as e:   # a spectrum that is not separated: the figures of the iterations still stand
                err = str(e)
            return time.perf_counter() - t0, err

        _, err = call()   # warm-up: allocations, code objects
        if err:
            say("note: " + err)
        walls = [call()[0] for _ in range(args.reps)]
        iters, res = ctx.diffmap_info()
        say("iterations %d, largest leading residual %.3e" % (iters, res))
        say("wall time per call (profiling off, %d calls): %s ms, median %.2f ms" % (
            args.reps, ", ".join("%.2f" % (1e3 * w) for w in walls), 1e3 * float(np.median(walls))))
        ctx.set_profiling(True)
        ctx.reset_stats()
        call()
        ctx.synchronize()
        st = ctx.stats()
        ctx.set_profiling(False)
        pair = st["gram"]       # this call books the pairwise kernel alone under it (the stacked Gram of the iteration is not booked)
        prod = st["project"]    # Kn V, the rotations, the residual vectors, the final vectors
        n_prod = iters          # one Kn V per iteration; the other launches of the class stream N x 2b, 1e-3 of the bytes
        say("pairwise kernel: %.3f ms, %.1f GFLOP formed (upper triangle), %.2f TFLOP/s = %.3f of the fp64 matrix peak; "
            "it writes %.2f GB: %.2f TB/s = %.3f of HBM spec" % (
                pair["ms"], pair["flops"] / 1e9, pair["flops"] / pair["ms"] / 1e9, pair["flops"] / pair["ms"] / 1e9 / (PEAK_F64_MATRIX / 1e12),
                pair["bytes"] / 1e9, pair["bytes"] / pair["ms"] / 1e9, pair["bytes"] / pair["ms"] / 1e9 / (PEAK_HBM / 1e12)))
        say("normalisation passes (two read-modify-write passes over Kmat): %.3f ms, %.2f TB/s" % (
            st["gram_reduce"]["ms"], st["gram_reduce"]["bytes"] / max(st["gram_reduce"]["ms"], 1e-9) / 1e9))
        say("products (class total %.3f ms over %d launches): %.3f ms per iteration; Kn is %.2f GB: %.2f TB/s = %.3f of HBM spec" % (
            prod["ms"], prod["launches"], prod["ms"] / max(n_prod, 1), n * n * 8 / 1e9, prod["bytes"] / prod["ms"] / 1e9,
            prod["bytes"] / prod["ms"] / 1e9 / (PEAK_HBM / 1e12)))
        say("host eigensolver + block algebra: %.3f ms over %d iterations" % (st["eig_host"]["ms"], st["eig_host"]["launches"]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
