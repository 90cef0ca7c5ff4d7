"""Times the decoder's two streaming kernels (csrc/kernels_decoder.hip: the last layer forward and its reverse) at BASELINE cfg2's
N = 1 047 361 with H = 20, for 1 and 8 points, with the parameters stored in fp64 and in fp32, next to their yardsticks on the same
context at the same N with M = H: K4 (reconstruct_kernel, class SI_K_RECON) and launch_ptg.  Reports achieved bytes/s.

    python tools/decoder_bench.py [--reps 200] [--out profiles/decoder_bench.log]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/decoder_bench.py --reps 50 --out DIR/run.log   (a run of its own)
    python tools/decoder_bench.py --parse DIR [--out profiles/decoder_bench_kernels.log]

The model is cfg2's chain on B = 16 observations: the streaming kernels depend on N, H and the point count only, and a small B keeps
the network's own kernels out of the way.  The decoder is D = 1 (identity, W_1 = P, zero bias): with fp64 storage it streams the
bytes K4 streams.  Needs a GPU (there is no fallback).

Forward: the library's event pairs around the weight-forming launches of si_logdensity (class "reconstruct"), `reps` calls per
variant in five blocks, the variants alternating block by block so that they share whatever else the machine is doing; the spread
is the range of the per-call means over the five blocks (a warm-up block in front is dropped).  Reverse: the pull-back has no event class of its own, so its kernel times come from
the kernel trace (`--parse` reads rocprofv3's kernel_stats.csv of a traced run and prints every kernel of interest by name).
Algorithmic bytes: forward  N * (e * (H + 1) + 8) read + 8 * N * C written (e = 8 or 4 bytes per parameter; K4 has no bias column:
8 * N * (M + 1) read); reverse  N * (e * H + 16) read (launch_ptg: 8 * N * (M + 1))."""
import argparse
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_CFG2, H = 1047361, 20
DIMS, ACTS = [128, 960, 960, 1], [1, 1, 0]
PEAK_HBM = 8.0e12


def fwd_bytes(n, h, c, e, bias=True):
    """decoder: W_D, the bias and W_swa read, C weight vectors written; K4 (bias=False) has no bias column"""
    return n * (e * (h + (1 if bias else 0)) + 8.0) + 8.0 * n * c


def rev_bytes(n, h, e):
    return n * (e * h + 16.0)


def parse(dirname, say):
    rows = {}
    for path in glob.glob(os.path.join(dirname, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            name = r.get("Name") or r.get("KernelName") or ""
            if any(k in name for k in ("reconstruct_kernel", "decoder_last_fwd", "decoder_last_rev", "ptg_partial", "ptg_final", "decoder_head")):
                calls, tot = int(r["Calls"]), float(r["TotalDurationNs"])
                c0, t0 = rows.get(name, (0, 0.0))
                rows[name] = (c0 + calls, t0 + tot)
    if not rows:
        raise SystemExit("no kernel_stats.csv with the kernels of interest under " + dirname)
    for name, (calls, tot) in sorted(rows.items()):
        us = tot / calls / 1e3
        e = 4.0 if "<float" in name else 8.0
        cb = 4 if ", 4>" in name or "<4>" in name else 2 if ", 2>" in name or "<2>" in name else 1
        note = ""
        if "last_fwd" in name or "reconstruct_kernel" in name:
            # this tool's calls: CB = 1 is the 1-point launch; CB = 4 is the 8-point launch, two passes of four stacked in grid.y
            by = fwd_bytes(N_CFG2, H, cb, e, "reconstruct_kernel" not in name) * (2 if cb == 4 else 1)
            note = "  %6.1f MB  %.2f TB/s (%d point%s)" % (by / 1e6, by / us / 1e6, 8 if cb == 4 else cb, "s" if cb > 1 else "")
        elif "last_rev_partial" in name or "ptg_partial" in name:
            by = rev_bytes(N_CFG2, H, e) if "last_rev" in name else 8.0 * N_CFG2 * (H + 1)
            note = "  %6.1f MB  %.2f TB/s" % (by / 1e6, by / us / 1e6)
        say("%-72s calls %5d  mean %8.2f us%s" % (name[:72], calls, us, note))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder_bench.log"))
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


def run(args, say):
    import subspaceinference_jl_amd as si
    from oracle import subspace_oracle as so

    table, n = so.layer_table(DIMS, ACTS)
    assert n == N_CFG2
    rng = np.random.default_rng(0)
    b = 16
    x, y = rng.standard_normal((DIMS[0], b)), rng.standard_normal((1, b))
    w_swa = (0.05 * rng.standard_normal(n)).astype(np.float64)
    p = np.asfortranarray(0.01 * rng.standard_normal((n, H)))
    dec_table = [(H, n, 0, 0, n * H)]
    wdec64 = np.concatenate([p.reshape(-1, order="F"), np.zeros(n)])
    variants = (("K4 (P route)", None, 8.0), ("decoder fp64", wdec64, 8.0), ("decoder fp32", wdec64.astype(np.float32), 4.0))
    with si.Context(0) as ctx:
        say("device: %s   N = %d, H = M = %d, B = %d, reps = %d" % (ctx.device_name(), n, H, b, args.reps))
        ctx.infer_setup(table, n, H, w_swa, p, x, y, 1.0)
        ctx.set_chain_loop(0)
        ref = {}
        for c in (1, 8):
            z = np.asfortranarray(0.1 * rng.standard_normal((H, c)))
            blocks = {v[0]: [] for v in variants}
            for blk in range(6):          # block 0 warms every shape up and is dropped
                r = max(1, args.reps // 5)
                for name, wdec, _e in variants:       # (setting a decoder re-lays N x H parameters out: once per block, not per call)
                    ctx.set_decoder(None, None) if wdec is None else ctx.set_decoder(dec_table, wdec)
                    ctx.set_profiling(True, ["reconstruct"])
                    ctx.reset_stats()
                    for _ in range(r):
                        lp = ctx.logdensity(z)
                    st = ctx.stats()["reconstruct"]
                    ctx.set_profiling(False)
                    if name == "decoder fp64":
                        assert np.array_equal(lp, ref[c]), "the fp64 identity decoder must give K4's bits"
                    elif wdec is None:
                        ref[c] = lp
                    if blk:
                        blocks[name].append(st["ms"] * 1e3 / r)
            k4 = float(np.mean(blocks["K4 (P route)"]))
            for name, _w, e in variants:
                us = np.array(blocks[name])
                by = fwd_bytes(n, H, c, e, not name.startswith("K4"))
                say("forward, %d point%s  %-14s %8.2f us (blocks %.2f .. %.2f)  %6.1f MB  %5.2f TB/s  %4.1f %% of %.0f TB/s   time / K4 = %.3f"
                    % (c, "s" if c > 1 else " ", name, us.mean(), us.min(), us.max(), by / 1e6, by / us.mean() / 1e6,
                       100.0 * by / us.mean() / 1e6 / (PEAK_HBM / 1e12), PEAK_HBM / 1e12, us.mean() / k4))
        # the reverse kernels, for the kernel trace of a run under rocprofv3 (no event class of their own)
        z1 = 0.1 * rng.standard_normal(H)
        for name, wdec, _e in variants:
            ctx.set_decoder(None, None) if wdec is None else ctx.set_decoder(dec_table, wdec)
            for _ in range(max(2, args.reps // 10)):
                g = ctx.logdensity_grad(z1)[1]
            say("reverse  %-14s ran %d times (gradient norm %.6e); kernel times: the kernel trace (--parse)" % (name, max(2, args.reps // 10),
                                                                                                               float(np.linalg.norm(g))))


if __name__ == "__main__":
    main()
