"""The case lists of tests/test_ae_train_cpu.py and tests/test_gpu_ae_train.py: the autoencoder training step (si_ae_train_*;
csrc/kernels_ae_train.hip) against its definition, subspaceinference_jl_amd/autoencoder.py: train_step.

Lattice cases: integer parameters and data, identity / relu, so that every sum of the step is an exact integer below 2^53 whatever
order the device takes it in and each gradient element is ONE rounded product s * G: the device is held to array_equal.  The shapes
are the smallest at which each piece can go wrong, computed from the constants read out of the kernel file.
Real-valued cases: all eight activations with and without the penalty, 12 ADAM steps over shuffled batches with a ragged last one,
plus Momentum and Descent; audited step by step within SPREAD_TOL (measured on the CPU, see there)."""
import os
import re
from collections import namedtuple

import numpy as np

from subspaceinference_jl_amd import flux

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "subspaceinference.jl_amd", "csrc", "kernels_ae_train.hip")


def kernel_constant(name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, open(KERNELS).read()).group(1))


AE_ROWS = kernel_constant("AE_ROWS")      # rows of a row block = a workgroup's row span
AE_GRID = kernel_constant("AE_GRID")      # most workgroups of a row kernel: more row blocks put it on a second grid-stride pass
I, R = flux.identity, flux.relu

Case = namedtuple("Case", "name n enc dec acts k batch")   # enc / dec: the hidden widths; layers N -> enc.. -> dec.. -> N


def widths(case):
    return (case.n,) + tuple(case.enc) + tuple(case.dec) + (case.n,)


def depth(case):
    """(E, D)"""
    return len(case.enc), len(case.dec) + 1


def table_of(case):
    w = widths(case)
    table, off = [], 0
    for l in range(len(w) - 1):
        table.append((w[l], w[l + 1], case.acts[l], off, off + w[l] * w[l + 1]))
        off += w[l] * w[l + 1] + w[l + 1]
    return table, off


B = AE_ROWS
LATTICE = [
    #    name            N            enc        dec      acts            K  batch
    Case("n1", 1, (1,), (), (I, I), 1, (0,)),
    Case("n2", 2, (3,), (), (R, I), 5, (4, 1)),
    Case("n3-e2", 3, (4, 1), (), (I, R, I), 5, (0, 1, 2, 3, 4)),
    Case("below-block-d2", B - 1, (17,), (3,), (I, R, I), 7, (6, 0, 3, 5, 2)),
    Case("at-block-e3-d3", B, (3, 4, 2), (3, 17), (R, I, I, R, I, I), 9, (8, 1, 0, 7, 2, 6, 3, 5)),
    Case("above-block", B + 1, (1,), (4,), (I, I, R), 7, (5, 6)),          # the ragged last batch of K = 7 at batchsize 5
    Case("three-blocks-e2-d2", 2 * B + 1, (4, 3), (17,), (R, R, I, I), 7, (3,)),      # a batch of one
    Case("h17-relu-out", B + 3, (17,), (), (I, R), 5, (1, 3, 0, 2, 4)),
    Case("second-pass", B * AE_GRID + B + 1, (3,), (), (I, I), 2, (1, 0)),            # row blocks > AE_GRID: a second grid-stride pass
]
OPTIMISERS = {"descent": (0, 2.0 ** -3, 0.0, 0.0), "momentum": (1, 0.01, 0.9, 0.0), "adam": (2, 0.001, 0.9, 0.999)}


def lattice_problem(case, dtype):
    """(table, w, X): integers in -1 .. 1 (parameters) and -2 .. 2 (data), exact in Float32"""
    table, npar = table_of(case)
    rng = np.random.default_rng(len(case.name) + case.n)
    w = rng.integers(-1, 2, size=npar).astype(dtype)
    x = np.asfortranarray(rng.integers(-2, 3, size=(case.n, case.k)).astype(np.float64))
    return table, w, x


def lattice_integers(case):
    """the step's unscaled sums in integer arithmetic: (sum r^2, G flat as int64, the largest sum of absolute terms met)"""
    table, w, x = lattice_problem(case, np.float64)
    wi, xb = w.astype(np.int64), x[:, list(case.batch)].astype(np.int64)
    big = 0
    outs, mats = [xb], []
    for fin, fout, act, w_off, b_off in table:
        W = wi[w_off:w_off + fin * fout].reshape((fout, fin), order="F")
        u = W @ outs[-1] + wi[b_off:b_off + fout][:, None]
        big = max(big, int((np.abs(W) @ np.abs(outs[-1])).max()) + 1)
        outs.append(np.maximum(u, 0) if act == R else u)
        mats.append(W)
    r = outs[-1] - xb
    ssq = int((r * r).sum())
    big = max(big, ssq)
    g = np.zeros(wi.size, dtype=np.int64)
    dt = r * ((outs[-1] > 0).astype(np.int64) if table[-1][2] == R else 1)
    for l in range(len(table) - 1, -1, -1):
        fin, fout, act, w_off, b_off = table[l]
        g[w_off:w_off + fin * fout] = (dt @ outs[l].T).reshape(-1, order="F")
        g[b_off:b_off + fout] = dt.sum(axis=1)
        big = max(big, int((np.abs(dt) @ np.abs(outs[l]).T).max()))
        if l > 0:
            back = mats[l].T @ dt
            big = max(big, int((np.abs(mats[l]).T @ np.abs(dt)).max()))
            dt = back * ((outs[l] > 0).astype(np.int64) if table[l - 1][2] == R else 1)
    return ssq, g, big


RealCase = namedtuple("RealCase", "name act penalty opt dtype")
REAL_N, REAL_ENC, REAL_DEC, REAL_K, REAL_BATCH, REAL_STEPS = 2 * AE_ROWS + 44, (5, 3), (4,), 13, 5, 12
ACTS = {"identity": flux.identity, "relu": flux.relu, "tanh": flux.tanh, "sigmoid": flux.sigmoid, "leakyrelu": flux.leakyrelu,
        "elu": flux.elu, "softplus": flux.softplus, "selu": flux.selu}
REAL = ([RealCase("%s%s" % (a, "-penalty" if p else ""), ACTS[a], p, "adam", np.float32 if i % 2 else np.float64)
         for i, a in enumerate(ACTS) for p in (False, True)]
        + [RealCase("tanh-momentum", flux.tanh, False, "momentum", np.float32), RealCase("elu-descent", flux.elu, True, "descent", np.float64)])


def real_problem(case, dtype=None):
    """(table, w, X, batches): Float32 or Float64 parameters (dtype overrides the case's), the 12 batches of shuffled epochs of 5, 5, 3"""
    shape = Case(case.name, REAL_N, REAL_ENC, REAL_DEC, (case.act,) * 3 + (flux.identity,), REAL_K, ())
    table, npar = table_of(shape)
    rng = np.random.default_rng(sum(case.name.encode()))
    w = np.zeros(npar)
    for fin, fout, act, w_off, b_off in table:                      # Glorot-sized weights, small biases
        w[w_off:w_off + fin * fout] = rng.standard_normal(fin * fout) * np.sqrt(2.0 / (fin + fout))
        w[b_off:b_off + fout] = 0.1 * rng.standard_normal(fout)
    x = np.asfortranarray(0.3 * rng.standard_normal((REAL_N, REAL_K)))
    batches = []
    while len(batches) < REAL_STEPS:
        batches += list(flux.DataLoader(x, batchsize=REAL_BATCH, shuffle=True, rng=rng).index_batches())
    return table, w.astype(dtype or case.dtype), x, [np.asarray(b, dtype=np.int64) for b in batches[:REAL_STEPS]]


# The largest spread of the definition over REAL (Float64 parameters, every step of every case) when the three N-long sums are
# taken in ascending, pairwise and the device's blocked order: max |a - b| / max |a| over the loss and the arrays w, m, v after
# the step.  tests/test_ae_train_cpu.py measures it and keeps this constant within 10 % above the measurement; the GPU audit
# allows 8 x it (the device's libm also differs from NumPy's by an ulp in tanh / exp / log1p), plus one Float32 ulp on a stored
# Float32 value.
SPREAD_TOL = 4.2e-15


def rel_gap(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = float(np.max(np.abs(a))) if a.size else 0.0
    return float(np.max(np.abs(a - b))) / scale if scale > 0.0 else float(np.max(np.abs(a - b)))
