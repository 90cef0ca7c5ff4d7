"""Problems of the autoencoder route's tests (si_infer_set_decoder; subspaceinference_jl_amd/autoencoder.py is the definition) --
TEST INFRASTRUCTURE, no GPU needed.

MODELS are the target models: Dense chains with N in {7, 65, 129, 682} parameters -- odd N, N below and above one 64-row wave,
and the README toy -- on B <= 64 observations.

LATTICE is the exact case list: decoder weights, biases, z and W_swa are small integers and the activations identity or relu, so
that every product and every sum of `decode` / `weights` is an integer far below 2^53 and exact in fp64 (and every parameter is
exact in Float32 storage): the device must return the same bits whatever order it sums in.  tests/test_autoencoder_cpu.py proves the
premise on the CPU by recomputing every case in int64 (`int_decode`).
"""
import functools
from dataclasses import dataclass

import numpy as np

from oracle import subspace_oracle as so

I, R, T = so.ACT_IDENTITY, so.ACT_RELU, so.ACT_TANH

# N -> (dims, acts, B)
MODELS = {
    7: ((1, 2, 1), (T, I), 9),
    65: ((4, 6, 5), (T, I), 33),
    129: ((5, 8, 9), (R, I), 64),
    682: ((10, 20, 20, 2), (I, I, I), 40),     # README.md: Chain(Dense(10, 20), Dense(20, 20), Dense(20, 2))
}
POINT_COUNTS = (1, 2, 3, 4, 5, 8, 9)           # every CB branch of the last-layer kernel (4 / 2 / 1) and the grid.y stacking (>= 8)


@dataclass(frozen=True)
class Problem:
    n: int
    table: tuple
    x: np.ndarray
    y: np.ndarray
    w_swa: np.ndarray
    sigma_m: float


@functools.lru_cache(maxsize=None)
def problem(n, lattice=False):
    """the target model of N parameters with its data; lattice: an integer W_swa (the exact tests), else a random one"""
    dims, acts, b = MODELS[n]
    table, n_par = so.layer_table(list(dims), list(acts))
    assert n_par == n
    rng = np.random.default_rng(1000 + n)
    x = np.asfortranarray(rng.standard_normal((dims[0], b)))
    y = np.asfortranarray(rng.standard_normal((dims[-1], b)))
    w = rng.integers(-4, 5, n).astype(np.float64) if lattice else 0.3 * rng.standard_normal(n)
    for a in (x, y, w):
        a.setflags(write=False)
    return Problem(n, tuple(tuple(r) for r in table), x, y, w, 0.8)


def decoder_table(widths, acts):
    """rows (in, out, act, w_off, b_off) of a Dense decoder widths[0] -> ... -> widths[-1] in Flux.destructure order, and Nd"""
    table, nd = so.layer_table(list(widths), list(acts))
    return [tuple(r) for r in table], nd


@dataclass(frozen=True)
class LatticeCase:
    name: str
    n: int            # the target model (MODELS)
    widths: tuple     # M, h_1, ..., h_{D-1}, N
    acts: tuple       # D activations, identity or relu

    @property
    def m(self):
        return self.widths[0]

    @property
    def depth(self):
        return len(self.acts)


def _lattice_cases():
    cases, k = [], 0
    ns = sorted(MODELS)
    for m in (1, 2, 5):
        n = ns[k % 4]
        k += 1
        cases.append(LatticeCase("D1-M%d-N%d" % (m, n), n, (m, n), (R if m == 2 else I,)))
    for depth in (2, 3):
        for h in (1, 3, 4, 17):
            for m in (1, 2, 5):
                n = ns[k % 4]
                k += 1
                hidden = (h,) if depth == 2 else (3 if h != 3 else 4, h)
                acts = tuple(R if (i + k) % 2 else I for i in range(depth))
                cases.append(LatticeCase("D%d-H%d-M%d-N%d" % (depth, h, m, n), n, (m,) + hidden + (n,), acts))
    return cases


LATTICE = _lattice_cases()


@functools.lru_cache(maxsize=None)
def lattice_ints(case):
    """(wdec, Z) as int64: parameters in [-2, 2], the M x 9 points in [-3, 3]"""
    _, nd = decoder_table(case.widths, case.acts)
    rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(case.name)))   # (a seed that does not depend on the run)
    wdec = rng.integers(-2, 3, nd)
    z = rng.integers(-3, 4, (case.m, max(POINT_COUNTS)))
    wdec.setflags(write=False)
    z.setflags(write=False)
    return wdec, z


def lattice_decoder(case, dtype):
    """(table, wdec in `dtype`, Z float64 M x 9)"""
    table, _ = decoder_table(case.widths, case.acts)
    wdec, z = lattice_ints(case)
    return table, wdec.astype(dtype), np.asfortranarray(z.astype(np.float64))


def int_decode(table, wdec, z):
    """decoder(z) in int64 arithmetic (identity / relu only): z is (M,) or (M, C)"""
    a = np.asarray(z, dtype=np.int64)
    for fin, fout, act, w_off, b_off in table:
        w = np.asarray(wdec[w_off:w_off + fin * fout], dtype=np.int64).reshape((fout, fin), order="F")
        b = np.asarray(wdec[b_off:b_off + fout], dtype=np.int64)
        u = w @ a + (b if a.ndim == 1 else b[:, None])
        assert act in (I, R)
        a = np.maximum(u, 0) if act == R else u
    return a


def random_decoder(widths, acts, seed, dtype=np.float64, scale=0.4):
    """a decoder with random O(1) weights and biases: (table, wdec)"""
    table, nd = decoder_table(widths, acts)
    rng = np.random.default_rng(seed)
    wdec = np.empty(nd)
    for fin, fout, _, w_off, b_off in table:
        wdec[w_off:w_off + fin * fout] = scale * rng.standard_normal(fin * fout) / np.sqrt(fin) * 2.0
        wdec[b_off:b_off + fout] = scale * rng.standard_normal(fout)
    return table, wdec.astype(dtype)
