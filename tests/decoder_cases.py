"""Problems of the autoencoder route's tests (si_infer_set_decoder; subspaceinference_jl_amd/autoencoder.py is the definition) --
TEST INFRASTRUCTURE, no GPU needed.

MODELS are the target models: Dense chains with N in {7, 65, 129, 682} parameters -- odd N, N below and above one 64-row wave,
and the README toy -- on B <= 64 observations.

LATTICE is the exact case list: decoder weights, biases, z and W_swa are small integers and the activations identity or relu, so
that every product and every sum of `decode` / `weights` is an integer far below 2^53 and exact in fp64 (and every parameter is
exact in Float32 storage): the device must return the same bits whatever order it sums in.  tests/test_autoencoder_cpu.py proves the
premise on the CPU by recomputing every case in int64 (`int_decode`).

BIG_MODELS are three larger target models that are only ever set up, never evaluated: their N puts the last layer's reverse kernels
on every wave, on a second pass of the thread-strided loop and on a clipped and an empty row block, and its forward on a second
pass of the grid-stride loop.  REVERSE_LATTICE and FORWARD_BIG are the exact case lists of tests/test_gpu_decoder_reverse.py;
`int_decode_vjp` is the pull-back in int64, `reach` computes from the kernels' own constants (read out of the sources by
`kernel_constants`) which branches a case runs, and `emulate_vjp` / `emulate_decode` restate the kernels' decomposition in int64 with
one fault each (MUTANTS), so that tests/test_autoencoder_cpu.py can show on the CPU that the lists catch every one of them.
"""
import functools
import os
import re
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
    model: str = ""   # a key of BIG_MODELS in place of MODELS[n]
    salt: str = ""    # appended to the name for the seed (chosen on the CPU: see MUTANT_CAUGHT_BY)

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
    rng = np.random.default_rng(_name_seed(case.name + case.salt))   # (a seed that does not depend on the run)
    wdec = rng.integers(-2, 3, nd)
    z = rng.integers(-3, 4, (case.m, max(POINT_COUNTS)))
    wdec.setflags(write=False)
    z.setflags(write=False)
    return wdec, z


def _name_seed(name):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name))


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


# ---- the reverse kernels' case lists -------------------------------------------------------------------------------------------------
# name -> (dims, acts, B): target models that are set up and never evaluated (the exact tests call si_decode, si_reconstruct and
# si_decode_vjp only)
BIG_MODELS = {
    "N_2WAVE": ((100, 600, 15), (T, I), 4),        # N =    69 615: 68 rows per block, lanes across two waves
    "N_STRIDE": ((300, 800, 36), (T, I), 4),       # N =   269 636: 264 rows per block, all four waves and a second r += 256 pass
    "N_GRID": ((1024, 1024, 48), (T, I), 4),       # N = 1 098 800: 549 400 row pairs, above the forward's grid of 8 * 256 threads per CU
}


def big_n(name):
    dims, acts, _ = BIG_MODELS[name]
    return so.layer_table(list(dims), list(acts))[1]


@functools.lru_cache(maxsize=None)
def big_problem(name):
    """a BIG_MODELS target model with its data and an integer W_swa"""
    dims, acts, b = BIG_MODELS[name]
    table, n = so.layer_table(list(dims), list(acts))
    rng = np.random.default_rng(_name_seed(name))
    x = np.asfortranarray(rng.standard_normal((dims[0], b)))
    y = np.asfortranarray(rng.standard_normal((dims[-1], b)))
    w = rng.integers(-4, 5, n).astype(np.float64)
    for a in (x, y, w):
        a.setflags(write=False)
    return Problem(n, tuple(tuple(r) for r in table), x, y, w, 0.8)


def case_problem(case):
    """the (lattice) target model of a case of either table"""
    return big_problem(case.model) if case.model else problem(case.n, lattice=True)


def _last_layer_cases():
    n2, ns, ng = big_n("N_2WAVE"), big_n("N_STRIDE"), big_n("N_GRID")
    # N = 129, D = 2, M = 2: H in {1, 3} a partial round alone, 4 exactly one, 5 one and a tail, 8 exactly two, 9 two and a tail
    cases = [LatticeCase("R-H%d-N129" % h, 129, (2, h, 129), (R, I) if h % 2 else (I, R)) for h in (1, 3, 4, 5, 8, 9)]
    cases.append(LatticeCase("R-2WAVE-H5", n2, (3, 5, n2), (R, R), model="N_2WAVE"))
    cases.append(LatticeCase("R-STRIDE-H9", ns, (2, 9, ns), (R, I), model="N_STRIDE"))          # three h0 rounds
    cases.append(LatticeCase("R-GRID-H2", ng, (2, 2, ng), (I, R), model="N_GRID"))
    cases.append(LatticeCase("R-STRIDE-D1-M5", ns, (5, ns), (R,), model="N_STRIDE"))            # ga is gz: no head
    return cases


# head shapes: widths on both sides of the 256-thread stride and at DEC_MAXW, M above 256, the deepest decoder allowed
HEAD_CASES = [
    LatticeCase("W-257-255", 129, (257, 255, 129), (R, I)),
    LatticeCase("W-5-256", 129, (5, 256, 129), (I, R)),
    LatticeCase("W-2-257", 129, (2, 257, 129), (R, R)),
    LatticeCase("W-1024x3", 129, (1024, 1024, 1024, 129), (R, I, R)),
    LatticeCase("W-D8", 65, (2, 3, 4, 3, 4, 3, 4, 3, 65), (R, I, R, I, R, I, R, R)),
]
GRID_CASE = "R-GRID-H2"
REVERSE_LATTICE = LATTICE + _last_layer_cases() + HEAD_CASES
FORWARD_BIG = HEAD_CASES + [c for c in REVERSE_LATTICE if c.name == GRID_CASE]
FORWARD_BIG_POINTS = (1, 3)
REVERSE_BY_NAME = {c.name: c for c in REVERSE_LATTICE}


@functools.lru_cache(maxsize=None)
def lattice_cotangent(case):
    """gy as int64: N integers in [-2, 2]"""
    gy = np.random.default_rng(_name_seed(case.name + case.salt + "/gy")).integers(-2, 3, case.widths[-1])
    gy.setflags(write=False)
    return gy


def _int_layers(table, wdec):
    for fin, fout, act, w_off, b_off in table:
        assert act in (I, R)
        yield (np.asarray(wdec[w_off:w_off + fin * fout], dtype=np.int64).reshape((fout, fin), order="F"),
               np.asarray(wdec[b_off:b_off + fout], dtype=np.int64), act)


def int_forward(table, wdec, z):
    """every layer's output at ONE point in int64, a_1 first"""
    a, outs = np.asarray(z, dtype=np.int64).reshape(-1), []
    for w, b, act in _int_layers(table, wdec):
        u = w @ a + b
        a = np.maximum(u, 0) if act == R else u
        outs.append(a)
    return outs


def int_decode_vjp(table, wdec, z, gy):
    """J_decoder(z)' gy in int64 arithmetic (identity / relu only) at one point: per layer, from the last, W' (g .* mask)"""
    outs = int_forward(table, wdec, z)
    g = np.asarray(gy, dtype=np.int64).reshape(-1)
    for (w, _, act), a in reversed(list(zip(_int_layers(table, wdec), outs))):
        g = w.T @ (g * (a > 0) if act == R else g)
    return g


def relu_masks(table, wdec, z):
    """the relu layers' masks at one point, concatenated (empty without a relu layer)"""
    outs = int_forward(table, wdec, z)
    return np.concatenate([np.zeros(0, dtype=bool)] + [a > 0 for a, row in zip(outs, table) if row[2] == R])


def reverse_points(case):
    """three columns of the case's Z for the pull-back: column 0, the first column whose relu masks differ from column 0's
    (column 1 when there is none) and the first column left"""
    table, _ = decoder_table(case.widths, case.acts)
    wdec, z = lattice_ints(case)
    m0 = relu_masks(table, wdec, z[:, 0])
    other = next((c for c in range(1, z.shape[1]) if not np.array_equal(relu_masks(table, wdec, z[:, c]), m0)), 1)
    return (0, other, 1 if other != 1 else 2)


# ---- what a case reaches, from the kernels' own constants ----------------------------------------------------------------------------
@dataclass(frozen=True)
class KernelConstants:
    blocks: int       # DEC_REV_BLOCKS
    ht: int           # DEC_REV_HT
    maxw: int         # DEC_MAXW
    threads: int      # every kernel's workgroup, and the stride of every thread-strided loop
    wave: int         # lanes of a shuffle tree
    grid_per_cu: int  # the forward's grid cap in workgroups per CU
    max_layers: int   # SI_DEC_MAX_LAYERS
    chunk: int        # SI_DEC_CHUNK


@functools.lru_cache(maxsize=None)
def kernel_constants():
    """read out of csrc/kernels_decoder.hip, si_internal.h and capi_infer.hip: a retune changes these and fails the tests that
    assert what the case lists reach, not their premise"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "subspaceinference.jl_amd", "csrc")

    def read(name):
        with open(os.path.join(csrc, name)) as f:
            return f.read()

    def one(pattern, text):
        found = set(re.findall(pattern, text))
        assert len(found) == 1, (pattern, found)
        return int(found.pop())
    k, internal, capi = read("kernels_decoder.hip"), read("si_internal.h"), read("capi_infer.hip")
    threads = one(r"__launch_bounds__\((\d+)\)", k)
    assert one(r"\b[rijb] \+= (\d+)\)", k) == threads and one(r"dim3\((\d+)\), 0, st", k) == threads
    assert one(r"threadIdx\.x & (\d+)\) == 0", k) + 1 == one(r"__shfl_down\([^,]+, off, (\d+)\)", k) == 2 * one(r"int off = (\d+); off > 0", k)
    wave = one(r"__shfl_down\([^,]+, off, (\d+)\)", k)
    assert one(r"__shared__ double red\[(\d+)\]", k) == threads // wave
    return KernelConstants(blocks=one(r"constexpr int DEC_REV_BLOCKS = (\d+);", k), ht=one(r"constexpr int DEC_REV_HT = (\d+);", k),
                           maxw=one(r"constexpr int DEC_MAXW = (\d+);", k), threads=threads, wave=wave,
                           grid_per_cu=one(r"\(int64_t\)num_cu \* (\d+);", k), max_layers=one(r"constexpr int SI_DEC_MAX_LAYERS = (\d+);", internal),
                           chunk=one(r"constexpr int32_t SI_DEC_CHUNK = (\d+);", capi))


def rows_per_block(n, k):
    """decoder_last_rev_partial_kernel's `per`: ceil(N / blocks) rounded up to an even count"""
    return ((n + k.blocks - 1) // k.blocks + 1) // 2 * 2


def forward_passes(n, k, num_cu):
    """passes of the last layer forward's grid-stride loop in its busiest thread"""
    npair = (n + 1) // 2
    grid = max(1, min((npair + k.threads - 1) // k.threads, k.grid_per_cu * num_cu))
    return -(-npair // (grid * k.threads))


def reach(case, k):
    """which branches of the reverse kernels the case runs on non-zero terms"""
    n, h = case.widths[-1], case.widths[-2]
    per = rows_per_block(n, k)
    rows = min(per, n)                                   # block 0's rows
    return dict(per=per, waves=min(-(-rows // k.wave), k.threads // k.wave), passes=-(-rows // k.threads),
                blocks_with_rows=-(-n // per), clipped=n % per != 0, empty=k.blocks - -(-n // per),
                rounds=-(-h // k.ht), tail=h % k.ht, head=case.widths[1:-1], m=case.m, depth=case.depth)


# ---- the kernels' decomposition restated in int64, with one fault each ---------------------------------------------------------------
MUTANTS = ("lanes_from_64_dropped", "rows_from_r0_plus_256_dropped", "last_h0_round_dropped", "tail_columns_dropped",
           "stale_wave_sums", "head_outputs_from_256_dropped", "head_inputs_from_256_dropped", "block_partials_from_256_dropped",
           "pairs_beyond_the_grid_dropped", "relu_mask_of_the_wrong_layer")
FORWARD_MUTANTS = ("head_outputs_from_256_dropped", "pairs_beyond_the_grid_dropped")
MI355X_CUS = 256


def emulate_decode(table, wdec, z, k, mutant=None, num_cu=MI355X_CUS):
    """decoder(z) at one point as the two forward kernels split it; a dropped element reads 0"""
    outs = int_forward(table, wdec, z)
    if mutant == "head_outputs_from_256_dropped":       # (the fault feeds the layers behind it)
        a = np.asarray(z, dtype=np.int64).reshape(-1)
        for l, (w, b, act) in enumerate(_int_layers(table, wdec)):
            u = w @ a + b
            a = np.maximum(u, 0) if act == R else u
            if l < len(table) - 1:
                a[k.threads:] = 0
        return a
    y = outs[-1].copy()
    if mutant == "pairs_beyond_the_grid_dropped":
        y[2 * k.grid_per_cu * num_cu * k.threads:] = 0
    return y


def emulate_vjp(table, wdec, z, gy, k, mutant=None):
    """J' gy at one point as the three reverse kernels split it: row blocks of `per`, lanes, waves and passes of the thread-strided
    loop, h0 rounds of `ht` columns, the final kernel's stride over the block partials, then the head layer by layer"""
    outs = int_forward(table, wdec, z)
    layers = list(_int_layers(table, wdec))
    wd, _, act = layers[-1]
    n, h = wd.shape
    gv = np.asarray(gy, dtype=np.int64).reshape(-1) * (outs[-1] > 0 if act == R else 1)
    per = rows_per_block(n, k)
    r = np.arange(n)
    loc, blk = r % per, r // per                          # r - r0 and blockIdx.x
    keep = np.ones(n, dtype=bool)
    if mutant == "lanes_from_64_dropped":
        keep = loc % k.threads < k.wave
    elif mutant == "rows_from_r0_plus_256_dropped":
        keep = loc < k.threads
    elif mutant == "block_partials_from_256_dropped":
        keep = blk < k.threads
    ga = wd[keep].T @ gv[keep]
    rounds, tail = -(-h // k.ht), h % k.ht
    if mutant == "last_h0_round_dropped":
        ga[(rounds - 1) * k.ht:] = 0
    elif mutant == "tail_columns_dropped" and tail:
        ga[h - tail:] = 0
    elif mutant == "stale_wave_sums":                     # round k > 0: wave 0's sum of its own columns, waves 1..3's of round k - 1
        w0 = loc % k.threads < k.wave
        for col in range(k.ht, h):
            ga[col] = wd[w0, col] @ gv[w0] + wd[~w0, col - k.ht] @ gv[~w0]
    g = ga
    hid = np.concatenate([np.zeros(0, dtype=np.int64)] + outs[:-1])
    offs = np.concatenate([[0], np.cumsum([a.size for a in outs[:-1]])]).astype(int)
    for l in range(len(layers) - 2, -1, -1):
        w, _, act = layers[l]
        a = outs[l]
        if mutant == "relu_mask_of_the_wrong_layer" and len(layers) > 2:      # the neighbouring head layer's rows of `hid`
            a = hid[(offs[l - 1 if l > 0 else l + 1] + np.arange(a.size)) % hid.size]
        delta = g * (a > 0) if act == R else g.copy()
        if mutant == "head_outputs_from_256_dropped":
            delta[k.threads:] = 0
        g = w.T @ delta
        if mutant == "head_inputs_from_256_dropped":
            g[k.threads:] = 0
    return g
