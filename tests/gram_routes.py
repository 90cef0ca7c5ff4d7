"""Which kernel instantiation the construction front end reaches -- the snapshot push K1 (csrc/kernels_stream.hip) and the Gram
matrix K2, G = A'A (csrc/kernels_gram.hip, csrc/kernels_gram_wave.hip) -- restated in plain Python, the list of instantiations
the shipped library can reach, and the lattice cases of tests/test_gpu_gram_exact.py, each there for the instantiations written
next to it (a helper module for the tests, not a conftest; the construction twin of tests/dense_routes.py).

Rules restated (function here <- function there):
  wave_blocks_per_cu <- gram_wave_blocks_per_cu;  wave_inst <- launch_gram_wave_part0/1/2 (the KS / KS2 template arguments of
  every tile count), launch_nt (the ragged rule K - 16 (NT - 1) <= 4) and launch_nt_q (KS2 with two workgroups per CU and a ring
  of two, else KS with one and as many ring buffers as 150 KB hold, four at the most);
  plan <- launch_gram (wave_path, npan, nb_diag, nb_off, nb_wave, the workspace `need`);
  panel_launches <- gram_panels with gram_diag_dispatch / gram_off_dispatch;
  stream_grid <- stream_grid;  push_inst <- launch_swa_dev_push_t (aligned);  push_batch_inst <- launch_swa_dev_push_batch_t (vec).
tests/test_gram_exact_cpu.py holds the restatement to the C++ text it mirrors and proves that the union of the routes of CASES
equals REACHABLE.  A kernel name is written as the kernel trace prints it, up to its argument list:
"gram_glds_kernel<7, 2, 2, 2, 1>" is "void si::gram_glds_kernel<7, 2, 2, 2, 1>(double const*, long, long, int, double*)" of
profiles/gram_exact_kernel_names.txt.

Only what the shipped library can reach counts as reachable.  The development build's knobs (SI_GRAM_PANELS, SI_GRAM_SPEC,
SI_GRAM_OCC1, SI_GW_KNOB: compiled in under SI_DEV_KNOBS only) select gram_spec_kernel, the one-workgroup-per-CU forms of
NT <= 9 and the panel kernels at K <= 208 in fp64; none of those is in the table and no test sets a knob.

Not in the table, held there: the refine and wide finish routes call launch_gram on other buffers -- si_construct_refine on
d_B (G2 = B'B, K x K), finish_wide on the transposed copy d_At (A A', N x N, with N in the role of K), both in csrc/capi.hip.
tests/test_gpu_finish_exact.py holds them (lattice.FINISH_REFINE, lattice.FINISH_WIDE).

Pointer alignment: every device buffer of the context is an allocation of its own (256-byte aligned base) and a column of A
starts at slot * pad_ld(N) elements, pad_ld(N) a multiple of 64: the mean and the columns of A are always 16-byte aligned.
The one pointer a caller controls is the snapshot's, through si_construct_push_dev / si_construct_push_batch_dev: a host
push stages the snapshot in a buffer of the library's own and is always `aligned`."""
import collections
import functools

import numpy as np

from oracle import subspace_oracle as so
from tests import lattice as lat

NUM_CU = 256   # MI355X
SI_F32, SI_F64 = 0, 1
GR = 32        # slab rows of every Gram kernel (GR, GR2)
GR2_Y = 16     # stage-1 workgroups per tile pair of the wave path's reduction
LD_ALIGN = 64
WAVE_MAX_NT = 13


def pad_ld(n):
    return (n + LD_ALIGN - 1) // LD_ALIGN * LD_ALIGN


def _ty(dtype):
    return "float" if dtype == SI_F32 else "double"


def _b(v):
    return "true" if v else "false"


# ---------------------------------------------------------------------------------------------- K2, the wave path (K <= 208, fp64)
# NT -> (KS, KS2) as launch_gram_wave_part0/1/2 instantiate launch_nt<NT, KS, KS2>; KS2 = 0: no two-per-CU form
WAVE_KS = {1: (4, 2), 2: (4, 2), 3: (4, 2), 4: (4, 2), 5: (4, 2), 6: (4, 2), 7: (4, 2), 8: (2, 2), 9: (2, 1), 10: (2, 0), 11: (1, 0),
           12: (1, 0), 13: (1, 0)}


def wave_blocks_per_cu(nt):   # <- gram_wave_blocks_per_cu (gram_two_per_cu() is true in the shipped build)
    return 2 if nt <= 9 else 1


def wave_inst(k):   # <- launch_nt, launch_nt_q: (NT, KS, NB, OCC, NQ) of gram_glds_kernel
    nt = (k + 15) // 16
    assert 1 <= nt <= WAVE_MAX_NT
    ks, ks2 = WAVE_KS[nt]
    nq = 1 if k - 16 * (nt - 1) <= 4 else 4
    if ks2 > 0:
        return nt, ks2, 2, 2, nq
    per = (150 * 1024) // (nt * 16 * GR * 8)
    nb = 4 if per >= 4 else 3 if per >= 3 else 2
    return nt, ks, nb, 1, nq


def k_wave(k):
    return "gram_glds_kernel<%d, %d, %d, %d, %d>" % wave_inst(k)


def k_small(nt, dtype):
    return "gram_small_kernel<%d, %s>" % (nt, _ty(dtype))


def k_off(ntj, dtype):
    return "gram_off_kernel<%d, %s>" % (ntj, _ty(dtype))


WAVE_REDUCE = ["gram_reduce_stage1_kernel", "gram_reduce_stage2_kernel"]
PANEL_REDUCE = ["gram_small_reduce_kernel", "gram_off_reduce_kernel"]

Plan = collections.namedtuple("Plan", "wave_path npan ntw nb_diag nb_off nb_wave need")


def plan(n, k, storage=SI_F64, num_cu=NUM_CU):   # <- launch_gram
    nslab = (n + GR - 1) // GR
    nb_diag = min(num_cu * 2, nslab)
    nb_off = min(num_cu * 2, nslab)
    npan = (k + 127) // 128
    ntw = (k + 15) // 16
    wave_path = ntw <= 13 and storage != SI_F32
    nb_wave = min(num_cu * wave_blocks_per_cu(ntw), nslab)
    if wave_path:
        need = (nb_wave + GR2_Y) * (ntw * (ntw + 1) // 2) * 256 * 8
    else:
        need = max(nb_diag * 36, nb_off * 64 if npan > 1 else 0) * 256 * 8
    return Plan(wave_path, npan, ntw, nb_diag, nb_off, nb_wave, need)


def panel_launches(k, storage):   # <- gram_panels: [(kernel, col0 | (ci0, cj0), tiles)] in launch order
    out = []
    npan = (k + 127) // 128
    for i in range(npan):
        ci0 = i * 128
        nti = (min(k, ci0 + 128) - ci0 + 15) // 16
        out.append((k_small(nti, storage), (ci0, ci0), nti))
        for j in range(i + 1, npan):
            cj0 = j * 128
            ntj = (min(k, cj0 + 128) - cj0 + 15) // 16
            out.append((k_off(ntj, storage), (ci0, cj0), ntj))
    return out


def gram_routes(n, k, storage=SI_F64, num_cu=NUM_CU):
    """the kernels of one si_construct_gram, in launch order (reduce kernels included)"""
    p = plan(n, k, storage, num_cu)
    if p.wave_path:
        return [k_wave(k)] + WAVE_REDUCE
    out = []
    for name, (ci0, cj0), _ in panel_launches(k, storage):
        out += [name, PANEL_REDUCE[0] if ci0 == cj0 else PANEL_REDUCE[1]]
    return out


def gram_launches(n, k, storage=SI_F64, num_cu=NUM_CU):
    """launches booked on the "gram" class of si_get_stats by one si_construct_gram"""
    p = plan(n, k, storage, num_cu)
    return 1 if p.wave_path else p.npan * (p.npan + 1) // 2


def gram_grid(n, k, storage=SI_F64, num_cu=NUM_CU):
    """workgroups of the partial-tile kernel(s) (the diagonal and the off-diagonal panel kernels start the same number)"""
    p = plan(n, k, storage, num_cu)
    assert p.nb_diag == p.nb_off
    return p.nb_wave if p.wave_path else p.nb_diag


def slabs_per_block(n, k, storage=SI_F64, num_cu=NUM_CU):
    """(min, max) 32-row slabs a workgroup runs: workgroup b takes slabs b, b + grid, ..."""
    nslab, nb = (n + GR - 1) // GR, gram_grid(n, k, storage, num_cu)
    return nslab // nb, (nslab + nb - 1) // nb


def ring_depth(k, storage=SI_F64):
    """NB of the wave path's LDS ring; the panel kernels stage one slab ahead in registers (counted as 2)"""
    return wave_inst(k)[2] if plan(1, k, storage).wave_path else 2


def k_split(k, storage=SI_F64):
    """KS: the residue classes the 8 k steps of a slab are dealt to (1 on the panel kernels)"""
    return wave_inst(k)[1] if plan(1, k, storage).wave_path else 1


# ---------------------------------------------------------------------------------------------- K1
def stream_grid(work_items, num_cu=NUM_CU):   # <- stream_grid
    return max(1, min((work_items + 255) // 256, num_cu * 8))


def push_inst(wdtype, aligned, storage):   # <- launch_swa_dev_push_t / launch_swa_dev_push
    return "swa_dev_push_kernel<%s, %s, %s>" % (_ty(wdtype), _b(aligned), _ty(storage))


def push_batch_inst(wdtype, vec, storage):   # <- launch_swa_dev_push_batch_t / launch_swa_dev_push_batch
    return "swa_dev_push_batch_kernel<%s, %s, %s>" % (_ty(wdtype), _b(vec), _ty(storage))


def push_aligned(byte_offset):   # the snapshot pointer = a 256-byte aligned base + byte_offset
    return byte_offset % 16 == 0


def push_batch_vec(n, ld, wdtype, byte_offset):
    esz = 4 if wdtype == SI_F32 else 8
    return ld % 2 == 0 and ld >= n + (n & 1) and byte_offset % (2 * esz) == 0


def push_passes(kind, n, num_cu=NUM_CU):
    """passes of the grid-stride loop of the busiest thread: single pushes work on quads, the batch kernel on pairs"""
    items = n >> 2 if kind == "single" else (n + 1) >> 1
    threads = stream_grid(items, num_cu) * 256
    return (items + threads - 1) // threads


def push_routes(kind, n, wdtype, storage, offset=0, ld=None):
    """the kernel a device push of `kind` ("single" | "batch") launches; offset in ELEMENTS of the snapshot type from an aligned base"""
    esz = 4 if wdtype == SI_F32 else 8
    if kind == "single":
        return [push_inst(wdtype, push_aligned(offset * esz), storage)]
    return [push_batch_inst(wdtype, push_batch_vec(n, n if ld is None else ld, wdtype, offset * esz), storage)]


# ---------------------------------------------------------------------------------------------- what shapes can reach
REACHABLE_WAVE = sorted({k_wave(k) for k in range(1, 16 * WAVE_MAX_NT + 1)})
REACHABLE_PANEL = sorted(f(nt, dt) for f in (k_small, k_off) for nt in range(1, 9) for dt in (SI_F32, SI_F64))
REACHABLE_PUSH = sorted([push_inst(w, a, s) for w in (SI_F32, SI_F64) for a in (False, True) for s in (SI_F32, SI_F64)] +
                        [push_batch_inst(w, v, s) for w in (SI_F32, SI_F64) for v in (False, True) for s in (SI_F32, SI_F64)])
REACHABLE = sorted(REACHABLE_WAVE + REACHABLE_PANEL + WAVE_REDUCE + PANEL_REDUCE + REACHABLE_PUSH)

# ---------------------------------------------------------------------------------------------- the cases
# A Gram case names its N by CLASS: the row count follows the grid of the case's route, so the class means the same on a device
# with another CU count (the GPU test feeds the device's own count to gram_n).  nb = gram_grid, NB = ring_depth:
#   "one"    N = 1 (one column tile) or 31: one partial slab, one workgroup.  (A one-row A of more than a few columns has a zero
#            column whatever the seed -- consecutive means agree in one entry of nine -- so N = 1 stays with K <= 16)
#   "slab"   N = 4097: 129 slabs, the last of one row; one slab per workgroup wherever the grid allows 129 workgroups
#   "two"    N = 32 nb + 32 * 7 + 5: eight workgroups run two slabs, the others one; a ragged last slab of 5 rows
#   "wrap"   N = 32 nb (NB + 1) + 32 * 3 + 9: every workgroup runs more slabs than the ring holds (the ring wraps), four of them
#            one more than the rest; a ragged last slab of 9 rows
# and the panel cases: "p33" N = 33, "slab", "pmany" N = 32 * 2 num_cu + 32 * 5 + 7 (some panel workgroups run two slabs).
GramCase = collections.namedtuple("GramCase", "name k storage nclass targets")
PushCase = collections.namedtuple("PushCase", "name kind wdtype offset storage nclass ld_extra count targets")

N_CLASSES_WAVE = ("one", "slab", "two", "wrap")
N_CLASSES_PANEL = ("p33", "slab", "pmany")


def gram_n(case, num_cu=NUM_CU):
    k, storage, c = case.k, case.storage, case.nclass
    if c == "one":
        return 1 if k <= 16 else 31
    if c == "p33":
        return 33
    if c == "slab":
        return 4097
    if c == "pmany":
        return GR * 2 * num_cu + GR * 5 + 7
    nb = gram_grid(1 << 40, k, storage, num_cu)   # the grid of a long A: num_cu * workgroups per CU
    if c == "two":
        return GR * nb + GR * 7 + 5
    assert c == "wrap"
    return GR * nb * (ring_depth(k, storage) + 1) + GR * 3 + 9


RAGGED_WIDTHS = (1, 2, 3, 4)      # NQ = 1
PLAIN_WIDTHS = (16, 5, 15, 9)     # NQ = 4


def _wave_cases():
    out = []
    for nt in range(1, WAVE_MAX_NT + 1):
        for nq, widths in ((1, RAGGED_WIDTHS), (4, PLAIN_WIDTHS)):
            for ci, c in enumerate(N_CLASSES_WAVE):
                # every tile count sees all four widths of its variant, one per N class
                k = 16 * (nt - 1) + widths[(nt + ci) % 4]
                assert wave_inst(k)[0] == nt and wave_inst(k)[4] == nq
                out.append(GramCase("wave_nt%d_nq%d_%s_k%d" % (nt, nq, c, k), k, SI_F64, c, (k_wave(k),) + tuple(WAVE_REDUCE)))
    return out


# fp64 panels (K > 208): two panels with a second panel of 6, 7, 8 tiles (209: a last tile of one column), three panels with a
# last panel of 1 .. 5 tiles (257, 287, 319: ragged last tiles of 1, 15 and 15 columns)
PANEL_K_F64 = (209, 224, 240, 256, 257, 287, 304, 319, 336)
# fp32 storage: one panel of NT tiles at K = 16 NT - r, two panels with a second of NTJ tiles at K = 128 + 16 NTJ - r
_R = (15, 0, 3, 0, 7, 0, 11, 0)
PANEL_K_F32 = tuple(16 * nt - _R[nt - 1] for nt in range(1, 9)) + tuple(128 + 16 * nt - _R[(nt + 2) % 8] for nt in range(1, 9))


def _panel_cases():
    out = []
    for storage, ks in ((SI_F64, PANEL_K_F64), (SI_F32, PANEL_K_F32)):
        for k in ks:
            names = tuple(dict.fromkeys(name for name, _, _ in panel_launches(k, storage)))
            red = tuple(PANEL_REDUCE[:1 if k <= 128 else 2])
            for c in N_CLASSES_PANEL:
                out.append(GramCase("panel_%s_k%d_%s" % (_ty(storage), k, c), k, storage, c, names + red))
    return out


GRAM_CASES = _wave_cases() + _panel_cases()


def _push_cases():
    out = []
    for wd in (SI_F32, SI_F64):
        for st in (SI_F64, SI_F32):
            for off in (0, 1):
                t = (push_inst(wd, off == 0, st),)
                for n in (4100, 4097, 4098, 4099):      # N % 4 = 0, 1, 2, 3
                    out.append(PushCase("push_%s_%s_off%d_n%d" % (_ty(wd), _ty(st), off, n), "single", wd, off, st, n, 0, 3, t))
            # (N, ld - N, offset): vec needs ld even, ld >= N + (N & 1) and a pointer aligned to two elements
            for n, ldx, off in ((1000, 0, 0), (1001, 1, 0), (1001, 3, 0), (1001, 0, 0), (1000, 1, 0), (1000, 0, 1), (1001, 1, 1)):
                vec = push_batch_vec(n, n + ldx, wd, off * (4 if wd == SI_F32 else 8))
                out.append(PushCase("batch_%s_%s_n%d_ld%d_off%d" % (_ty(wd), _ty(st), n, n + ldx, off), "batch", wd, off, st, n, ldx, 5,
                                    (push_batch_inst(wd, vec, st),)))
    # tail only (no quad), and the grid-stride loops' second pass (three columns each)
    out.append(PushCase("push_double_double_off0_n3", "single", SI_F64, 0, SI_F64, 3, 0, 3, (push_inst(SI_F64, True, SI_F64),)))
    out.append(PushCase("push_double_double_off1_wrap", "single", SI_F64, 1, SI_F64, "wrap", 0, 3, (push_inst(SI_F64, False, SI_F64),)))
    out.append(PushCase("batch_float_float_wrap", "batch", SI_F32, 0, SI_F32, "wrap", 1, 3, (push_batch_inst(SI_F32, True, SI_F32),)))
    return out


def push_n(case, num_cu=NUM_CU):
    """N of a push case; "wrap": just past what one pass of the full grid covers (num_cu * 8 * 256 threads x 4 | 2 elements), odd"""
    if case.nclass != "wrap":
        return case.nclass
    per = 4 if case.kind == "single" else 2
    return num_cu * 8 * 256 * per + per * 256 * 3 + (3 if case.kind == "single" else 1)


PUSH_CASES = _push_cases()
CASES = GRAM_CASES + PUSH_CASES


def case_routes(case, num_cu=NUM_CU):
    if isinstance(case, GramCase):
        return gram_routes(gram_n(case, num_cu), case.k, case.storage, num_cu)
    n = push_n(case, num_cu)
    return push_routes(case.kind, n, case.wdtype, case.storage, case.offset, n + case.ld_extra)


# ---------------------------------------------------------------------------------------------- the lattice problems
def epoch_counters(k):
    """n_j >= 1: no deviation column n_j (m_j - m_{j-1}) is zero by construction (n_0 = 0 would zero column 0)"""
    return [1 + j // 3 for j in range(k)]


def blocks_nonzero(a):
    """no 4-row x 4-column block of A (aligned to 4; ragged ones at the edges included) is all zero"""
    n, k = a.shape
    nz = np.zeros(((n + 3) // 4 * 4, (k + 3) // 4 * 4), dtype=bool)
    nz[:n, :k] = a != 0
    return bool(nz.reshape(nz.shape[0] // 4, 4, nz.shape[1] // 4, 4).any(axis=(1, 3)).all())


def lattice_snapshots(n, k, seed0, dtype=np.float64):
    """lat.snapshots with n_j >= 1, the first seed of seed0, seed0 + 1000, ... whose A has no zero column and no all-zero 4 x 4
    block (a one-row A has a zero entry in one place of nine).  Returns (snaps, ns, means, A)."""
    for t in range(256):
        snaps, ns, means, a = lat.snapshots(n, k, seed=seed0 + 1000 * t, ns=epoch_counters(k), dtype=dtype)
        if blocks_nonzero(a) and not np.any(np.all(a == 0, axis=0)):
            return snaps, ns, means, a
    raise AssertionError("no seed gives a block-dense A at %d x %d" % (n, k))


@functools.lru_cache(maxsize=2)
def gram_problem(n, k):
    """(snapshots, epoch counters, A, exact A'A) of an n x k case.  The snapshots are below 2^24 and A's entries are integers
    below 2^24, so fp32 snapshots and fp32 storage give the same A"""
    snaps, ns, _, a = lattice_snapshots(n, k, seed0=n + 7 * k)
    assert max(float(np.max(np.abs(s))) for s in snaps) < lat.F32_LIMIT and float(np.max(np.abs(a))) < lat.F32_LIMIT
    return snaps, ns, a, lat.gram_exact_certified(a)


PUSH_NS = (1.0, 1.0, 2.0, 2.0, 3.0)   # the epoch counter, repeated per batch


def push_problem(case, num_cu=NUM_CU):
    """(snapshots in the case's type, epoch counters, W_swa, A) -- W_swa and A from the oracle's three rounded operations per push.
    fp64 storage: random data (every operation rounds).  fp32 storage: lattice snapshots, whose deviations are integers, so the
    rounding of A to fp32 is exact and the fp64 oracle stays the reference bit for bit."""
    n = push_n(case, num_cu)
    dt = np.float32 if case.wdtype == SI_F32 else np.float64
    ns = list(PUSH_NS[:case.count])
    if case.storage == SI_F32:
        snaps, ns, _, _ = lat.snapshots(n, case.count, seed=n + case.count, ns=[int(v) for v in ns], dtype=dt)
    else:
        rng = np.random.default_rng(n + 31 * case.count)
        w0 = rng.standard_normal(n)
        snaps = [(w0 + c).astype(dt) for c in np.cumsum(0.01 * rng.standard_normal((case.count, n)), axis=0)]
    w_ref, a_ref = so.construct_stream(snaps, ns)
    return snaps, ns, w_ref, a_ref


def gpu_order(cases, num_cu=NUM_CU):
    """large and small N x K alternate: the largest, the smallest, the second largest, ..."""
    def size(c):
        return (gram_n(c, num_cu) if isinstance(c, GramCase) else push_n(c, num_cu)) * (c.k if isinstance(c, GramCase) else c.count)
    s = sorted(cases, key=lambda c: (size(c), c.name))
    out = []
    while s:
        out.append(s.pop())
        if s:
            out.append(s.pop(0))
    return out
