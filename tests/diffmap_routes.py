"""Which kernel instantiation a diffusion finish (si_construct_finish_diffmap, csrc/capi_diffmap.hip) reaches: its block sizes and
the shape rules of the projection and Gram launchers it calls, restated in plain Python, the list of instantiations reachable at
N <= 300, and the cases of tests/test_gpu_diffmap_exact.py, whose routes together are that list (a helper module for the tests,
not a conftest; the diffusion twin of tests/dense_routes.py and tests/gram_routes.py).

Rules restated (function here <- function there):
  block_sizes <- si_construct_finish_diffmap (b, n2, Kp, nb, Npad, Mpad_b, Mpad_m);  project_mpad <- project_mpad (kernels_gram.hip);
  valu_kernels <- project_valu;  stream_kernels <- launch_project_stream with launch_project_nt (kernels_project.hip);
  mfma_kernels <- launch_project_mfma's panel loop with the `vec` rule of launch_gemm (kernels_bwd.hip);
  project_kernels <- launch_project (fp64 A);  project_calls <- the four launch_project calls of si_construct_finish_diffmap;
  gram_kernels <- launch_gram at (N, n2), through gram_routes.gram_routes (held to its text by tests/test_gram_exact_cpu.py);
  front_kernels <- launch_dm_rescale and steps 1-3 of si_construct_finish_diffmap.
tests/test_diffmap_routes_cpu.py holds the restatement to the C++ text it mirrors, proves that REACHABLE is what the shapes
N <= 300 reach and that the union of the routes of CASES equals it, and asserts the separation condition of every case.  A kernel
name is written as the kernel trace prints it, up to its argument list: "project_glds_kernel<5, 2, 2>" is
"void si::project_glds_kernel<5, 2, 2>(double const*, long, ..." of profiles/diffmap_exact_kernel_names.txt.

Pointer alignment (the `vec` rule): Kn, both blocks Z, R, the coefficient buffer and V' are allocations of their own (256-byte
aligned), ldn = pad_ld(N) is a multiple of 64, the second half of a block starts b * ldn elements in, a panel of the right factor
64 elements in and Mpad is a multiple of 8: every pointer and leading dimension passes, and `vec` reduces to N even and the
panel's width even.

A finish that converges after two or more iterations runs every launch below at least once (one that converges in its first
never forms a next block: see routes); the routes do not depend on K or on the data (K enters the front end's loop bounds only,
the storage type its two template arguments)."""
import functools

import numpy as np

from tests import gram_routes as gr

N_MAX = 300
LD_ALIGN = 64


def pad_ld(n):
    return (n + LD_ALIGN - 1) // LD_ALIGN * LD_ALIGN


def project_mpad(m):   # <- project_mpad
    m0 = 0
    while m0 < m:
        rem = m - m0
        m0 += 32 if rem > 24 else 24 if rem > 16 else 16 if rem > 8 else 8
    return m0


def block_sizes(n, k, m):   # <- si_construct_finish_diffmap
    b = min(n - 1, 2 * m + 16)
    nb = (n + 63) // 64
    return dict(b=b, n2=2 * b, Kp=(k + 3) // 4 * 4, nb=nb, Npad=nb * 64, ldn=pad_ld(n), ldt=pad_ld(b), Mpad_b=project_mpad(b),
                Mpad_m=project_mpad(m), tiles=nb * (nb + 1) // 2)


def valu_kernels(m):   # <- project_valu
    out, m0 = [], 0
    while m0 < m:
        rem = m - m0
        mt = 32 if rem > 24 else 24 if rem > 16 else 16 if rem > 8 else 8
        out.append("project_kernel<%d, double>" % mt)
        m0 += mt
    return out


def stream_kernels(k, m):   # <- launch_project_stream / launch_project_nt (two workgroups per CU, a ring of two); None: not covered
    if k > 128 or k <= 0:
        return None
    return ["project_glds_kernel<%d, 2, 2>" % min((k + 15) // 16, 8) for _ in range(0, m, 64)]


def mfma_kernels(n, m):   # <- launch_project_mfma + `vec` of launch_gemm (Mrows = N, Ncols = the panel's width)
    out = []
    for m0 in range(0, m, 64):
        mc = min(m - m0, 64)
        out.append("gemm_f64_kernel<128, 64, 2, 4, 4, 0, 0, %s, 2>" % ("true" if n % 2 == 0 and mc % 2 == 0 else "false"))
    return out


def project_kernels(n, k, m):   # <- launch_project, a_dtype = SI_F64, N < 2^31
    if m > 32:
        s = stream_kernels(k, m)
        return s if s is not None else mfma_kernels(n, m)
    return valu_kernels(m)


def project_calls(n, m):   # <- si_construct_finish_diffmap: (what, K, M, Mpad) of its four launch_project calls
    s = block_sizes(n, 1, m)
    return [("Kn V'", n, s["b"], s["ldt"]), ("next block", s["n2"], s["b"], s["Mpad_b"]), ("residuals", s["n2"], m, s["Mpad_m"]),
            ("vectors", s["b"], m, s["Mpad_m"])]


def gram_kernels(n, m):   # <- launch_gram(st, Z, ldn, N, n2, ...): the stacked block is fp64
    return gr.gram_routes(n, block_sizes(n, 1, m)["n2"], gr.SI_F64)


def front_kernels(rescale=True, f32=False):   # <- launch_dm_rescale, steps 1-3 and the iteration's streaming kernels
    ty = "float" if f32 else "double"
    return (["dm_minmax_kernel<%s>" % ty] if rescale else []) + [
        "dm_rescale_kernel<%s>" % ty, "dm_pairwise_kernel", "dm_sum_parts_kernel", "dm_scale_rows_kernel", "dm_unit_kernel",
        "dm_deflate_kernel", "transpose_kernel<double>", "dm_colnorm_kernel", "dm_finish_kernel"]


def routes(n, k, m, rescale=True, f32=False, next_block=True):
    """the set of kernel instantiations of one converged si_construct_finish_diffmap.  next_block = False: the finish that
    converges in its first iteration and never forms a second block -- with b = N - 1 the start block already spans the whole
    complement of u_1 and most such finishes do (measured: 1 or 2 iterations); with b < N - 1 a random block holds no
    eigenvector and there are always at least two (the GPU test asserts it)."""
    assert n >= 3 and 1 <= m <= n - 2 and k >= 1
    s = set(front_kernels(rescale, f32)) | set(gram_kernels(n, m))
    for what, kk, mm, _ in project_calls(n, m):
        if next_block or what != "next block":
            s |= set(project_kernels(n, kk, mm))
    return s


# ---------------------------------------------------------------------------------------------- what shapes N <= 300 can reach
# b = 2 (N = 3) .. 299, n2 = 4 .. 598: every wave instantiation of an even K <= 208 and both panel families with 1 .. 8 tiles;
# the slab stream needs M > 32, so K >= 33 in every one of the four calls: NT = 3 .. 8
REACHABLE = sorted(
    set(front_kernels(True, False)) | set(front_kernels(True, True))
    | {"project_kernel<%d, double>" % mt for mt in (8, 16, 24, 32)}
    | {"project_glds_kernel<%d, 2, 2>" % nt for nt in range(3, 9)}
    | {"gemm_f64_kernel<128, 64, 2, 4, 4, 0, 0, %s, 2>" % v for v in ("true", "false")}
    | {gr.k_wave(n2) for n2 in range(4, 209, 2)} | set(gr.WAVE_REDUCE)
    | {f(nt, gr.SI_F64) for f in (gr.k_small, gr.k_off) for nt in range(1, 9)} | set(gr.PANEL_REDUCE))


# ---------------------------------------------------------------------------------------------- the cases
TOL = 1e-12
GAP_MIN = 1e-3


@functools.lru_cache(maxsize=None)
def uniform(n, k, seed):
    a = np.asfortranarray(np.random.default_rng(seed).random((n, k)))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def uniform32(n, k, seed):
    """the same, representable in fp32: for the case with fp32 storage of A"""
    a = np.asfortranarray(uniform(n, k, seed).astype(np.float32).astype(np.float64))
    a.setflags(write=False)
    return a


GENERATORS = {"uniform": uniform, "uniform32": uniform32}


def exempt(n, m, sign):
    """the cases that may do without the vector comparison: the block spans the whole complement of u_1 and M is at its bound
    (all but one eigenvalue lead: the last gap is never wide), or kernel_sign = +1 at M >= 24"""
    return m == n - 2 or (sign == 1 and m >= 24)


# (N, K, M, kernel_sign, eps, (generator, seed)).  The seeds were chosen on the CPU from the dense spectrum alone, so that every
# case that is not exempt has spectrum_gap >= GAP_MIN (tests/test_diffmap_routes_cpu.py asserts it).  "free": the case keeps only
# the reference-free checks and the eigenvalues.
U0, U1, U4 = ("uniform", 0), ("uniform", 1), ("uniform", 4)
CASES = [
    # ---- b = N - 1: the block spans the whole complement of u_1
    (3, 2, 1, -1, 0.25, U0),       # free (M = N - 2).  The smallest legal N: b = 2, K2 at n2 = 4
    (5, 3, 3, -1, 0.25, U0),       # free (M = N - 2)
    (12, 5, 10, -1, 0.25, U0),     # free (M = N - 2): M at its bound
    (17, 4, 2, -1, 0.25, U1),
    (17, 4, 2, 1, 0.25, U0),
    (10, 4, 2, -1, 0.25, U0),      # n2 = 18: two column tiles, the second two columns wide
    (11, 4, 3, 1, 0.25, U0),
    (16, 4, 2, -1, 0.25, ("uniform32", 0)),   # fp32 storage of A: dm_minmax_kernel<float>, dm_rescale_kernel<float>
    # ---- b = 32 | 34, either side of the switch to the matrix-core kernels, at N <= 128 and beyond
    (64, 6, 8, -1, 0.25, U1),
    (64, 6, 8, 1, 0.25, U0),
    (64, 6, 9, -1, 0.25, U1),      # the slab stream with K = N = 64 and K = n2 = 68
    (200, 8, 8, -1, 0.25, U0),
    (200, 8, 9, -1, 0.25, U0),     # N > 128: Kn V' on gemm_f64_kernel<128, 64>, the next block on the slab stream
    (200, 8, 9, 1, 0.25, U1),
    # ---- 32 < b <= 64
    (40, 5, 10, -1, 0.25, U0),     # b = 36 = N - 4; K = N = 40: three tiles
    (100, 8, 24, -1, 0.25, U4),    # b = 64, n2 = 128: the widest slab stream
    (128, 8, 10, -1, 0.25, U0),
    (129, 8, 10, -1, 0.25, U0),    # odd N: the unvectorised GEMM
    (90, 8, 13, -1, 0.25, U1),     # K = N = 90 and K = n2 = 84: six tiles
    # ---- b > 64: two 64-column panels in the next-block product, n2 > 128
    (129, 8, 25, -1, 0.25, U4),
    (129, 8, 25, 1, 0.25, U0),     # free (kernel_sign = +1 at M >= 24)
    (200, 8, 25, -1, 0.25, U4),    # even N: the vectorised GEMM, panels of 64 and 2 columns
    (200, 8, 33, -1, 0.25, U4),    # M > 32: the residual (K = 164) and final (K = 82) products leave the VALU kernel
    # ---- the other tile counts of K2 at n2 = 4 M + 32, at N = 64 k, 64 k + 1 and between
    (65, 6, 1, -1, 0.25, U0),
    (192, 8, 2, -1, 0.25, U0),
    (193, 8, 5, -1, 0.25, U0),
    (192, 8, 14, -1, 0.25, U0),
    (193, 8, 17, -1, 0.25, U1),
    (150, 8, 18, -1, 0.25, U0),
    (160, 8, 21, -1, 0.25, U1),
    # ---- wide blocks, b = N - 1 with M = N - 2 (all free): K2's tile counts 9 .. 13 on the wave path ...
    (71, 8, 69, -1, 0.25, U0), (75, 8, 73, -1, 0.25, U0), (81, 8, 79, -1, 0.25, U0), (89, 8, 87, -1, 0.25, U0), (91, 8, 89, -1, 0.25, U0),
    (97, 8, 95, -1, 0.25, U0), (99, 8, 97, -1, 0.25, U0), (105, 8, 103, -1, 0.25, U0),
    # ... and n2 > 208, the panel kernels with a last panel of 6, 7, 8, 1, 2, 3, 4, 5 tiles
    (106, 8, 104, -1, 0.25, U0), (118, 8, 116, -1, 0.25, U0), (128, 8, 126, -1, 0.25, U0), (133, 8, 131, -1, 0.25, U0),
    (141, 8, 139, -1, 0.25, U0), (149, 8, 147, -1, 0.25, U0), (157, 8, 155, -1, 0.25, U0), (165, 8, 163, -1, 0.25, U0),
]
assert len(set(CASES)) == len(CASES)


def case_input(case):
    n, k, _, _, _, (gen, seed) = case
    return GENERATORS[gen](n, k, seed)


def case_routes(case):
    """what the case is certain to run: the next-block product only where b < N - 1"""
    n, k, m, _, _, (gen, _) = case
    return routes(n, k, m, True, gen == "uniform32", next_block=block_sizes(n, k, m)["b"] < n - 1)
