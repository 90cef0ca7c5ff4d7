"""tests/diffmap_routes.py certified without a GPU: the restated rules are held to the C++ text they mirror, REACHABLE is what the
shapes N <= 300 reach, the union of the routes of CASES equals it, CASES holds the cells it was written for, and every case that
is compared with the dense reference has a separated leading spectrum."""
import os
import re

import numpy as np
import pytest

from tests import diffmap_routes as dr
from tests import gram_routes as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "subspaceinference.jl_amd", "csrc")


def _squeeze(text):
    return re.sub(r"\s+", "", text)


def _src(name):
    return _squeeze(open(os.path.join(CSRC, name)).read())


def _body(src, start, end):
    i = src.index(_squeeze(start))
    return src[i:src.index(_squeeze(end), i)]


def test_rules_still_what_the_helper_restates():
    """a change of a shape rule must fail here and not as a mystery on the GPU"""
    dm = _body(_src("capi_diffmap.hip"), "int32_t si_construct_finish_diffmap(", "int32_t si_diffmap_info(")
    for stmt in ("if ((int64_t)M + 1 > N - 1) return fail(",
                 "const int64_t N = ctx->N, K = ctx->K, ldn = ctx->ldA;",
                 "const int b = (int)std::min<int64_t>(N - 1, 2 * (int64_t)M + 16), n2 = 2 * b;",
                 "const int Kp = (int)((K + 3) / 4 * 4), nb = dm_blocks(N);",
                 "const int64_t Npad = (int64_t)nb * 64, ldt = pad_ld(b);",
                 "const int Mpad_b = project_mpad(b), Mpad_m = project_mpad(M);",
                 "launch_dm_rescale(st, ctx->d_A, ctx->a_dtype, ldn, N, (int)K, Kp, rescale ? 1 : 0, dm.mm, dm.Xr, dm.s);",
                 "launch_transpose(st, Z, SI_F64, ldn, N, b, dm.Vt, ldt);",
                 "launch_project(st, dm.Kn, ldn, N, N, dm.Vt, b, (int32_t)ldt, Z + (size_t)b * ldn, ldn, ctx->num_cu);",
                 "launch_gram(st, Z, ldn, N, n2, dm.Gpart, dm.G, ctx->num_cu, nullptr);",
                 "launch_project(st, Z, ldn, N, n2, dm.coef, M, Mpad_m, dm.R, ldn, ctx->num_cu);",
                 "launch_project(st, Z, ldn, N, n2, dm.coef, b, Mpad_b, dm.Z[cur ^ 1], ldn, ctx->num_cu);",
                 "launch_project(st, dm.Z[cur], ldn, N, b, dm.coef, M, Mpad_m, U, ldn, ctx->num_cu);",
                 "launch_dm_colnorm(st, dm.R, ldn, N, M, dm.res);",
                 "launch_dm_finish(st, U, ldn, N, M, dm.u1, ctx->d_P, ldn);"):
        assert _squeeze(stmt) in dm, stmt
    assert dm.count("launch_project(") == 4 and dm.count("launch_gram(") == 2      # (one of the two sizes the workspace)
    assert "inlineint64_tpad_ld(int64_tn){return(n+LD_ALIGN-1)/LD_ALIGN*LD_ALIGN;}" in _src("si_internal.h")
    assert "c->ldA=pad_ld(N);" in _src("capi.hip")

    kd = _src("kernels_diffmap.hip")
    for stmt in ("constexpr int DM_T = 64;",
                 "int dm_blocks(int64_t N) { return (int)((N + DM_T - 1) / DM_T); }",
                 "const unsigned tiles = (unsigned)((int64_t)nb * (nb + 1) / 2);",
                 "if (rescale) hipLaunchKernelGGL(dm_minmax_kernel<float>,",
                 "if (rescale) hipLaunchKernelGGL(dm_minmax_kernel<double>,",
                 "hipLaunchKernelGGL(dm_rescale_kernel<float>,", "hipLaunchKernelGGL(dm_rescale_kernel<double>,"):
        assert _squeeze(stmt) in kd, stmt

    kg = _src("kernels_gram.hip")
    mpad = _body(kg, "int project_mpad(int M) {", "template <typename AT> static void project_valu(")
    assert _squeeze("m0 += rem > 24 ? 32 : rem > 16 ? 24 : rem > 8 ? 16 : 8;") in mpad
    valu = _body(kg, "static void project_valu(", "void launch_project(")
    for stmt in ("if (rem > 24) { hipLaunchKernelGGL((project_kernel<32, AT>),", "m0 += 32; } else if (rem > 16) { hipLaunchKernelGGL((project_kernel<24, AT>),",
                 "m0 += 24; } else if (rem > 8) { hipLaunchKernelGGL((project_kernel<16, AT>),",
                 "m0 += 16; } else { hipLaunchKernelGGL((project_kernel<8, AT>),"):
        assert _squeeze(stmt) in valu, stmt
    lp = kg[kg.index(_squeeze("void launch_project(hipStream_t st, const void* Av,")):]
    for stmt in ("if (M > 32) {",
                 "if (!project_force_gemm() && launch_project_stream(st, A, ldA, N, K, V, M, Mpad, P, ldP, num_cu)) return;",
                 "if (N < 0x7fffffff) { launch_project_mfma(st, A, ldA, N, K, V, M, Mpad, P, ldP); return; }",
                 "project_valu<double>(st, A, ldA, N, K, V, M, Mpad, P, ldP, num_cu);"):
        assert _squeeze(stmt) in lp, stmt
    assert _squeeze("static constexpr bool project_force_gemm() { return false; }") in kg

    kp = _src("kernels_project.hip")
    stream = kp[kp.index(_squeeze("bool launch_project_stream(hipStream_t st, const double* A,")):]
    for stmt in ("if (K > 128 || K <= 0) return false;", "for (int m0 = 0; m0 < M; m0 += 64) {", "switch ((int)(K + 15) / 16) {",
                 "default: launch_project_nt<8>(") + tuple("case %d: launch_project_nt<%d>(" % (t, t) for t in range(1, 8)):
        assert _squeeze(stmt) in stream, stmt
    nt = _body(kp, "static void launch_project_nt(", "template <int NT> __device__ __forceinline__ void project_glds_f32_body(")
    for stmt in ("if (project_two_per_cu()) {", "constexpr int NB = 2;", "hipLaunchKernelGGL((project_glds_kernel<NT, NB, 2>),"):
        assert _squeeze(stmt) in nt, stmt
    assert _squeeze("static constexpr bool project_two_per_cu() { return true; }") in kp

    kb = _src("kernels_bwd.hip")
    mfma = _body(kb, "void launch_project_mfma(", "__global__ __launch_bounds__(256) void split_reduce_kernel(")
    for stmt in ("for (int32_t m0 = 0; m0 < M; m0 += 64) {", "const int32_t mc = M - m0 < 64 ? M - m0 : 64;",
                 "launch_gemm<128, 64, 0, 0, EPI_RAW>(st, A, ldA, V + m0, Mpad, P + (int64_t)m0 * ldP, ldP, (int)std::min<int64_t>(N, 0x7fffffff), mc, K, 1, ks, nullptr, 0);"):
        assert _squeeze(stmt) in mfma, stmt
    for stmt in ("enum { EPI_DACT = 1, EPI_RAW = 2 };", "constexpr int WM = 2, WN = 4, NT = 512;",
                 "const bool vec = al(A) && al(Bm) && al(C) && (aux == nullptr || al(aux)) && lda % 2 == 0 && ldb % 2 == 0 && ldc % 2 == 0 && "
                 "Mrows % 2 == 0 && (ALAY == 0 || Kdim % 2 == 0) && (BLAY == 0 ? Ncols % 2 == 0 : Kdim % 2 == 0) && ksplit % 2 == 0;",
                 "auto kern = gemm_f64_kernel<BM, BN, WM, WN, 4, ALAY, BLAY, true, EPI>;",
                 "auto kern = gemm_f64_kernel<BM, BN, WM, WN, 4, ALAY, BLAY, false, EPI>;"):
        assert _squeeze(stmt) in kb, stmt


def test_block_sizes_and_mpad():
    for m in range(1, 300):
        mp = dr.project_mpad(m)
        widths = [int(k.split("<")[1].split(",")[0]) for k in dr.valu_kernels(m)]
        assert mp >= m and mp % 8 == 0 and mp - m < 8 and mp == sum(widths) and all(w == 32 for w in widths[:-1])
    s = dr.block_sizes(129, 5, 25)
    assert (s["b"], s["n2"], s["Kp"], s["nb"], s["Npad"], s["ldn"], s["ldt"], s["Mpad_b"], s["Mpad_m"], s["tiles"]) == (
        66, 132, 8, 3, 192, 192, 128, 72, 32, 6)
    s = dr.block_sizes(64, 8, 62)
    assert (s["b"], s["Kp"], s["Npad"], s["ldn"]) == (63, 8, 64, 64)      # N a multiple of 64: no padding rows or columns
    assert dr.block_sizes(3, 1, 1)["b"] == 2 and dr.block_sizes(12, 5, 10)["b"] == 11


def test_routes_of_the_named_cells():
    g = "gemm_f64_kernel<128, 64, 2, 4, 4, 0, 0, %s, 2>"
    def pk(n, k, m): return dr.project_kernels(n, k, m)
    assert pk(200, 200, 32) == ["project_kernel<32, double>"] and pk(200, 68, 34) == ["project_glds_kernel<5, 2, 2>"]
    assert pk(64, 64, 34) == ["project_glds_kernel<4, 2, 2>"] and pk(128, 128, 36) == ["project_glds_kernel<8, 2, 2>"]
    assert pk(129, 129, 36) == [g % "false"] and pk(200, 200, 34) == [g % "true"]
    assert pk(200, 132, 66) == [g % "true"] * 2 and pk(129, 132, 66) == [g % "false"] * 2      # two panels, 64 and 2 columns
    assert pk(200, 164, 33) == [g % "false"] and pk(200, 82, 33) == ["project_glds_kernel<6, 2, 2>"]
    assert pk(100, 128, 64) == ["project_glds_kernel<8, 2, 2>"] and pk(100, 100, 64) == ["project_glds_kernel<7, 2, 2>"]
    assert pk(12, 22, 11) == ["project_kernel<16, double>"] and pk(3, 4, 2) == ["project_kernel<8, double>"]
    assert pk(200, 100, 40) == ["project_glds_kernel<7, 2, 2>"] and pk(200, 129, 130) == [g % "true"] * 3
    assert dr.valu_kernels(26) == ["project_kernel<32, double>"] and dr.valu_kernels(20) == ["project_kernel<24, double>"]
    assert [c[1:3] for c in dr.project_calls(200, 33)] == [(200, 82), (164, 82), (164, 33), (82, 33)]
    assert dr.gram_kernels(3, 1)[0] == gr.k_wave(4) and dr.gram_kernels(200, 33)[0] == gr.k_wave(164)
    assert "gram_small_kernel<8, double>" in dr.gram_kernels(106, 104) and "gram_off_kernel<6, double>" in dr.gram_kernels(106, 104)


def test_reachable_is_what_shapes_reach():
    reach = set(dr.front_kernels(True, True)) | set(dr.front_kernels(False, True))
    for n in range(3, dr.N_MAX + 1):
        for m in range(1, n - 1):
            reach |= dr.routes(n, 1, m) | dr.routes(n, 1, m, rescale=False)
    assert sorted(reach) == dr.REACHABLE


def test_cases_cover_reachable():
    union = set()
    for c in dr.CASES:
        union |= dr.case_routes(c)
    assert sorted(union) == dr.REACHABLE, (sorted(set(dr.REACHABLE) - union), sorted(union - set(dr.REACHABLE)))
    assert all(3 <= c[0] <= dr.N_MAX and 1 <= c[2] <= c[0] - 2 for c in dr.CASES)


def _trace_name(line):
    """the kernel name of a line of the committed trace as the table writes it: no `void si::`, no argument list"""
    n = line.split(None, 1)[1].strip()
    n = n[5:] if n.startswith("void ") else n
    n = n[4:] if n.startswith("si::") else n
    depth = 0
    for i, ch in enumerate(n):
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            return n[:i]
    return n


def test_committed_trace_agrees_with_reachable():
    """profiles/diffmap_exact_kernel_names.txt, the kernel trace of tests/test_gpu_diffmap_exact.py alone: every declared
    instantiation ran, and no kernel of these families outside the declared list did"""
    lines = [l for l in open(os.path.join(ROOT, "profiles", "diffmap_exact_kernel_names.txt")) if l.strip() and not l.startswith("#")]
    seen = {_trace_name(l) for l in lines}
    assert len(dr.REACHABLE) == len(set(dr.REACHABLE)) == 70
    assert not set(dr.REACHABLE) - seen, sorted(set(dr.REACHABLE) - seen)
    assert not [n for n in seen - set(dr.REACHABLE) if n.startswith(("dm_", "project_", "gram_", "gemm_f64", "transpose_"))]
    assert all(int(l.split()[0]) > 0 for l in lines)


def test_cases_hold_the_cells_they_were_written_for():
    nm = {(c[0], c[2]) for c in dr.CASES}
    for cell in ((3, 1), (5, 3), (17, 2), (12, 10), (64, 8), (64, 9), (200, 8), (200, 9), (100, 24), (128, 10), (129, 10), (129, 25),
                 (200, 25), (200, 33)):
        assert cell in nm, cell
    assert {64, 128, 192, 65, 129, 193} <= {c[0] for c in dr.CASES}
    b = {c: dr.block_sizes(c[0], c[1], c[2])["b"] for c in dr.CASES}
    assert {32, 34} <= {b[c] for c in dr.CASES if c[0] <= 128} and {32, 34} <= {b[c] for c in dr.CASES if c[0] > 128}
    assert any(b[c] == c[0] - 1 and c[2] < c[0] - 2 for c in dr.CASES)
    assert any(32 < b[c] <= 64 and c[0] <= 128 for c in dr.CASES) and any(32 < b[c] <= 64 and c[0] > 128 for c in dr.CASES)
    assert any(b[c] > 64 and 2 * b[c] > 128 and c[2] <= 32 for c in dr.CASES) and any(c[2] > 32 and c[2] < c[0] - 2 for c in dr.CASES)
    assert {-1, 1} == {c[3] for c in dr.CASES}


def test_exempt_cases_are_only_the_two_kinds():
    free = [c for c in dr.CASES if dr.exempt(c[0], c[2], c[3])]
    assert all(c[2] == c[0] - 2 or (c[3] == 1 and c[2] >= 24) for c in free)
    assert len(free) == 20 and len(dr.CASES) == 46
    assert sum(1 for c in free if c[2] == c[0] - 2) == 19


@pytest.fixture(scope="module")
def dmp(si):
    from subspaceinference_jl_amd import diffmap
    return diffmap


@pytest.mark.parametrize("case", [c for c in dr.CASES if not dr.exempt(c[0], c[2], c[3])])
def test_compared_cases_are_well_separated(dmp, case):
    n, k, m, sign, eps, _ = case
    a = dr.case_input(case)
    assert a.shape == (n, k)
    if case[5][0] == "uniform32":
        assert np.array_equal(a, a.astype(np.float32))
    kn = dmp.diffmap_kernel(a, eps, 1.0, sign, True)[0]
    gap = dmp.spectrum_gap(kn, m)
    print("case %s: gap %.2e" % (case, gap))
    assert gap >= dr.GAP_MIN


@pytest.mark.parametrize("case", [c for c in dr.CASES if dr.exempt(c[0], c[2], c[3])])
def test_free_cases_have_a_finite_operator(dmp, case):
    n, k, m, sign, eps, _ = case
    kn = dmp.diffmap_kernel(dr.case_input(case), eps, 1.0, sign, True)[0]
    assert np.all(np.isfinite(kn)) and np.array_equal(kn, kn.T)
