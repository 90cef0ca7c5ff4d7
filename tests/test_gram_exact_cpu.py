"""The case list of tests/test_gpu_gram_exact.py, certified without a GPU: the route table of tests/gram_routes.py still restates
the dispatch text it mirrors; the routes give the values worked out by hand; the union of the instantiations the cases reach
EQUALS the declared reachable list (26 LDS-DMA + 32 panel Gram instantiations, the four reduce kernels, 16 push instantiations)
and every N class gives the slabs per workgroup it is there for; every case builds and certifies (integer A, every partial sum
below 2^53, fp32 twins representable); and the cases are not hollow: each of a catalogue of small kernel mistakes, applied as a
correction to the exact G, changes G in every case."""
import os
import re

import numpy as np
import pytest

from tests import gram_routes as gr
from tests import lattice as lat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = gr.SI_F32, gr.SI_F64


def _squeeze(text):
    return re.sub(r"\s+", "", text)


def _src(name):
    return _squeeze(open(os.path.join(ROOT, "subspaceinference.jl_amd", "csrc", name)).read())


# ----------------------------------------------------------------------------------------------- the restatement
DISPATCH_TEXT = {
    "kernels_gram_wave.hip": (
        "constexpr int GR = 32;", "constexpr int GW_WAVES = 4;",
        # the slab deal of a workgroup
        "const int64_t nslab = (N + GR - 1) / GR; const int64_t stride = gridDim.x; int64_t slab = blockIdx.x;",
        # launch_nt_q: two workgroups per CU with a ring of two, else one with the ring 150 KB hold
        "static constexpr bool gram_two_per_cu() { return true; }",
        """if constexpr (KS2 > 0) {
           if (gram_two_per_cu()) {
           constexpr int NB = 2;""",
        "hipLaunchKernelGGL((gram_glds_kernel<NT, KS2, NB, 2, NQ>), dim3(nblocks), dim3(64 * GW_WAVES), lds, st, A, ldA, N, K, tiles);",
        "constexpr int NB = (150 * 1024) / (NT * 16 * GR * 8) >= 4 ? 4 : (150 * 1024) / (NT * 16 * GR * 8) >= 3 ? 3 : 2;",
        "hipLaunchKernelGGL((gram_glds_kernel<NT, KS, NB, 1, NQ>), dim3(nblocks), dim3(64 * GW_WAVES), lds, st, A, ldA, N, K, tiles);",
        # launch_nt: the ragged rule
        """if (K - 16 * (NT - 1) <= 4)
           launch_nt_q<NT, KS, KS2, 1>(st, A, ldA, N, K, tiles, nblocks);
           else
           launch_nt_q<NT, KS, KS2, 4>(st, A, ldA, N, K, tiles, nblocks);""",
        "return (nt <= 9 && gram_two_per_cu()) ? 2 : 1;",
        # the three parts
        "switch ((K + 15) / 16) { case 1: launch_nt<1, 4, 2>(", "case 2: launch_nt<2, 4, 2>(", "case 3: launch_nt<3, 4, 2>(",
        "case 4: launch_nt<4, 4, 2>(", "case 5: launch_nt<5, 4, 2>(", "case 6: launch_nt<6, 4, 2>(",
        "#endif launch_nt<7, 4, 2>(st, A, ldA, N, K, tiles, nblocks, 0);", "#endif launch_nt<8, 2, 2>(st, A, ldA, N, K, tiles, nblocks, 0);",
        "switch ((K + 15) / 16) { case 9: launch_nt<9, 2, 1>(", "case 10: launch_nt<10, 2, 0>(", "case 11: launch_nt<11, 1, 0>(",
        "switch ((K + 15) / 16) { case 12: launch_nt<12, 1, 0>(", "case 13: launch_nt<13, 1, 0>(",
    ),
    "kernels_gram.hip": (
        "constexpr int GR2 = 32;", "constexpr int GR2_Y = 16;", "static constexpr bool gram_force_panels() { return false; }",
        # launch_gram
        """const int64_t nslab_d = (N + GR - 1) / GR, nslab_o = (N + GR2 - 1) / GR2;
           int64_t nb_diag = std::min<int64_t>((int64_t)num_cu * 2, nslab_d);
           int64_t nb_off = std::min<int64_t>((int64_t)num_cu * 2, nslab_o);
           const int npan = (int)((K + 127) / 128);
           const int ntw = (int)((K + 15) / 16);
           const bool wave_path = ntw <= 13 && !gram_force_panels() && a_dtype != SI_F32;
           const int64_t nb_wave = std::min<int64_t>((int64_t)num_cu * gram_wave_blocks_per_cu(ntw), nslab_d);
           const size_t need = wave_path ? ((size_t)nb_wave + GR2_Y) * (size_t)(ntw * (ntw + 1) / 2) * 256 * sizeof(double)
           : (size_t)std::max<int64_t>(nb_diag * 36, npan > 1 ? nb_off * 64 : 0) * 256 * sizeof(double);""",
        "if (wave_path && gram_wave_dispatch(st, A, ldA, N, (int)K, Gpart, G, (int)nb_wave, prof, tot_flops, tot_bytes)) return need;",
        """if (a_dtype == SI_F32)
           gram_panels<float>(st, static_cast<const float*>(Av), ldA, N, K, Gpart, G, nb_diag, nb_off, npan, prof, tot_flops, tot_bytes);
           else
           gram_panels<double>(st, A, ldA, N, K, Gpart, G, nb_diag, nb_off, npan, prof, tot_flops, tot_bytes);""",
        # gram_wave_dispatch: one launch booked on the Gram class, the two-stage reduction
        """ProfScope ps(prof, SI_K_GRAM, flops, bytes);
           if (!(launch_gram_wave_part0(st, A, ldA, N, K, Gpart, nblocks) || launch_gram_wave_part1(st, A, ldA, N, K, Gpart, nblocks) ||
           launch_gram_wave_part2(st, A, ldA, N, K, Gpart, nblocks)))""",
        "hipLaunchKernelGGL(gram_reduce_stage1_kernel, dim3(P, GR2_Y), dim3(256), 0, st, Gpart, nblocks, P, scr);",
        "hipLaunchKernelGGL(gram_reduce_stage2_kernel, dim3(P), dim3(256), 0, st, scr, nt, K, G);",
        "const int per = (nblocks + GR2_Y - 1) / GR2_Y; const int sp0 = y * per, sp1 = sp0 + per < nblocks ? sp0 + per : nblocks;",
        # gram_panels
        """for (int I = 0; I < npan; ++I) {
           const int ci0 = I * 128;
           const int nti = (int)((std::min<int64_t>(K, ci0 + 128) - ci0 + 15) / 16);""",
        """for (int J = I + 1; J < npan; ++J) {
           const int cj0 = J * 128;
           const int ntj = (int)((std::min<int64_t>(K, cj0 + 128) - cj0 + 15) / 16);
           gram_off_dispatch<AT>(st, A, ldA, N, (int)K, ci0, cj0, ntj, Gpart, G, (int)nb_off, prof, 0.0, 0.0);""",
        "switch (nt) { case 1: launch_gram_small<1, AT>(", "case 7: launch_gram_small<7, AT>(", "default: launch_gram_small<8, AT>(",
        "switch (ntj) { case 1: launch_gram_off<1, AT>(", "case 7: launch_gram_off<7, AT>(", "default: launch_gram_off<8, AT>(",
        "hipLaunchKernelGGL((gram_small_kernel<NT, AT>), dim3(nblocks), dim3(512), lds, st, A, ldA, N, K, col0, Gpart);",
        "hipLaunchKernelGGL(gram_small_reduce_kernel, dim3(NT * (NT + 1) / 2), dim3(1024), 0, st, Gpart, nblocks, NT, K, col0, G);",
        "hipLaunchKernelGGL((gram_off_kernel<NTJ, AT>), dim3(nblocks), dim3(512), lds, st, A, ldA, N, K, ci0, cj0, Gpart);",
        "hipLaunchKernelGGL(gram_off_reduce_kernel, dim3(8 * NTJ), dim3(256), 0, st, Gpart, nblocks, NTJ, K, ci0, cj0, G);",
        "for (; sp < nblocks; sp += 4) s += src[(int64_t)sp * stride];",    # gram_small_reduce: lane ln adds partials ln, ln + 4, ...
    ),
    "kernels_stream.hip": (
        "int64_t blocks = (work_items + 255) / 256; const int64_t cap = (int64_t)num_cu * 8;",
        "if (blocks > cap) blocks = cap; if (blocks < 1) blocks = 1; return (int)blocks;",
        "const int grid = stream_grid(N >> 2, num_cu); const bool aligned = (reinterpret_cast<uintptr_t>(w) & 15u) == 0;",
        "hipLaunchKernelGGL((swa_dev_push_kernel<float, true, AT>),", "hipLaunchKernelGGL((swa_dev_push_kernel<float, false, AT>),",
        "hipLaunchKernelGGL((swa_dev_push_kernel<double, true, AT>),", "hipLaunchKernelGGL((swa_dev_push_kernel<double, false, AT>),",
        """const int grid = stream_grid((N + 1) >> 1, num_cu);
           const size_t esz = w_dtype == SI_F32 ? 4 : 8;""",
        "const bool vec = (ld % 2 == 0) && (ld >= N + (N & 1)) && ((reinterpret_cast<uintptr_t>(w) & (2 * esz - 1)) == 0);",
        "hipLaunchKernelGGL((swa_dev_push_batch_kernel<float, true, AT>),", "hipLaunchKernelGGL((swa_dev_push_batch_kernel<float, false, AT>),",
        "hipLaunchKernelGGL((swa_dev_push_batch_kernel<double, true, AT>),", "hipLaunchKernelGGL((swa_dev_push_batch_kernel<double, false, AT>),",
        "launch_swa_dev_push_t<float>(st, w, w_dtype, s, static_cast<float*>(acol), N, n, num_cu);",
        "launch_swa_dev_push_batch_t<float>(st, w, w_dtype, ld, s, static_cast<float*>(A), ldA, N, count, nvals_dev, slot0, kcap, num_cu);",
    ),
    "si_internal.h": ("constexpr int64_t LD_ALIGN = 64;",),
    "capi.hip": (
        "launch_gram(ctx->stream, ctx->d_A, ctx->ldA, ctx->N, K, ctx->d_Gpart, ctx->d_G, ctx->num_cu, ctx, ctx->a_dtype);",
        "ctx->d_A + (size_t)slot * ctx->ldA * asz,",      # a column of A starts at a multiple of pad_ld(N)
        "ctx->ldA = pad_ld(N);",
        # the call sites NOT in the table (held by tests/test_gpu_finish_exact.py)
        "launch_gram(ctx->stream, ctx->d_B, ctx->ldA, N, K, ctx->d_Gpart, ctx->d_G, ctx->num_cu, ctx);",
        "launch_gram(ctx->stream, ctx->d_At, ldt, K, N, ctx->d_Gpart, ctx->d_G, ctx->num_cu, ctx);",
    ),
}


@pytest.mark.parametrize("name", list(DISPATCH_TEXT))
def test_dispatch_text_still_what_the_table_restates(name):
    """a change of a shape rule must fail here and not as a missing kernel in a trace nobody reads"""
    src = _src(name)
    for text in DISPATCH_TEXT[name]:
        assert _squeeze(text) in src, text


def test_no_development_knob_in_the_tests():
    """only what the shipped library reaches counts: neither the table nor the GPU file sets a knob of the development build"""
    for f in ("test_gpu_gram_exact.py",):
        text = open(os.path.join(ROOT, "tests", f)).read()
        assert not re.search(r"SI_GRAM_|SI_GW_KNOB|environ", text)


# ----------------------------------------------------------------------------------------------- values worked by hand
def test_routes_by_hand():
    # K = 100: 7 tiles, the last of 4 columns -> ragged; NT <= 9 runs two workgroups per CU on KS2 = 2 with a ring of two
    assert gr.gram_routes(100003, 100) == ["gram_glds_kernel<7, 2, 2, 2, 1>", "gram_reduce_stage1_kernel", "gram_reduce_stage2_kernel"]
    assert gr.wave_blocks_per_cu(7) == 2 and gr.plan(100003, 100).nb_wave == 512
    # K = 176: 11 full tiles, one workgroup per CU, KS = 1, 150 KB / (11 * 16 * 32 * 8 B = 44 KB) = 3 ring buffers
    assert gr.gram_routes(4097, 176)[0] == "gram_glds_kernel<11, 1, 3, 1, 4>"
    # K = 208: 13 tiles, 52 KB a buffer: two
    assert gr.gram_routes(4097, 208)[0] == "gram_glds_kernel<13, 1, 2, 1, 4>"
    assert [gr.wave_inst(k)[2] for k in (144, 145, 160, 161, 192, 193)] == [2, 3, 3, 3, 3, 2]
    assert gr.wave_inst(97) == (7, 2, 2, 2, 1) and gr.wave_inst(101) == (7, 2, 2, 2, 4) and gr.wave_inst(129) == (9, 1, 2, 2, 1)
    # K = 209, fp64: the wave path ends at 13 tiles; panels of 8 and 6 tiles (81 columns), one off-diagonal pair
    assert gr.gram_routes(4097, 209) == ["gram_small_kernel<8, double>", "gram_small_reduce_kernel", "gram_off_kernel<6, double>",
                                         "gram_off_reduce_kernel", "gram_small_kernel<6, double>", "gram_small_reduce_kernel"]
    assert gr.gram_launches(4097, 209) == 3 and gr.gram_launches(4097, 208) == 1 and gr.gram_launches(33, 336) == 6
    # fp32 storage never takes the wave path
    assert gr.gram_routes(4097, 100, F32) == ["gram_small_kernel<7, float>", "gram_small_reduce_kernel"]
    # workspace: (512 + 16) workgroups' worth of 28 tile pairs; panels: 36 diagonal pairs | 64 off-diagonal tiles per workgroup
    assert gr.plan(100003, 100).need == 528 * 28 * 2048
    assert gr.plan(4097, 100, F32).need == 129 * 36 * 2048 and gr.plan(100003, 209).need == 512 * 64 * 2048
    assert gr.slabs_per_block(100003, 100) == (6, 7) and gr.slabs_per_block(4097, 100) == (1, 1)
    assert gr.slabs_per_block(100003, 100, num_cu=64) == (24, 25)


def test_push_routes_by_hand():
    assert gr.stream_grid(0) == 1 and gr.stream_grid(257) == 2 and gr.stream_grid(10 ** 7) == 2048
    assert gr.push_routes("single", 4097, F32, F64) == ["swa_dev_push_kernel<float, true, double>"]
    assert gr.push_routes("single", 4097, F64, F32, offset=1) == ["swa_dev_push_kernel<double, false, float>"]     # 8 bytes off
    assert gr.push_routes("single", 4097, F32, F64, offset=4) == ["swa_dev_push_kernel<float, true, double>"]      # 16 bytes off
    assert gr.push_routes("batch", 1001, F32, F64, ld=1001) == ["swa_dev_push_batch_kernel<float, false, double>"]
    assert gr.push_routes("batch", 1001, F32, F64, ld=1002) == ["swa_dev_push_batch_kernel<float, true, double>"]
    assert gr.push_routes("batch", 1000, F64, F32, ld=1000, offset=1) == ["swa_dev_push_batch_kernel<double, false, float>"]
    # one pass of the full grid covers 2048 * 256 threads x 4 (single) | 2 (batch) elements
    assert gr.push_passes("single", 2097152) == 1 and gr.push_passes("single", 2097156) == 2
    assert gr.push_passes("batch", 1048576) == 1 and gr.push_passes("batch", 1048577) == 2


# ----------------------------------------------------------------------------------------------- coverage
@pytest.mark.parametrize("num_cu", [256, 64])
def test_cases_reach_exactly_the_declared_instantiations(num_cu):
    reached = set()
    for c in gr.CASES:
        r = gr.case_routes(c, num_cu)
        missing = [t for t in c.targets if t not in r]
        assert c.targets and not missing, "%s does not reach what it is there for: %s" % (c.name, missing)
        reached |= set(r)
    assert len(gr.REACHABLE_WAVE) == 26 and len(gr.REACHABLE_PANEL) == 32 and len(gr.REACHABLE_PUSH) == 16
    assert len(set(gr.REACHABLE)) == len(gr.REACHABLE) == 26 + 32 + 4 + 16
    assert sorted(reached) == gr.REACHABLE, (sorted(set(gr.REACHABLE) - reached), sorted(reached - set(gr.REACHABLE)))
    assert len({c.name for c in gr.CASES}) == len(gr.CASES)


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
    """profiles/gram_exact_kernel_names.txt, the kernel trace of tests/test_gpu_gram_exact.py alone: every declared instantiation ran,
    and no Gram or push kernel outside the declared list did"""
    lines = [l for l in open(os.path.join(ROOT, "profiles", "gram_exact_kernel_names.txt")) if l.strip() and not l.startswith("#")]
    seen = {_trace_name(l) for l in lines}
    assert not set(gr.REACHABLE) - seen, sorted(set(gr.REACHABLE) - seen)
    assert not [n for n in seen - set(gr.REACHABLE) if n.startswith(("gram_", "swa_"))]
    assert all(int(l.split()[0]) > 0 for l in lines)


def test_every_instantiation_at_every_n_class():
    """per instantiation and not per "a few K": each of the 26 wave instantiations at the four N classes, each of the 32 panel
    instantiations at the three; the width of the last tile takes each of 1, 2, 3, 4, 5, 15, 16"""
    seen = {}
    for c in gr.GRAM_CASES:
        for t in c.targets:
            seen.setdefault(t, set()).add(c.nclass)
    for name in gr.REACHABLE_WAVE:
        assert seen[name] == set(gr.N_CLASSES_WAVE), name
    for name in gr.REACHABLE_PANEL:
        assert seen[name] == set(gr.N_CLASSES_PANEL), name
    wave = [c for c in gr.GRAM_CASES if c.name.startswith("wave")]
    assert {c.k - 16 * ((c.k + 15) // 16 - 1) for c in wave} >= {1, 2, 3, 4, 5, 15, 16}
    for nt in range(1, 14):   # and every tile count sees every width of both variants
        assert {c.k - 16 * (nt - 1) for c in wave if (c.k + 15) // 16 == nt} == set(gr.RAGGED_WIDTHS) | set(gr.PLAIN_WIDTHS)
    # fp32 panels and fp64 panels: K % 16 == 0 and K % 16 != 0 both appear, in one, two and three panels
    for ks in (gr.PANEL_K_F64, gr.PANEL_K_F32):
        assert any(k % 16 == 0 for k in ks) and any(k % 16 for k in ks)
    assert {(k + 127) // 128 for k in gr.PANEL_K_F64} == {2, 3} and {(k + 127) // 128 for k in gr.PANEL_K_F32} == {1, 2}
    assert min(gr.PANEL_K_F64) == 209 and max(gr.gram_n(c) * c.k for c in gr.GRAM_CASES) <= 49257 * 208


@pytest.mark.parametrize("num_cu", [256, 64])
def test_n_classes_give_their_slab_counts(num_cu):
    for c in gr.GRAM_CASES:
        n = gr.gram_n(c, num_cu)
        nslab, nb = (n + 31) // 32, gr.gram_grid(n, c.k, c.storage, num_cu)
        lo, hi = gr.slabs_per_block(n, c.k, c.storage, num_cu)
        assert n % 32 != 0, c.name            # every class ends in a partial slab
        if c.nclass == "one":
            assert n in (1, 31) and (nslab, nb, lo, hi) == (1, 1, 1, 1), c.name
        elif c.nclass == "p33":
            assert (nslab, nb, lo, hi) == (2, 2, 1, 1), c.name
        elif c.nclass == "slab":
            assert n == 4097 and nslab == 129 and n - 32 * 128 == 1, c.name
            if num_cu == 256:
                assert (nb, lo, hi) == (129, 1, 1), c.name   # one slab per workgroup: the ring prologue's clamped re-fetch alone
        elif c.nclass in ("two", "pmany"):
            assert (lo, hi) == (1, 2) and 0 < nslab - nb < nb // 2, c.name       # some workgroups run two slabs, most run one
        else:
            nbuf = gr.ring_depth(c.k, c.storage)
            assert c.nclass == "wrap" and (lo, hi) == (nbuf + 1, nbuf + 2) and nslab - nb * lo == 4, c.name   # the ring wraps, uneven
    if num_cu == 256:
        assert sorted({gr.gram_n(c) for c in gr.GRAM_CASES if c.nclass == "wrap"}) == [24681, 32873, 49257]
        assert {gr.ring_depth(c.k) for c in gr.GRAM_CASES if c.nclass == "wrap"} == {2, 3}


def test_push_cases_cover_their_legs():
    single = [c for c in gr.PUSH_CASES if c.kind == "single"]
    batch = [c for c in gr.PUSH_CASES if c.kind == "batch"]
    for name in gr.REACHABLE_PUSH:
        mine = [c for c in gr.PUSH_CASES if name in c.targets]
        if "batch" not in name:    # every single-push instantiation at N % 4 = 0, 1, 2, 3
            assert {gr.push_n(c) % 4 for c in mine} == {0, 1, 2, 3}, name
        elif "true" in name:       # vec: even N with ld = N, odd N with the pair of the last element inside the padded row
            assert {(c.nclass % 2, c.ld_extra) for c in mine if c.nclass != "wrap"} == {(0, 0), (1, 1), (1, 3)}, name
        else:                      # not vec: an odd ld (ld = N odd, ld = N + 1 odd) or a pointer one element off
            assert {((c.nclass + c.ld_extra) % 2, c.offset) for c in mine} == {(1, 0), (0, 1)}, name
    assert [gr.push_passes(c.kind, gr.push_n(c)) for c in single if c.nclass == "wrap"] == [2]
    assert [gr.push_passes(c.kind, gr.push_n(c)) for c in batch if c.nclass == "wrap"] == [2]
    assert all(gr.push_passes(c.kind, gr.push_n(c)) <= 1 for c in gr.PUSH_CASES if c.nclass != "wrap")   # (0: N = 3 has no quad)
    assert all(c.count == 3 for c in gr.PUSH_CASES if c.nclass == "wrap")
    assert any(gr.push_n(c) < 4 for c in single)          # the tail alone


def test_gpu_order_alternates():
    order = gr.gpu_order(gr.GRAM_CASES)
    assert sorted(c.name for c in order) == sorted(c.name for c in gr.GRAM_CASES)
    size = [gr.gram_n(c) * c.k for c in order]
    assert all(size[i] >= size[i + 1] for i in range(0, len(size) - 1, 2)) and size[0] == max(size) and size[1] == min(size)


# ----------------------------------------------------------------------------------------------- certificates and mutants
def _tiles(g, k):
    """the 16 x 16 tiles of a K x K matrix, zero padded: array (NT, NT, 16, 16), [a, b] = rows of tile a, columns of tile b"""
    nt = (k + 15) // 16
    p = np.zeros((nt * 16, nt * 16))
    p[:k, :k] = g
    return p.reshape(nt, 16, nt, 16).transpose(0, 2, 1, 3)


def _upper(nt):
    return [(a, b) for a in range(nt) for b in range(a, nt)]


def _assert_changes_every_tile_pair(delta, k, what):
    """the correction is nonzero in EVERY upper-triangular tile pair (so whichever wave, chunk or panel launch owns a pair, the
    mistake shows there)"""
    t = _tiles(delta, k)
    dead = [(a, b) for a, b in _upper(t.shape[0]) if not t[a, b].any()]
    assert not dead, "%s: leaves tile pairs %s of G unchanged" % (what, dead[:4])


def _rows_of_slabs(slabs, n):
    return np.concatenate([np.arange(32 * s, min(32 * s + 32, n)) for s in slabs])


def _gram_of(a, rows):
    sub = a[rows]
    return sub.T @ sub


def _reduce_groups(c, nb):
    """the addends of the last stage of the fixed-order sum, as lists of workgroups: the 16 stage-2 addends of the wave path
    (stage 1's workgroup y adds partials y * per .. ), the four lane sums of gram_small_reduce_kernel on the panel path"""
    if gr.plan(1, c.k, c.storage).wave_path:
        per = (nb + gr.GR2_Y - 1) // gr.GR2_Y
        groups = [list(range(y * per, min(y * per + per, nb))) for y in range(gr.GR2_Y)]
    else:
        groups = [list(range(ln, nb, 4)) for ln in range(4)]
    return [g for g in groups if g]


def _check_mutants(c, n, a, g):
    k = c.k
    nt = (k + 15) // 16
    nslab, nb, ks = (n + 31) // 32, gr.gram_grid(n, k, c.storage), gr.k_split(k, c.storage)
    tiles = _tiles(g, k)
    # one 32-row slab dropped: the first, one in the middle, the last; the ragged last slab's rows
    for s in sorted({0, nslab // 2, nslab - 1}):
        _assert_changes_every_tile_pair(_gram_of(a, _rows_of_slabs([s], n)), k, "slab %d dropped" % s)
    assert n % 32 != 0
    _assert_changes_every_tile_pair(_gram_of(a, np.arange(32 * (nslab - 1), n)), k, "the rows of the ragged last slab dropped")
    # one 4-row k step of one slab dropped, for each residue class mod KS of the route (its first and its last step).  A class
    # with no row in the case cannot be dropped: N = 1 has k step 0 alone
    done = set()
    for s0 in sorted({0, nslab // 2}):
        for kg in range(ks):
            for step in sorted({kg, kg + ks * (8 // ks - 1)}):
                rows = np.arange(32 * s0 + 4 * step, min(32 * s0 + 4 * step + 4, n))
                if rows.size:
                    _assert_changes_every_tile_pair(_gram_of(a, rows), k, "k step %d of slab %d dropped" % (step, s0))
                    done.add(kg)
    assert done == set(range(ks)) or n < 4 * ks
    # two tile pairs swapped: no two of the upper-triangular tiles (zero padded) hold the same numbers
    flat = [tiles[p].tobytes() for p in _upper(nt)]
    assert len(set(flat)) == len(flat), "two tile pairs of G are equal: a swap would not show"
    # an off-diagonal tile written transposed
    same = [(x, y) for x, y in _upper(nt) if x != y and np.array_equal(tiles[x, y], tiles[x, y].T)]
    assert not same, "off-diagonal tiles %s equal their transposes" % same[:4]
    # the last 4-column block of the (ragged) last tile left out: it holds a nonzero in every tile row
    c0 = 4 * ((k - 1) // 4)
    for x in range(nt):
        assert g[16 * x:16 * x + 16, c0:k].any(), "the last 4-column block is zero in tile row %d" % x
    # column K - 1 read in place of column K - 2: the two differ in every tile row (K = 1 has one column)
    if k >= 2:
        for x in range(nt):
            assert not np.array_equal(g[16 * x:16 * x + 16, k - 2], g[16 * x:16 * x + 16, k - 1]), "columns K-2 and K-1 agree in tile row %d" % x
        assert not np.array_equal(a[:, k - 2], a[:, k - 1])
    # column 0 zeroed: row 0 of G holds a nonzero in every tile column
    assert a[:, 0].any() and all(g[0, 16 * y:16 * y + 16].any() for y in range(nt)), "column 0 does not reach every tile of G"
    # the last workgroup's partial left out of the first-stage sum
    _assert_changes_every_tile_pair(_gram_of(a, _rows_of_slabs(range(nb - 1, nslab, nb), n)), k, "the partial of workgroup %d left out" % (nb - 1))
    # one addend of the last stage left out (the first, a middle and the last of those that hold a workgroup)
    groups = _reduce_groups(c, nb)
    for gi in sorted({0, len(groups) // 2, len(groups) - 1}):
        rows = _rows_of_slabs([s for b in groups[gi] for s in range(b, nslab, nb)], n)
        _assert_changes_every_tile_pair(_gram_of(a, rows), k, "addend %d of the last reduction stage left out" % gi)


@pytest.mark.parametrize("name", [c.name for c in gr.GRAM_CASES])
def test_gram_case_certifies_and_is_not_hollow(name):
    c = next(x for x in gr.GRAM_CASES if x.name == name)
    n = gr.gram_n(c)
    snaps, ns, a, g = gr.gram_problem(n, c.k)
    assert a.shape == (n, c.k) and min(ns) >= 1 and len(snaps) == c.k
    # the certificate of lat.gram_exact_certified, restated on this case; max |a|^2 N < 2^53 is the cruder form of it
    amax = float(np.max(np.abs(a)))
    assert amax <= 8 * max(ns) and amax * amax * n < lat.F64_LIMIT
    assert float(np.max(np.abs(a).T @ np.abs(a))) < lat.F64_LIMIT
    # fp32 snapshots and fp32 storage hold the same integers
    assert all(lat.f32_exact(s) for s in snaps) and lat.f32_exact(a)
    assert gr.blocks_nonzero(a) and not np.any(np.all(a == 0, axis=0))
    assert np.array_equal(g, g.T) and np.array_equal(g, np.rint(g))
    if n * c.k <= 4097 * 64:      # the int64 product agrees (small cases: it takes three times as long)
        assert np.array_equal(g, lat.gram_exact(a).astype(np.float64))
    _check_mutants(c, n, a, g)


def test_gram_exact_certified_refuses_what_could_round():
    a = np.full((4, 2), 2.0 ** 25)
    a[:, 1] = 1.0
    g = lat.gram_exact_certified(a)               # 4 * 2^50 = 2^52: still exact
    assert g[0, 0] == 2.0 ** 52 and g[0, 1] == 2.0 ** 27
    with pytest.raises(AssertionError):
        lat.gram_exact_certified(np.full((8, 1), 2.0 ** 25))      # 8 * 2^50 = 2^53
    with pytest.raises(AssertionError):
        lat.gram_exact_certified(np.array([[0.5]]))


@pytest.mark.parametrize("name", [c.name for c in gr.PUSH_CASES])
def test_push_case_builds(name):
    c = next(x for x in gr.PUSH_CASES if x.name == name)
    n = gr.push_n(c)
    snaps, ns, w_ref, a_ref = gr.push_problem(c)
    assert len(snaps) == c.count == len(ns) and all(s.size == n for s in snaps)
    assert all(s.dtype == (np.float32 if c.wdtype == F32 else np.float64) for s in snaps)
    assert a_ref.shape == (n, c.count) and not np.any(np.all(a_ref == 0, axis=0))
    if c.storage == F32:     # the rounding of A to fp32 is exact on the lattice: the fp64 oracle is the reference as it stands
        assert lat.f32_exact(a_ref)
    else:                    # random data: the three rounded operations of a push all round
        assert not lat.f32_exact(a_ref) and not np.array_equal(a_ref, np.rint(a_ref))


# ----------------------------------------------------------------------------------------------- the older exact test
def test_existing_gram_cases_have_no_zero_column():
    """tests/test_gpu_lattice.py::test_gram_exact ran with n_0 = 0: column 0 of A, row and column 0 of G were zero and a kernel
    that mishandles lane 0 of tile 0 went unseen.  Its problems now start the epoch counters at 1."""
    from tests import test_gpu_lattice as tl
    for n, k in tl.GRAM_CASES:
        snaps, ns, a, g = tl.gram_problem(n, k)
        assert min(ns) >= 1 and not np.any(np.all(a == 0, axis=0)), (n, k)
        assert np.all(np.diag(g) > 0) and g[0].any()


def _reached_by_older_test():
    from tests import test_gpu_lattice as tl
    out = set()
    for n, k in tl.GRAM_CASES:
        out |= set(gr.gram_routes(n, k, F64)) | set(gr.gram_routes(n, k, F32))
    return out


def test_existing_gram_cases_reach_fewer():
    """what test_gram_exact reached before this table: 7 of the 26 wave instantiations, the NB = 3 ring never"""
    r = _reached_by_older_test()
    wave = sorted(x for x in r if x.startswith("gram_glds"))
    assert len(wave) == 7 and not [x for x in wave if x.split(", ")[2] == "3"]
    assert r < set(gr.REACHABLE)
    assert not [x for x in r if x.startswith(("gram_off_kernel<2", "gram_off_kernel<3", "gram_off_kernel<4", "gram_off_kernel<6", "gram_off_kernel<7"))]
