"""The case list of tests/test_gpu_dense_exact.py, certified without a GPU: the route table of tests/dense_routes.py still
restates the dispatch text it mirrors; plan_dw and the row classes give the values worked out by hand; every case builds and
certifies (fp64 under 2^53 and its SI_F32 twin under 2^24: the forward pass, the gradient of the log-density, the training
gradient on every index set); each case reaches what it is there for and the union of the instantiations the cases reach
EQUALS the declared reachable list; the weight gradients the GPU is held to are not hollow."""
import os
import re

import numpy as np
import pytest

from oracle import subspace_oracle as so
from tests import dense_routes as dr
from tests import lattice as lat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, I = dr.R, dr.I


def _squeeze(text):
    return re.sub(r"\s+", "", text)


def _src(name):
    return _squeeze(open(os.path.join(ROOT, "subspaceinference.jl_amd", "csrc", name)).read())


# ----------------------------------------------------------------------------------------------- the restatement
DISPATCH_TEXT = {
    "kernels_gemm.hip": (
        # pick_bm
        """if (out <= 32) return 32;
           auto padded = [&](int bm) { return (out + bm - 1) / bm * bm; };
           const int p96 = padded(96), p128 = padded(128), p64 = padded(64);
           if (p96 <= p128 && p96 <= p64) return 96;
           return p128 <= p64 ? 128 : 64;""",
        # launch_dense_cfg: VEC and KEDGE
        """const bool vec = (out % 2 == 0) && (in % 2 == 0) && ((reinterpret_cast<uintptr_t>(W) & 15u) == 0) &&
           ((reinterpret_cast<uintptr_t>(Hin) & 15u) == 0) &&
           (FUSE || (((reinterpret_cast<uintptr_t>(Hout) & 15u) == 0) && ((reinterpret_cast<uintptr_t>(bias) & 15u) == 0))) &&
           (((fa.cb.w | fa.cb.hin | fa.cb.hout) & 1) == 0);
           const bool kedge = (in % 16) != 0;""",
        "auto kern = dense_f64_kernel<BM, BN, WM, WN, MINW, VEC, KEDGE, FUSE>;",
        # launch_dense_f64: small, panel (one chain only), then the tile by pick_bm
        "if (dense_small_applies(out, in, B, cb.n, pick_bm(out))) {",
        "launch_dense_small_f64(st, W, bias, Hin, Hout, out, in, B, act, dense_fused_slot_feats(out), cb);",
        "if (cb.n <= 1 && dense_panel_applies(W, out, in, B, act) && launch_dense_f64_panel(st, W, bias, Hin, Hout, out, in, B, act)) return;",
        """case 32: launch_dense_cfg<32, 128, 1, 4, 2>(st, W, bias, Hin, Hout, out, in, B, act, fa); break;
           case 96: launch_dense_cfg<96, 128, 2, 4, 4>(st, W, bias, Hin, Hout, out, in, B, act, fa); break;
           case 128: launch_dense_cfg<128, 128, 2, 4, 4>(st, W, bias, Hin, Hout, out, in, B, act, fa); break;
           default: launch_dense_cfg<64, 128, 2, 4, 4>(st, W, bias, Hin, Hout, out, in, B, act, fa); break;""",
        # the fused head: slots, features per slot, no panel form
        "const int wm = bm == 32 ? 1 : 2; return (out + bm - 1) / bm * wm;",
        "return bm == 32 ? 32 : bm / 2;",
        """case 32: launch_dense_cfg<32, 128, 1, 4, 2, true>(st, W, bias, Hin, Hkeep, out, in, B, act, fa); break;
           case 96: launch_dense_cfg<96, 128, 2, 4, 4, true>(st, W, bias, Hin, Hkeep, out, in, B, act, fa); break;
           case 128: launch_dense_cfg<128, 128, 2, 4, 4, true>(st, W, bias, Hin, Hkeep, out, in, B, act, fa); break;
           default: launch_dense_cfg<64, 128, 2, 4, 4, true>(st, W, bias, Hin, Hkeep, out, in, B, act, fa); break;""",
    ),
    "kernels_gemm_small.hip": (
        """const int64_t big = (int64_t)((out + bm - 1) / bm) * ((B + 127) / 128) * (nchains > 0 ? nchains : 1);
           return big <= 128 && in <= 2048 && out >= 1 && B >= 1;""",
        "switch (slot_feats / 16) { case 2: hipLaunchKernelGGL((dense_small_f64_kernel<2, FUSE>),",
        "case 3: hipLaunchKernelGGL((dense_small_f64_kernel<3, FUSE>),", "default: hipLaunchKernelGGL((dense_small_f64_kernel<4, FUSE>),",
    ),
    "kernels_gemm_panel.hip": (
        """if (in < 1 || in > 128 || out < 64 || out > 1024 || out % 2 != 0 || act_is_extra(act) || B < 1) return false;
           if ((reinterpret_cast<uintptr_t>(W) & 15) != 0) return false;
           return (int64_t)((out + 15) / 16) * ((B + 127) / 128) >= 16 * (int64_t)panel_grid();""",
        "g = 2 * cus;", "constexpr int RD = 4;", "if (in == 16 * KT) hipLaunchKernelGGL((dense_f64_panel_kernel<KT, RD, false>),",
        "else hipLaunchKernelGGL((dense_f64_panel_kernel<KT, RD, true>),",
        "switch ((in + 15) / 16) { case 1: launch_panel_inst<1>(", "case 7: launch_panel_inst<7>(", "default: launch_panel_inst<8>(",
    ),
    "si_internal.h": ("constexpr int SI_FUSE_MAX_OUT = 4;", "constexpr int64_t LD_ALIGN = 64;", "int n = 1; int64_t w = 0, hin = 0, hout = 0, part = 0;"),
    "capi_common.h": (   # head_fused: the one statement of the narrow-head rule
        """return !plan.has_conv && (L >= 2) && layers[L - 1].out <= SI_FUSE_MAX_OUT &&
           layers[L - 1].act < SI_ACT_LEAKYRELU && layers[L - 2].act < SI_ACT_LEAKYRELU;""",),
    "capi_infer.hip": (
        "su.act_elems = pad_ld(su.model.max_stored * B);",
        "static constexpr int SI_FUSED_MAX_WIDTH = 256;", "if (ctx->setup.fused_ok && ctx->chain_mode != 0 && !out) {",
        "cb.n = nc; cb.w = ldw; cb.hout = v.act_elems;",
        "ctx->fw.part, ctx->fw.yhat, ctx->setup.act_elems, ctx->setup.model.f32, defer_sse_final, true};",   # setup_view: the set-up's own stride and type
        """const double per = (cm.f32 ? 4.0 : 8.0) * 2.0 * (double)su.act_elems +
           8.0 * (((double)cm.part_slots() + 1.0) * (double)cm.out_dim * (double)su.B + (cm.f32 ? 1.5 : 1.0) * (double)pad_ld(cm.N) +
           (double)su.sse_blocks);
           const double fit = std::floor(SI_BATCH_BYTES / per);
           return (int)std::max(1.0, std::min({(double)C, fit, 1024.0}));""",
        # si_predict: fp64, its own workspace, through a view of its own
        "const int64_t act_elems = pad_ld(ctx->setup.model.max_stored * Bn);",
        "const DensityView v{tX, tXc, nullptr, tY, Bn, tA, nullptr, tS, sse_blocks, tP, tYh, act_elems, /*f32=*/false,",
    ),
    "capi.hip": (
        "hipError_t raw_dev_malloc(void** out, size_t bytes) { return hipMalloc(out, bytes); }",   # A1: every buffer its own allocation
        # chain_model_build: where the narrow-head rule is applied (off for a NeuralODE), the widest stored output
        "m.fuse_tail = node_d == 0 && head_fused(m.plan, layers, L);",
        "if (l < (m.fuse_tail ? L - 2 : L)) m.max_stored = std::max<int64_t>(m.max_stored, q.out_elems);",
        "if (f32) m.fuse_slots32 = dense_f32_fused_slots(lf.out, lf.in, lf.w_off % 4 == 0);",
        # dense_forward
        "const size_t nl = a.m->layers.size(), nplain = fuse_tail ? nl - 2 : nl;",
        "launch_dense_f64(st, a.w + ly.w_off, a.w + ly.b_off, h, o, ly.out, ly.in, B, ly.act, cb);",
        "launch_dense_f64_fused(st, a.w + ly.w_off, a.w + ly.b_off, h, ly.out, ly.in, B, ly.act, a.w + ll.w_off, ll.out, a.part, cb, keep);",
        "launch_tail_sse(st, a.part, a.slots, ll.out, B, a.w64 + ll.b_off, ll.act, a.Y, a.yhat, a.ssepart, a.sse_blocks, cb);",
        "launch_sse(st, h, a.Y, di, a.ssepart, a.sse_blocks, a.sse, cb.n, cb.hout, !a.defer_sse_final);",
        "launch_sse_f32(st, h, a.Y, di, a.ssepart, a.sse_blocks, a.sse, cb.n, cb.hout, a.yhat, a.yhat ? di : 0, !a.defer_sse_final);",
        # dense_reverse_sweep
        "launch_rowsum(st, s.delta[cur], ll.out, s.B, s.rspart, s.gw + ll.b_off);",
        """launch_tail_bwd(st, s.w + ll.w_off, s.delta[cur], s.hs[nl - 2], ll.out, ll.in, s.B, lp.act, s.delta[cur ^ 1], s.bwpart,
           s.gw + ll.w_off, s.gw + lp.b_off);""",
        """launch_backward_weight(st, s.delta[cur], hprev, s.bwpart, ly.out, ly.in, s.B, ctx->num_cu, s.gw + ly.w_off,
           (have_db && li + 1 == top) ? nullptr : s.gw + ly.b_off);
           if (li > 0) { launch_backward_data(st, s.w + ly.w_off, s.delta[cur], hprev, s.delta[cur ^ 1], ly.out, ly.in, s.B, layers[li - 1].act);""",
    ),
    "kernels_bwd.hip": (
        "enum { EPI_DACT = 1, EPI_RAW = 2 };",
        # the `vec` rule of launch_gemm
        """const bool vec = al(A) && al(Bm) && al(C) && (aux == nullptr || al(aux)) && lda % 2 == 0 && ldb % 2 == 0 &&
           ldc % 2 == 0 && Mrows % 2 == 0 && (ALAY == 0 || Kdim % 2 == 0) &&
           (BLAY == 0 ? Ncols % 2 == 0 : Kdim % 2 == 0) && ksplit % 2 == 0;""",
        "auto kern = gemm_f64_kernel<BM, BN, WM, WN, 4, ALAY, BLAY, true, EPI>;", "constexpr int WM = 2, WN = 4, NT = 512;",
        # dw_dma_ok, pick_bm_bwd
        "return B % 16 == 0 && B >= 16 && out % 2 == 0 && in % 2 == 0 && out >= 2 && in >= 2 && al(Delta) && al(Hprev) && al(part);",
        """if (rows <= 64) return 64;
           auto padded = [&](int bm) { return (rows + bm - 1) / bm * bm; };
           const int p96 = padded(96), p128 = padded(128), p64 = padded(64);
           if (p96 <= p128 && p96 <= p64) return 96;
           return p128 <= p64 ? 128 : 64;""",
        # launch_backward_data
        "const int64_t ks = ((int64_t)out + 15) / 16 * 16; switch (pick_bm_bwd(in)) {",
        "case 96: launch_gemm<96, 128, 1, 1, EPI_DACT>(st, W, out, Delta, out, DeltaPrev, in, in, B, out, 1, ks, Hprev, act_prev); break;",
        "default: launch_gemm<64, 128, 1, 1, EPI_DACT>(st, W, out, Delta, out, DeltaPrev, in, in, B, out, 1, ks, Hprev, act_prev); break;",
        # plan_dw
        """static constexpr int DW_BM[DW_NCAND] = {96, 128, 64, 96};
           static constexpr int DW_BN[DW_NCAND] = {128, 128, 128, 192};""",
        """const int64_t slots = (int64_t)num_cu * 2;
           const int64_t maxsplit = (B + 255) / 256;
           DwPlan best{96, 128, 1, B};
           double best_score = -1.0;""",
        "if (bn != 128 && !dma) continue;",
        """const int64_t pm = (out + bm - 1) / bm, pn = (in + bn - 1) / bn;
           const int64_t tiles = pm * pn;
           int64_t ns = slots / tiles;
           if (ns > maxsplit) ns = maxsplit;
           if (ns < 1) ns = 1;
           const double useful = ((double)out * in) / ((double)pm * bm * (double)pn * bn);
           const double fill = (double)(tiles * ns) / (double)((tiles * ns + slots - 1) / slots * slots);
           if (useful * fill > best_score * 1.0001) {""",
        """best.ks = ((B + best.nsplit - 1) / best.nsplit + 15) / 16 * 16;
           best.nsplit = (int)((B + best.ks - 1) / best.ks);""",
        # launch_backward_weight
        "bool dma = dw_dma_ok(Delta, Hprev, part, out, in, B);", "const DwPlan p = plan_dw(out, in, B, num_cu, dma);",
        """if (dma && p.bm == 96 && (p.bn == 192 || p.bn == 128)) {
           if (p.bn == 192) launch_dw_dma<96, 192>(st, Delta, Hprev, part, out, in, B, p.nsplit, p.ks, db ? extra : nullptr);
           else launch_dw_dma<96, 128>(st, Delta, Hprev, part, out, in, B, p.nsplit, p.ks, db ? extra : nullptr);
           if (db) launch_split_reduce(st, extra, p.nsplit, out, db);
           } else {
           if (db) launch_rowsum(st, Delta, out, B, extra, db);""",
        "case 96: launch_gemm<96, 128, 0, 0, EPI_RAW>(st, Delta, out, Hprev, in, part, out, out, in, B, p.nsplit, p.ks, nullptr, 0); break;",
        "case 128: launch_gemm<128, 128, 0, 0, EPI_RAW>(st, Delta, out, Hprev, in, part, out, out, in, B, p.nsplit, p.ks, nullptr, 0); break;",
        "default: launch_gemm<64, 128, 0, 0, EPI_RAW>(st, Delta, out, Hprev, in, part, out, out, in, B, p.nsplit, p.ks, nullptr, 0); break;",
        "launch_split_reduce(st, part, p.nsplit, (int64_t)out * in, dW);",
        # launch_rowsum, launch_tail_bwd
        "if (out <= 8) { hipLaunchKernelGGL(rowsum_narrow_kernel,",
        """const bool vec = (F % 2 == 0) && ((reinterpret_cast<uintptr_t>(H) & 15u) == 0) && ((reinterpret_cast<uintptr_t>(DeltaPrev) & 15u) == 0);""",
        "hipLaunchKernelGGL((tail_bwd_kernel<OLV, 2>),", "hipLaunchKernelGGL((tail_bwd_kernel<OLV, 1>),",
        "case 3: SI_TAILB(3); break; default: SI_TAILB(4); break;",
    ),
    "kernels_gemm_f32.hip": (
        "static bool f32_fast_shape(int32_t out, int32_t in) { return in >= 16 && in % 16 == 0 && out >= 4 && out % 4 == 0; }",
        """return f32_fast_shape(out, in) && (reinterpret_cast<uintptr_t>(W) & 15u) == 0 && (reinterpret_cast<uintptr_t>(Hin) & 15u) == 0 &&
           (reinterpret_cast<uintptr_t>(Hout) & 15u) == 0 && ((cb.w | cb.hin | cb.hout) & 3) == 0;""",
        "const int p192 = (out + 191) / 192 * 192, p128 = (out + 127) / 128 * 128; return p192 < p128 ? 192 : 128;",
        """if (f32_pick_bm(out) == 192) launch_f32_dma<192, 128, 2, 4, 2, 4, FUSE>(st, W, bias, Hin, Hout, out, in, B, act, fa);
           else launch_f32_dma<128, 128, 2, 4, 2, 4, FUSE>(st, W, bias, Hin, Hout, out, in, B, act, fa);""",
        "template <int BM, int BN, int WM, int WN, int NB, int MINW, bool FUSE, int BK = 16> static void launch_f32_dma(",
        "const bool fused = f32_fast_ok(Wt, Delta, Dout, out, in, fa.cb) && (reinterpret_cast<uintptr_t>(Hprev) & 15u) == 0;",
        """if (aligned && f32_fast_shape(out, in)) { const int bm = f32_pick_bm(out); return (out + bm - 1) / bm * 2; } return (out + 63) / 64 * 2;""",
    ),
    "kernels_bwd_f32.hip": (
        "p.dma = B % 16 == 0 && B >= 16 && out % 4 == 0 && in % 4 == 0 && out >= 4 && in >= 4 && al(Delta) && al(Hprev) && al(part);",
        """const int64_t tiles = p.dma ? (int64_t)((out + 127) / 128) * ((in + 127) / 128) : ((int64_t)out * in + 255) / 256;
           const int64_t slots = (int64_t)num_cu * (p.dma ? 4 : 16), maxsplit = (B + 255) / 256;
           int64_t ns = std::max<int64_t>(1, std::min(slots / std::max<int64_t>(tiles, 1), maxsplit));""",
        "if (p.dma) {", "hipLaunchKernelGGL((dw_f32_dma_kernel<128, 128>),", "hipLaunchKernelGGL(dw_f32_generic_kernel,",
        "if (H == nullptr && D == nullptr && rows % 4 == 0 && (reinterpret_cast<uintptr_t>(G) & 15u) == 0) {",
        "if (H == nullptr && D == nullptr && rows <= 8) {",
        "if (Yhat64) hipLaunchKernelGGL(delta_out_f32_kernel<double>,", "else hipLaunchKernelGGL(delta_out_f32_kernel<float>,",
        "case 3: hipLaunchKernelGGL((tail_bwd_f32_kernel<3>),", "default: hipLaunchKernelGGL((tail_bwd_f32_kernel<4>),",
    ),
    "capi_train.hip": (
        "launch_delta_out_f32(st, s.Y, fuse_tail ? ws.yhat64 : nullptr, fuse_tail ? nullptr : h, d, s.scale, ll.act, ws.delta32[cur]);",
        "launch_mul_dact_rowsum_f32(st, ws.delta32[cur], nullptr, ll.out, nb, SI_ACT_IDENTITY, nullptr, ws.rspart64, ws.gw32 + ll.b_off);",
        "launch_backward_weight_f32(st, ws.delta32[cur], hprev, ws.part32, ly.out, ly.in, nb, ctx->num_cu, ws.gw32 + ly.w_off);",
        """if (!have_db)
           launch_mul_dact_rowsum_f32(st, ws.delta32[cur], nullptr, ly.out, nb, SI_ACT_IDENTITY, nullptr, ws.rspart64, ws.gw32 + ly.b_off);""",
        """launch_transpose_f32(st, w + ly.w_off, ly.out, ly.in, ws.wt32);
           if (launch_dense_f32_dx(st, ws.wt32, ws.zero32, ws.delta32[cur], ws.delta32[cur ^ 1], ly.in, ly.out, nb, ws.hs32[li - 1], lq.act))
           launch_mul_dact_rowsum_f32(st, ws.delta32[cur ^ 1], nullptr, ly.in, nb, SI_ACT_IDENTITY, nullptr, ws.rspart64, ws.gw32 + lq.b_off);
           else
           launch_mul_dact_rowsum_f32(st, ws.delta32[cur ^ 1], ws.hs32[li - 1], ly.in, nb, lq.act, ws.delta32[cur ^ 1], ws.rspart64,
           ws.gw32 + lq.b_off);""",
        "v = TrainBatchView{t->X, t->X32, t->Y}; if (in_order) return SI_OK;",   # A4: an in-order batch uses X in place (train_batch)
        "const int32_t prc = chain_model_build(ctx, \"si_train_setup\", layers, L, N, in_dim, out_dim, f32, 0, model);",
    ),
}


@pytest.mark.parametrize("name", list(DISPATCH_TEXT))
def test_dispatch_text_still_what_the_table_restates(name):
    """a change of a shape rule must fail here and not as a missing kernel in a trace nobody reads"""
    src = _src(name)
    for text in DISPATCH_TEXT[name]:
        assert _squeeze(text) in src, text


# ----------------------------------------------------------------------------------------------- values worked by hand
def test_pick_bm_row_classes():
    """the tile that pads least, 96 winning ties; the forward kernel alone has 32-row tiles"""
    rows = (1, 32, 33, 64, 65, 96, 97, 128, 129, 192, 193, 256, 257, 384, 385, 960, 1010)
    fwd = {r: dr.pick_bm(r) for r in rows}
    assert fwd == {1: 32, 32: 32, 33: 64, 64: 64, 65: 96, 96: 96, 97: 128, 128: 128, 129: 96, 192: 96, 193: 128, 256: 128, 257: 96,
                   384: 96, 385: 64, 960: 96, 1010: 128}     # 385: 448 | 480 | 512 padded rows; 1010: 1024 | 1056 | 1024, 128 before 64
    assert {r: dr.pick_bm_bwd(r) for r in rows} == {r: (64 if r <= 32 else v) for r, v in fwd.items()}
    assert [dr.slot_feats(o) // 16 for o in (32, 64, 96, 128)] == [2, 2, 3, 4]       # TM of the small kernel
    assert [dr.fused_slots(o) for o in (32, 64, 96, 128, 130, 960)] == [1, 2, 2, 2, 4, 20]


def test_plan_dw_by_hand():
    # cfg2, 960 x 960: 96 x 192 tiles are 10 x 5 = 50 without padding, 512 / 50 = 10 splits fill 500 slots (score 0.977);
    # 96 x 128 pads the columns to 1024: 80 tiles x 6 splits = 480 slots, score 0.9375 x 0.9375
    assert dr.plan_dw(960, 960, 100000) == (96, 192, 10, 10000)
    assert dr.plan_dw(960, 960, 3200) == (96, 192, 10, 320)           # tests/test_gpu_parity.py's batch: 13 splits allowed, 10 taken
    assert dr.plan_dw(960, 960, 100000, dma=False) == (96, 128, 6, 16672)   # without the DMA kernel: 80 tiles x 6; 6 x 16672 >= 100000
    # the first layer of cfg2, 960 x 128: 10 tiles x 51 splits = 510 slots
    assert dr.plan_dw(960, 128, 100000) == (96, 128, 51, 1968)
    # 130 x 902 at B = 7952 (32 splits allowed): 96 x 128 = 2 x 8 tiles x 32 = 512 slots, useful 117260 / (192 x 1024) = 0.596;
    # 64 x 128 = 24 tiles x 21 = 504 slots at the same useful share: 0.587; 128 x 128 pads the rows to 256: 0.447
    assert dr.plan_dw(130, 902, 7952) == (96, 128, 32, 256) and 31 * 256 + 16 == 7952
    # few tiles: every candidate is limited by ceil(B / 256) splits and the 64-row tile has the most tiles to fill slots with
    assert dr.plan_dw(100, 6, 4096) == (64, 128, 16, 256)
    assert dr.plan_dw(190, 100, 4096) == (64, 128, 16, 256)
    assert dr.plan_dw(130, 902, 3981) == (64, 128, 16, 256)           # half the batch: 16 splits allowed, 24 tiles x 16 > 16 tiles x 16
    # the split count after rounding ks up to whole k tiles: 7951 columns in 32 splits of 256, the last one 15 columns
    assert dr.dw_route(130, 902, 7951, True)[1] == ("reg", 96, 128, 32, 256)
    assert dr.dw_route(130, 902, 7952, True)[1] == ("dma", 96, 128, 32, 256)
    assert dr.dw_route(1154, 130, 7952, True)[1] == ("dma", 96, 192, 32, 256)
    assert dr.dw_route(962, 130, 7952, True)[1] == ("reg", 128, 128, 32, 256)     # the DMA kernel has no 128-row tile
    assert dr.dw_route(129, 902, 7952, True)[1] == ("reg", 96, 128, 32, 256)      # odd out: no 16-byte pairs


def test_existing_lattice_cases_reach_fewer():
    """what tests/test_gpu_lattice.py (_SPECS with GRAD_CASES, cfg2, TRAIN_CASES at the batches it uses) reached before this table:
    no LDS-DMA weight gradient and no register-staged one above 64 rows, no 64-row forward tile, four of the panel kernel's
    sixteen instantiations"""
    from tests import test_gpu_lattice as tl
    reached = set()
    for name, ((dims, acts, b), kw) in tl._SPECS.items():
        entries = ("forward", "logdensity", "predict") + (("grad",) if name in tl.GRAD_CASES else ())
        f32 = kw.get("f32", False)
        reached |= dr.all_routes(dims, acts, b, kw.get("ncols", 1), entries=entries, dtypes=(f32,))
    reached |= dr.all_routes(*tl.CFG2, ncols=1, entries=("forward", "logdensity"), dtypes=(False,))
    for dims, nbt in tl.TRAIN_CASES:
        table, n = so.layer_table(dims, [R, R, I])
        for nb in (nbt, nbt - 37, nbt // 2 + 5):
            for f32 in (False, True):
                reached |= dr.routes(table, n, nb, "train", f32)
            for fin, fout, _, _, _ in table:
                assert dr.dw_route(fout, fin, nb, True)[1][:3] == ("reg", 64, 128), (dims, nb)
    assert reached < set(dr.REACHABLE)
    assert not [k for k in reached if k.startswith(("dw_f64_dma_kernel", "dense_f64_kernel<64,", "gemm_f64_kernel<96, 128, 2, 4, 4, 0",
                                                     "gemm_f64_kernel<128, 128, 2, 4, 4, 0"))]
    assert sorted(k for k in reached if "panel" in k) == [dr.k_panel(1, True), dr.k_panel(2, True), dr.k_panel(7, True), dr.k_panel(8, False)]
    assert len(reached & set(dr.REACHABLE_F64)) == 41 and len(reached & set(dr.REACHABLE_F32)) == 21


# ----------------------------------------------------------------------------------------------- coverage
def test_cases_reach_exactly_the_declared_instantiations():
    reached = set()
    for name, dims, b, targets in dr.CASES:
        r = dr.all_routes(dims, dr.case(name)[1], b)
        missing = [t for t in targets if t not in r]
        assert targets and not missing, "%s does not reach what it is there for: %s" % (name, missing)
        reached |= r
    assert len(set(dr.REACHABLE)) == len(dr.REACHABLE) == 87 + 22
    assert sorted(reached) == dr.REACHABLE, (sorted(set(dr.REACHABLE) - reached), sorted(reached - set(dr.REACHABLE)))


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
    """profiles/dense_exact_kernel_names.txt, the kernel trace of tests/test_gpu_dense_exact.py alone: every declared instantiation
    ran, and no kernel of a Dense family outside the declared list did"""
    lines = [l for l in open(os.path.join(ROOT, "profiles", "dense_exact_kernel_names.txt")) if l.strip() and not l.startswith("#")]
    seen = {_trace_name(l) for l in lines}
    assert not set(dr.REACHABLE) - seen, sorted(set(dr.REACHABLE) - seen)
    families = ("dense_f64", "dense_small", "dense_f32", "gemm_f64_kernel", "dw_f", "tail_", "rowsum", "mul_dact", "act_inplace", "delta_out",
                "split_reduce", "sse_", "ptg_", "transpose_f32")
    assert not [n for n in seen - set(dr.REACHABLE) if n.startswith(families)]
    assert all(int(l.split()[0]) > 0 for l in lines)


def test_weight_gradient_legs():
    """the LDS-DMA cases have ragged last row and column tiles, several splits with a shorter last one that is exactly one 16-deep
    k tile, and a smaller batch that takes another plan"""
    dims, _, b = dr.case("dw_dma")
    for (fin, fout), bn in (((902, 130), 128), ((130, 1154), 192)):
        kern, bm, bn_, ns, ks = dr.dw_route(fout, fin, b, True)[1]
        assert (kern, bm, bn_) == ("dma", 96, bn) and fout % 96 and fin % bn and ns > 1 and b - (ns - 1) * ks == 16
        assert [dr.dw_route(fout, fin, nb, True)[1][:3] for nb in dr.train_sizes(b)[1:]] in (
            [("reg", 96, 128), ("reg", 64, 128)], [("reg", 64, 128), ("reg", 64, 128)])
    assert dims == [902, 130, 1154, 2]


def test_case_sizes():
    """a case is at most a few 10^9 multiply-adds a pass and trains with a power-of-two output width or not at all"""
    for name, dims, b, _ in dr.CASES:
        assert sum(a * c for a, c in zip(dims[:-1], dims[1:])) * b < 3e9, name
    assert sorted(set(dr.NAMES) - set(dr.TRAIN_NAMES)) == ["small_100_8_3", "small_3_3_3"]     # heads of three outputs


# ----------------------------------------------------------------------------------------------- certificates
def _blocks_all_zero(g):
    """16 x 16 blocks aligned to 16 (ragged ones at the edges included) of a matrix that hold no nonzero"""
    return [(r, c) for r in range(0, g.shape[0], 16) for c in range(0, g.shape[1], 16) if not g[r:r + 16, c:c + 16].any()]


def _assert_not_hollow(name, table, gw, f32, what):
    for i in lat._param_rows(table):
        ws, _ = lat._row_slices(table[i])
        g = gw[ws].reshape((table[i][1], table[i][0]), order="F")
        if not f32:
            frac = float(np.mean(g != 0))
            assert frac >= 0.5, "%s, %s, layer %d: only %.0f %% of the exact dW entries are nonzero" % (name, what, i, 100 * frac)
        assert not _blocks_all_zero(g), "%s, %s, layer %d: all-zero 16 x 16 blocks of dW at %s" % (name, what, i, _blocks_all_zero(g)[:4])


@pytest.mark.parametrize("name", dr.NAMES)
@pytest.mark.parametrize("f32", [False, True])
def test_case_certifies(name, f32):
    """the forward certificate (asserted by the builder), the gradient of the log-density, the training gradient on every index
    set, and the hollow-gradient condition on each of them"""
    pb = dr.problem(name, f32)
    assert pb.f32 == f32 and pb.bound_bits < (24 if f32 else 53)
    assert lat.lp_cases(pb, "r") and lat.lp_cases(pb, "null")
    _, _, gw = lat.logdensity_grad_certified(pb, 0, pb.y1)
    _assert_not_hollow(name, pb.table, gw, f32, "d lp / d w")
    if name not in dr.TRAIN_NAMES:
        return
    table, n, w, x, y = dr.train_problem(name, f32)
    assert lat.f32_exact(w) and lat.f32_exact(x) and lat.f32_exact(y)
    b = x.shape[1]
    sizes = [idx.size for idx in dr.train_batches(b)]
    assert sizes[0] == sizes[1] == b and sizes[2] % 16 and sizes[3] < sizes[2]
    for idx in dr.train_batches(b):
        _, gw = lat.mse_grad_exact(table, w, x[:, idx], y[:, idx], dr.nb_total(name), lat.F32_LIMIT if f32 else lat.F64_LIMIT)
        _assert_not_hollow(name, table, gw, f32, "training gradient of %d" % idx.size)
