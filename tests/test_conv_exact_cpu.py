"""The case list of tests/test_gpu_conv_exact.py, certified without a GPU: the route table of tests/conv_routes.py still
restates the dispatch text it mirrors; every case builds and certifies (fp64 and its SI_F32 twin, the gradient of the
log-density, the training gradient); the union of the instantiations the cases reach EQUALS the declared reachable list;
the weight gradients the GPU is held to are not hollow (at least half of every layer's exact dW entries are nonzero); the
MaxPool cases include tied and untied maxima."""
import os
import re

import numpy as np
import pytest

from tests import conv_routes as cr
from tests import lattice as lat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _squeeze(text):
    return re.sub(r"\s+", "", text)


def _src(name):
    return _squeeze(open(os.path.join(ROOT, "subspaceinference.jl_amd", "csrc", name)).read())


# ----------------------------------------------------------------------------------------------- the restatement
def test_dispatch_text_still_what_the_table_restates():
    """a change of a shape rule must fail here and not as a missing kernel in a trace nobody reads"""
    conv, net = _src("kernels_conv.hip"), _src("capi_net.hip")
    for text in (
        # conv_pick_bm
        """if (rows <= 64) return 64;
           auto padded = [&](int bm) { return (rows + bm - 1) / bm * bm; };
           const int p96 = padded(96), p128 = padded(128), p64 = padded(64);
           if (p96 < p128 && p96 <= p64) return 96;
           return p128 <= p64 ? 128 : 64;""",
        # conv_first_applies, NS and NTM
        """return g.Kvalid <= 36 && COUTp <= 64 && g.sden_w == 1 && g.sden_h == 1 && g.Cp <= 64 && g.pad_w < 100 && g.pad_h < 100 &&
           (g.KW - 1) * g.dil_w < 100 && (g.KH - 1) * g.dil_h < 100;""",
        "const int ns = (g.Kvalid + 3) / 4;", "if (ns <= 5) launch_conv_first_ns<5, IDX>", "else launch_conv_first_ns<9, IDX>",
        "const int ntm = (COUTp + 15) / 16;", "case 3: SI_FIRST_CASE(3) break; default: SI_FIRST_CASE(4) break;",
        # CELLU and BM of the forward / data-gradient GEMM and of the fused pool kernel
        "const bool cellu = g.Cp % 16 == 0; const int bm = conv_pick_bm(Mp);",
        "const bool cellu = g.Cp % 16 == 0; const int bm = conv_pick_bm(COUTp);",
        "constexpr int BN = 128, WM = 2, WN = 4, NT = 512;",
        "auto kern = conv_gemm_kernel<BM, BN, WM, WN, 4, CELLU, DEN, BIASACT>;",
        "auto kern = conv_gemm_pool_kernel<BM, BN, WM, WN, 4, CELLU, IDX>;",
        # DEN
        """if (gT.sden_w > 1 || gT.sden_h > 1) launch_conv_gemm<true, false>(st, Wt, CINp, Delta, dX, nullptr, gT, npos_in, KpT, 0);
           else launch_conv_gemm<false, false>(st, Wt, CINp, Delta, dX, nullptr, gT, npos_in, KpT, 0);""",
        # dW: narrow, NOEDGE, the ladder, the split count
        "static bool conv_dw_narrow(int COUTp, int Kp) { return Kp <= 64 && COUTp <= 64; }",
        "if (npos % 16 == 0) { // (ksplit is a multiple of 16 by construction) auto kern = conv_dw_kernel<BM, BN, WM, WN, MINW, true>;",
        "launch_conv_dw_bm<64, 64, 6>(", "case 64: launch_conv_dw_bm<64, 128, 4>(", "case 96: launch_conv_dw_bm<96, 128, 4>(",
        "default: launch_conv_dw_bm<128, 128, 4>(",
        """const int64_t tiles = (int64_t)((COUTp + bm - 1) / bm) * (narrow ? 1 : (Kp + 127) / 128);""",
        """int64_t ns = ((int64_t)num_cu * (narrow ? 3 : 2)) / tiles;
           const int64_t maxsplit = (npos + 255) / 256;
           ns = std::max<int64_t>(1, std::min(ns, maxsplit));
           const int64_t ks = ((npos + ns - 1) / ns + 15) / 16 * 16;
           *ksplit_out = ks;
           return (int)((npos + ks - 1) / ks);""",
        # the narrow Dense layer
        "return out <= 16 && in >= 256 && (B + 127) / 128 < 2 * (int64_t)num_cu;", "constexpr int CW = 2;",
    ):
        assert _squeeze(text) in conv, text
    for text in (
        "return m.kind == SI_LAYER_MAXPOOL && m.KW == 2 && m.KH == 2 && m.sw == 2 && m.sh == 2 && q.Wo % 2 == 0 && q.Ho % 2 == 0;",
        "bool net_grad_fused(const NetPlan& p, size_t l) { return net_pool_fusable(p, l) && !act_is_extra(p.L[l].act); }",
        "q.Kp = (q.Cp * ly.kw * ly.kh + 15) / 16 * 16;", "static int even(int c) { return (c + 1) & ~1; }",
        "if (!pingpong && pidx && pidx[l] && net_grad_fused(p, l)) {", "const bool fuse_pool = pingpong && net_pool_fusable(p, l);",
        "if (li > 0 && s.pidx && s.pidx[li - 1] && net_grad_fused(p, li - 1)) {", "} else if (li > 0 && p.L[li - 1].kind == SI_LAYER_CONV) {",
        "launch_conv_backward_data(st, s.wt, g, gn, q.gT, q.Cp, q.KpT, (int64_t)q.Wi * q.Hi * B);",
        "if (dense_narrow_applies(q.out_feat, q.in_feat, B, c->num_cu))",
    ):
        assert _squeeze(text) in net, text


def test_pick_bm_row_classes():
    """the classes the issue of this table names: 64 | 66, 96 | 98, 128 | 130, 192 | 194 (rows are even)"""
    got = {r: cr.pick_bm(r) for r in (2, 64, 66, 96, 98, 128, 130, 192, 194, 256, 258, 384, 386)}
    assert got == {2: 64, 64: 64, 66: 96, 96: 96, 98: 128, 128: 128, 130: 96, 192: 96, 194: 128, 256: 128, 258: 96, 384: 128, 386: 64}


def test_dw_splits_by_hand():
    # narrow, one tile: 3 workgroups per CU allowed, but one split per 256 positions at most
    assert cr.dw_splits(64, 64, 256, 256) == (1, 256)
    assert cr.dw_splits(64, 64, 257, 256) == (2, 144)        # 257 = 144 + 113: a ragged last split
    assert cr.dw_splits(64, 64, 425, 256) == (2, 224)
    assert cr.dw_splits(64, 80, 272, 256) == (2, 144)        # 144 + 128: NOEDGE, unequal splits
    assert cr.dw_splits(64, 80, 525, 256) == (3, 176)        # 176 + 176 + 173
    # 194 rows at BM 128 (2 tiles) x 15 column tiles of Kp = 1808: 30 tiles -> 17 splits allowed on 256 CUs, none on 8
    assert cr.dw_splits(194, 1808, 100000, 256) == (17, 5888)
    assert cr.dw_splits(194, 1808, 100000, 8) == (1, 100000)
    assert cr.dw_splits(64, 64, 800, 1) == (3, 272)          # narrow on one CU: three resident workgroups


# ----------------------------------------------------------------------------------------------- coverage
@pytest.mark.parametrize("num_cu", [256, 64])
def test_cases_reach_exactly_the_declared_instantiations(num_cu):
    reached = set()
    for name, whc, spec, b, targets, _ in cr.CASES:
        r = cr.all_routes(spec, whc, b, num_cu)
        missing = [t for t in targets if t not in r]
        assert not missing, "%s does not reach what it is there for: %s" % (name, missing)
        reached |= r
    assert len(set(cr.REACHABLE)) == len(cr.REACHABLE) == 60 + 22
    assert sorted(reached) == cr.REACHABLE, (sorted(set(cr.REACHABLE) - reached), sorted(reached - set(cr.REACHABLE)))


def test_existing_conv_cases_reach_fewer():
    """what tests/test_gpu_conv.py::CASES (the shapes of the lattice test before this table) reach, with every activation
    taken as relu: a strict subset, without any BM = 128 instantiation"""
    from tests.test_gpu_lattice import CONV_CASES
    reached = set()
    for whc, spec, b in CONV_CASES:
        reached |= cr.all_routes(spec, whc, b)
    assert reached < set(cr.REACHABLE)
    assert not [k for k in reached if "<128," in k]
    assert len(reached) == 32


def test_weight_gradient_legs_are_covered():
    legs = set()
    for _, whc, spec, b, _, _ in cr.CASES:
        legs |= cr.dw_legs(spec, whc, b)
    for need in cr.DW_LEGS_REQUIRED:
        assert any(g[:4] == need for g in legs), need
    for bn in (64, 128):     # several splits with a ragged last one, with and without the ragged-tile code
        for noedge in (False, True):
            assert (64, bn, noedge, True, True) in legs


def test_case_sizes():
    for name, whc, spec, b, _, _ in cr.CASES:
        assert b <= 40 and whc[0] <= 8 and whc[1] <= 8, name
        npos = max(q["Wo"] * q["Ho"] * b for q in cr.plan(spec, whc) if q["kind"] == "conv")
        assert npos <= 800, (name, npos)
        out = cr.plan(spec, whc)[-1]["out_feat"]
        assert out & (out - 1) == 0, name    # si_train_grad's scale 2 / (out * nb_total) must be a power of two


# ----------------------------------------------------------------------------------------------- certificates
@pytest.mark.parametrize("name", cr.NAMES)
def test_case_certifies(name):
    """fp64 and SI_F32 forward certificates (asserted by the builder), the gradient of the log-density, the training gradient
    on every index set, and the hollow-gradient condition"""
    pb = cr.problem(name, False)
    pf = cr.problem(name, True)
    assert pf.f32 and pf.bound_bits < 24 and pb.bound_bits < 53
    assert lat.lp_cases(pb, "r") and lat.lp_cases(pb, "null") and lat.lp_cases(pf, "r")
    lat.pool_ties_are_exact(pb, 0)
    lat.logdensity_grad_certified(pb, 0, pb.y1)
    table, n, w, x, y = cr.train_problem(name)
    assert lat.f32_exact(w) and lat.f32_exact(x) and lat.f32_exact(y)
    b = x.shape[1]
    for idx in cr.train_batches(b):
        assert idx.size == b or idx.size % 16
        _, gw = lat.mse_grad_exact(table, w, x[:, idx], y[:, idx], cr.NB_TOTAL)
        if idx.size == b:
            for i in lat._param_rows(table):
                ws, _ = lat._row_slices(table[i])
                frac = float(np.mean(gw[ws] != 0))
                assert frac >= 0.5, "%s, row %d: only %.0f %% of the exact dW entries are nonzero" % (name, i, 100 * frac)
    # one Descent step with eta = 2^-3 stays exact in Float32
    _, gw = lat.mse_grad_exact(table, w, x, y, cr.NB_TOTAL)
    assert lat.f32_exact(w - 2.0 ** -3 * gw)


def test_pool_cases_have_tied_and_untied_maxima():
    tied, untied = [], []
    for name, _, spec, _, _, _ in cr.CASES:
        if any(e[0] == "maxpool" for e in spec):
            t, wins = lat.pool_tie_count(cr.problem(name, False), 0)
            assert wins > 0
            (tied if t else untied).append(name)
    assert tied and untied, (tied, untied)
    assert "first_5_3" in untied
