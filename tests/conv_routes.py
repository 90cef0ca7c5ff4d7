"""Which conv kernel instantiation a chain reaches: the shape rules of csrc/kernels_conv.hip and csrc/capi_net.hip restated
in plain Python, the list of instantiations shapes can reach, and the lattice chains of tests/test_gpu_conv_exact.py, each
the smallest that reaches the instantiations written next to it (a helper module for the tests, not a conftest).

Rules restated (function here <- function there):
  pick_bm <- conv_pick_bm;  first_applies, first_ns_ntm <- conv_first_applies, launch_conv_first(_ns);
  pool_fusable <- net_pool_fusable / net_grad_fused (identical on the lattice: identity and relu are not "extra" activations);
  CELLU = (channel pitch of the gathered tensor) % 16 == 0;  DEN <- launch_conv_backward_data (any stride > 1);
  dw_narrow <- conv_dw_narrow;  NOEDGE = npos % 16 == 0;  dw_splits <- conv_dw_splits;  dense_narrow <- dense_narrow_applies.
tests/test_conv_exact_cpu.py holds the restatement to the C++ text it mirrors and proves that the union of the routes of CASES
equals REACHABLE.  A kernel name is written as the kernel trace prints it, with the element type of its arguments in
brackets: "conv_gemm_kernel<64, 128, 2, 4, 4, false, false, true>(double)" is
"void si::conv_gemm_kernel<64, 128, 2, 4, 4, false, false, true>(double const*, ..." of profiles/conv_exact_kernel_names.txt.

Not in the table: the kernels every conv chain launches whatever its shapes (conv_pack_kernel, conv_pack_t_kernel,
conv_unpack_dw_kernel, whcn_to_cwhn_kernel, cwhn_to_whcn_kernel, rowsum_chunks_final_kernel) and the Dense kernels behind
`flatten` other than dense_narrow_kernel (their routes are held by tests/test_gpu_lattice.py)."""
import functools

import numpy as np

from oracle import subspace_oracle as so

R, I = so.ACT_RELU, so.ACT_IDENTITY
NUM_CU = 256   # MI355X


def even(c):
    return (c + 1) & ~1


def pick_bm(rows):
    if rows <= 64:
        return 64
    p96, p128, p64 = ((rows + bm - 1) // bm * bm for bm in (96, 128, 64))
    if p96 < p128 and p96 <= p64:
        return 96
    return 128 if p128 <= p64 else 64


def plan(spec, whc):
    """the geometry net_plan derives for every row of the chain (names as in LayerPlan)"""
    table, _ = so.conv_table(spec, whc)
    out = []
    for row in table:
        if row[0] == "conv":
            _, (kw, kh, c, co), (wi, hi), (sw, sh), (pw, ph), (dw, dh), act, _, _ = row
            cp, cop = even(c), even(co)
            out.append(dict(kind="conv", C=c, Co=co, Cp=cp, Cop=cop, Wi=wi, Hi=hi, KW=kw, KH=kh, sw=sw, sh=sh, pw=pw, ph=ph, dw=dw,
                            dh=dh, Wo=so.conv_out_size(wi, kw, sw, pw, dw), Ho=so.conv_out_size(hi, kh, sh, ph, dh),
                            Kvalid=cp * kw * kh, Kp=(cp * kw * kh + 15) // 16 * 16, KpT=(cop * kw * kh + 15) // 16 * 16, act=act))
        elif row[0] == "maxpool":
            _, (pw, ph), c, (wi, hi), (sw, sh) = row
            out.append(dict(kind="maxpool", C=c, Cp=even(c), Wi=wi, Hi=hi, KW=pw, KH=ph, sw=sw, sh=sh, Wo=(wi - pw) // sw + 1,
                            Ho=(hi - ph) // sh + 1))
        elif row[0] == "flatten":
            out.append(dict(kind="flatten", C=row[1], Cp=even(row[1]), Wi=row[2][0], Hi=row[2][1]))
        else:
            out.append(dict(kind="dense", in_feat=row[0], out_feat=row[1], act=row[2]))
    return out


def first_applies(q):
    return (q["Kvalid"] <= 36 and q["Cop"] <= 64 and q["Cp"] <= 64 and q["pw"] < 100 and q["ph"] < 100
            and (q["KW"] - 1) * q["dw"] < 100 and (q["KH"] - 1) * q["dh"] < 100)


def first_ns_ntm(q):
    ns = 5 if (q["Kvalid"] + 3) // 4 <= 5 else 9
    return ns, min(4, (q["Cop"] + 15) // 16)


def pool_fusable(p, l):
    if l + 1 >= len(p) or p[l]["kind"] != "conv" or p[l + 1]["kind"] != "maxpool":
        return False
    q, m = p[l], p[l + 1]
    return (m["KW"], m["KH"], m["sw"], m["sh"]) == (2, 2, 2, 2) and q["Wo"] % 2 == 0 and q["Ho"] % 2 == 0


def dw_narrow(cop, kp):
    return kp <= 64 and cop <= 64


def dw_splits(cop, kp, npos, num_cu):
    """(number of splits, positions per split)"""
    bm = pick_bm(cop)
    narrow = dw_narrow(cop, kp)
    tiles = ((cop + bm - 1) // bm) * (1 if narrow else (kp + 127) // 128)
    ns = (num_cu * (3 if narrow else 2)) // tiles
    ns = max(1, min(ns, (npos + 255) // 256))
    ks = ((npos + ns - 1) // ns + 15) // 16 * 16
    return (npos + ks - 1) // ks, ks


def dense_narrow(out, fin, b, num_cu):
    return out <= 16 and fin >= 256 and (b + 127) // 128 < 2 * num_cu


def _b(v):
    return "true" if v else "false"


def _t(f32):
    return "(float)" if f32 else "(double)"


def k_gemm(bm, cellu, den, biasact, f32=False):
    return "conv_gemm_kernel<%d, 128, 2, 4, 4, %s, %s, %s>%s" % (bm, _b(cellu), _b(den), _b(biasact), _t(f32))


def k_pool(bm, cellu, idx, f32=False):
    return "conv_gemm_pool_kernel<%d, 128, 2, 4, 4, %s, %s>%s" % (bm, _b(cellu), _b(idx), _t(f32))


def k_first(ns, ntm, idx, f32=False):
    return "conv_first_pool_kernel<%d, %d, %s>%s" % (ns, ntm, _b(idx), _t(f32))


def k_dw(bm, bn, noedge):
    return "conv_dw_kernel<%d, %d, 2, 4, %d, %s>(double)" % (bm, bn, 6 if bn == 64 else 4, _b(noedge))


def k_plain(name, f32=False):
    return name + _t(f32)


MODES = ("sample", "grad_forward", "reverse")


def routes(spec, whc, b, mode, f32=False, num_cu=NUM_CU):
    """[set of kernel names] per row of the chain.  mode "sample": net_forward with ping-pong activations (si_forward,
    si_logdensity, si_predict, the samplers; fp64 or SI_F32); "grad_forward": the forward of net_value_and_grad (kept outputs
    and pool indices; fp64 only); "reverse": net_backward (fp64 only)."""
    assert mode in MODES and not (f32 and mode != "sample")
    p = plan(spec, whc)
    out = [set() for _ in p]
    if mode != "reverse":
        idx = mode == "grad_forward"
        l = 0
        while l < len(p):
            q = p[l]
            if q["kind"] == "dense":
                if dense_narrow(q["out_feat"], q["in_feat"], b, num_cu):
                    out[l].add(k_plain("dense_narrow_kernel<2>", f32))
            elif q["kind"] == "conv":
                if pool_fusable(p, l):
                    if first_applies(q):
                        out[l].add(k_first(*first_ns_ntm(q), idx, f32))
                    else:
                        out[l].add(k_pool(pick_bm(q["Cop"]), q["Cp"] % 16 == 0, idx, f32))
                    l += 1   # the MaxPool row is skipped
                else:
                    out[l].add(k_gemm(pick_bm(q["Cop"]), q["Cp"] % 16 == 0, False, True, f32))
            elif q["kind"] == "maxpool":
                out[l].add(k_plain("maxpool_kernel", f32))
            l += 1
        return out
    delta_ready = False
    for li in range(len(p) - 1, -1, -1):
        q = p[li]
        if q["kind"] == "dense":
            out[li].add("dact_rowsum_kernel<false>(double)")
        elif q["kind"] == "maxpool":
            if li > 0 and pool_fusable(p, li - 1):
                out[li].add("pool2_bwd_idx_kernel(double)")
                delta_ready = True
            elif li > 0 and p[li - 1]["kind"] == "conv":
                out[li].add("dact_rowsum_kernel<true>(double)")
                delta_ready = True
            else:
                out[li].add("maxpool_bwd_kernel(double)")
        elif q["kind"] == "conv":
            npos = q["Wo"] * q["Ho"] * b
            if not delta_ready:
                out[li].add("dact_rowsum_kernel<false>(double)")
            delta_ready = False
            if dw_narrow(q["Cop"], q["Kp"]):
                out[li].add(k_dw(64, 64, npos % 16 == 0))
            else:
                out[li].add(k_dw(pick_bm(q["Cop"]), 128, npos % 16 == 0))
            if li > 0:   # the data gradient: rows = CINp, gathered tensor = Delta with pitch COUTp
                out[li].add(k_gemm(pick_bm(q["Cp"]), q["Cop"] % 16 == 0, q["sw"] > 1 or q["sh"] > 1, False))
    return out


def all_routes(spec, whc, b, num_cu=NUM_CU, modes=None):
    """the union over the modes the GPU test runs: sample (fp64 and SI_F32), grad_forward, reverse"""
    s = set()
    for mode, f32 in modes or (("sample", False), ("sample", True), ("grad_forward", False), ("reverse", False)):
        for r in routes(spec, whc, b, mode, f32, num_cu):
            s |= r
    return s


def dw_legs(spec, whc, b, num_cu=NUM_CU):
    """{(BM, BN, NOEDGE, several splits, ragged last split)} of the weight-gradient launches of the chain"""
    legs = set()
    for q in plan(spec, whc):
        if q["kind"] == "conv":
            npos = q["Wo"] * q["Ho"] * b
            ns, ks = dw_splits(q["Cop"], q["Kp"], npos, num_cu)
            narrow = dw_narrow(q["Cop"], q["Kp"])
            legs.add((64 if narrow else pick_bm(q["Cop"]), 64 if narrow else 128, npos % 16 == 0, ns > 1, ns > 1 and npos % ks != 0))
    return legs


# ---------------------------------------------------------------------------------------------- what shapes can reach
# Read off the ladders of launch_conv_gemm / launch_conv_pool_any / launch_conv_first / launch_conv_backward_weight /
# launch_conv_backward_data / net_forward / net_backward, once for real = double and once for the -DSI_CONV_F32 build.
_BM, _TF = (64, 96, 128), (False, True)
REACHABLE_F64 = sorted(
    [k_gemm(bm, ce, False, True) for bm in _BM for ce in _TF]                     # forward, no fused pool
    + [k_gemm(bm, ce, den, False) for bm in _BM for ce in _TF for den in _TF]     # data gradient
    + [k_pool(bm, ce, idx) for bm in _BM for ce in _TF for idx in _TF]
    + [k_first(ns, ntm, idx) for ns in (5, 9) for ntm in (1, 2, 3, 4) for idx in _TF]
    + [k_dw(bm, bn, ne) for bm, bn in ((64, 64), (64, 128), (96, 128), (128, 128)) for ne in _TF]
    + ["dense_narrow_kernel<2>(double)", "maxpool_kernel(double)", "maxpool_bwd_kernel(double)", "dact_rowsum_kernel<false>(double)",
       "dact_rowsum_kernel<true>(double)", "pool2_bwd_idx_kernel(double)"])
REACHABLE_F32 = sorted(
    [k_gemm(bm, ce, False, True, True) for bm in _BM for ce in _TF]
    + [k_pool(bm, ce, False, True) for bm in _BM for ce in _TF]
    + [k_first(ns, ntm, False, True) for ns in (5, 9) for ntm in (1, 2, 3, 4)]
    + ["dense_narrow_kernel<2>(float)", "maxpool_kernel(float)"])
REACHABLE = sorted(REACHABLE_F64 + REACHABLE_F32)
# Compiled but not reachable from any shape, and why:
#   * conv_gemm_kernel<.., DEN = true, BIASACT = true>: a forward gather never divides by a stride (sden = 1 in LayerPlan::g);
#     conv_gemm_kernel<.., BIASACT = false> with double only: the data gradient exists in the fp64 build alone.
#   * (float) conv_gemm_pool_kernel / conv_first_pool_kernel with IDX = true: launch_conv_forward_pool2_idx is compiled into
#     the SI_CONV_F32 object but net_forward<float> never takes the gradient branch (`if constexpr (f64)`); si_infer_setup
#     and si_train_setup reject SI_F32 gradients on a conv chain.
#   * (float) conv_dw_kernel, maxpool_bwd_kernel, dact_rowsum_kernel, pool2_bwd_idx_kernel: behind #ifndef SI_CONV_F32.
#   * act_inplace_kernel: reached by the four later activations only, which are not exact; tests/test_gpu_conv.py runs it.
#   * mul_dact_kernel: no caller in the library (launch_mul_dact_rowsum replaced it).
# BM = 64 on more than 64 rows (conv_pick_bm from 386 rows on) is no instantiation of its own and lies beyond small chains.

# the weight-gradient legs the case list must cover at NUM_CU (narrow and the 64 x 128 tile: every combination of
# NOEDGE and one / several splits, the several with a ragged last split at least once per tile shape)
DW_LEGS_REQUIRED = ([(64, bn, ne, sev) for bn in (64, 128) for ne in _TF for sev in _TF]
                    + [(bm, 128, ne, False) for bm in (96, 128) for ne in _TF])


# ---------------------------------------------------------------------------------------------- the chains
def C(k, cout, act=R, stride=(1, 1), pad=(0, 0), dil=(1, 1)):
    return ("conv", k, cout, act, stride, pad, dil)


MP, FL = ("maxpool", (2, 2)), ("flatten",)


def D(out, act=I):
    return ("dense", out, act)


P1 = (1, 1)
# (name, (W, H, C), spec, B, instantiations the case is there for [checked by the CPU test], keyword arguments of lat.conv)
# Channels are written so that COUTp / CINp can be read off: a conv row C(k, cout, ...) has COUTp = even(cout).
CASES = [
    # ---- row classes: layer 1 sets COUTp (forward, dW), layer 2 (1 x 1) takes it as CINp (dX); 16 positions per image
    ("rows64_66", (4, 4, 3), [C((3, 3), 64, R, P1, P1), C((1, 1), 66, R), FL, D(2)], 8,
     [k_gemm(64, False, False, True), k_gemm(96, True, False, True), k_gemm(64, False, False, False), k_dw(64, 64, True),
      k_dw(96, 128, True), "dense_narrow_kernel<2>(double)", k_gemm(64, False, False, True, True), k_gemm(96, True, False, True, True),
      "dense_narrow_kernel<2>(float)"], {}),
    ("rows66_96", (4, 4, 3), [C((3, 3), 66, R, P1, P1), C((1, 1), 96, I), FL, D(4)], 5,
     [k_gemm(96, False, False, True), k_gemm(96, True, False, False), k_gemm(96, False, False, True, True)], {}),
    ("rows96_98", (4, 4, 2), [C((3, 3), 96, R, P1, P1), C((1, 1), 98, R), FL, D(2)], 3,
     [k_gemm(128, True, False, True), k_gemm(96, False, False, False), k_dw(128, 128, True), k_gemm(128, True, False, True, True)], {}),
    ("rows98_128", (4, 4, 3), [C((3, 3), 98, R, P1, P1), C((1, 1), 128, R), FL, D(2)], 7,
     [k_gemm(128, False, False, True), k_gemm(128, True, False, False), k_gemm(128, False, False, True, True)], {}),
    ("rows128_130", (4, 4, 3), [C((3, 3), 128, R, P1, P1), C((1, 1), 130, R), FL, D(2)], 4,
     [k_gemm(128, False, False, False), k_gemm(96, True, False, True)], {}),                      # 130 rows at BM 96: ragged second tile
    ("rows130_192", (4, 4, 3), [C((3, 3), 130, R, P1, P1), C((1, 1), 192, R, (2, 1)), FL, D(2)], 6,
     [k_gemm(96, True, True, False), k_gemm(96, False, False, True)], {}),                        # asymmetric stride (2, 1)
    ("rows192_194", (4, 4, 2), [C((3, 3), 192, R, P1, P1), C((1, 1), 194, R, (2, 2)), FL, D(2)], 5,
     [k_gemm(96, False, True, False), k_gemm(128, True, False, True), k_dw(128, 128, False), k_dw(96, 128, True)], {}),
    ("rows194_s2", (4, 4, 2), [C((3, 3), 194, R, P1, P1), C((1, 1), 20, R, (2, 2)), FL, D(2)], 3,
     [k_gemm(128, False, True, False), k_dw(128, 128, True), k_dw(64, 128, False)], {}),
    ("rows100_s2", (4, 4, 2), [C((3, 3), 100, R, P1, P1), C((2, 2), 16, I, (2, 2)), FL, D(2)], 5,
     [k_gemm(128, True, True, False)], {}),
    # ---- the first-layer kernel: <NS, NTM>, its edges, and the BM 64 data gradients behind it
    ("first_5_1", (4, 4, 2), [C((3, 3), 8, R, P1, P1), MP, C((1, 1), 16, R), C((1, 1), 16, I), FL, D(2)], 7,
     [k_first(5, 1, False), k_first(5, 1, True), k_first(5, 1, False, True), k_gemm(64, True, False, True), k_gemm(64, True, False, False),
      k_gemm(64, True, False, True, True), "pool2_bwd_idx_kernel(double)", k_dw(64, 64, False)], {}),
    ("first_5_2_k20", (5, 4, 10), [C((2, 1), 18, R), MP, C((2, 2), 32, R, (2, 2), P1), FL, D(2)], 6,     # Kvalid 20
     [k_first(5, 2, False), k_first(5, 2, True), k_first(5, 2, False, True), k_gemm(64, True, True, False)], {}),
    ("first_9_1_k24", (5, 4, 12), [C((2, 1), 16, R), MP, C((1, 1), 6, I, (2, 2)), FL, D(2)], 6,         # Kvalid 24
     [k_first(9, 1, False), k_first(9, 1, True), k_first(9, 1, False, True), k_gemm(64, False, True, False)], {}),
    ("first_5_3", (6, 6, 4), [C((2, 2), 34, I, (1, 1), (0, 0), (2, 2)), MP, FL, D(2)], 2,    # dilation 2: 4 x 4 out; wide ranges: no tied maxima
     [k_first(5, 3, False), k_first(5, 3, True), k_first(5, 3, False, True)], dict(x_range=32, w_range=8, seed=0)),
    ("first_5_4", (6, 6, 2), [C((3, 3), 50, I, P1, P1), MP, FL, D(2)], 5,                     # 45 windows: not a multiple of 4
     [k_first(5, 4, False), k_first(5, 4, True), k_first(5, 4, False, True)], {}),
    ("first_9_2_k36", (4, 4, 3), [C((3, 3), 32, R, P1, P1), MP, FL, D(2)], 9,
     [k_first(9, 2, False), k_first(9, 2, True), k_first(9, 2, False, True)], {}),
    ("first_9_3", (6, 4, 3), [C((3, 3), 48, R, P1, P1), MP, MP, FL, D(2)], 5,                  # a pool behind a pool
     [k_first(9, 3, False), k_first(9, 3, True), k_first(9, 3, False, True), "maxpool_bwd_kernel(double)", "maxpool_kernel(double)",
      "maxpool_kernel(float)"], {}),
    ("first_9_4_c64", (4, 4, 4), [C((3, 3), 64, R, P1, P1), MP, FL, D(16)], 8,                # COUTp 64; flatten 256 -> 16: narrow on
     [k_first(9, 4, False), k_first(9, 4, True), k_first(9, 4, False, True), "dense_narrow_kernel<2>(double)"], {}),
    ("pool96_c66", (4, 4, 4), [C((3, 3), 66, R, P1, P1), MP, FL, D(17, R), D(2)], 8,    # COUTp 66: the general kernel; 264 -> 17: narrow off
     [k_pool(96, False, False), k_pool(96, False, True), k_pool(96, False, False, True)], {}),
    ("pool64_k40", (4, 4, 10), [C((2, 2), 48, R, P1, P1, (2, 2)), MP, FL, D(2)], 5,           # Kvalid 40
     [k_pool(64, False, False), k_pool(64, False, True), k_pool(64, False, False, True)], {}),
    # pad 99 | 100 on a 2-pixel-wide image (tap offsets are packed into a byte biased by 128): dilation 99 and the stride put
    # both taps on the image at some output column; Wo = 26 | 52, most outputs see padding only
    ("first_pad99", (2, 4, 2), [C((2, 1), 8, I, (4, 1), (99, 0), (99, 1)), MP, FL, D(2)], 3,
     [k_first(5, 1, False), k_first(5, 1, True)], {}),
    ("pool_pad100", (2, 4, 2), [C((2, 1), 8, I, (2, 1), (100, 0), (99, 1)), MP, FL, D(2)], 2,
     [k_pool(64, False, False), k_pool(64, False, True)], {}),
    ("pool_dil100", (2, 4, 2), [C((2, 1), 8, I, (33, 1), (99, 0), (100, 1)), MP, FL, D(2)], 9,
     [k_pool(64, False, False), k_pool(64, False, True)], {}),
    ("odd_wo", (5, 5, 2), [C((3, 3), 8, R, P1, P1), MP, FL, D(2)], 7,                          # 5 x 5 out: the un-fused pool
     [k_gemm(64, False, False, True), "maxpool_kernel(double)", "dact_rowsum_kernel<true>(double)", k_dw(64, 64, False)], {}),
    # ---- the general fused pool kernel: BM x CELLU (x IDX by the modes); window counts that are no multiple of 4
    ("pool64_cellu", (6, 6, 16), [C((3, 3), 32, R, P1, P1), MP, FL, D(2)], 5,                 # 45 windows
     [k_pool(64, True, False), k_pool(64, True, True), k_pool(64, True, False, True), k_dw(64, 128, False)], {}),
    ("pool96_cellu", (6, 4, 16), [C((3, 3), 96, R, P1, P1), MP, FL, D(2)], 5,                 # 30 windows
     [k_pool(96, True, False), k_pool(96, True, True), k_pool(96, True, False, True)], {}),
    ("pool128", (6, 6, 3), [C((3, 3), 128, R, P1, P1), MP, FL, D(2)], 3,                     # 27 windows
     [k_pool(128, False, False), k_pool(128, False, True), k_pool(128, False, False, True)], {}),
    ("pool128_cellu", (6, 4, 16), [C((3, 3), 100, R, P1, P1), MP, FL, D(2)], 3,               # 18 windows
     [k_pool(128, True, False), k_pool(128, True, True), k_pool(128, True, False, True)], {}),
    # ---- dW: narrow (Kp 64) | 64 x 128 (Kp 80), COUTp 64 | 66, NOEDGE, one | several splits with a ragged last one
    ("dw_kp64_ragged", (4, 4, 4), [C((4, 4), 64, R, P1, (2, 2)), FL, D(2)], 17,                # 5 x 5 out x 17 = 425: ragged, 2 splits
     [k_dw(64, 64, False)], {}),
    ("dw_kp64_noedge", (4, 4, 4), [C((4, 4), 64, R, P1, (2, 2)), C((1, 1), 64, R), FL, D(2)], 32,   # 800 positions: 4 splits
     [k_dw(64, 64, True)], {}),
    ("dw_kp80", (4, 4, 8), [C((3, 3), 64, R, P1, P1), C((1, 1), 66, I), FL, D(2)], 17,        # Kp 80; 272 positions: NOEDGE, 2 splits
     [k_dw(64, 128, True), k_dw(96, 128, True)], {}),
    ("dw_kp80_ragged", (5, 5, 8), [C((3, 3), 64, R, P1, P1), FL, D(2)], 21,                    # 525 positions: 3 splits, ragged
     [k_dw(64, 128, False)], {}),
    ("dw_kp80_one", (4, 4, 8), [C((3, 3), 64, R, P1, P1), FL, D(2)], 4,
     [k_dw(64, 128, True)], {}),
    # ---- the tail: a chain starting on a pool; dense_narrow just off (in 255)
    ("pool_first", (4, 4, 2), [MP, C((2, 2), 6, R, P1, P1), FL, D(2)], 9,
     ["maxpool_bwd_kernel(double)", "maxpool_kernel(double)", k_gemm(64, False, False, False)], {}),
    ("narrow_off_255", (5, 3, 2), [C((3, 3), 17, R, P1, P1), FL, D(16)], 7,                    # flatten 255 -> 16
     [k_gemm(64, False, False, True)], {}),
]

NAMES = [c[0] for c in CASES]
assert len(set(NAMES)) == len(NAMES)


@functools.lru_cache(maxsize=4)
def problem(name, f32):
    """the lattice problem of a case (tests/lattice.py): dense weights in fp64, the SI_F32 twin with half of them zero"""
    from tests import lattice as lat
    i = NAMES.index(name)
    _, whc, spec, b, _, kw = CASES[i]
    kw = dict(kw)
    seed = kw.pop("seed", i)
    return lat.conv(spec, whc, b, m=3, ncols=2, seed=seed, f32=f32, w_density=0.5 if f32 else 1.0, **kw)


NB_TOTAL = 64   # a power of two, like every case's output width: the scale 2 / (out * nb_total) of si_train_grad is exact


def train_problem(name):
    """(table, n, w, x, y) for si_train_setup: the weights of column 0, the targets with small integer residuals"""
    pb = problem(name, False)
    return pb.table, pb.n, pb.w_swa + pb.p @ pb.z[:, 0], pb.x, pb.y1


def train_batches(b):
    """index sets of si_train_grad: the full batch in order, shuffled, and a subset whose size is no multiple of 16"""
    rng = np.random.default_rng(b)
    k = b - 1 if (b - 1) % 16 else b - 2
    return [np.arange(b), rng.permutation(b), rng.permutation(b)[:k]]
