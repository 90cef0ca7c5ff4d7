"""Which Dense kernel instantiation a chain reaches: the shape rules of csrc/kernels_gemm.hip, kernels_gemm_small.hip,
kernels_gemm_panel.hip, kernels_gemm_f32.hip, kernels_bwd.hip, kernels_bwd_f32.hip, capi.hip, capi_infer.hip and capi_train.hip
restated in plain Python, the list of instantiations shapes can reach, and the lattice chains of tests/test_gpu_dense_exact.py,
each there for the instantiations written next to it (a helper module for the tests, not a conftest; the Dense twin of
tests/conv_routes.py).

Rules restated (function here <- function there):
  pick_bm <- pick_bm (kernels_gemm.hip; 32-row tiles up to out = 32);  pick_bm_bwd <- pick_bm_bwd (kernels_bwd.hip);
  small_applies <- dense_small_applies;  slot_feats, fused_slots <- dense_fused_slot_feats, dense_fused_slots;
  panel_applies, panel_kt <- dense_panel_applies, launch_dense_f64_panel / launch_panel_inst;
  tile_vec_kedge <- launch_dense_cfg;  fuse_tail <- si_infer_setup / si_train_setup (SI_FUSE_MAX_OUT);
  batch_width <- batch_width;  maybe_narrow_class <- the width bound of fused_chain_class;
  f32_fast_shape, f32_pick_bm <- f32_fast_shape / f32_fast_ok, f32_pick_bm;
  dw_dma_ok, plan_dw <- dw_dma_ok, plan_dw;  dw_route <- launch_backward_weight and the `vec` rule of launch_gemm;
  dx_kernel <- launch_backward_data and the same rule;  rowsum_kernel <- launch_rowsum;  plan_dw_f32 <- plan_dw_f32;
  rowsum_f32_kernel <- launch_mul_dact_rowsum_f32;  forward_routes <- dense_forward;
  reverse_routes <- dense_reverse_sweep / dense_value_and_grad_f64 (with the `vec` rule of launch_tail_bwd);
  reverse_routes_f32 <- dense_value_and_grad_f32 (with launch_dense_f32_dx).
tests/test_dense_exact_cpu.py holds the restatement to the C++ text it mirrors and proves that the union of the routes of CASES
equals REACHABLE.  A kernel name is written as the kernel trace prints it, up to its argument list:
"dense_f64_kernel<96, 128, 2, 4, 4, true, false, false>" is "void si::dense_f64_kernel<96, 128, 2, 4, 4, true, false, false>(double
const*, ..." of profiles/dense_exact_kernel_names.txt.

Pointer alignment, from how the buffers are laid out (every rule below enters a `vec` / `fast` / `dma` decision):
  A1  every device buffer is an allocation of its own (DevBuf<T>::alloc = hipMalloc): its base is 256-byte aligned.  That holds
      for X, the ping-pong activations, every kept output hs[l], both Delta buffers, the split-K scratch, the fp32 twins.
  A2  the flat weight vector of chain slot s starts at base + s * pad_ld(N), pad_ld(N) a multiple of 64 elements: W of a layer
      is 16-byte aligned iff w_off is even (fp64) / w_off % 4 == 0 (fp32), its bias iff b_off is even / b_off % 4 == 0.
  A3  the activations of chain slot s start at base + s * act_elems, act_elems = pad_ld(widest stored output * B) a multiple of
      64: the slot strides cb.w, cb.hin, cb.hout are always even (and multiples of 4), with one chain and with several.
  A4  an in-order batch of si_train_grad uses X in place, any other the gathered copy Xb: both are bases (A1).
  A5  the split-K range ks of a weight gradient is a multiple of 16 by construction, so `ksplit % 2 == 0` always holds.
So on this library's own buffers every alignment test reduces to parities of out, in, w_off, b_off and B.

Not in the table: the kernels in front of the chain (reconstruct_kernel, convert_kernel<float, double>, gather_cols_kernel<double | float>), the chain-grid
kernels that take the log-density of a narrow chain (every hidden width <= 256; kernels_chain_grid.hip, held by
tests/test_gpu_lattice.py and tests/test_gpu_chain_grid.py -- for such a chain the log-density mode is left out of the route
set, see maybe_narrow_class), and the later activations (leakyrelu, elu, softplus, selu: not exact)."""
import functools

import numpy as np

from oracle import subspace_oracle as so

R, I = so.ACT_RELU, so.ACT_IDENTITY
NUM_CU = 256   # MI355X
SI_FUSE_MAX_OUT = 4
LD_ALIGN = 64


def pad_ld(n):
    return (n + LD_ALIGN - 1) // LD_ALIGN * LD_ALIGN


def _padded(v, t):
    return (v + t - 1) // t * t


# ---------------------------------------------------------------------------------------------- forward, fp64
def pick_bm(out):   # <- pick_bm, kernels_gemm.hip
    if out <= 32:
        return 32
    p96, p128, p64 = _padded(out, 96), _padded(out, 128), _padded(out, 64)
    if p96 <= p128 and p96 <= p64:
        return 96
    return 128 if p128 <= p64 else 64


def slot_feats(out):   # <- dense_fused_slot_feats
    bm = pick_bm(out)
    return 32 if bm == 32 else bm // 2


def fused_slots(out):   # <- dense_fused_slots
    bm = pick_bm(out)
    return (out + bm - 1) // bm * (1 if bm == 32 else 2)


def small_applies(out, fin, b, nchains, bm):   # <- dense_small_applies
    big = ((out + bm - 1) // bm) * ((b + 127) // 128) * max(nchains, 1)
    return big <= 128 and fin <= 2048 and out >= 1 and b >= 1


def panel_applies(w_off, out, fin, b, num_cu=NUM_CU):   # <- dense_panel_applies (identity and relu are epilogue activations)
    if fin < 1 or fin > 128 or out < 64 or out > 1024 or out % 2 != 0 or b < 1:
        return False
    if w_off % 2 != 0:   # A2
        return False
    return ((out + 15) // 16) * ((b + 127) // 128) >= 16 * 2 * num_cu


def panel_kt(fin):   # <- launch_dense_f64_panel / launch_panel_inst: (KT, ragged k)
    kt = min((fin + 15) // 16, 8)
    return kt, fin != 16 * kt


def tile_vec_kedge(out, fin, w_off, b_off, fuse):   # <- launch_dense_cfg with A1..A3
    vec = out % 2 == 0 and fin % 2 == 0 and w_off % 2 == 0 and (fuse or b_off % 2 == 0)
    return vec, fin % 16 != 0


def fuse_tail(table):   # <- si_infer_setup / si_train_setup (Dense chains of identity / relu layers)
    return len(table) >= 2 and table[-1][1] <= SI_FUSE_MAX_OUT


def maybe_narrow_class(table):
    """the width bound of fused_chain_class (capi_infer.hip): a chain that fails it never takes the chain-grid kernels; one
    that passes may (the LDS plan of chain_fused_plan is not restated)"""
    ft = fuse_tail(table)
    return all(r[1] <= 256 for r in table[:-1]) and (ft or table[-1][1] <= 256)


def batch_width(table, n, b, c, f32, num_cu=NUM_CU):   # <- batch_width + si_infer_setup (act_elems, fuse_slots, sse_blocks)
    ft = fuse_tail(table)
    stored = table[:-2] if ft else table
    act_elems = pad_ld(max([r[1] for r in stored] + [1]) * b)
    ps = 0
    if ft:
        ps = fused_slots(table[-2][1])
        if f32:
            ps = max(ps, f32_fused_slots(table[-2][1], table[-2][0], table[-2][3] % 4 == 0))
    sse_blocks = max(1, min((table[-1][1] * b + 255) // 256, 4 * num_cu))   # <- sse_num_blocks
    per = (4.0 if f32 else 8.0) * 2.0 * act_elems + 8.0 * ((ps + 1.0) * table[-1][1] * b + (1.5 if f32 else 1.0) * pad_ld(n) + sse_blocks)
    return int(max(1.0, min(float(c), float(int(2.0 * 1024 ** 3 / per)), 1024.0)))


def _b(v):
    return "true" if v else "false"


def k_tile(bm, vec, kedge, fuse):
    return "dense_f64_kernel<%d, 128, %d, 4, %d, %s, %s, %s>" % (bm, 1 if bm == 32 else 2, 2 if bm == 32 else 4, _b(vec), _b(kedge), _b(fuse))


def k_small(tm, fuse):
    return "dense_small_f64_kernel<%d, %s>" % (tm, _b(fuse))


def k_panel(kt, rag):
    return "dense_f64_panel_kernel<%d, 4, %s>" % (kt, _b(rag))


# ---------------------------------------------------------------------------------------------- forward, SI_F32
def f32_fast_shape(out, fin):   # <- f32_fast_shape
    return fin >= 16 and fin % 16 == 0 and out >= 4 and out % 4 == 0


def f32_pick_bm(out):   # <- f32_pick_bm
    return 192 if _padded(out, 192) < _padded(out, 128) else 128


def f32_fused_slots(out, fin, aligned):   # <- dense_f32_fused_slots
    if aligned and f32_fast_shape(out, fin):
        bm = f32_pick_bm(out)
        return (out + bm - 1) // bm * 2
    return (out + 63) // 64 * 2


def k_f32(out, fin, w_aligned, fuse):   # <- launch_f32_any with f32_fast_ok under A1..A3
    if f32_fast_shape(out, fin) and w_aligned:
        return "dense_f32_dma_kernel<%d, 128, 2, 4, 2, 4, %s, 16>" % (f32_pick_bm(out), _b(fuse))
    return "dense_f32_generic_kernel<%s>" % _b(fuse)


def forward_routes(table, b, nchains=1, f32=False, num_cu=NUM_CU):   # <- dense_forward (capi.hip)
    """[set of kernel names] per layer, the loss kernels with the last layer.  nchains: chain slots stacked in grid.y"""
    out = [set() for _ in table]
    ft = fuse_tail(table)
    for l, (fin, fout, _, w_off, b_off) in enumerate(table[:-2] if ft else table):
        if f32:
            out[l].add(k_f32(fout, fin, w_off % 4 == 0, False))
        elif small_applies(fout, fin, b, nchains, pick_bm(fout)):
            out[l].add(k_small(slot_feats(fout) // 16, False))
        elif nchains <= 1 and panel_applies(w_off, fout, fin, b, num_cu):
            out[l].add(k_panel(*panel_kt(fin)))
        else:
            out[l].add(k_tile(pick_bm(fout), *tile_vec_kedge(fout, fin, w_off, b_off, False), False))
    if ft:
        fin, fout, _, w_off, b_off = table[-2]
        if f32:
            out[-2].add(k_f32(fout, fin, w_off % 4 == 0, True))
        elif small_applies(fout, fin, b, nchains, pick_bm(fout)):
            out[-2].add(k_small(slot_feats(fout) // 16, True))
        else:
            out[-2].add(k_tile(pick_bm(fout), *tile_vec_kedge(fout, fin, w_off, b_off, True), True))
        out[-1] |= {"tail_sse_kernel", "sse_final_kernel"}
    else:
        out[-1] |= {"sse_partial_f32_kernel" if f32 else "sse_partial_kernel", "sse_final_kernel"}
    return out


# ---------------------------------------------------------------------------------------------- reverse, fp64
def pick_bm_bwd(rows):   # <- pick_bm_bwd
    if rows <= 64:
        return 64
    p96, p128, p64 = _padded(rows, 96), _padded(rows, 128), _padded(rows, 64)
    if p96 <= p128 and p96 <= p64:
        return 96
    return 128 if p128 <= p64 else 64


def dw_dma_ok(out, fin, b):   # <- dw_dma_ok with A1
    return b % 16 == 0 and b >= 16 and out % 2 == 0 and fin % 2 == 0 and out >= 2 and fin >= 2


DW_BM, DW_BN = (96, 128, 64, 96), (128, 128, 128, 192)


def plan_dw(out, fin, b, num_cu=NUM_CU, dma=True):   # <- plan_dw: (bm, bn, nsplit, ks)
    slots, maxsplit = num_cu * 2, (b + 255) // 256
    best, best_score = (96, 128, 1), -1.0
    for bm, bn in zip(DW_BM, DW_BN):
        if bn != 128 and not dma:
            continue
        pm, pn = (out + bm - 1) // bm, (fin + bn - 1) // bn
        tiles = pm * pn
        ns = max(1, min(slots // tiles, maxsplit))
        useful = (float(out) * fin) / (float(pm) * bm * float(pn) * bn)
        fill = float(tiles * ns) / float((tiles * ns + slots - 1) // slots * slots)
        if useful * fill > best_score * 1.0001:
            best_score, best = useful * fill, (bm, bn, ns)
    bm, bn, ns = best
    ks = ((b + ns - 1) // ns + 15) // 16 * 16
    return bm, bn, (b + ks - 1) // ks, ks


def k_gemm(bm, kfast, vec, epi):
    """gemm_f64_kernel: kfast 0 = both operands row-fast (the weight gradient, EPI_RAW = 2), 1 = k-fast (the data gradient,
    EPI_DACT = 1)"""
    return "gemm_f64_kernel<%d, 128, 2, 4, 4, %d, %d, %s, %d>" % (bm, kfast, kfast, _b(vec), epi)


def k_dw_dma(bn):
    return "dw_f64_dma_kernel<96, %d>" % bn


def rowsum_kernel(out):   # <- launch_rowsum
    return "rowsum_narrow_kernel" if out <= 8 else "rowsum_partial_kernel"


def dw_route(out, fin, b, with_db, num_cu=NUM_CU):   # <- launch_backward_weight
    """(set of kernel names, (kernel, bm, bn, nsplit, ks))"""
    dma = dw_dma_ok(out, fin, b)
    bm, bn, ns, ks = plan_dw(out, fin, b, num_cu, dma)
    s = {"split_reduce_kernel"}
    if dma and bm == 96:
        s.add(k_dw_dma(bn))
        kern = "dma"
    else:
        if with_db:
            s |= {rowsum_kernel(out), "rowsum_final_kernel"}
        s.add(k_gemm(bm, 0, out % 2 == 0 and fin % 2 == 0, 2))   # `vec` of launch_gemm with A1, A5: lda = Mrows = out, ldb = Ncols = in
        kern = "reg"
    return s, (kern, bm, bn, ns, ks)


def dx_kernel(out, fin, w_off):   # <- launch_backward_data + `vec` of launch_gemm: A = W (A2), lda = ldb = Kdim = out, ldc = Mrows = in
    return k_gemm(pick_bm_bwd(fin), 1, w_off % 2 == 0 and out % 2 == 0 and fin % 2 == 0, 1)


def reverse_routes(table, b, num_cu=NUM_CU):   # <- dense_value_and_grad_f64 behind its forward, dense_reverse_sweep
    out = [set() for _ in table]
    out[-1].add("delta_out_kernel")
    top, have_db = len(table), False
    if fuse_tail(table):
        fin, fout = table[-1][0], table[-1][1]
        out[-1] |= {rowsum_kernel(fout), "rowsum_final_kernel", "tail_bwd_kernel<%d, %d>" % (fout, 2 if fin % 2 == 0 else 1),
                    "tail_bwd_reduce_kernel"}
        top, have_db = len(table) - 1, True
    for li in range(top - 1, -1, -1):
        fin, fout, _, w_off, _ = table[li]
        out[li] |= dw_route(fout, fin, b, not (have_db and li + 1 == top), num_cu)[0]
        if li > 0:
            out[li].add(dx_kernel(fout, fin, w_off))
    return out


# ---------------------------------------------------------------------------------------------- reverse, SI_F32
def plan_dw_f32(out, fin, b, num_cu=NUM_CU):   # <- plan_dw_f32 with A1: (dma, nsplit, ks)
    dma = b % 16 == 0 and b >= 16 and out % 4 == 0 and fin % 4 == 0 and out >= 4 and fin >= 4
    tiles = ((out + 127) // 128) * ((fin + 127) // 128) if dma else (out * fin + 255) // 256
    slots, maxsplit = num_cu * (4 if dma else 16), (b + 255) // 256
    ns = max(1, min(slots // max(tiles, 1), maxsplit))
    ks = ((b + ns - 1) // ns + 15) // 16 * 16
    return dma, (b + ks - 1) // ks, ks


def rowsum_f32_kernel(rows, plain):   # <- launch_mul_dact_rowsum_f32 (plain: H == nullptr && D == nullptr; G is a base, A1)
    if plain and rows % 4 == 0:
        return "rowsum4_f32_kernel"
    if plain and rows <= 8:
        return "rowsum_narrow_f32_kernel"
    return "mul_dact_rowsum_f32_kernel"


def reverse_routes_f32(table, b, num_cu=NUM_CU):   # <- dense_value_and_grad_f32 behind its forward
    out = [set() for _ in table]
    ft = fuse_tail(table)
    out[-1].add("delta_out_f32_kernel<%s>" % ("double" if ft else "float"))
    top, have_db = len(table), False
    if ft:
        fout = table[-1][1]
        out[-1] |= {rowsum_f32_kernel(fout, True), "rowsum_final_f32_kernel", "tail_bwd_f32_kernel<%d>" % fout, "tail_bwd_reduce_f32_kernel"}
        top, have_db = len(table) - 1, True
    for li in range(top - 1, -1, -1):
        fin, fout = table[li][0], table[li][1]
        out[li] |= {"dw_f32_dma_kernel<128, 128>" if plan_dw_f32(fout, fin, b, num_cu)[0] else "dw_f32_generic_kernel", "split_reduce_f32_kernel"}
        if not have_db:
            out[li] |= {rowsum_f32_kernel(fout, True), "rowsum_final_f32_kernel"}
        if li > 0:
            # launch_dense_f32_dx: the forward kernel on W' (out' = in, in' = out; the transposed copy is a base, A1)
            fused = f32_fast_shape(fin, fout)
            out[li] |= {"transpose_f32_kernel", k_f32(fin, fout, True, False), rowsum_f32_kernel(fin, fused), "rowsum_final_f32_kernel"}
            have_db = True
    return out


# ---------------------------------------------------------------------------------------------- entry points
ENTRIES = ("forward", "logdensity", "predict", "grad", "train")


def routes(table, n, b, entry, f32=False, nchains=1, num_cu=NUM_CU):
    """the set of kernel names of one call.  forward: si_forward (one chain, per-layer launches);  logdensity: si_logdensity of
    `nchains` stacked columns (None for an fp64 chain that may be of the narrow class);  predict: si_predict of `nchains` columns on b
    new inputs (fp64 in either mode);  grad: si_logdensity_grad;  train: si_train_grad on a batch of b"""
    assert entry in ENTRIES
    if entry == "predict":
        f32 = False
    if entry == "logdensity" and not f32 and maybe_narrow_class(table):
        return None
    if entry in ("forward", "grad", "train"):
        nchains = 1
    else:
        nchains = batch_width(table, n, b, nchains, f32, num_cu)
    s = set()
    for r in forward_routes(table, b, nchains, f32, num_cu):
        s |= r
    if entry in ("grad", "train"):
        for r in (reverse_routes_f32 if f32 else reverse_routes)(table, b, num_cu):
            s |= r
        if entry == "grad":
            s |= {"ptg_partial_kernel", "ptg_final_kernel"}
    return s


# ---------------------------------------------------------------------------------------------- what shapes can reach
_TF = (False, True)
REACHABLE_F64 = sorted(
    [k_tile(bm, v, ke, fu) for bm in (32, 64, 96, 128) for v in _TF for ke in _TF for fu in _TF]
    + [k_small(tm, fu) for tm in (2, 3, 4) for fu in _TF]
    + [k_panel(kt, rag) for kt in range(1, 9) for rag in _TF]
    + [k_gemm(bm, kf, v, epi) for bm in (64, 96, 128) for v in _TF for kf, epi in ((0, 2), (1, 1))]
    + [k_dw_dma(128), k_dw_dma(192)]
    + ["tail_bwd_kernel<%d, %d>" % (ol, e) for ol in (1, 2, 3, 4) for e in (1, 2)]
    + ["tail_sse_kernel", "sse_partial_kernel", "sse_final_kernel", "delta_out_kernel", "rowsum_narrow_kernel", "rowsum_partial_kernel",
       "rowsum_final_kernel", "tail_bwd_reduce_kernel", "split_reduce_kernel", "ptg_partial_kernel", "ptg_final_kernel"])
REACHABLE_F32 = sorted(
    ["dense_f32_dma_kernel<%d, 128, 2, 4, 2, 4, %s, 16>" % (bm, _b(fu)) for bm in (128, 192) for fu in _TF]
    + ["dense_f32_generic_kernel<%s>" % _b(fu) for fu in _TF]
    + ["tail_bwd_f32_kernel<%d>" % ol for ol in (1, 2, 3, 4)]
    + ["delta_out_f32_kernel<double>", "delta_out_f32_kernel<float>", "sse_partial_f32_kernel", "dw_f32_dma_kernel<128, 128>",
       "dw_f32_generic_kernel", "split_reduce_f32_kernel", "transpose_f32_kernel", "rowsum4_f32_kernel", "rowsum_narrow_f32_kernel",
       "mul_dact_rowsum_f32_kernel", "rowsum_final_f32_kernel", "tail_bwd_reduce_f32_kernel"])
REACHABLE = sorted(REACHABLE_F64 + REACHABLE_F32)
# In the binary next to these, but reached by no shape of an identity / relu Dense chain, and why:
#   * gemm_f64_kernel<128, 64, 2, 4, 4, 0, 0, *, 2>: launch_project_mfma, the projection P = A V of wide subspaces -- no Dense
#     route; tests/test_gpu_finish_exact.py holds it.
#   * act_inplace_kernel, mul_dact_kernel, act_inplace_f32_kernel: behind act_is_extra(act), the four later activations, which
#     are not exact; tests/test_gpu_parity.py runs them.
#   * narrow_f64_f32_kernel / narrow_copy_f32_kernel: conversions at set-up, not part of a Dense route.
# The weight-gradient tiles 96 x 128 and 96 x 192 with the register-staged kernel: plan_dw offers 96 x 192 to the DMA kernel
# only, so gemm_f64_kernel has no <96, 192, ...> instantiation at all.


# ---------------------------------------------------------------------------------------------- what a case runs
PREDICT_B = 37    # columns of the new inputs si_predict gets (no multiple of 16)


def train_sizes(b):
    """batch sizes of si_train_grad: the full batch, a subset that is no multiple of 16, and a smaller batch (about half: another
    split plan wherever the plan depends on the batch)"""
    k = b - 1 if (b - 1) % 16 else b - 2
    s = b // 2 + 5
    return b, max(k, 1), min(s, b)


def train_batches(b):
    """index sets of si_train_grad: the full batch in order, shuffled, the subset and the smaller batch of train_sizes"""
    rng = np.random.default_rng(b)
    _, k, s = train_sizes(b)
    return [np.arange(b), rng.permutation(b), rng.permutation(b)[:k], rng.permutation(b)[:s]]


def all_routes(dims, acts, b, ncols=2, num_cu=NUM_CU, entries=ENTRIES, dtypes=(False, True)):
    """the union over what tests/test_gpu_dense_exact.py runs on a case: forward, log-density (one column and `ncols` stacked) and
    predict, si_logdensity_grad in fp64 and SI_F32, si_train_grad in both on every batch size of train_sizes where the chain
    trains exactly (trains_exactly)"""
    table, n = so.layer_table(dims, acts)
    s = set()
    for f32 in dtypes:
        for e in entries:
            if e == "logdensity":
                for nc in (1, ncols):
                    s |= routes(table, n, b, e, f32, nc, num_cu) or set()
            elif e == "predict":
                s |= routes(table, n, PREDICT_B, e, f32, ncols, num_cu)
            elif e == "train":
                if trains_exactly(dims):
                    for nb in train_sizes(b):
                        s |= routes(table, n, nb, e, f32, 1, num_cu)
            else:
                s |= routes(table, n, b, e, f32, 1, num_cu)
    return s


def trains_exactly(dims):
    """the scale 2 / (out * nb_total) of si_train_grad is a power of two only when the output width is: a head of 3 outputs is held
    through si_logdensity_grad alone (scale 1 / sigma^2)"""
    return dims[-1] & (dims[-1] - 1) == 0


# ---------------------------------------------------------------------------------------------- the chains
B_TILE = 16385    # one 32..128-row feature tile x 129 batch tiles > 128 big tiles: the tile kernel, not the small one; last tile 1 column
B_PANEL = 16257   # 64 sixteen-row tiles x 128 batch panels = 16 x 512 units, the least dense_panel_applies takes; last panel 1 column
B_DW = 7952       # 31 splits of 256 + one of 16: the last split is one 16-deep k tile

# (name, dims, B, instantiations the case is there for [checked by the CPU test]).  Every layer is relu but the last (identity).
# The chains are the smallest the table finds for what is written next to them, by the sum of out * in over the layers times B:
# widths from a greedy cover over the row classes (31 | 32 | 33, 64 | 65 | 66, 96 | 97 | 98), the parities that decide VEC and
# the k raggedness (in = 15 | 16 | 18), at the least batch the rule forces.
CASES = [
    # ---- the weight gradient.  plan_dw takes 64 x 128 tiles until a layer has several hundred of them (`fill` rewards more
    # tiles while slots are idle): the other plans start near out * in = 10^5 with 32 splits.
    # 130 x 902: 2 x 8 tiles of 96 x 128, ragged last row tile (34) and column tile (6) -> dw_f64_dma_kernel<96, 128>, 32 splits;
    # 1154 x 130: 13 x 1 tiles of 96 x 192, ragged (2 rows, 130 of 192 columns) -> <96, 192>, 32 splits; both with a last split of
    # one k tile.  The subset 7951: the register-staged kernel at BM 96 (130 x 902).  Least out * in * B a search over out, in
    # < 1300 and 16 | B <= 8192 finds per route: <96, 128> 1154 x 1026 x 528 (but three equal splits), <96, 192> 1154 x 130 x
    # 7440, BM 128 962 x 130 x 7952.  The chain 902 -> 130 -> 1154 reaches both DMA tiles at one batch.
    ("dw_dma", [902, 130, 1154, 2], B_DW,
     [k_dw_dma(128), k_dw_dma(192), k_gemm(96, 0, True, 2), k_gemm(96, 1, True, 1), k_tile(96, True, True, False), k_tile(64, True, True, True),
      "tail_bwd_kernel<2, 2>", "tail_bwd_f32_kernel<2>"]),
    ("dw_reg128", [130, 962, 2], B_DW, [k_gemm(128, 0, True, 2), k_tile(128, True, True, True), k_small(4, True)]),       # 962 = 7.5 x 128
    ("dw_reg128_odd", [131, 962, 1], B_DW, [k_gemm(128, 0, False, 2), k_gemm(64, 0, False, 2), k_tile(128, False, True, True),
                                           "tail_bwd_kernel<1, 2>", "tail_bwd_f32_kernel<1>"]),                          # in = 131: no 16-byte pairs
    ("dw_reg96_odd", [902, 129, 2], B_DW, [k_gemm(96, 0, False, 2), "tail_bwd_kernel<2, 1>", k_small(3, True)]),          # odd out
    # ---- SI_F32: the 192-row tile of the LDS-DMA kernel, stored and with the fused head (144 and 132 pad less to 192 than to 256)
    ("f32_bm192", [16, 144, 132, 1], 48,
     ["dense_f32_dma_kernel<192, 128, 2, 4, 2, 4, false, 16>", "dense_f32_dma_kernel<192, 128, 2, 4, 2, 4, true, 16>", "dw_f32_dma_kernel<128, 128>"]),
    # ---- small chains: the small kernel, the narrow heads 1..4 with an odd and an even input width, a wide last layer, the data
    # gradient's row classes with odd widths
    ("small_97_8_16", [3, 97, 8, 16], 17,
     ["delta_out_f32_kernel<float>", "sse_partial_f32_kernel", "sse_partial_kernel", "dense_f32_dma_kernel<128, 128, 2, 4, 2, 4, false, 16>",
      k_small(2, False), k_small(4, False), k_gemm(128, 1, False, 1), k_gemm(64, 1, True, 1), "rowsum4_f32_kernel"]),
    ("small_3_3_3", [3, 3, 3, 3], 17, ["tail_bwd_kernel<3, 1>", "tail_bwd_f32_kernel<3>", k_gemm(64, 1, False, 1)]),
    ("small_8_4", [16, 8, 4], 17, ["dense_f32_dma_kernel<128, 128, 2, 4, 2, 4, true, 16>", "tail_bwd_kernel<4, 2>", "tail_bwd_f32_kernel<4>"]),
    ("small_65_3_1", [3, 65, 3, 1], 17, [k_gemm(96, 1, False, 1), "tail_bwd_kernel<1, 1>"]),
    ("small_100_8_3", [3, 100, 8, 3], 17, [k_gemm(128, 1, True, 1), "tail_bwd_kernel<3, 2>"]),
    ("small_3_4", [3, 3, 4], 17, ["tail_bwd_kernel<4, 1>"]),
    # ---- the tile kernel: BM x VEC x KEDGE, the stored layer (layer 1) and the layer with the fused head (layer 2)
    ("tile_15_31_31", [15, 31, 31, 1], B_TILE, [k_tile(32, False, True, False), k_tile(32, False, True, True)]),
    ("tile_16_32_31", [16, 32, 31, 1], B_TILE, [k_tile(32, True, False, False), k_tile(32, False, False, True)]),
    ("tile_16_31_33", [16, 31, 33, 1], B_TILE, [k_tile(32, False, False, False), k_tile(64, False, True, True)]),
    ("tile_15_34_32", [15, 34, 32, 1], B_TILE, [k_tile(64, False, True, False), k_tile(32, True, True, True)]),
    ("tile_18_32_32", [18, 32, 32, 1], B_TILE, [k_tile(32, True, True, False), k_tile(32, True, False, True)]),
    ("tile_16_48_33", [16, 48, 33, 1], B_TILE, [k_tile(64, True, False, False), k_tile(64, False, False, True)]),
    ("tile_18_48_34", [18, 48, 34, 1], B_TILE, [k_tile(64, True, True, False), k_tile(64, True, False, True)]),
    ("tile_16_33_65", [16, 33, 65, 1], B_TILE, [k_tile(64, False, False, False), k_tile(96, False, True, True)]),
    ("tile_15_32_65", [15, 32, 65, 1], B_TILE, [k_tile(96, False, False, True)]),
    ("tile_15_66_66", [15, 66, 66, 1], B_TILE, [k_tile(96, False, True, False), k_tile(96, True, True, True)]),
    ("tile_15_32_66", [15, 32, 66, 1], B_TILE, [k_tile(96, True, False, True)]),
    ("tile_16_65_31", [16, 65, 31, 1], B_TILE, [k_tile(96, False, False, False)]),
    ("tile_16_66_31", [16, 66, 31, 1], B_TILE, [k_tile(96, True, False, False)]),
    ("tile_15_32_97", [15, 32, 97, 1], B_TILE, [k_tile(128, False, False, True)]),
    ("tile_15_32_98", [15, 32, 98, 1], B_TILE, [k_tile(128, True, False, True)]),
    ("tile_15_97_31", [15, 97, 31, 1], B_TILE, [k_tile(128, False, True, False)]),
    ("tile_16_97_31", [16, 97, 31, 1], B_TILE, [k_tile(128, False, False, False)]),
    ("tile_16_98_31", [16, 98, 31, 1], B_TILE, [k_tile(128, True, False, False)]),
    ("tile_18_98_31", [18, 98, 31, 1], B_TILE, [k_tile(128, True, True, False)]),
    # ---- the panel kernel: KT = 1..8 with the least ragged (in = 16 KT - 15) and the whole (in = 16 KT) reduction; out = 1010
    # is the least even width with 64 sixteen-row tiles (the last one 2 rows).  The panel layer is stored: the head sits two
    # layers behind it.
] + [("panel_in%d" % fin, [fin, 1010, 31, 1], B_PANEL, [k_panel(kt, fin != 16 * kt)]) for kt in range(1, 9) for fin in (16 * kt - 15, 16 * kt)]

NAMES = [c[0] for c in CASES]
assert len(set(NAMES)) == len(NAMES)
M = 3   # columns of P


def case(name):
    _, dims, b, _ = CASES[NAMES.index(name)]
    return dims, [R] * (len(dims) - 2) + [I], b


# Seeds: the position in CASES, moved on by 100 until the weight gradient is not hollow (tests/test_dense_exact_cpu.py: at least
# half of every layer's exact dW entries nonzero in fp64, no all-zero 16 x 16 block in either precision -- a ragged last row block
# of two relu units is all zero as soon as both are dead or unfed).
SEEDS = {("tile_15_32_65", True): 119, ("panel_in1", False): 130}


@functools.lru_cache(maxsize=4)
def problem(name, f32):
    """the lattice problem of a case (tests/lattice.py), every weight nonzero with probability 4/5 (fp64: [-2, 2]) or 2/3 (the
    SI_F32 twin: weights, inputs and residuals in [-1, 1], which keeps every partial sum of every case below 2^24 without thinning
    the weights)"""
    from tests import lattice as lat
    dims, acts, b = case(name)
    seed = SEEDS.get((name, f32), NAMES.index(name))
    if f32:
        return lat.dense(dims, acts, b, m=M, ncols=2, seed=seed, f32=True, w_range=1, x_range=1, r_max=1)
    return lat.dense(dims, acts, b, m=M, ncols=2, seed=seed)


def nb_total(name):
    """a power of two (like the output width of every case that trains) no smaller than the batch: the scale of si_train_grad is exact"""
    b = case(name)[2]
    return 1 << (b - 1).bit_length()


TRAIN_NAMES = [n for n in NAMES if trains_exactly(case(n)[0])]


def train_problem(name, f32):
    """(table, n, w, x, y) for si_train_setup: the weights of column 0, the targets with small integer residuals"""
    pb = problem(name, f32)
    return pb.table, pb.n, pb.w_swa + pb.p @ pb.z[:, 0], pb.x, pb.y1
