// C ABI, inference side: si_infer_setup*, the density (si_logdensity, si_forward, si_predict) and its gradient
// (si_logdensity_grad) -- reference src/space_inference.jl:88-95,107 and src/libs.jl:55-57,75-77.  Host-side orchestration only:
// every arithmetic step runs in the kernels of kernels_*.hip.  No CPU fallback anywhere in this file.  eval_density is K4, the
// optional prior sum and ONE of three routes (density_net, density_fused, density_layers); the data and workspace it runs on
// come in a DensityView (capi_common.h), so no caller steers it through the context -- si_predict hands it its own.  The per-layer passes over a
// chain are shared with the training step: dense_forward and net_forward for the density; for the gradient the whole pass --
// workspace (SweepWs, sized by sweep_ws_alloc), route and dispatch (chain_value_and_grad, capi.hip) -- and the narrow-head rule
// (head_fused).  si_logdensity_grad keeps form_weights, the prior's two launches, pull_back_to_z and the read-back.
#include "capi_common.h"
#include "chain_spec_rtc.h"

using namespace si;

extern "C" {

// =================================================================================================
// density + sampling
// =================================================================================================
// ---- narrow Dense chains: every layer in one launch (kernels_chain_grid.hip) ---------------------------------------
// The class: fp64 Dense chains with the four MFMA-epilogue activations, hidden widths <= 256 (the weights of a layer stream
// from L2 per workgroup: wide layers belong on the big-tile kernel, which shares W between 128 observations), an LDS plan that
// fits at 16 observations per workgroup, and one squared error per thread in the SSE kernels (the order the fused loop
// reproduces).  docs/src/nn_example.md:112-118 is the model this is for.
static constexpr int SI_FUSED_MAX_WIDTH = 256;
static bool fused_chain_class(const si_ctx* ctx) {
  if (ctx->setup.model.f32 || ctx->setup.model.plan.has_conv) return false;
  const int L = (int)ctx->setup.model.layers.size();
  if (L < 1 || L > SI_CHAIN_MAX_LAYERS) return false;
  for (int l = 0; l + 1 < L; ++l)
    if (ctx->setup.model.layers[(size_t)l].out > SI_FUSED_MAX_WIDTH) return false;
  if (!ctx->setup.model.fuse_tail && ctx->setup.model.layers[(size_t)L - 1].out > SI_FUSED_MAX_WIDTH) return false;
  if ((int64_t)ctx->setup.model.out_dim * ctx->setup.B > (int64_t)256 * ctx->setup.sse_blocks) return false;
  ChainFusedPlan fp;
  return chain_fused_plan(fp, ctx->setup.model.layers.data(), L, ctx->setup.B, 1, ctx->setup.model.fuse_tail,
                          ctx->setup.model.fuse_tail ? dense_fused_slot_feats(ctx->setup.model.layers[(size_t)L - 2].out) : 0, ctx->setup.model.fuse_slots) != 0;
}
// batch tile of the stacked launch (16 NB observations per workgroup; the 16-feature tiles of a layer dealt over its four
// waves).  Measured on docs/src/nn_example.md's model at 512 chains (profiles/r05_chain_grid_knockouts.log): 32 observations
// per workgroup 730 us, 16 per workgroup 780 us, one WAVE per 16-observation tile without any barrier (launch_chain_fused's
// wave_tiles form, kept for the harness) 1430 us -- a single wave's stream of small dependent steps leaves the SIMD idle.
void fused_fill_program(const si_ctx* ctx, ChainFusedPlan& fp) {
  fp.prog = ctx->loop.cgprog;
  for (int i = 0; i < 5; ++i) {
    fp.prog_start[i] = ctx->loop.cg_start[i];
    fp.prog_count[i] = ctx->loop.cg_count[i];
    fp.prog_chunks[i] = ctx->loop.cg_chunks[i];
  }
}
static size_t fused_plan_for(const si_ctx* ctx, int nchains, ChainFusedPlan& fp, int* nb_out, bool* wave_tiles) {
  fused_fill_program(ctx, fp);
  const int L = (int)ctx->setup.model.layers.size();
  const int sf = ctx->setup.model.fuse_tail ? dense_fused_slot_feats(ctx->setup.model.layers[(size_t)L - 2].out) : 0;
  *wave_tiles = false;
  for (int nb : {2, 1}) {
    const size_t lds = chain_fused_plan(fp, ctx->setup.model.layers.data(), L, ctx->setup.B, nb, ctx->setup.model.fuse_tail, sf, ctx->setup.model.fuse_slots);
    const int64_t wgs = (ctx->setup.B + 16 * nb - 1) / (16 * nb) * nchains;
    if (lds != 0 && (nb == 1 || (lds <= (size_t)80 * 1024 && wgs >= (int64_t)2 * ctx->num_cu))) {
      *nb_out = nb;
      return lds;
    }
  }
  return 0;
}

// forward workspace for `slots` chains evaluated in one launch (grid.y = chain slot)
static bool alloc_forward(si_ctx* ctx, int slots) {
  for (DevBuf<double>* b : {&ctx->fw.w, &ctx->fw.act[0], &ctx->fw.act[1], &ctx->fw.ssepart, &ctx->fw.part, &ctx->fw.yhat}) b->reset();
  for (DevBuf<float>* b : {&ctx->fw.w32, &ctx->fw.act32[0], &ctx->fw.act32[1]}) b->reset();
  ctx->fw.slots = 0;
  const size_t S = (size_t)slots, dB = (size_t)ctx->setup.model.out_dim * (size_t)ctx->setup.B;
  const bool node = ctx->node.d > 0;   // a NeuralODE set-up: its layers run inside the integration kernel, which keeps its own per-trajectory sums
  // SI_F32: fp32 weights + fp32 ping-pong activations INSTEAD of the fp64 activations (the fp64 weights stay: K4 writes
  // both, the output map / prior / gradient read them); the head partials serve both paths (the larger slot count)
  const size_t pslots = (size_t)ctx->setup.model.part_slots();
  if (!ctx->fw.w.alloc(S * (size_t)pad_ld(ctx->setup.model.N)) ||
      (!ctx->setup.model.f32 && !node && (!ctx->fw.act[0].alloc(S * (size_t)ctx->setup.act_elems) || !ctx->fw.act[1].alloc(S * (size_t)ctx->setup.act_elems))) ||
      (ctx->setup.model.f32 && (!ctx->fw.w32.alloc(S * (size_t)pad_ld(ctx->setup.model.N)) || !ctx->fw.act32[0].alloc(S * (size_t)ctx->setup.act_elems) ||
                    !ctx->fw.act32[1].alloc(S * (size_t)ctx->setup.act_elems))) ||
      (!node && !ctx->fw.ssepart.alloc(S * (size_t)ctx->setup.sse_blocks)) ||
      (ctx->setup.model.fuse_tail && !ctx->fw.part.alloc(S * pslots * dB)) ||
      ((ctx->setup.model.fuse_tail || ctx->setup.model.f32 || ctx->setup.fused_ok) && !ctx->fw.yhat.alloc(S * dB)))
    return false;
  if (!ctx->fw.wsqpart.alloc(S * (size_t)ctx->setup.wsq_blocks)) return false;
  ctx->fw.slots = slots;
  return true;
}

// where the arrays of an inference set-up live: host (si_infer_setup), device copied (si_infer_setup_dev, borrow = 0),
// device used in place (borrow = 1)
enum SetupSrc { SRC_HOST = 0, SRC_DEV_COPY = 1, SRC_DEV_BORROW = 2 };

static int32_t infer_setup_common(si_ctx* ctx, const si_layer* layers, int32_t L, int64_t N, int32_t M, const double* W_swa,
                                  const double* P, int64_t ldP_in, const double* X, const double* Y, int32_t in_dim,
                                  int32_t out_dim, int64_t B, double sigma_m, int32_t compute_dtype, SetupSrc src, int32_t node_d = 0) {
  CHECK_CTX(ctx);
  const std::string who = node_d > 0 ? "si_infer_setup_node" : "si_infer_setup";   // (the entry point the caller used, for the messages)
  if (!layers || L <= 0 || N <= 0 || M <= 0 || !X || !Y || in_dim <= 0 || out_dim <= 0 || B <= 0)
    return fail(ctx, SI_ERR_INVALID, who + ": bad argument");
  if (!(sigma_m > 0.0)) return fail(ctx, SI_ERR_INVALID, who + ": sigma_m must be positive");
  if (compute_dtype != SI_F64 && compute_dtype != SI_F32)
    return fail(ctx, SI_ERR_INVALID, who + ": compute_dtype must be SI_F64 (the reference's arithmetic) or SI_F32");
  if ((W_swa == nullptr) != (P == nullptr))
    return fail(ctx, SI_ERR_INVALID, who + ": W_swa and P must both be given or both be NULL");
  // the Chain: Dense / Conv / MaxPool / flatten layers (anything else: the reference's "model_re function is not available for this model", libs.jl:59)
  ChainModel model;
  const int32_t prc = chain_model_build(ctx, who.c_str(), layers, L, N, in_dim, out_dim, compute_dtype == SI_F32, node_d, model);
  if (prc != SI_OK) return prc;
  BIND(ctx);
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  free_infer(ctx);
  if (!W_swa) {
    if (!ctx->c_finished) return fail(ctx, SI_ERR_STATE, who + ": no finished construction to take W_swa / P from");
    if (ctx->N != N || ctx->M_built != M)
      return fail(ctx, SI_ERR_INVALID, who + ": N / M differ from the finished construction");
    ctx->setup.swa = ctx->d_swa;
    ctx->setup.P = ctx->d_P;
    ctx->setup.ldP = ctx->ldA;
  } else {
    if (src == SRC_DEV_BORROW) {
      // used in place: the caller keeps both buffers alive (and unchanged) until the next set-up / si_destroy
      ctx->setup.ldP = ldP_in;
      ctx->setup.swa = W_swa;
      ctx->setup.P = P;
    } else {
      const hipMemcpyKind kind = src == SRC_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
      ctx->setup.ldP = pad_ld(N);
      if (!ctx->setup.swa_own.alloc((size_t)ctx->setup.ldP) || !ctx->setup.P_own.alloc((size_t)ctx->setup.ldP * M)) {
        free_infer(ctx);
        return fail(ctx, SI_ERR_NOMEM, who + ": allocation of W_swa / P failed");
      }
      SI_HIP(ctx, hipMemsetAsync(ctx->setup.swa_own, 0, (size_t)ctx->setup.ldP * sizeof(double), ctx->stream));
      SI_HIP(ctx, hipMemsetAsync(ctx->setup.P_own, 0, (size_t)ctx->setup.ldP * M * sizeof(double), ctx->stream));
      SI_HIP(ctx, hipMemcpyAsync(ctx->setup.swa_own, W_swa, (size_t)N * sizeof(double), kind, ctx->stream));
      SI_HIP(ctx, hipMemcpy2DAsync(ctx->setup.P_own, (size_t)ctx->setup.ldP * sizeof(double), P, (size_t)ldP_in * sizeof(double),
                                   (size_t)N * sizeof(double), (size_t)M, kind, ctx->stream));
      ctx->setup.swa = ctx->setup.swa_own;
      ctx->setup.P = ctx->setup.P_own;
    }
  }
  ctx->node.d = node_d;   // (> 0 from here on: alloc_forward leaves the Chain kernels' activation and SSE-partial buffers out)
  InferSetup& su = ctx->setup;
  su.model = std::move(model);
  const NetPlan& plan = su.model.plan;
  su.M = M, su.B = B, su.sigma_m = sigma_m;
  su.act_elems = pad_ld(su.model.max_stored * B);
  su.sse_blocks = sse_num_blocks((int64_t)out_dim * B, ctx->num_cu);
  su.wsq_blocks = sse_num_blocks(N, ctx->num_cu);
  ctx->setup.fused_ok = node_d == 0 && fused_chain_class(ctx);   // (the chain kernels evaluate a Chain: never for a NeuralODE's right-hand side)
  if (ctx->setup.fused_ok) {   // the chain's tile program (64 bytes per 16-feature tile), uploaded once
    std::vector<CgTileD> prog;
    chain_fused_program(ctx->setup.model.layers.data(), L, ctx->setup.model.fuse_tail, prog, ctx->loop.cg_start, ctx->loop.cg_count, ctx->loop.cg_chunks);
    if (!ctx->loop.cgprog.alloc(prog.size())) {
      free_infer(ctx);
      return fail(ctx, SI_ERR_NOMEM, who + ": device allocation failed");
    }
    SI_HIP(ctx, hipMemcpy(ctx->loop.cgprog, prog.data(), prog.size() * sizeof(CgTileD), hipMemcpyHostToDevice));
  }
  if (!ctx->setup.X.alloc((size_t)in_dim * B) || !ctx->setup.Y.alloc((size_t)out_dim * B) ||
      (ctx->setup.model.f32 && !ctx->setup.X32.alloc((size_t)pad_ld(std::max<int64_t>((int64_t)in_dim * B, plan.input_spatial ? plan.in_elems * B : 0)))) ||
      (ctx->setup.model.f32 && plan.has_conv && !ctx->fw.wpack32.alloc(plan.wpack_elems)) ||
      !alloc_forward(ctx, 1) ||
      (plan.has_conv && !ctx->fw.wpack.alloc(plan.wpack_elems)) ||
      (plan.input_spatial && !ctx->setup.Xc.alloc((size_t)plan.in_elems * B))) {
    free_infer(ctx);
    return fail(ctx, SI_ERR_NOMEM, who + ": device allocation failed");
  }
  {
    const hipMemcpyKind kind = src == SRC_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    SI_HIP(ctx, hipMemcpyAsync(ctx->setup.X, X, (size_t)in_dim * B * sizeof(double), kind, ctx->stream));
    SI_HIP(ctx, hipMemcpyAsync(ctx->setup.Y, Y, (size_t)out_dim * B * sizeof(double), kind, ctx->stream));
  }
  if (plan.input_spatial) net_input(ctx, plan, ctx->setup.X, ctx->setup.Xc, B);  // (W, H, C, N) -> channel-fastest, once
  if (ctx->setup.model.f32 && plan.input_spatial)   // X rounded to fp32 once, in the layout the conv kernels read (pad channels: zero)
    launch_narrow_f32(ctx->stream, ctx->setup.Xc, ctx->setup.X32, plan.in_elems * B);
  else if (ctx->setup.model.f32)
    launch_narrow_f32(ctx->stream, ctx->setup.X, ctx->setup.X32, (int64_t)in_dim * B);   // X rounded to fp32 once
  SI_HIP(ctx, hipGetLastError());
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->setup.ready = true;
  return SI_OK;
}

int32_t si_infer_setup(si_ctx* ctx, const si_layer* layers, int32_t L, int64_t N, int32_t M, const double* W_swa,
                       const double* P, const double* X, const double* Y, int32_t in_dim, int32_t out_dim,
                       int64_t B, double sigma_m, int32_t compute_dtype) {
  return infer_setup_common(ctx, layers, L, N, M, W_swa, P, N, X, Y, in_dim, out_dim, B, sigma_m, compute_dtype, SRC_HOST);
}

// si_infer_setup_node's share of the set-up (capi_node.hip): W_swa / P, the layer table, X = the initial states, Y = the observed
// trajectories, the forward workspace -- everything but the Chain kernels' plans
int32_t infer_setup_node_base(si_ctx* ctx, const si_layer* layers, int32_t L, int64_t N, int32_t M, const double* W_swa, const double* P,
                              const double* U0, const double* Y, int32_t d, int32_t S, int64_t f) {
  return infer_setup_common(ctx, layers, L, N, M, W_swa, P, N, U0, Y, d, d * S, f, 1.0, SI_F64, SRC_HOST, d);
}

int32_t si_infer_setup_dev(si_ctx* ctx, const si_layer* layers, int32_t L, int64_t N, int32_t M, const double* W_swa_dev,
                           const double* P_dev, int64_t ldP, int32_t borrow, const double* X_dev, const double* Y_dev,
                           int32_t in_dim, int32_t out_dim, int64_t B, double sigma_m, int32_t compute_dtype) {
  CHECK_CTX(ctx);
  if (W_swa_dev && P_dev) {
    if (ldP < N) return fail(ctx, SI_ERR_INVALID, "si_infer_setup_dev: ldP < N");
    if (borrow) {
      // the streaming kernels read rows in 16-byte pairs: row N of an odd-length column must exist and be aligned
      if ((ldP & 1) || ldP < N + (N & 1) || (reinterpret_cast<uintptr_t>(P_dev) & 15u) ||
          (reinterpret_cast<uintptr_t>(W_swa_dev) & 15u))
        return fail(ctx, SI_ERR_INVALID,
                    "si_infer_setup_dev: borrowed W_swa / P need 16-byte aligned bases, an even ldP >= N + (N mod 2) and "
                    "N + (N mod 2) readable elements of W_swa");
    }
  }
  return infer_setup_common(ctx, layers, L, N, M, W_swa_dev, P_dev, ldP, X_dev, Y_dev, in_dim, out_dim, B, sigma_m,
                            compute_dtype, borrow ? SRC_DEV_BORROW : SRC_DEV_COPY);
}

int32_t si_construct_result_ptr(si_ctx* ctx, double** W_swa_dev_out, double** P_dev_out, int64_t* ld_out, int32_t* M_out) {
  CHECK_CTX(ctx);
  if (!ctx->c_finished) return fail(ctx, SI_ERR_STATE, "si_construct_result_ptr: no finished construction");
  if (W_swa_dev_out) *W_swa_dev_out = ctx->d_swa;
  if (P_dev_out) *P_dev_out = ctx->d_P;
  if (ld_out) *ld_out = ctx->ldA;
  if (M_out) *M_out = ctx->M_built;
  return SI_OK;
}

// How many chains one forward launch carries.  Small models leave most of the 256 CUs idle with one chain per launch
// (a 20-wide Dense layer on 1000 observations is 8 workgroups), so independent chains are stacked in grid.y; the
// workspace for that is capped so that a model whose single chain already fills the chip (cfg2: 1.5 GB of activations
// per chain) keeps one slot.
static int batch_width(const si_ctx* ctx, int C) {
  const InferSetup& su = ctx->setup;
  const ChainModel& cm = su.model;
  if (cm.plan.has_conv) return 1;  // chains with Conv layers fill the chip one chain at a time
  const double per = (cm.f32 ? 4.0 : 8.0) * 2.0 * (double)su.act_elems +
                     8.0 * (((double)cm.part_slots() + 1.0) * (double)cm.out_dim * (double)su.B + (cm.f32 ? 1.5 : 1.0) * (double)pad_ld(cm.N) +
                            (double)su.sse_blocks);
  const double fit = std::floor(SI_BATCH_BYTES / per);
  return (int)std::max(1.0, std::min({(double)C, fit, 1024.0}));
}

int32_t ensure_chains(si_ctx* ctx, int32_t C) {
  const int want = batch_width(ctx, C);
  if (ctx->fw.slots < want) {
    SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (!alloc_forward(ctx, want)) {
      if (!alloc_forward(ctx, 1)) {
        ctx->setup.ready = false;
        return fail(ctx, SI_ERR_NOMEM, "forward workspace allocation failed");
      }
    }
  }
  if (ctx->chains.cap >= C) return SI_OK;
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (DevBuf<double>* b : {&ctx->chains.zcur, &ctx->chains.zprop, &ctx->chains.lpcur, &ctx->chains.sse, &ctx->chains.wsq}) b->reset();
  ctx->chains.nacc.reset();
  ctx->chains.steps.reset();
  ctx->chains.cap = 0;
  if (!ctx->chains.wsq.alloc((size_t)C) || !ctx->chains.zcur.alloc((size_t)ctx->setup.M * C) || !ctx->chains.zprop.alloc((size_t)ctx->setup.M * C) ||
      !ctx->chains.lpcur.alloc((size_t)C) || !ctx->chains.sse.alloc((size_t)C) || !ctx->chains.nacc.alloc((size_t)C) || !ctx->chains.steps.alloc((size_t)C))
    return fail(ctx, SI_ERR_NOMEM, "sampler state allocation failed");
  ctx->chains.cap = C;
  return SI_OK;
}

DensityView setup_view(const si_ctx* ctx, bool defer_sse_final) {
  return {ctx->setup.X, ctx->setup.Xc, ctx->setup.X32, ctx->setup.Y, ctx->setup.B, ctx->fw.act, ctx->fw.act32, ctx->fw.ssepart, ctx->setup.sse_blocks,
          ctx->fw.part, ctx->fw.yhat, ctx->setup.act_elems, ctx->setup.model.f32, defer_sse_final, true};
}

// ---- the seam between z and the weights: W_swa + P z (K4, P' g) or, while a decoder is set, W_swa + decoder(z) ------------------
// The decoder's launches carry at most SI_DEC_CHUNK points; `hid` (every head layer's output per point) grows to the chunk.
static constexpr int32_t SI_DEC_CHUNK = 16384;
static int32_t decoder_reserve_hid(si_ctx* ctx, int32_t n) {
  DecoderState& d = ctx->dec;
  if (d.SH == 0 || d.hid_cap >= n) return SI_OK;
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (launches queued on the old buffer)
  d.hid_cap = 0;
  if (!d.hid.alloc((size_t)d.SH * (size_t)n)) return fail(ctx, SI_ERR_NOMEM, "decoder: allocation of the hidden activations failed");
  d.hid_cap = n;
  return SI_OK;
}
// decoder(z) of n <= SI_DEC_CHUNK points: w = swa + y and / or y alone (either may be null)
static int32_t decoder_forward(si_ctx* ctx, const double* z_dev, int32_t n, double* w, int64_t ldw, double* y, int64_t ldy) {
  DecoderState& d = ctx->dec;
  const int32_t rc = decoder_reserve_hid(ctx, n);
  if (rc != SI_OK) return rc;
  launch_decoder_head_fwd(ctx->stream, d.head, d.params, d.dtype, z_dev, ctx->setup.M, d.hid, d.SH, n);
  const double* a = d.D > 1 ? d.hid + d.head.hid_off[d.D - 2] : z_dev;   // the last layer's input: a_{D-1}, or z itself
  launch_decoder_last_fwd(ctx->stream, ctx->setup.swa, d.lastW, pad_ld(ctx->setup.model.N), d.lastb, d.dtype, ctx->setup.model.N, d.H, d.last_act, a,
                          d.D > 1 ? d.SH : ctx->setup.M, n, w, ldw, y, ldy, ctx->num_cu);
  return SI_OK;
}

int32_t form_weights(si_ctx* ctx, const double* z_dev, int32_t n, double* w, int64_t ldw, float* w32, bool keep_y) {
  if (!ctx->dec.on) {
    launch_reconstruct(ctx->stream, ctx->setup.swa, ctx->setup.P, ctx->setup.ldP, ctx->setup.model.N, ctx->setup.M, z_dev, n, w, ldw, ctx->num_cu, w32, ldw);
    return SI_OK;
  }
  // (w32 is never asked for here: si_infer_set_decoder refuses a set-up with compute_dtype = SI_F32)
  for (int32_t p0 = 0; p0 < n; p0 += SI_DEC_CHUNK) {
    const int32_t np = std::min(SI_DEC_CHUNK, n - p0);
    const int32_t rc = decoder_forward(ctx, z_dev + (size_t)ctx->setup.M * p0, np, w + (size_t)ldw * p0, ldw,
                                       keep_y ? ctx->dec.y.get() : nullptr, pad_ld(ctx->setup.model.N));
    if (rc != SI_OK) return rc;
  }
  return SI_OK;
}

void pull_back_to_z(si_ctx* ctx, const double* gw, double* gz) {
  DecoderState& d = ctx->dec;
  if (!d.on) {
    launch_ptg(ctx->stream, ctx->setup.P, ctx->setup.ldP, ctx->setup.model.N, ctx->setup.M, gw, ctx->grad.ptgpart, gz);
    return;
  }
  launch_decoder_last_rev(ctx->stream, d.lastW, pad_ld(ctx->setup.model.N), d.dtype, ctx->setup.model.N, d.H, d.last_act, gw, d.y, d.part, d.ga);
  launch_decoder_head_rev(ctx->stream, d.head, d.params, d.dtype, d.ga, d.H, d.hid, d.SH, gz, ctx->setup.M, 1);
}

// ---- the three routes of a density evaluation: K4 has left the weights of chain slots [c0, c0 + nc) in fw.w (and fw.w32) ------------
// Conv / MaxPool / flatten / Dense layers one after the other (capi_net.hip), ping-pong activations, one chain per pass.
// T = float is compute_dtype = SI_F32 on a Conv chain: the same pass on fp32 operands, the squared errors in fp64 with the
// fp64 outputs written beside them on request.  (the template has C++ linkage inside this extern "C" block)
static void net_sse(si_ctx* ctx, const DensityView& v, const double* last, int64_t d, int c0, DensityOutputs* out) {
  launch_sse(ctx->stream, last, v.Y, d, v.ssepart, v.sse_blocks, ctx->chains.sse + c0, 1, v.act_elems, !v.defer_sse_final);
  if (out) *out = {last, v.act_elems};
}
static void net_sse(si_ctx* ctx, const DensityView& v, const float* last, int64_t d, int c0, DensityOutputs* out) {
  launch_sse_f32(ctx->stream, last, v.Y, d, v.ssepart, v.sse_blocks, ctx->chains.sse + c0, 1, v.act_elems, out ? v.yhat : nullptr, d,
                 !v.defer_sse_final);
  if (out) *out = {v.yhat, d};
}
extern "C++" template <typename T>
static int32_t density_net(si_ctx* ctx, const DensityView& v, const T* w, const T* x, const DevBuf<T>* act, T* wpack, int c0,
                           DensityOutputs* out) {
  T* last = nullptr;
  const int32_t rc = net_forward<T>(ctx, ctx->setup.model.plan, w, x, v.B, act, wpack, /*pingpong=*/true, &last);
  if (rc != SI_OK) return rc;
  const int64_t d = (int64_t)ctx->setup.model.out_dim * v.B;
  {
    ProfScope ps(ctx, SI_K_SSE, 3.0 * (double)d, (8.0 + (double)sizeof(T)) * (double)d);
    net_sse(ctx, v, last, d, c0, out);
  }
  SI_HIP(ctx, hipGetLastError());
  return SI_OK;
}

// Narrow chain: every layer of all nc chains in ONE launch, activations in LDS; the model outputs go through the plain SSE
// kernels (one squared error per thread: the same partial sums as tail_sse_kernel's).  Its plan and tile program were built for
// the set-up's B, so a view of other data is refused.  SI_NOT_TAKEN: no LDS plan at this nc, nothing launched.
static int32_t density_fused(si_ctx* ctx, const DensityView& v, int c0, int nc) {
  if (lik_on(ctx)) return SI_NOT_TAKEN;   // (its SSE is the squared error's: the per-layer route hands the outputs to launch_lik)
  if (!v.is_setup_data) return fail(ctx, SI_ERR_STATE, "eval_density: the narrow-chain launch is built for the set-up's own data");
  const int64_t N = ctx->setup.model.N, B = v.B, ldw = pad_ld(N);
  const double dn = (double)nc;
  ChainFusedPlan fp;
  int nb = 1;
  bool wave_tiles = false;
  const size_t lds = fused_plan_for(ctx, nc, fp, &nb, &wave_tiles);
  if (lds == 0) return SI_NOT_TAKEN;
  const int64_t d = (int64_t)ctx->setup.model.out_dim * B;
  {
    const double fl = 2.0 * (double)N * (double)B * dn;
    const double by = ((double)N * dn + (double)ctx->setup.model.in_dim * (double)B + (double)d * dn) * 8.0;
    ProfScope ps(ctx, SI_K_DENSE, fl, by);
    ProfScope pm(ctx, SI_K_DENSE_MAIN, fl, by);
    const SpecKernels* sk = nullptr;
    if (ctx->chain_spec && ctx->setup.model.fuse_tail)   // the same kernel compiled for this chain's shapes (chain_spec_rtc.cpp; same bits)
      sk = spec_kernels(ctx->setup.model.layers.data(), (int)ctx->setup.model.layers.size(), nb, dense_fused_slot_feats(ctx->setup.model.layers[ctx->setup.model.layers.size() - 2].out), 0, false,
                        &ctx->spec_message);
    ctx->loop.last_density_spec = sk != nullptr;
    if (sk) {
      const double* wp = ctx->fw.w;
      const double* xp = v.X;
      double* yp = v.yhat;
      long long ws = ldw, ys = d;
      int Bi = (int)B;
      void* args[] = {&wp, &ws, &xp, &yp, &ys, &Bi};
      if (sk->stack && nc >= 16) {
        // many chains: a wave per 16 observations with the activations in registers and the chain's weights in LDS, no barrier
        // between layers (329 against 495 us at 512 chains of the nn_example model, 48 against 71 at 64; 24 against 14 at 8)
        const int splits = nc >= ctx->num_cu ? 1 : std::min(8, (ctx->num_cu + nc - 1) / nc);
        SI_HIP(ctx, hipModuleLaunchKernel(sk->stack, (unsigned)splits, (unsigned)nc, 1, 512, 1, 1,
                                          (unsigned)((size_t)sk->wvec_doubles * sizeof(double)), ctx->stream, args, nullptr));
      } else {
        SI_HIP(ctx, hipModuleLaunchKernel(sk->fused, (unsigned)((B + 16 * nb - 1) / (16 * nb)), (unsigned)nc, 1, 256, 1, 1,
                                          (unsigned)((size_t)sk->lds_doubles * sizeof(double)), ctx->stream, args, nullptr));
      }
    } else {
      launch_chain_fused(ctx->stream, fp, nb, wave_tiles, lds, ctx->fw.w, ldw, v.X, v.yhat, d, nc);
    }
  }
  {
    ProfScope ps(ctx, SI_K_SSE, 3.0 * (double)d * dn, 16.0 * (double)d * dn);
    launch_sse(ctx->stream, v.yhat, v.Y, d, v.ssepart, v.sse_blocks, ctx->chains.sse + c0, nc, d, !v.defer_sse_final);
  }
  SI_HIP(ctx, hipGetLastError());
  return SI_OK;
}

// The per-layer launches (dense_forward), nc chain slots per launch, outputs ping-pong.  compute_dtype = SI_F32 runs them on the
// fp32 matrix instruction (kernels_gemm_f32.hip): K4 has left W_swa + P z in fw.w (fp64) AND rounded once in fw.w32; X32 /
// activations are fp32; the narrow head's partial sums, the last bias + activation (tail_sse_kernel) and the sum of squared
// errors are fp64 -- the precision option of SURVEY section 0 Q6 on the same reference lines, src/space_inference.jl:92-94
static int32_t density_layers(si_ctx* ctx, const DensityView& v, int c0, int nc, DensityOutputs* out) {
  const ChainModel& cm = ctx->setup.model;
  const int64_t B = v.B, ldw = pad_ld(cm.N), d = (int64_t)cm.out_dim * B;
  const int slots = v.f32 ? cm.fuse_slots32 : cm.fuse_slots;
  ChainBatch cb;
  cb.n = nc;
  cb.w = ldw;
  cb.hout = v.act_elems;
  cb.part = (int64_t)slots * d;
  // the outputs: v.yhat, slots out_dim * B apart, behind the fused tail and on the fp32 route (the fp64 copy); else the last activation buffer
  DensityOutputs o{v.yhat, d};
  double* yhat = out ? v.yhat : nullptr;
  if (v.f32) {
    const DenseForward<float> fw{&cm, ctx->fw.w32, ctx->fw.w, v.X32, v.Y, B, nullptr, {v.act32[0], v.act32[1]}, cb, slots, v.part, yhat,
                                 v.ssepart, v.sse_blocks, ctx->chains.sse + c0, v.defer_sse_final, true, true};
    dense_forward(ctx, ctx->stream, fw);
  } else {
    const DenseForward<double> fw{&cm, ctx->fw.w, ctx->fw.w, v.X, v.Y, B, nullptr, {v.act[0], v.act[1]}, cb, slots, v.part, yhat,
                                  v.ssepart, v.sse_blocks, ctx->chains.sse + c0, v.defer_sse_final, true, true};
    const double* h = dense_forward(ctx, ctx->stream, fw);
    if (!cm.fuse_tail) o = {h, v.act_elems};
  }
  SI_HIP(ctx, hipGetLastError());
  if (out) *out = o;
  return SI_OK;
}

// the route of the chain set up: Conv, the one-launch narrow chain, or the per-layer launches
static int32_t density_route(si_ctx* ctx, const DensityView& v, int c0, int nc, DensityOutputs* out) {
  if (ctx->setup.model.plan.has_conv)
    return v.f32 ? density_net<float>(ctx, v, ctx->fw.w32, v.X32, v.act32, ctx->fw.wpack32, c0, out)
                 : density_net<double>(ctx, v, ctx->fw.w, ctx->setup.model.plan.input_spatial ? v.Xc : v.X, v.act, ctx->fw.wpack, c0, out);
  if (ctx->setup.fused_ok && ctx->chain_mode != 0 && !out) {   // (never with compute_dtype = SI_F32: fused_chain_class)
    const int32_t rc = density_fused(ctx, v, c0, nc);
    if (rc != SI_NOT_TAKEN) return rc;
  }
  return density_layers(ctx, v, c0, nc, out);
}

// density evaluations for chain slots [c0, c0 + nc), nc <= fw.slots, in ONE pass of launches:
// chains.zprop[:, c] -> chains.sse[c]; optionally leaves the model outputs where *out says
int32_t eval_density(si_ctx* ctx, const DensityView& v, int c0, int nc, DensityOutputs* out) {
  ctx->loop.last_density_spec = 0;   // (si_chain_kernel_info reports the last evaluation)
  if (ctx->node.on) return node_density(ctx, v, c0, nc, out);   // form_weights, ||W||^2, the integrations (capi_node.hip)
  const int64_t N = ctx->setup.model.N, ldw = pad_ld(N);
  const int32_t M = ctx->setup.M;
  const double dn = (double)nc;
  {
    ProfScope ps(ctx, SI_K_RECON, 2.0 * (double)N * M * dn, (double)N * (M + 1 + dn) * 8.0);
    const int32_t rc = form_weights(ctx, ctx->chains.zprop + (size_t)c0 * M, nc, ctx->fw.w, ldw, v.f32 ? ctx->fw.w32.get() : nullptr);
    if (rc != SI_OK) return rc;
  }
  if (ctx->setup.sigma_p > 0.0)  // ||new_W||^2 per chain for the optional prior term (same fixed-order reduction as the SSE)
    launch_sse(ctx->stream, ctx->fw.w, nullptr, N, ctx->fw.wsqpart, ctx->setup.wsq_blocks, ctx->chains.wsq + c0, nc, ldw);
  // A categorical / Bernoulli likelihood (si_infer_set_likelihood) reads the model outputs of the set-up's data: the Conv route and
  // the per-layer route run as they are with the outputs requested (which keeps density_fused away), and launch_lik overwrites the
  // squared errors' partials and sum.
  const bool lik = lik_on(ctx) && v.is_setup_data;
  DensityOutputs o_lik;
  DensityOutputs* yo = lik && !out ? &o_lik : out;
  const int32_t rc = density_route(ctx, v, c0, nc, yo);
  if (rc != SI_OK || !lik) return rc;
  {
    const int64_t d = (int64_t)ctx->setup.model.out_dim * v.B;
    ProfScope ps(ctx, SI_K_SSE, 8.0 * (double)d * dn, 8.0 * (double)d * (dn + 1.0));
    launch_lik(ctx->stream, ctx->setup.lik, v.Y, yo->p, yo->stride, ctx->setup.model.out_dim, v.B, v.ssepart, v.sse_blocks, ctx->chains.sse + c0, nc,
               !v.defer_sse_final);
  }
  SI_HIP(ctx, hipGetLastError());
  return SI_OK;
}

// all C chain slots, fw.slots at a time
int32_t eval_density_all(si_ctx* ctx, const DensityView& v, int C) {
  const int w = std::max(1, ctx->fw.slots);
  for (int c0 = 0; c0 < C; c0 += w) {
    const int32_t rc = eval_density(ctx, v, c0, std::min(w, C - c0), nullptr);
    if (rc != SI_OK) return rc;
  }
  return SI_OK;
}

double mvnormal_c0(double d, double sigma) {
  // Distributions.mvnormal_c0: -(d*log(2pi) + logdet(Sigma))/2 with logdet = d*log(sigma^2)
  return -(d * std::log(2.0 * 3.14159265358979323846) + d * std::log(sigma * sigma)) / 2.0;
}

// log N(w; 0, sigma_p^2 I) = c0p - ||w||^2 / (2 sigma_p^2): the term the reference writes AFTER its `return` (Q4)
double prior_c0(const si_ctx* ctx) { return ctx->setup.sigma_p > 0.0 && !ctx->node.on ? mvnormal_c0((double)ctx->setup.model.N, ctx->setup.sigma_p) : 0.0; }
// The constants of lp = c0 - (sse / s2) / 2 [+ prior_c0 - (wsq / sp2) / 2].  A NeuralODE set-up (reference
// src/space_inference.jl:96-101: lp = -sse - ||W||^2, sigma_m and sigma_p unused) is c0 = 0, s2 = 1/2, the prior term on (the set-up
// holds sigma_p at 1), prior_c0 = 0, sp2 = 1/2: every division is exact, so the RWMH kernels carry it with these constants alone.
// A categorical / Bernoulli likelihood (si_infer_set_likelihood) likewise: chains.sse holds the negative log-likelihood, c0 = 0 and
// s2 = 1/2 make lp = -nll exactly; sigma_m is unused, the prior term is the Chain's.
double lik_c0(const si_ctx* ctx, double d) { return ctx->node.on || lik_on(ctx) ? 0.0 : mvnormal_c0(d, ctx->setup.sigma_m); }
double lik_s2(const si_ctx* ctx) { return ctx->node.on || lik_on(ctx) ? 0.5 : ctx->setup.sigma_m * ctx->setup.sigma_m; }
double prior_sp2(const si_ctx* ctx) { return ctx->node.on ? 0.5 : ctx->setup.sigma_p * ctx->setup.sigma_p; }

// the value of the log-density from the device's sums, as the host forms it: lp = c0 - (sse / s2) / 2 [+ prior_c0 - (wsq / sp2) / 2]
static double lp_from_sums(const si_ctx* ctx, double sse, double wsq) {
  const double c0 = lik_c0(ctx, (double)ctx->setup.model.out_dim * (double)ctx->setup.B), s2 = lik_s2(ctx);
  double lp = c0 - (sse / s2) / 2.0;
  if (ctx->setup.sigma_p > 0.0) lp += prior_c0(ctx) - (wsq / prior_sp2(ctx)) / 2.0;
  return lp;
}

int32_t si_infer_set_prior(si_ctx* ctx, double sigma_p) {
  CHECK_CTX(ctx);
  int32_t rc = need_setup(ctx, "si_infer_set_prior");
  if (rc != SI_OK) return rc;
  if (ctx->node.on) return fail(ctx, SI_ERR_INVALID, "si_infer_set_prior: not available for NeuralODE models (their density carries -||W||^2 itself)");
  if ((rc = no_session(ctx, "si_infer_set_prior", SESSION_SETTING)) != SI_OK) return rc;
  if (!(sigma_p >= 0.0)) return fail(ctx, SI_ERR_INVALID, "si_infer_set_prior: sigma_p must be >= 0 (0 = off, the reference's behaviour)");
  ctx->setup.sigma_p = sigma_p;
  return SI_OK;
}

int32_t si_infer_set_likelihood(si_ctx* ctx, int32_t kind) {
  CHECK_CTX(ctx);
  const int32_t rc = infer_entry_check(ctx, "si_infer_set_likelihood", nullptr, SESSION_SETTING);
  if (rc != SI_OK) return rc;
  if (kind < 0 || kind > 2) return fail(ctx, SI_ERR_INVALID, "si_infer_set_likelihood: kind must be 0 gaussian, 1 categorical or 2 bernoulli");
  if (ctx->node.on) return fail(ctx, SI_ERR_INVALID, "si_infer_set_likelihood: not available for NeuralODE models (their density is the sum of squared errors of the trajectories)");
  ctx->setup.lik = kind;
  return SI_OK;
}

int32_t si_infer_likelihood_info(si_ctx* ctx, int32_t* kind_out) {
  CHECK_CTX(ctx);
  if (!kind_out) return fail(ctx, SI_ERR_INVALID, "si_infer_likelihood_info: bad argument");
  *kind_out = ctx->setup.ready ? ctx->setup.lik : 0;
  return SI_OK;
}

// the decoder's last layer as the streaming kernels read it: W (N x H) with its columns ldD apart, b, both with zero padding rows
extern "C++" template <typename T>
static bool decoder_upload(si_ctx* ctx, DecoderState& d, const si_layer& last, const void* wdec, int64_t Nd, int64_t N, int64_t ldD) {
  const T* src = static_cast<const T*>(wdec);
  std::vector<T> Wp((size_t)ldD * (size_t)last.in, T(0)), bp((size_t)ldD, T(0));
  for (int32_t h = 0; h < last.in; ++h)
    std::memcpy(Wp.data() + (size_t)ldD * h, src + last.w_off + (int64_t)N * h, (size_t)N * sizeof(T));
  std::memcpy(bp.data(), src + last.b_off, (size_t)N * sizeof(T));
  return d.params.alloc((size_t)Nd * sizeof(T)) && d.lastW.alloc(Wp.size() * sizeof(T)) && d.lastb.alloc(bp.size() * sizeof(T)) &&
         hipMemcpy(d.params, src, (size_t)Nd * sizeof(T), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d.lastW, Wp.data(), Wp.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d.lastb, bp.data(), bp.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
}

int32_t si_infer_set_decoder(si_ctx* ctx, const si_layer* dec_layers, int32_t D, int64_t Nd, const void* wdec_host, int32_t wdec_dtype) {
  CHECK_CTX(ctx);
  const int32_t rc = infer_entry_check(ctx, "si_infer_set_decoder", nullptr, SESSION_SETTING);
  if (rc != SI_OK) return rc;
  BIND(ctx);
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (!dec_layers && D == 0) {   // clear: the P route returns
    ctx->dec = DecoderState();
    return SI_OK;
  }
  auto bad = [&](const char* what) { return fail(ctx, SI_ERR_INVALID, std::string("si_infer_set_decoder: ") + what); };
  if (!dec_layers || D < 1 || D > SI_DEC_MAX_LAYERS || Nd <= 0 || !wdec_host) return bad("bad argument (1 <= D <= 8 layers, Nd > 0, parameters given)");
  if (wdec_dtype != SI_F32 && wdec_dtype != SI_F64) return bad("wdec_dtype must be SI_F32 or SI_F64");
  if (ctx->setup.model.f32) return bad("the set-up's compute_dtype is SI_F32: the fp32 weight vector is not fed on the decoder route (set up with SI_F64)");
  const int64_t N = ctx->setup.model.N;
  if (ctx->setup.M > 1024) return bad("M exceeds 1024");
  for (int32_t l = 0; l < D; ++l) {
    const si_layer& ly = dec_layers[l];
    if (ly.kind != SI_LAYER_DENSE) return bad("every decoder layer must be SI_LAYER_DENSE");
    if (ly.in < 1 || ly.out < 1) return bad("layer widths must be positive");
    if (ly.act < 0 || ly.act >= SI_ACT_COUNT) return bad("unknown activation");
    if (l == 0 && ly.in != ctx->setup.M) return bad("the first layer's `in` differs from the set-up's M");
    if (l > 0 && ly.in != dec_layers[l - 1].out) return bad("consecutive layer widths do not chain");
    if (l == D - 1 && ly.out != N) return bad("the last layer's `out` differs from the set-up's N");
    if (l < D - 1 && ly.out > 1024) return bad("a hidden width exceeds 1024");
    const int64_t wn = (int64_t)ly.in * ly.out;
    if (ly.w_off < 0 || ly.w_off > Nd - wn || ly.b_off < 0 || ly.b_off > Nd - ly.out) return bad("a layer's offset range falls outside [0, Nd)");
  }
  DecoderState d;
  d.D = D, d.dtype = wdec_dtype, d.H = dec_layers[D - 1].in, d.last_act = dec_layers[D - 1].act;
  d.head.n = D - 1;
  for (int32_t l = 0; l < D - 1; ++l) {
    const si_layer& ly = dec_layers[l];
    d.head.in[l] = ly.in, d.head.out[l] = ly.out, d.head.act[l] = ly.act, d.head.hid_off[l] = d.SH;
    d.head.w_off[l] = ly.w_off, d.head.b_off[l] = ly.b_off;
    d.SH += ly.out;
  }
  const int64_t ldD = pad_ld(N);
  const bool up = wdec_dtype == SI_F32 ? decoder_upload<float>(ctx, d, dec_layers[D - 1], wdec_host, Nd, N, ldD)
                                       : decoder_upload<double>(ctx, d, dec_layers[D - 1], wdec_host, Nd, N, ldD);
  if (!up || !d.y.alloc((size_t)ldD) || !d.part.alloc((size_t)decoder_rev_blocks() * (size_t)d.H) || !d.ga.alloc((size_t)d.H))
    return fail(ctx, SI_ERR_NOMEM, "si_infer_set_decoder: device allocation / upload failed");   // (the decoder set before stays)
  d.on = true;
  ctx->dec = std::move(d);
  return SI_OK;
}

int32_t si_infer_decoder_info(si_ctx* ctx, int32_t* D_out, int32_t* H_out, int32_t* storage_dtype_out) {
  CHECK_CTX(ctx);
  if (D_out) *D_out = ctx->dec.on ? ctx->dec.D : 0;
  if (H_out) *H_out = ctx->dec.on ? ctx->dec.H : 0;
  if (storage_dtype_out) *storage_dtype_out = ctx->dec.on ? ctx->dec.dtype : SI_F64;
  return SI_OK;
}

int32_t si_decode(si_ctx* ctx, const double* Z, int64_t C, double* Y_out) {
  CHECK_CTX(ctx);
  if (need_setup(ctx, "si_decode") != SI_OK) return SI_ERR_STATE;
  if (!ctx->dec.on) return fail(ctx, SI_ERR_STATE, "si_decode: no decoder is set (si_infer_set_decoder)");
  if (!Z || C <= 0 || !Y_out) return fail(ctx, SI_ERR_INVALID, "si_decode: bad argument");
  BIND(ctx);
  const int64_t N = ctx->setup.model.N, ldy = pad_ld(N);
  const int32_t M = ctx->setup.M;
  // a test and audit read-back, not a hot path: groups of at most 64 points (~32 MB of output), one synchronisation per group
  const int64_t group = std::max<int64_t>(1, std::min<int64_t>(64, ((int64_t)32 << 20) / (N * 8)));
  DevBuf<double> dZ, dY;
  if (!dZ.alloc((size_t)M * (size_t)group) || !dY.alloc((size_t)ldy * (size_t)group)) return fail(ctx, SI_ERR_NOMEM, "si_decode: device allocation failed");
  for (int64_t c0 = 0; c0 < C; c0 += group) {
    const int32_t nc = (int32_t)std::min(group, C - c0);
    SI_HIP(ctx, hipMemcpyAsync(dZ, Z + c0 * M, (size_t)M * nc * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    const int32_t rc = decoder_forward(ctx, dZ, nc, nullptr, 0, dY, ldy);
    if (rc != SI_OK) return rc;
    SI_HIP(ctx, hipGetLastError());
    SI_HIP(ctx, hipMemcpy2DAsync(Y_out + c0 * N, (size_t)N * sizeof(double), dY, (size_t)ldy * sizeof(double), (size_t)N * sizeof(double),
                                 (size_t)nc, hipMemcpyDeviceToHost, ctx->stream));
    SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return SI_OK;
}

// gz = J_decoder(z)' gy at one point, through the seam alone: form_weights(.., keep_y = true) and pull_back_to_z are, launch for
// launch, what si_logdensity_grad runs around its model sweep; chains.zprop, fw.w, grad.gw and grad.gz are the buffers it uses.
int32_t si_decode_vjp(si_ctx* ctx, const double* z, const double* gy, double* gz_out) {
  CHECK_CTX(ctx);
  if (!z || !gy || !gz_out) return fail(ctx, SI_ERR_INVALID, "si_decode_vjp: bad argument");
  if (need_setup(ctx, "si_decode_vjp") != SI_OK) return SI_ERR_STATE;
  if (!ctx->dec.on) return fail(ctx, SI_ERR_STATE, "si_decode_vjp: no decoder is set (si_infer_set_decoder)");
  int32_t rc = no_session(ctx, "si_decode_vjp", SESSION_SHARED);
  if (rc != SI_OK) return rc;
  BIND(ctx);
  if ((rc = ensure_chains(ctx, 1)) != SI_OK) return rc;
  const int64_t N = ctx->setup.model.N;
  const int32_t M = ctx->setup.M;
  if (!ctx->grad.gw.reserve((size_t)pad_ld(N)) || !ctx->grad.gz.reserve((size_t)M)) return fail(ctx, SI_ERR_NOMEM, "si_decode_vjp: device allocation failed");
  SI_HIP(ctx, hipMemcpyAsync(ctx->chains.zprop, z, (size_t)M * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  SI_HIP(ctx, hipMemcpyAsync(ctx->grad.gw, gy, (size_t)N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if ((rc = form_weights(ctx, ctx->chains.zprop, 1, ctx->fw.w, pad_ld(N), nullptr, /*keep_y=*/true)) != SI_OK) return rc;
  pull_back_to_z(ctx, ctx->grad.gw, ctx->grad.gz);
  SI_HIP(ctx, hipGetLastError());
  SI_HIP(ctx, hipMemcpyAsync(gz_out, ctx->grad.gz, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SI_OK;
}

int32_t si_logdensity(si_ctx* ctx, const double* Z, int32_t C, double* lp_out) {
  CHECK_CTX(ctx);
  int32_t rc = infer_entry_check(ctx, "si_logdensity", bad_if(!Z || C <= 0 || !lp_out));
  if (rc != SI_OK) return rc;
  BIND(ctx);
  if ((rc = ensure_chains(ctx, C)) != SI_OK) return rc;
  SI_HIP(ctx, hipMemcpyAsync(ctx->chains.zprop, Z, (size_t)ctx->setup.M * C * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if ((rc = eval_density_all(ctx, setup_view(ctx), C)) != SI_OK) return rc;
  std::vector<double> sse((size_t)C), wsq((size_t)C, 0.0);
  SI_HIP(ctx, hipMemcpyAsync(sse.data(), ctx->chains.sse, (size_t)C * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (ctx->setup.sigma_p > 0.0)
    SI_HIP(ctx, hipMemcpyAsync(wsq.data(), ctx->chains.wsq, (size_t)C * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int c = 0; c < C; ++c) lp_out[c] = lp_from_sums(ctx, sse[(size_t)c], wsq[(size_t)c]);
  return SI_OK;
}

// a gradient workspace that could not be allocated in full is dropped whole
static int32_t drop_grad(si_ctx* ctx) {
  ctx->grad = InferGrad();
  return fail(ctx, SI_ERR_NOMEM, "si_logdensity_grad: workspace allocation failed");
}

static int32_t ensure_grad(si_ctx* ctx) {
  InferGrad& g = ctx->grad;
  if (g.ws.ready) return SI_OK;
  if (ctx->setup.model.plan.has_conv && ctx->setup.model.f32)
    return fail(ctx, SI_ERR_INVALID, "si_logdensity_grad: compute_dtype = SI_F32 has a reverse sweep for Dense chains only; set a Conv chain up with SI_F64 for gradients");
  if (!sweep_ws_alloc(ctx, g.ws, ctx->setup.model, ctx->setup.B) ||
      !g.gw.alloc((size_t)pad_ld(ctx->setup.model.N)) || !g.ptgpart.alloc((size_t)ptg_blocks() * ctx->setup.M) || !g.gz.alloc((size_t)ctx->setup.M) ||
      !g.likpart.alloc((size_t)SI_COST_MAX_BLOCKS))
    return drop_grad(ctx);
  return SI_OK;
}

// value and gradient at ONE point through the per-layer launches (synchronises): the body of si_logdensity_grad, and what
// si_logdensity_grad_batch and StackedVgrad walk column by column for every chain outside the fused class (checked and bound
// by the caller)
static int32_t logdensity_grad_point(si_ctx* ctx, const double* z, double* lp_out, double* grad_out) {
  int32_t rc = ensure_chains(ctx, 1);
  if (rc != SI_OK) return rc;
  if (ctx->node.on) return node_grad_point(ctx, z, lp_out, grad_out);   // the discrete adjoint through the solver (capi_node.hip)
  if ((rc = ensure_grad(ctx)) != SI_OK) return rc;
  const int64_t N = ctx->setup.model.N, B = ctx->setup.B;
  const int32_t M = ctx->setup.M;
  const double s2 = ctx->setup.sigma_m * ctx->setup.sigma_m;
  SI_HIP(ctx, hipMemcpyAsync(ctx->chains.zprop, z, (size_t)M * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  {
    ProfScope ps(ctx, SI_K_RECON, 2.0 * (double)N * M, (double)N * (M + 2) * 8.0);
    if ((rc = form_weights(ctx, ctx->chains.zprop, 1, ctx->fw.w, pad_ld(N), ctx->setup.model.f32 ? ctx->fw.w32.get() : nullptr, /*keep_y=*/true)) != SI_OK)
      return rc;
  }
  const bool prior = ctx->setup.sigma_p > 0.0;
  if (prior) launch_sse(ctx->stream, ctx->fw.w, nullptr, N, ctx->fw.wsqpart, ctx->setup.wsq_blocks, ctx->chains.wsq, 1, pad_ld(N));
  // d (-SSE / (2 sigma^2)) / dw into grad.gw and the SSE into chains.sse by the chain's route: Delta_L = d lp / d yhat = (y - yhat) / sigma^2.
  // compute_dtype = SI_F32: on the fp32 density's own arithmetic (W_swa + P z rounded once); P' g and the prior term stay fp64.
  // A categorical / Bernoulli likelihood: the training step's cost tail with inv_denom = -1, so that Delta_L = -d nll / d yhat .*
  // act' = d lp / d yhat and the numerator -- the negative log-likelihood -- lands in chains.sse (lp = -nll through lik_c0 / lik_s2)
  const CostTail lik_tail{ctx->setup.lik == 1 ? SI_COST_LOGITCE : SI_COST_LOGITBCE, 0.0, -1.0, ctx->grad.likpart};
  double bflops = 0.0;   // (what a Conv chain reports for its SI_K_BACKWARD scope)
  for (const auto& q : ctx->setup.model.plan.L)
    bflops += q.kind == SI_LAYER_DENSE ? 4.0 * (double)q.in_feat * q.out_feat * (double)B
              : q.kind == SI_LAYER_CONV ? 4.0 * (double)q.KW * q.KH * q.C * q.Co * (double)q.Wo * q.Ho * (double)B : 0.0;
  const ChainValueGrad in{&ctx->setup.model, ctx->fw.w, ctx->fw.w32, ctx->setup.X, ctx->setup.Xc, ctx->setup.X32, ctx->setup.Y, B, ctx->fw.part,
                          ctx->fw.ssepart, ctx->chains.sse, ctx->setup.sse_blocks, ctx->grad.gw, ctx->fw.wpack, 1.0 / s2,
                          lik_on(ctx) ? &lik_tail : nullptr, true, bflops};
  if ((rc = chain_value_and_grad(ctx, ctx->stream, ctx->grad.ws, in)) != SI_OK) return rc;
  if (prior) launch_prior_grad(ctx->stream, ctx->grad.gw, ctx->fw.w, N, 1.0 / (ctx->setup.sigma_p * ctx->setup.sigma_p), ctx->num_cu);
  pull_back_to_z(ctx, ctx->grad.gw, ctx->grad.gz);
  SI_HIP(ctx, hipGetLastError());
  double sse = 0.0, wsq = 0.0;
  SI_HIP(ctx, hipMemcpyAsync(&sse, ctx->chains.sse, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  SI_HIP(ctx, hipMemcpyAsync(grad_out, ctx->grad.gz, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (prior) SI_HIP(ctx, hipMemcpyAsync(&wsq, ctx->chains.wsq, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *lp_out = lp_from_sums(ctx, sse, wsq);
  return SI_OK;
}

int32_t need_setup(si_ctx* ctx, const char* who) {
  return ctx->setup.ready ? SI_OK : fail(ctx, SI_ERR_STATE, std::string(who) + ": call si_infer_setup first");
}
int32_t no_session(si_ctx* ctx, const char* who, SessionRule rule) {
  if (rule == SESSION_ANY || !ctx->chains.session.open()) return SI_OK;
  return fail(ctx, SI_ERR_STATE, std::string(who) + ": a step-wise RWMH session is open" +
                                     (rule == SESSION_SHARED ? "; its proposal / SSE buffers are shared (si_rwmh_end or si_rwmh_abort first)" : ""));
}
int32_t infer_entry_check(si_ctx* ctx, const char* who, const char* bad_args, SessionRule rule, bool grad) {
  const int32_t rc = need_setup(ctx, who);
  if (rc != SI_OK) return rc;
  if (grad && ctx->node.on && !ctx->node.grad)   // (the switch: si_node_set_grad)
    return fail(ctx, SI_ERR_INVALID, std::string(who) + ": not available for NeuralODE models (the gradient through the solver is not built "
                                                        "for this set-up: si_node_set_grad(ctx, 1) turns the discrete adjoint on)");
  if (bad_args) return fail(ctx, SI_ERR_INVALID, std::string(who) + ": " + bad_args);
  return no_session(ctx, who, rule);
}

int32_t si_logdensity_grad(si_ctx* ctx, const double* z, double* lp_out, double* grad_out) {
  CHECK_CTX(ctx);
  const int32_t rc = infer_entry_check(ctx, "si_logdensity_grad", bad_if(!z || !lp_out || !grad_out), SESSION_SHARED, true);
  if (rc != SI_OK) return rc;
  BIND(ctx);
  return logdensity_grad_point(ctx, z, lp_out, grad_out);
}

// ---- many points in one call: narrow Dense chains on the fused forward + reverse kernel (kernels_chain_grad.hip) ---------------
// The class: compute_dtype = SI_F64, every layer Dense with one of the four MFMA-epilogue activations, at most
// SI_CHAIN_MAX_LAYERS layers, an LDS plan (every layer's image + two Delta buffers) within 160 KiB at 16 observations per
// workgroup, and a flat weight vector that the layers' W / b ranges cover exactly once (every workgroup writes every element
// of its partial).  32 observations per workgroup where that plan leaves room for two workgroups per CU (half the partials).
// The choice depends on the chain and B only -- never on C -- so a point's bits do not depend on the call it arrives in.
static int vgrad_class(si_ctx* ctx) {
  if (ctx->vg.cls >= 0) return ctx->vg.cls;
  ctx->vg.cls = 0;
  if (ctx->setup.model.f32 || ctx->setup.model.plan.has_conv) return 0;
  const int L = (int)ctx->setup.model.layers.size();
  ChainVgradPlan vp;
  if (chain_vgrad_plan(vp, ctx->setup.model.layers.data(), L, ctx->setup.B, 1) == 0) return 0;
  if (ctx->setup.model.layers[0].in != ctx->setup.model.in_dim || ctx->setup.model.layers[(size_t)L - 1].out != ctx->setup.model.out_dim) return 0;
  std::vector<char> seen((size_t)ctx->setup.model.N, 0);
  auto mark = [&](int64_t off, int64_t n) {
    if (off < 0 || off + n > ctx->setup.model.N) return false;
    for (int64_t i = off; i < off + n; ++i) {
      if (seen[(size_t)i]) return false;
      seen[(size_t)i] = 1;
    }
    return true;
  };
  int64_t total = 0;
  for (const si_layer& ly : ctx->setup.model.layers) {
    if (!mark(ly.w_off, (int64_t)ly.in * ly.out) || !mark(ly.b_off, ly.out)) return 0;
    total += (int64_t)ly.in * ly.out + ly.out;
  }
  if (total != ctx->setup.model.N) return 0;
  const size_t lds2 = chain_vgrad_plan(vp, ctx->setup.model.layers.data(), L, ctx->setup.B, 2);
  ctx->vg.cls = (lds2 != 0 && lds2 <= (size_t)64 * 1024) ? 2 : 1;
  return ctx->vg.cls;
}

// The fused route's pieces, for si_logdensity_grad_batch (points from the host, staged per pass) and StackedVgrad (points on the
// device) below.  vgrad_route: the batch-tile class of the chain set up (0: not of the fused class), the workgroups per point and
// the points one pass of launches may carry.
static int vgrad_route(si_ctx* ctx, int64_t* G_out, int64_t* fit_out) {
  const int64_t B = ctx->setup.B, ldw = pad_ld(ctx->setup.model.N);
  // (chain_vgrad_reduce_kernel forms P' g itself: not taken with a decoder; chain_vgrad_kernel seeds the sweep with the squared
  //  error's derivative: not taken with a categorical / Bernoulli likelihood)
  const int nb = ctx->dec.on || lik_on(ctx) ? 0 : vgrad_class(ctx);
  const int64_t G = nb > 0 ? (B + 16 * nb - 1) / (16 * nb) : 0;
  // points per pass of launches: the workspace (weights, G partials of grad_w, grad_w per point) is capped like the forward
  // workspace of the stacked density (SI_BATCH_BYTES), and a launch carries at most 65535 points in grid.y
  const double per = 8.0 * ((double)ldw * ((double)G + 2.0) + (double)G + 2.0 * ctx->setup.M + 1.0);
  *G_out = G;
  *fit_out = nb > 0 ? (int64_t)std::min(65535.0, std::floor(SI_BATCH_BYTES / per)) : 0;
  return nb;
}

// its workspace for `cap` points per pass
static int32_t vgrad_ensure(si_ctx* ctx, const char* who, int cap, int64_t G) {
  if (ctx->vg.cap >= cap) return SI_OK;
  const int64_t ldw = pad_ld(ctx->setup.model.N);
  const int32_t M = ctx->setup.M;
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const size_t S = (size_t)cap;
  ctx->vg.cap = 0;
  if (!ctx->vg.z.alloc(S * M) || !ctx->vg.w.alloc(S * (size_t)ldw) || !ctx->vg.part.alloc(S * (size_t)G * (size_t)ldw) ||
      !ctx->vg.ssepart.alloc(S * (size_t)G) || !ctx->vg.gw.alloc(S * (size_t)ldw) || !ctx->vg.lp.alloc(S) ||
      !ctx->vg.gz.alloc(S * M)) {
    for (DevBuf<double>* b : {&ctx->vg.z, &ctx->vg.w, &ctx->vg.part, &ctx->vg.ssepart, &ctx->vg.gw, &ctx->vg.lp, &ctx->vg.gz})
      b->reset();
    return fail(ctx, SI_ERR_NOMEM, std::string(who) + ": workspace allocation failed");
  }
  ctx->vg.cap = cap;
  return SI_OK;
}

// one pass of launches: value and gradient at the n <= vg.cap points z_dev[:, 0 .. n) (device) into lp_dev[n] / gz_dev[M x n]
// (device).  Queued on the stream; nothing is copied, nothing synchronises.
static void vgrad_pass(si_ctx* ctx, int nb, int64_t G, const double* z_dev, int n, double* lp_dev, double* gz_dev) {
  const int64_t N = ctx->setup.model.N, B = ctx->setup.B, ldw = pad_ld(N);
  const int32_t M = ctx->setup.M;
  ChainVgradPlan vp;
  const size_t lds = chain_vgrad_plan(vp, ctx->setup.model.layers.data(), (int)ctx->setup.model.layers.size(), B, nb);
  const double s2 = ctx->setup.sigma_m * ctx->setup.sigma_m;
  const double c0 = mvnormal_c0((double)ctx->setup.model.out_dim * (double)B, ctx->setup.sigma_m);
  {
    ProfScope ps(ctx, SI_K_RECON, 2.0 * (double)N * M * n, (double)N * (M + 1 + n) * 8.0);
    (void)form_weights(ctx, z_dev, n, ctx->vg.w, ldw);   // (the P route: vgrad_route keeps this pass away from a decoder, whose reverse it does not carry)
  }
  {
    ProfScope ps(ctx, SI_K_BACKWARD, 6.0 * (double)N * (double)B * n, 0.0);
    launch_chain_vgrad(ctx->stream, vp, nb, lds, ctx->vg.w, ldw, ctx->setup.X, ctx->setup.Y, 1.0 / s2, ctx->vg.part, ldw, ctx->vg.ssepart, n);
    launch_chain_vgrad_reduce(ctx->stream, ctx->vg.part, (int)G, N, ldw, ctx->vg.ssepart, ctx->vg.w, ldw, ctx->setup.P, ctx->setup.ldP, M,
                              ctx->setup.sigma_p, prior_c0(ctx), c0, s2, ctx->vg.gw, lp_dev, gz_dev, n);
  }
}

}  // extern "C"

namespace si {

// ---- value and gradient at C stacked points that already live on the device (si_sample_mala, si_sample_hmc, si_fit_advi) ---------
// Two routes, chosen by the chain set up, never by the caller:
//   fused   chains of the class above: per evaluation launch_reconstruct, launch_chain_vgrad and launch_chain_vgrad_reduce are
//           queued once per pass of vg.cap points, outputs left on the device.  Nothing is copied and nothing synchronises, so a
//           caller that queues its own kernel between evaluations keeps its state on the device until its tail.  A launch-queued
//           loop: no persistent kernel, no grid barrier, nothing that can spin.
//   other   every other chain (Conv / MaxPool / flatten, SI_F32, the four later activations, wide layers): the points come down
//           to the host, their values and gradients are computed column by column by si_logdensity_grad's own path and go back up.
//           SLOW AND SYNCHRONISING: one round trip per point and evaluation; it exists so that every chain the gradient covers
//           has the device samplers' definitions.
int32_t StackedVgrad::open(si_ctx* c, const char* who, int32_t npoints) {
  ctx = c, C = npoints;
  node = ctx->node.on && !ctx->dec.on;   // (with a decoder a node set-up goes column by column, as Chains do)
  if (node) {
    const int32_t rc = node_grad_ensure(ctx, who, C);
    if (rc != SI_OK) return rc;
    passes = (C + ctx->node.g_cap - 1) / ctx->node.g_cap;
    return SI_OK;
  }
  int64_t fit = 0;
  nb = vgrad_route(ctx, &G, &fit);
  fused = fit >= 1;
  if (fused) {
    const int32_t rc = vgrad_ensure(ctx, who, (int)std::min<int64_t>(fit, C), G);
    if (rc != SI_OK) return rc;
  } else {
    hz.resize((size_t)ctx->setup.M * C);
    hlp.resize((size_t)C);
    hg.resize((size_t)ctx->setup.M * C);
  }
  passes = fused ? (C + ctx->vg.cap - 1) / ctx->vg.cap : C;
  return SI_OK;
}

void StackedVgrad::eval(const double* z_dev, double* lp_dev, double* g_dev, hipError_t& e, int32_t& rc) {
  const size_t M = (size_t)ctx->setup.M;
  if (node) {
    for (int32_t p0 = 0; p0 < C && rc == SI_OK; p0 += ctx->node.g_cap)
      rc = node_value_and_grad(ctx, z_dev + M * p0, std::min<int32_t>(ctx->node.g_cap, C - p0), lp_dev + p0, g_dev + M * p0);
    e = hipGetLastError();
    return;
  }
  if (fused) {
    for (int32_t p0 = 0; p0 < C; p0 += ctx->vg.cap)
      vgrad_pass(ctx, nb, G, z_dev + M * p0, std::min<int32_t>(ctx->vg.cap, C - p0), lp_dev + p0, g_dev + M * p0);
    e = hipGetLastError();
    return;
  }
  e = hipMemcpyAsync(hz.data(), z_dev, hz.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // (also: the uploads of the evaluation before have left hlp / hg)
  for (int32_t c = 0; c < C && e == hipSuccess && rc == SI_OK; ++c)
    rc = logdensity_grad_point(ctx, hz.data() + M * c, hlp.data() + c, hg.data() + M * c);
  if (rc != SI_OK) return;
  // (hlp / hg outlive these uploads: the caller's tail synchronises before the evaluator goes)
  if (e == hipSuccess) e = hipMemcpyAsync(lp_dev, hlp.data(), hlp.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(g_dev, hg.data(), hg.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
}

int32_t finish_downloads(si_ctx* ctx, const char* who, hipError_t e, int32_t rc, std::initializer_list<Download> downs) {
  for (const Download& d : downs)
    if (e == hipSuccess && rc == SI_OK && d.dst) e = hipMemcpyAsync(d.dst, d.src, d.bytes, hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t e2 = hipStreamSynchronize(ctx->stream);
  if (rc != SI_OK) return rc;
  if (e != hipSuccess) return fail(ctx, SI_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
  if (e2 != hipSuccess) return fail(ctx, SI_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e2));
  return SI_OK;
}

}  // namespace si

extern "C" {

int32_t si_logdensity_grad_batch(si_ctx* ctx, const double* Z, int32_t C, double* lp_out, double* grad_out) {
  CHECK_CTX(ctx);
  int32_t rc = infer_entry_check(ctx, "si_logdensity_grad_batch", bad_if(!Z || C < 1 || !lp_out || !grad_out), SESSION_SHARED, true);
  if (rc != SI_OK) return rc;
  BIND(ctx);
  ctx->vg.last_fused = 0;
  const int32_t M = ctx->setup.M;
  if (ctx->node.on && !ctx->dec.on) return node_grad_batch(ctx, Z, C, lp_out, grad_out);   // all points of a pass in one launch each
  int64_t G = 0, fit = 0;
  const int nb = vgrad_route(ctx, &G, &fit);
  if (fit < 1) {
    // every other chain (Conv / MaxPool / flatten, SI_F32, the four later activations, wide layers): column by column through the
    // single-point path -- the same code, the same bits as C calls of si_logdensity_grad
    for (int32_t c = 0; c < C; ++c)
      if ((rc = logdensity_grad_point(ctx, Z + (size_t)M * c, lp_out + c, grad_out + (size_t)M * c)) != SI_OK) return rc;
    return SI_OK;
  }
  if ((rc = vgrad_ensure(ctx, "si_logdensity_grad_batch", (int)std::min<int64_t>(fit, C), G)) != SI_OK) return rc;
  for (int32_t p0 = 0; p0 < C; p0 += ctx->vg.cap) {
    const int n = std::min<int32_t>(ctx->vg.cap, C - p0);
    SI_HIP(ctx, hipMemcpyAsync(ctx->vg.z, Z + (size_t)M * p0, (size_t)M * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    vgrad_pass(ctx, nb, G, ctx->vg.z, n, ctx->vg.lp, ctx->vg.gz);
    SI_HIP(ctx, hipGetLastError());
    SI_HIP(ctx, hipMemcpyAsync(lp_out + p0, ctx->vg.lp, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SI_HIP(ctx, hipMemcpyAsync(grad_out + (size_t)M * p0, ctx->vg.gz, (size_t)M * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  }
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->vg.last_fused = 1;
  return SI_OK;
}

int32_t si_grad_kernel_info(si_ctx* ctx, int32_t* fused_out) {
  CHECK_CTX(ctx);
  if (!fused_out) return fail(ctx, SI_ERR_INVALID, "si_grad_kernel_info: bad argument");
  *fused_out = ctx->vg.last_fused;
  return SI_OK;
}

int32_t si_forward(si_ctx* ctx, const double* z, double* Yhat_out) {
  CHECK_CTX(ctx);
  int32_t rc = infer_entry_check(ctx, "si_forward", bad_if(!z || !Yhat_out));
  if (rc != SI_OK) return rc;
  BIND(ctx);
  if ((rc = ensure_chains(ctx, 1)) != SI_OK) return rc;
  SI_HIP(ctx, hipMemcpyAsync(ctx->chains.zprop, z, (size_t)ctx->setup.M * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  DensityOutputs yh;
  if ((rc = eval_density(ctx, setup_view(ctx), 0, 1, &yh)) != SI_OK) return rc;
  SI_HIP(ctx, hipMemcpyAsync(Yhat_out, yh.p, (size_t)ctx->setup.model.out_dim * ctx->setup.B * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SI_OK;
}

int32_t si_predict(si_ctx* ctx, const double* Z, int32_t C, const double* Xnew, int64_t Bn, double* Yhat_out) {
  CHECK_CTX(ctx);
  int32_t rc = infer_entry_check(ctx, "si_predict", bad_if(!Z || C <= 0 || !Xnew || Bn <= 0 || !Yhat_out));
  if (rc != SI_OK) return rc;
  BIND(ctx);
  if ((rc = ensure_chains(ctx, C)) != SI_OK) return rc;
  if (ctx->node.on) return node_predict(ctx, Z, C, Xnew, Bn, Yhat_out);   // new initial states d x Bn (capi_node.hip)
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  // run the ordinary forward path on temporary data buffers sized for Bn, through a view of its own: the context is only read;
  // like the density, up to `wb` samples share one pass of launches (grid.y), within the same workspace cap
  // (with compute_dtype = SI_F32 the predictive forward still runs in fp64: it owns its fp64 workspace below, and the fp64
  //  weights are what K4 writes in either mode -- the fp32 option covers the density / the RWMH samplers)
  const int64_t act_elems = pad_ld(ctx->setup.model.max_stored * Bn);
  const int sse_blocks = sse_num_blocks((int64_t)ctx->setup.model.out_dim * Bn, ctx->num_cu);
  const size_t dB = (size_t)ctx->setup.model.out_dim * (size_t)Bn;
  const double per = 8.0 * (2.0 * (double)act_elems + ((double)ctx->setup.model.fuse_slots + 1.0) * (double)dB + (double)sse_blocks);
  const size_t wb = (size_t)std::max(1.0, std::min({(double)C, (double)ctx->fw.slots, std::floor(SI_BATCH_BYTES / per)}));
  DevBuf<double> tX, tY, tA[2], tS, tP, tYh, tXc;
  bool ok = tX.alloc((size_t)ctx->setup.model.in_dim * Bn) && tY.alloc(dB) &&
            (!ctx->setup.model.plan.input_spatial || tXc.alloc((size_t)ctx->setup.model.plan.in_elems * Bn)) &&
            tA[0].alloc(wb * (size_t)act_elems) && tA[1].alloc(wb * (size_t)act_elems) && tS.alloc(wb * (size_t)sse_blocks) &&
            (!ctx->setup.model.fuse_tail || (tP.alloc(wb * (size_t)ctx->setup.model.fuse_slots * dB) && tYh.alloc(wb * dB)));
  hipError_t e = hipSuccess;
  if (ok) {
    const DensityView v{tX, tXc, nullptr, tY, Bn, tA, nullptr, tS, sse_blocks, tP, tYh, act_elems, /*f32=*/false,
                        /*defer_sse_final=*/false, /*is_setup_data=*/false};
    e = hipMemcpyAsync(tX, Xnew, (size_t)ctx->setup.model.in_dim * Bn * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(tY, 0, dB * sizeof(double), ctx->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(ctx->chains.zprop, Z, (size_t)ctx->setup.M * C * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (ctx->setup.model.plan.input_spatial) net_input(ctx, ctx->setup.model.plan, tX, tXc, Bn);
    for (int c0 = 0; c0 < C && e == hipSuccess && rc == SI_OK; c0 += (int)wb) {
      const int nc = std::min<int>((int)wb, C - c0);
      DensityOutputs yh;
      rc = eval_density(ctx, v, c0, nc, &yh);
      if (rc == SI_OK)
        e = hipMemcpy2DAsync(Yhat_out + (size_t)c0 * dB, dB * sizeof(double), yh.p, (size_t)yh.stride * sizeof(double), dB * sizeof(double),
                             (size_t)nc, hipMemcpyDeviceToHost, ctx->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // the outputs are overwritten by the next batch
    }
  }
  (void)hipStreamSynchronize(ctx->stream);
  for (DevBuf<double>* b : {&tX, &tY, &tA[0], &tA[1], &tS, &tP, &tYh, &tXc}) b->reset();
  if (!ok) return fail(ctx, SI_ERR_NOMEM, "si_predict: device allocation failed");
  if (rc != SI_OK) return rc;
  if (e != hipSuccess) return fail(ctx, SI_ERR_HIP, std::string("si_predict: ") + hipGetErrorString(e));
  return SI_OK;
}

}  // extern "C"
