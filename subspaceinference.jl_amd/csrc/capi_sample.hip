// C ABI, sampling side: the RWMH samplers (si_sample_rwmh*, the step-wise session si_rwmh_*), the output map
// (si_sample_rwmh_weights, si_reconstruct) -- reference src/space_inference.jl:111-116,125.  Three sampler forms behind one
// entry point, one function each, tried in this order: the one-workgroup device-resident loop (rwmh_one_workgroup,
// kernels_chain.hip), the persistent grid loop (rwmh_grid, kernels_chain_grid.hip; prepare_spec_loop readies its run-time
// specialised variant) and the launch-per-step loop (rwmh_per_step, with WeightRing for the streamed output map).
// sample_rwmh_impl checks and reserves once and hands them an RwmhCall; finish_chains is their common end.  Host-side
// orchestration only; no CPU fallback anywhere in this file.
#include <cstring>

#include "capi_common.h"
#include "chain_spec_args.h"
#include "chain_spec_rtc.h"

using namespace si;

extern "C" {

// ---- streamed output map (a13, src/space_inference.jl:125: `map(z -> W_swa + P*z.params, chm)`) ------------------------
// K4 has already produced W_swa + P z' for every proposal (fw.w); the weight vector of sample t is that vector when the
// proposal was accepted and the previous sample's otherwise.  A select kernel keeps the CURRENT weights of every chain in
// a small device ring (8 bytes read + 8 written per weight, ~4 us at cfg2 -- instead of a second K4 pass over P), a DMA
// on the second stream moves ring slot t into pinned memory while transition t+1 computes, and the host copy pool
// moves it into the caller's array R-1 transitions later.  The chain never waits for PCIe.
static constexpr int SI_WRING = 4;

static void free_wstream(si_ctx* ctx) {
  ctx->d_wring.reset();
  ctx->d_accflag.reset();
  for (int r = 0; r < SI_WRING; ++r) {
    ctx->h_wring[r].reset();
    ctx->ev_wcomp[r].reset();
    ctx->ev_wcopy[r].reset();
  }
  ctx->wring_N = 0;
  ctx->wring_C = 0;
}

static int32_t ensure_wstream(si_ctx* ctx, int32_t C) {
  const size_t need = (size_t)C * (size_t)pad_ld(ctx->setup.model.N);
  if (!ctx->stream2) SI_HIP(ctx, hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking));
  if (ctx->wring_N == ctx->setup.model.N && ctx->wring_C >= C) return SI_OK;
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  free_wstream(ctx);
  bool ok = ctx->d_wring.alloc(need * SI_WRING) && ctx->d_accflag.alloc((size_t)C);
  for (int r = 0; r < SI_WRING && ok; ++r)
    ok = ctx->h_wring[r].alloc((size_t)C * (size_t)ctx->setup.model.N) && ctx->ev_wcomp[r].create() && ctx->ev_wcopy[r].create();
  if (!ok) {
    free_wstream(ctx);
    return fail(ctx, SI_ERR_NOMEM, "si_sample_rwmh_weights: allocation of the weight ring / pinned staging failed");
  }
  ctx->wring_N = ctx->setup.model.N;
  ctx->wring_C = C;
  return SI_OK;
}

// the device-resident loop covers: Dense chains in fp64 with the head folded into the layer before it (fuse_tail), the
// four activations the MFMA epilogues carry, no prior term, and little enough arithmetic that ONE CU per chain beats ~8
// launches per transition spread over the chip (2 N B <= 3 MFLOP: the README toy is 0.14)
static constexpr size_t SI_CHAIN_LDS_LIMIT = 160 * 1024 - 256;
static bool chain_loop_applies(const si_ctx* ctx) {
  if (ctx->setup.model.f32 || ctx->setup.model.plan.has_conv || !ctx->setup.model.fuse_tail || ctx->setup.sigma_p > 0.0 || ctx->dec.on || lik_on(ctx)) return false;   // (dec: the loop forms W_swa + P z itself; lik: it forms the squared errors itself)
  if (ctx->setup.model.layers.size() > (size_t)SI_CHAIN_MAX_LAYERS || ctx->setup.model.N > (1 << 20) || ctx->setup.B > (1 << 20)) return false;
  if (ctx->setup.M > 1024) return false;   // (rwmh_chain_kernel keeps z one element per thread of its 1024-thread workgroup)
  for (const auto& ly : ctx->setup.model.layers)
    if (ly.kind != SI_LAYER_DENSE || ly.act >= SI_ACT_LEAKYRELU) return false;
  return 2.0 * (double)ctx->setup.model.N * (double)ctx->setup.B <= 3.0e6;
}

// The common end of the three sampler forms.  `e` is the state of what the form has queued so far.  Z / lp (from chains.outZ /
// chains.outlp) and the accept counts come down -- Z and lp through the pinned `stage` where the form hands one in; with W_out the
// weight samples of the finished chains come from ONE K4 pass over all itr * C samples into a temporary (the kernel
// si_reconstruct runs: same bits) and a 2-D copy; one synchronisation; the first error is reported; a raised barrier word
// of the grid loop (grid_status) is one; the accept rates are filled in.
static int32_t finish_chains(si_ctx* ctx, const char* who, hipError_t e, int64_t itr, int32_t C, double* Z_out, double* lp_out,
                             double* accept_rate_out, double* W_out, size_t wall_elems, char* stage, const unsigned* grid_status) {
  const int32_t M = ctx->setup.M;
  const int64_t N = ctx->setup.model.N, ldw = pad_ld(N);
  const size_t zbytes = Z_out ? (size_t)M * itr * C * sizeof(double) : 0, lbytes = lp_out ? (size_t)itr * C * sizeof(double) : 0;
  std::vector<int64_t> nacc((size_t)C);
  if (e == hipSuccess && Z_out) e = hipMemcpyAsync(stage ? (void*)stage : (void*)Z_out, ctx->chains.outZ, zbytes, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && lp_out)
    e = hipMemcpyAsync(stage ? (void*)(stage + zbytes) : (void*)lp_out, ctx->chains.outlp, lbytes, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(nacc.data(), ctx->chains.nacc, (size_t)C * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream);
  DevBuf<double> dW;
  if (e == hipSuccess && W_out) {   // src/space_inference.jl:125 for every sample of every chain
    if (!dW.alloc(wall_elems)) e = hipErrorOutOfMemory;   // (ldw * itr * C: the caller has held it to its 512 MB gate)
    if (e == hipSuccess) {
      ProfScope ps(ctx, SI_K_RECON, 2.0 * (double)N * M * (double)itr * C, (double)N * (M + 1 + (double)itr * C) * 8.0);
      const int32_t rcw = form_weights(ctx, ctx->chains.outZ, (int32_t)(itr * C), dW, ldw);
      e = rcw == SI_OK ? hipGetLastError() : hipErrorOutOfMemory;
    }
    if (e == hipSuccess)
      e = hipMemcpy2DAsync(W_out, (size_t)N * sizeof(double), dW, (size_t)ldw * sizeof(double), (size_t)N * sizeof(double),
                           (size_t)itr * C, hipMemcpyDeviceToHost, ctx->stream);
  }
  const hipError_t e2 = hipStreamSynchronize(ctx->stream);
  dW.reset();
  if (e != hipSuccess) return fail(ctx, SI_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
  if (e2 != hipSuccess) return fail(ctx, SI_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e2));
  if (stage) {
    if (Z_out) std::memcpy(Z_out, stage, zbytes);
    if (lp_out) std::memcpy(lp_out, stage + zbytes, lbytes);
  }
  if (grid_status && *grid_status != 0)
    return fail(ctx, SI_ERR_HIP, std::string(who) + ": the grid barrier of the device-resident loop timed out (its workgroups were not all resident: "
                                 "is another process holding compute units of this GPU?); si_set_chain_loop(ctx, 2) runs the launch-per-step loop");
  accept_rates(nacc, itr, accept_rate_out);
  return SI_OK;
}

// One si_sample_rwmh* call, as sample_rwmh_impl hands it to the sampler forms: the arguments, and what the entry has checked,
// reserved (ensure_chains / ensure_wstream, chains.outZ / chains.outlp) and worked out once.
struct RwmhCall {
  const char* who;
  int64_t itr;
  double sigma_z;
  uint64_t seed;
  int32_t chain_id0, C;
  double *Z_out, *lp_out, *accept_rate_out, *W_out;
  double c0, s2;
  size_t wall_elems;   // ldw * itr * C: the output map of the whole call
  bool map_fits;       // no output map asked for, or one within the 512 MB that finish_chains writes in ONE K4 pass: the loops' gate
};

// the fields that the argument structs of the three device-resident kernels share (a template: C++ linkage inside this block)
extern "C++" template <typename Args>
static void fill_common_args(Args& a, const si_ctx* ctx, const RwmhCall& k) {
  a.swa = ctx->setup.swa; a.P = ctx->setup.P; a.X = ctx->setup.X; a.Y = ctx->setup.Y;
  a.Z_out = ctx->chains.outZ; a.lp_out = ctx->chains.outlp; a.nacc_out = reinterpret_cast<decltype(a.nacc_out)>(ctx->chains.nacc.get());
  a.ldP = ctx->setup.ldP; a.itr = k.itr; a.seed = k.seed; a.sigma_z = k.sigma_z; a.c0 = k.c0; a.sigma2 = k.s2;
  a.N = (int)ctx->setup.model.N; a.chain_id0 = k.chain_id0;
}

// ---- K6 as a device-resident loop (kernels_chain.hip): small Dense chains whose weights, data and activations fit one
// workgroup's LDS run ALL transitions in one launch, one workgroup per chain -- the launch-per-step loop below costs ~8
// dependent launches (25 us) per transition whatever the size.  Same bits (tests/test_gpu_chain.py).
// (with the output map requested -- what the drop-in sub_inference call does -- the weight samples of the finished chains
//  come from ONE K4 pass over all itr * C samples, the kernel si_reconstruct runs: same bits, no streaming needed at this size)
static int32_t rwmh_one_workgroup(si_ctx* ctx, const RwmhCall& k) {
  if (!k.map_fits || !chain_loop_applies(ctx) || ctx->chain_mode != 1) return SI_NOT_TAKEN;
  ChainLoopArgs a{};
  const int L = (int)ctx->setup.model.layers.size();
  for (int l = 0; l < L; ++l) a.lay[l] = ctx->setup.model.layers[(size_t)l];
  fill_common_args(a, ctx, k);
  a.M = ctx->setup.M; a.B = (int)ctx->setup.B; a.L = L;
  a.slot_feats = dense_fused_slot_feats(ctx->setup.model.layers[(size_t)L - 2].out);
  a.fuse_slots = ctx->setup.model.fuse_slots;
  const size_t lds = chain_loop_plan(a, SI_CHAIN_LDS_LIMIT);
  if (lds == 0) return SI_NOT_TAKEN;
  {
    const double fl = 2.0 * (double)ctx->setup.model.N * (double)ctx->setup.B * (double)k.itr * k.C;
    ProfScope ps(ctx, SI_K_RWMH, fl, 0.0);
    launch_chain_loop(ctx->stream, a, k.C, lds);
  }
  return finish_chains(ctx, k.who, hipGetLastError(), k.itr, k.C, k.Z_out, k.lp_out, k.accept_rate_out, k.W_out, k.wall_elems, nullptr, nullptr);
}

// The grid loop specialised to this chain's shapes (chain_spec.inc through hiprtc; same bits): ONE barrier per transition, the
// weights handed over in fragment order.  Class: a narrow head, at most 1024 model outputs (four blocks of the SSE tree),
// every weight fragment in registers (spec_applies).  Lays out its LDS behind the images of the forward (sa, *lds_spec), keeps
// loop.specw / loop.specy for C chains and the fragment-order permutation of these kernels.  Returns the kernels, or null with *rc
// SI_OK (not of the class: the generic loop runs) or the call's error.
static const SpecKernels* prepare_spec_loop(si_ctx* ctx, const RwmhCall& k, int G, int nb, int sf, SiSpecGridArgs& sa, size_t* lds_spec,
                                            int32_t* rc) {
  const int32_t C = k.C, M = ctx->setup.M;
  const int64_t N = ctx->setup.model.N, d = (int64_t)ctx->setup.model.out_dim * ctx->setup.B;
  *rc = SI_OK;
  auto bad = [&](int32_t code, const char* what) {
    *rc = fail(ctx, code, std::string(k.who) + what);
    return (const SpecKernels*)nullptr;
  };
  if (!ctx->chain_spec || !ctx->setup.model.fuse_tail || d > 1024 || M > 256) return nullptr;
  const int rs = (int)((((N + G - 1) / G) + 15) & ~(int64_t)15);
  const SpecKernels* sk = spec_kernels(ctx->setup.model.layers.data(), (int)ctx->setup.model.layers.size(), nb, sf, M, rs <= 256 && M <= 32, &ctx->spec_message);
  if (!sk) return nullptr;
  auto even = [](int64_t v) { return (v + 1) & ~(int64_t)1; };
  int64_t off = sk->lds_doubles;
  sa.y_in_lds = 1;
  sa.o_y = (int)off;
  off += even(d);
  sa.o_blk = (int)off;
  off += even(ctx->setup.sse_blocks);
  sa.o_z = (int)off;
  off += even(5 * (int64_t)M);
  sa.o_red = (int)off;
  off += 24;
  sa.o_flag = (int)off;
  off += 2;
  *lds_spec = std::max((size_t)off * sizeof(double), (size_t)(81 * 1024));   // (more than half a CU's LDS: one workgroup per CU)
  if (*lds_spec > (size_t)160 * 1024 - 256) return nullptr;
  if (ctx->loop.spec_chains < C || ctx->loop.spec_fo != sk->fo_total) {
    ctx->loop.specw.reset();
    ctx->loop.specy.reset();
    ctx->loop.spec_chains = 0;
    if (!ctx->loop.specw.alloc((size_t)4 * (size_t)sk->fo_total * (size_t)C) || !ctx->loop.specy.alloc((size_t)2 * (size_t)d * (size_t)C))
      return bad(SI_ERR_NOMEM, ": allocation failed");
    // (the padding elements of the fragment-ordered vectors are never written by K4: they must be finite)
    if (hipMemsetAsync(ctx->loop.specw, 0, (size_t)4 * (size_t)sk->fo_total * (size_t)C * sizeof(double), ctx->stream) != hipSuccess)
      return bad(SI_ERR_HIP, ": hipMemsetAsync failed");
    ctx->loop.spec_chains = C;
    ctx->loop.spec_fo = sk->fo_total;
  }
  if (ctx->loop.specperm_for != (const void*)sk) {
    ctx->loop.specperm_for = nullptr;
    if (!ctx->loop.specperm.alloc((size_t)N)) return bad(SI_ERR_NOMEM, ": allocation failed");
    int* pp = ctx->loop.specperm;
    void* pargs[] = {&pp};
    if (hipModuleLaunchKernel(sk->perm, (unsigned)((sk->max_wn + 255) / 256), 1, 1, 256, 1, 1, 0, ctx->stream, pargs, nullptr) != hipSuccess)
      return bad(SI_ERR_HIP, ": launch of the fragment-order permutation failed");
    ctx->loop.specperm_for = (const void*)sk;
  }
  return sk;
}

// ---- K6 as a persistent loop over a GRID of workgroups (kernels_chain_grid.hip): a narrow chain too large for one
// workgroup (docs/src/nn_example.md's MLP) runs all transitions in one launch, G = ceil(B / tile) resident workgroups per
// chain, two bounded grid barriers per transition.  Same bits as the launch-per-step loop (tests/test_gpu_chain_grid.py).
static int32_t rwmh_grid(si_ctx* ctx, const RwmhCall& k) {
  const int32_t C = k.C, M = ctx->setup.M;
  if (!k.map_fits || !ctx->setup.fused_ok || ctx->chain_mode != 1 || ctx->setup.sigma_p > 0.0 || C > ctx->fw.slots || k.itr >= ((int64_t)1 << 24) ||
      ctx->dec.on || lik_on(ctx))   // (both grid loops, the run-time specialised one included, form W_swa + P z in their own K4 and the squared errors in their own tail)
    return SI_NOT_TAKEN;
  ChainGridArgs a{};
  const int L = (int)ctx->setup.model.layers.size();
  const int sf = ctx->setup.model.fuse_tail ? dense_fused_slot_feats(ctx->setup.model.layers[(size_t)L - 2].out) : 0;
  int nb = 0;
  size_t lds = 0;
  for (int cand : {1, 2, 4}) {   // the smallest tile whose grid is resident: one workgroup per CU
    const int64_t G = (ctx->setup.B + 16 * cand - 1) / (16 * cand);
    if (G * C > ctx->num_cu) continue;
    const size_t lf = chain_fused_plan(a.p, ctx->setup.model.layers.data(), L, ctx->setup.B, cand, ctx->setup.model.fuse_tail, sf, ctx->setup.model.fuse_slots);
    fused_fill_program(ctx, a.p);
    a.M = M;
    a.nblocks = ctx->setup.sse_blocks;
    a.G = (int)G;
    lds = chain_grid_plan(a, lf);
    if (lds != 0) {
      nb = cand;
      break;
    }
  }
  if (nb == 0) return SI_NOT_TAKEN;
  SiSpecGridArgs sa{};
  size_t lds_spec = 0;
  int32_t rc = SI_OK;
  const SpecKernels* sk = prepare_spec_loop(ctx, k, a.G, nb, sf, sa, &lds_spec, &rc);
  if (rc != SI_OK) return rc;
  const size_t sync_lines = sk ? (size_t)8 * (size_t)C + 1 : (size_t)C + 1;   // (the specialised loop shards each chain's counter over 8 lines)
  if (!ctx->loop.gridsync.reserve((size_t)32 * sync_lines)) return fail(ctx, SI_ERR_NOMEM, std::string(k.who) + ": allocation failed");
  fill_common_args(a, ctx, k);
  a.wbuf = ctx->fw.w; a.w_stride = pad_ld(ctx->setup.model.N);
  a.ybuf = ctx->fw.yhat; a.y_stride = (int64_t)ctx->setup.model.out_dim * ctx->setup.B;
  a.cnt = ctx->loop.gridsync; a.status = ctx->loop.gridsync + (size_t)32 * (sync_lines - 1);
  hipError_t e = hipMemsetAsync(ctx->loop.gridsync, 0, (size_t)32 * sync_lines * sizeof(unsigned), ctx->stream);
  if (e == hipSuccess) {
    const double fl = 2.0 * (double)ctx->setup.model.N * (double)ctx->setup.B * (double)k.itr * C;
    ProfScope ps(ctx, SI_K_RWMH, fl, 0.0);
    if (sk) {
      fill_common_args(sa, ctx, k);
      sa.perm = ctx->loop.specperm;
      sa.wbuf = ctx->loop.specw; sa.w_stride = sk->fo_total;
      sa.ybuf = ctx->loop.specy; sa.y_stride = a.y_stride;
      sa.cnt = a.cnt; sa.status = a.status;
      sa.M = M; sa.G = a.G; sa.B = (int)ctx->setup.B; sa.nblocks = ctx->setup.sse_blocks;
      void* gargs[] = {&sa};
      e = hipModuleLaunchKernel(sk->grid, (unsigned)(a.G * C), 1, 1, 256, 1, 1, (unsigned)lds_spec, ctx->stream, gargs, nullptr);
      ctx->loop.last_loop_spec = e == hipSuccess;
    } else {
      e = launch_chain_grid(ctx->stream, a, nb, C, lds);
    }
  }
  unsigned status = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&status, a.status, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream);
  // the samples and lp go through pinned staging: a device-to-host copy straight into the caller's array pins its pages on the
  // fly, and for an array nobody has touched yet (np.empty, Matrix{Float64}(undef, ...)) that costs ~9 us per page -- 7 ms for the
  // 3.4 MB of a 20 000-transition chain, 0.35 us per transition of a 9.8 us loop
  const size_t zbytes = k.Z_out ? (size_t)M * k.itr * C * sizeof(double) : 0, lbytes = k.lp_out ? (size_t)k.itr * C * sizeof(double) : 0;
  const bool staged = zbytes + lbytes >= ((size_t)128 << 10) && zbytes + lbytes <= ((size_t)128 << 20) &&
                      ctx->h_outpin.reserve(zbytes + lbytes);   // (the direct copy is always possible)
  return finish_chains(ctx, k.who, e, k.itr, C, k.Z_out, k.lp_out, k.accept_rate_out, k.W_out, k.wall_elems,
                       staged ? ctx->h_outpin.get() : nullptr, &status);
}

// The streamed output map of the launch-per-step loop (the note at the top of this file): after transition t, push(t) puts the
// chains' current weights into ring slot t -- K4's own output where the proposal was accepted, the previous slot otherwise --
// and queues its DMA into pinned memory on the second stream; the host moves sample t - (R - 1) into the caller's array meanwhile.
struct WeightRing {
  si_ctx* ctx;
  const RwmhCall& k;
  bool select_path;   // the proposal weights of ALL chains are still in fw.w at accept time: one pass of launches carries them all
  double* slot(int64_t t) const { return ctx->d_wring + (size_t)(t % SI_WRING) * (size_t)k.C * (size_t)pad_ld(ctx->setup.model.N); }
  hipError_t drain(int64_t u) const {   // sample u of every chain: pinned slot -> the caller's (pageable) N x itr x C array
    const int64_t N = ctx->setup.model.N;
    const int r = (int)(u % SI_WRING);
    hipError_t w = hipEventSynchronize(ctx->ev_wcopy[r]);
    for (int c = 0; c < k.C && w == hipSuccess; ++c)
      host_copy(k.W_out + (size_t)N * ((size_t)u + (size_t)k.itr * c), ctx->h_wring[r] + (size_t)c * N, (size_t)N * sizeof(double));
    return w;
  }
  hipError_t push(int64_t t) const {
    const int64_t N = ctx->setup.model.N, ldw = pad_ld(N);
    const int32_t C = k.C;
    const int r = (int)(t % SI_WRING);
    hipError_t e = hipSuccess;
    if (t >= SI_WRING) e = hipStreamWaitEvent(ctx->stream, ctx->ev_wcopy[r], 0);  // the DMA of sample t - R has read this slot
    if (e != hipSuccess) return e;
    {
      ProfScope ps(ctx, SI_K_RECON, 0.0, 16.0 * (double)N * C);
      if (select_path)
        launch_weights_select(ctx->stream, ctx->d_accflag, ctx->fw.w, ldw, t > 0 ? slot(t - 1) : nullptr, slot(t), ldw, N, C, ctx->num_cu);
      else  // more chains than one pass of launches carries: K4 on the current states (same kernel, same bits)
        if (form_weights(ctx, ctx->chains.zcur, C, slot(t), ldw) != SI_OK) return hipErrorOutOfMemory;
    }
    e = hipEventRecord(ctx->ev_wcomp[r], ctx->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream2, ctx->ev_wcomp[r], 0);
    if (e == hipSuccess)
      e = hipMemcpy2DAsync(ctx->h_wring[r], (size_t)N * sizeof(double), slot(t), (size_t)ldw * sizeof(double), (size_t)N * sizeof(double),
                           (size_t)C, hipMemcpyDeviceToHost, ctx->stream2);
    if (e == hipSuccess) e = hipEventRecord(ctx->ev_wcopy[r], ctx->stream2);
    if (e == hipSuccess && t >= SI_WRING - 1) e = drain(t - (SI_WRING - 1));   // frees the pinned slot sample t + 1 will use
    return e;
  }
};

// ---- the launch-per-step loop: every chain the two loops above do not take.  One transition for all chains per pass; the
// transition index is a device-side counter, so the launches are identical.  When one pass of launches carries all chains (and
// the prior term is off) the tail of a transition is ONE launch: the last stage of the SSE reduction, the accept step and the
// next transition's proposal (rwmh_tail_kernel) -- same functions, same order, same bits; otherwise sse_final / accept / propose
// stay separate kernels.
// Replaying one captured transition as a hipGraph was measured and dropped: the README-toy transition takes 27.8 us graphed vs
// 25.7 us eager -- it is bound by the serial latency of its 8 dependent small kernels, not by host launches -- and at cfg2 a
// transition is 3.3 ms of kernel time.
static int32_t rwmh_per_step(si_ctx* ctx, const RwmhCall& k) {
  const int32_t C = k.C, M = ctx->setup.M;
  double* const dZ = ctx->chains.outZ;
  double* const dlp = ctx->chains.outlp;
  {
    ProfScope ps(ctx, SI_K_RWMH, 0, 0);
    launch_rwmh_init(ctx->stream, ctx->chains.zcur, ctx->chains.lpcur, ctx->chains.nacc, ctx->chains.steps, M, C);
  }
  const WeightRing ring{ctx, k, k.W_out && C <= ctx->fw.slots};
  int* const accflag = ring.select_path ? ctx->d_accflag.get() : nullptr;
  const bool fused_tail = C <= ctx->fw.slots && !(ctx->setup.sigma_p > 0.0) && ctx->chain_loop_enabled;
  const DensityView view = setup_view(ctx, /*defer_sse_final=*/fused_tail);   // the tail kernel sums the SSE block partials
  int32_t rc = SI_OK;
  hipError_t e = hipSuccess;
  for (int64_t t = 0; t < k.itr && rc == SI_OK && e == hipSuccess; ++t) {
    if (!fused_tail || t == 0) {
      ProfScope ps(ctx, SI_K_RWMH, 0, 0);
      launch_rwmh_propose(ctx->stream, ctx->chains.zcur, ctx->chains.zprop, M, C, k.sigma_z, k.seed, k.chain_id0, ctx->chains.steps);
    }
    if ((rc = eval_density_all(ctx, view, C)) != SI_OK) break;
    {
      ProfScope ps(ctx, SI_K_RWMH, 0, 0);
      if (fused_tail)
        launch_rwmh_tail(ctx->stream, ctx->fw.ssepart, ctx->setup.sse_blocks, ctx->chains.sse, ctx->chains.zcur, ctx->chains.zprop, ctx->chains.lpcur, ctx->chains.nacc, M,
                         C, k.c0, k.s2, k.sigma_z, k.seed, k.chain_id0, ctx->chains.steps, dZ, dlp, k.itr, accflag, t + 1 < k.itr);
      else
        launch_rwmh_accept(ctx->stream, ctx->chains.zcur, ctx->chains.zprop, ctx->chains.lpcur, ctx->chains.sse, ctx->chains.nacc, M, C, k.c0, k.s2, k.seed,
                           k.chain_id0, ctx->chains.steps, dZ, dlp, k.itr, ctx->setup.sigma_p > 0.0 ? ctx->chains.wsq.get() : nullptr, prior_c0(ctx),
                           prior_sp2(ctx), accflag);
    }
    if (k.W_out) e = ring.push(t);
  }
  if (rc == SI_OK && e == hipSuccess && k.W_out)   // the samples no later push has drained
    for (int64_t u = std::max<int64_t>(0, k.itr - (SI_WRING - 1)); u < k.itr && e == hipSuccess; ++u) e = ring.drain(u);
  if (k.W_out) (void)hipStreamSynchronize(ctx->stream2);
  if (rc != SI_OK || e != hipSuccess) {
    (void)hipStreamSynchronize(ctx->stream);
    if (rc != SI_OK) return rc;
    return fail(ctx, SI_ERR_HIP, std::string(k.who) + ": " + hipGetErrorString(e));
  }
  return finish_chains(ctx, k.who, hipGetLastError(), k.itr, C, k.Z_out, k.lp_out, k.accept_rate_out, nullptr, 0, nullptr, nullptr);
}

// The entry of si_sample_rwmh / si_sample_rwmh_weights: checks, the chains' state and the output arrays, then the three forms in
// this order -- the first that applies runs the call; finish_chains is their common end.
static int32_t sample_rwmh_impl(si_ctx* ctx, const char* who, int64_t itr, double sigma_z, uint64_t seed, int32_t chain_id0,
                                int32_t nchains, double* Z_out, double* lp_out, double* accept_rate_out, double* W_out) {
  CHECK_CTX(ctx);
  ctx->loop.last_density_spec = ctx->loop.last_loop_spec = 0;   // (si_chain_kernel_info reports THIS call)
  int32_t rc = infer_entry_check(ctx, who, bad_if(itr <= 0 || nchains <= 0 || chain_id0 < 0 || !(sigma_z > 0.0), "itr, nchains, sigma_z must be positive"));
  if (rc != SI_OK) return rc;
  BIND(ctx);
  const int32_t C = nchains;
  if ((rc = ensure_chains(ctx, C)) != SI_OK) return rc;
  if (W_out && (rc = ensure_wstream(ctx, C)) != SI_OK) return rc;
  // the device-side output arrays stay with the ctx (grown on demand, released with the inference set-up)
  if (!ctx->chains.outZ.reserve((size_t)ctx->setup.M * itr * C) || !ctx->chains.outlp.reserve((size_t)itr * C))
    return fail(ctx, SI_ERR_NOMEM, std::string(who) + ": output allocation failed");
  const double d = (double)ctx->setup.model.out_dim * (double)ctx->setup.B;
  const size_t wall_elems = (size_t)pad_ld(ctx->setup.model.N) * (size_t)itr * (size_t)C;
  const RwmhCall k{who, itr, sigma_z, seed, chain_id0, C, Z_out, lp_out, accept_rate_out, W_out, lik_c0(ctx, d),
                   lik_s2(ctx), wall_elems, !W_out || wall_elems <= ((size_t)512 << 20) / sizeof(double)};
  if ((rc = rwmh_one_workgroup(ctx, k)) != SI_NOT_TAKEN) return rc;
  if ((rc = rwmh_grid(ctx, k)) != SI_NOT_TAKEN) return rc;
  return rwmh_per_step(ctx, k);
}

int32_t si_sample_rwmh(si_ctx* ctx, int64_t itr, double sigma_z, uint64_t seed, int32_t chain_id0, int32_t nchains,
                       double* Z_out, double* lp_out, double* accept_rate_out) {
  return sample_rwmh_impl(ctx, "si_sample_rwmh", itr, sigma_z, seed, chain_id0, nchains, Z_out, lp_out, accept_rate_out, nullptr);
}

int32_t si_sample_rwmh_weights(si_ctx* ctx, int64_t itr, double sigma_z, uint64_t seed, int32_t chain_id0, int32_t nchains,
                               double* Z_out, double* lp_out, double* accept_rate_out, double* W_out) {
  if (ctx && !W_out) return fail(ctx, SI_ERR_INVALID, "si_sample_rwmh_weights: W_out is NULL (use si_sample_rwmh)");
  return sample_rwmh_impl(ctx, "si_sample_rwmh_weights", itr, sigma_z, seed, chain_id0, nchains, Z_out, lp_out, accept_rate_out, W_out);
}

// ---- step-wise RWMH: the same chain as si_sample_rwmh, but the SSE of every proposal passes through the caller
// between evaluation and acceptance, so that a DATA-SHARDED density (each rank holds B/world observations of X, Y and
// the same W_swa, P) can all-reduce the per-rank partial sums.  Every rank draws the same Philox
// stream (same seed / chain ids), so all ranks take identical accept decisions and keep identical chains.
int32_t si_set_chain_loop(si_ctx* ctx, int32_t on) {
  CHECK_CTX(ctx);
  if (on < 0 || on > 4)
    return fail(ctx, SI_ERR_INVALID, "si_set_chain_loop: 0 (one launch per layer and step), 1 (automatic), 2 (fused launches, no device-resident loop), "
                                     "3 / 4 (1 / 2 without the run-time specialised kernels)");
  ctx->chain_mode = on >= 3 ? on - 2 : on;
  ctx->chain_spec = on < 3;
  ctx->chain_loop_enabled = on != 0;
  return SI_OK;
}

int32_t si_chain_kernel_info(si_ctx* ctx, int32_t* density_specialised, int32_t* loop_specialised) {
  CHECK_CTX(ctx);
  if (density_specialised) *density_specialised = ctx->loop.last_density_spec;
  if (loop_specialised) *loop_specialised = ctx->loop.last_loop_spec;
  return SI_OK;
}

const char* si_chain_spec_message(si_ctx* ctx) { return ctx ? ctx->spec_message.c_str() : ""; }

int32_t si_rwmh_begin(si_ctx* ctx, int64_t itr, double sigma_z, uint64_t seed, int32_t chain_id0, int32_t nchains,
                      int64_t d_total) {
  CHECK_CTX(ctx);
  int32_t rc = infer_entry_check(ctx, "si_rwmh_begin", bad_if(itr <= 0 || nchains <= 0 || chain_id0 < 0 || !(sigma_z > 0.0) || d_total < 0, "itr, nchains, sigma_z must be positive"), SESSION_ANY);   // (an open session is replaced)
  if (rc != SI_OK) return rc;
  if (ctx->node.on && d_total > 0) return fail(ctx, SI_ERR_INVALID, "si_rwmh_begin: a data-sharded density (d_total > 0) is not available for NeuralODE models");
  if (lik_on(ctx) && d_total > 0)
    return fail(ctx, SI_ERR_INVALID, "si_rwmh_begin: a data-sharded density (d_total > 0) is not available with a categorical or bernoulli likelihood (si_infer_set_likelihood)");
  BIND(ctx);
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if ((rc = ensure_chains(ctx, nchains)) != SI_OK) return rc;
  StepSession& s = ctx->chains.session;
  s = StepSession();
  if (!s.Z.alloc((size_t)ctx->setup.M * itr * nchains) || !s.lp.alloc((size_t)itr * nchains)) {
    s = StepSession();
    return fail(ctx, SI_ERR_NOMEM, "si_rwmh_begin: output allocation failed");
  }
  s.itr = itr, s.sigma_z = sigma_z, s.seed = seed, s.chain0 = chain_id0, s.C = nchains;
  s.d = d_total > 0 ? (double)d_total : (double)ctx->setup.model.out_dim * (double)ctx->setup.B;
  launch_rwmh_init(ctx->stream, ctx->chains.zcur, ctx->chains.lpcur, ctx->chains.nacc, ctx->chains.steps, ctx->setup.M, nchains);
  SI_HIP(ctx, hipGetLastError());
  return SI_OK;
}

int32_t si_rwmh_step_eval(si_ctx* ctx, double* sse_local_out) {
  CHECK_CTX(ctx);
  StepSession& s = ctx->chains.session;
  if (!s.open() || s.next >= s.itr || s.evaluated)
    return fail(ctx, SI_ERR_STATE, "si_rwmh_step_eval: call si_rwmh_begin first / accept the pending step / chain finished");
  BIND(ctx);
  const int32_t C = s.C;
  launch_rwmh_propose(ctx->stream, ctx->chains.zcur, ctx->chains.zprop, ctx->setup.M, C, s.sigma_z, s.seed, s.chain0,
                      ctx->chains.steps);
  {
    const int32_t rc = eval_density_all(ctx, setup_view(ctx), C);   // (the deferred SSE stage off: chains.sse goes to the caller)
    if (rc != SI_OK) return rc;
  }
  if (sse_local_out) {  // NULL: the partial sums stay on the device (si_rwmh_sse_ptr) -- no copy, no synchronisation
    SI_HIP(ctx, hipMemcpyAsync(sse_local_out, ctx->chains.sse, (size_t)C * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  s.evaluated = true;
  return SI_OK;
}

int32_t si_rwmh_step_accept(si_ctx* ctx, const double* sse_total) {
  CHECK_CTX(ctx);
  StepSession& s = ctx->chains.session;
  if (!s.open() || !s.evaluated) return fail(ctx, SI_ERR_STATE, "si_rwmh_step_accept: no evaluated step pending");
  BIND(ctx);
  const int32_t C = s.C;
  if (sse_total) {  // NULL: the device buffer of si_rwmh_sse_ptr already holds the totals (all-reduced in place)
    SI_HIP(ctx, hipMemcpyAsync(ctx->chains.sse, sse_total, (size_t)C * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    SI_HIP(ctx, hipStreamSynchronize(ctx->stream));  // sse_total is caller-owned
  }
  const double c0 = lik_c0(ctx, s.d), s2 = lik_s2(ctx);
  launch_rwmh_accept(ctx->stream, ctx->chains.zcur, ctx->chains.zprop, ctx->chains.lpcur, ctx->chains.sse, ctx->chains.nacc, ctx->setup.M, C, c0, s2,
                     s.seed, s.chain0, ctx->chains.steps, s.Z, s.lp, s.itr,
                     ctx->setup.sigma_p > 0.0 ? ctx->chains.wsq : nullptr, prior_c0(ctx), prior_sp2(ctx));
  SI_HIP(ctx, hipGetLastError());
  s.next += 1;
  s.evaluated = false;
  return SI_OK;
}

int32_t si_rwmh_sse_ptr(si_ctx* ctx, double** sse_dev_out, int32_t* nchains_out) {
  CHECK_CTX(ctx);
  const StepSession& s = ctx->chains.session;
  if (!s.open()) return fail(ctx, SI_ERR_STATE, "si_rwmh_sse_ptr: call si_rwmh_begin first");
  if (sse_dev_out) *sse_dev_out = ctx->chains.sse;
  if (nchains_out) *nchains_out = s.C;
  return SI_OK;
}

int32_t si_rwmh_abort(si_ctx* ctx) {
  CHECK_CTX(ctx);
  BIND(ctx);
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->chains.session = StepSession();
  return SI_OK;
}

int32_t si_rwmh_end(si_ctx* ctx, double* Z_out, double* lp_out, double* accept_rate_out) {
  CHECK_CTX(ctx);
  StepSession& s = ctx->chains.session;
  if (!s.open() || s.next != s.itr || s.evaluated)
    return fail(ctx, SI_ERR_STATE, "si_rwmh_end: the chain is not complete");
  BIND(ctx);
  const int32_t C = s.C, M = ctx->setup.M;
  const int64_t itr = s.itr;
  std::vector<int64_t> nacc((size_t)C);
  if (Z_out) SI_HIP(ctx, hipMemcpyAsync(Z_out, s.Z, (size_t)M * itr * C * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (lp_out) SI_HIP(ctx, hipMemcpyAsync(lp_out, s.lp, (size_t)itr * C * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  SI_HIP(ctx, hipMemcpyAsync(nacc.data(), ctx->chains.nacc, (size_t)C * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  s = StepSession();
  accept_rates(nacc, itr, accept_rate_out);
  return SI_OK;
}

// Output map a13 (space_inference.jl:125: one W_swa + P z per sample, itr x N doubles on the host -- 8.4 GB at cfg2).
// A three-stage pipeline so that the PCIe link, not a single host thread, sets the pace: K4 writes a group of samples
// into one of two device buffers (compute stream) -> DMA into one of two PINNED staging buffers (copy stream) -> a few
// host threads move the previous group from the staging buffer into the caller's (pageable, usually never-touched)
// array (its first-touch page faults are spread over those threads too; a MADV_HUGEPAGE hint was tried and gained nothing).  A plain hipMemcpy into pageable memory does the last two steps on one thread: 0.79 ms per 8.4 MB sample.
int32_t si_reconstruct(si_ctx* ctx, const double* Z, int64_t C, double* W_out) {
  CHECK_CTX(ctx);
  const int32_t rc0 = infer_entry_check(ctx, "si_reconstruct", bad_if(!Z || C <= 0 || !W_out), SESSION_ANY);
  if (rc0 != SI_OK) return rc0;
  BIND(ctx);
  const int64_t N = ctx->setup.model.N, ldw = pad_ld(N);
  const int32_t M = ctx->setup.M;
  // samples per pipeline stage: ~32 MB of output, at most 64 samples, and at least four stages when C allows it
  const int64_t group_cap = std::max<int64_t>(1, std::min<int64_t>(64, ((int64_t)32 << 20) / (N * 8)));   // sizes the buffers once per N
  const int64_t group = std::max<int64_t>(1, std::min<int64_t>((C + 3) / 4, group_cap));
  Event ev_comp[2], ev_copy[2];
  hipError_t e = hipSuccess;
  if (!ctx->stream2) e = hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking);
  // (the last buffer of each group tells whether all of the group are there and large enough)
  if (e == hipSuccess && (ctx->d_stage[1].size() < (size_t)ldw * (size_t)group_cap || ctx->d_zstage[1].size() < (size_t)M * (size_t)group_cap)) {
    (void)hipStreamSynchronize(ctx->stream);
    for (int b = 0; b < 2; ++b) {
      ctx->d_stage[b].reset();
      ctx->d_zstage[b].reset();
    }
    for (int b = 0; b < 2 && e == hipSuccess; ++b)
      if (!ctx->d_stage[b].alloc((size_t)ldw * group_cap) || !ctx->d_zstage[b].alloc((size_t)M * group_cap)) e = hipErrorOutOfMemory;
    if (e != hipSuccess) ctx->d_stage[1].reset(), ctx->d_zstage[1].reset();
  }
  const DevBuf<double>* dW = ctx->d_stage;
  const DevBuf<double>* dZ = ctx->d_zstage;
  if (e == hipSuccess && ctx->h_stage[1].size() < (size_t)N * (size_t)group_cap) {   // the staging buffers stay with the context
    for (int b = 0; b < 2; ++b) ctx->h_stage[b].reset();
    for (int b = 0; b < 2 && e == hipSuccess; ++b) e = ctx->h_stage[b].try_alloc((size_t)N * group_cap);
  }
  const PinBuf<double>* hp = ctx->h_stage;
  for (int b = 0; b < 2 && e == hipSuccess; ++b) {
    e = ev_comp[b].try_create();
    if (e == hipSuccess) e = ev_copy[b].try_create();
  }
  auto drain = [&](int64_t g) {   // group g has been DMA'd into its staging buffer: move it into the caller's array
    const int b = (int)(g & 1);
    const int64_t c0 = g * group, nc = std::min(group, C - c0);
    hipError_t w = hipEventSynchronize(ev_copy[b]);
    if (w == hipSuccess) host_copy(W_out + c0 * N, hp[b], (size_t)N * (size_t)nc * sizeof(double));
    return w;
  };
  const int64_t ngroups = (C + group - 1) / group;
  for (int64_t g = 0; g < ngroups && e == hipSuccess; ++g) {
    const int b = (int)(g & 1);
    const int64_t c0 = g * group, nc = std::min(group, C - c0);
    // dW[b] / dZ[b] are free once the DMA of group g - 2 has read them; hp[b] once that group has been drained (below)
    if (g >= 2) e = hipStreamWaitEvent(ctx->stream, ev_copy[b], 0);
    if (e == hipSuccess) e = hipMemcpyAsync(dZ[b], Z + c0 * M, (size_t)M * nc * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) break;
    {
      ProfScope ps(ctx, SI_K_RECON, 2.0 * (double)N * M * nc, (double)N * (M + 1 + nc) * 8.0);
      if (form_weights(ctx, dZ[b], (int32_t)nc, dW[b], ldw) != SI_OK) e = hipErrorOutOfMemory;
    }
    if (e != hipSuccess) break;
    e = hipEventRecord(ev_comp[b], ctx->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream2, ev_comp[b], 0);
    if (e == hipSuccess)
      e = hipMemcpy2DAsync(hp[b], (size_t)N * sizeof(double), dW[b], (size_t)ldw * sizeof(double), (size_t)N * sizeof(double), (size_t)nc,
                           hipMemcpyDeviceToHost, ctx->stream2);
    if (e == hipSuccess) e = hipEventRecord(ev_copy[b], ctx->stream2);
    if (e == hipSuccess && g >= 1) e = drain(g - 1);   // overlaps the DMA of group g
  }
  if (e == hipSuccess) e = drain(ngroups - 1);
  (void)hipStreamSynchronize(ctx->stream2);
  (void)hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return fail(ctx, e == hipErrorOutOfMemory ? SI_ERR_NOMEM : SI_ERR_HIP, std::string("si_reconstruct: ") + hipGetErrorString(e));
  return SI_OK;
}

}  // extern "C"
