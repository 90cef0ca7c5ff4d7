// C ABI, MALA (reference src/space_inference.jl:117-120): si_sample_mala, si_mala_kernel_info.  The transition is defined once, in
// kernels_mala.hip; this file queues it.  Host-side orchestration only; no CPU fallback anywhere in this file.
//
// Two routes, one definition, one audit (tests/mala_audit.py):
//   fused   chains of si_logdensity_grad_batch's fused class: per transition launch_reconstruct, launch_chain_vgrad,
//           launch_chain_vgrad_reduce (once per pass of vg_cap chains, outputs left on the device) and mala_accept_kernel are queued
//           on the stream; the chain state never leaves the device, nothing is copied and nothing synchronises until the tail.
//           A launch-queued loop: no persistent kernel, no grid barrier, nothing that can spin.
//   other   every other chain (Conv / MaxPool / flatten, SI_F32, the four later activations, wide layers): the same two MALA
//           kernels, but the proposals come down to the host, their values and gradients are computed column by column by
//           si_logdensity_grad's own path and go back up before the accept kernel.  SLOW AND SYNCHRONISING: one round trip per
//           chain and transition; it exists so that every chain the gradient covers has the device sampler's definition.
#include "capi_common.h"

using namespace si;

extern "C" {

int32_t si_sample_mala(si_ctx* ctx, int64_t itr, double sigma_z, uint64_t seed, int32_t chain_id0, int32_t nchains, double* Z_out,
                       double* lp_out, double* accept_rate_out, double* G_out) {
  CHECK_CTX(ctx);
  const char* who = "si_sample_mala";
  ctx->last_mala_fused = ctx->last_mala_passes = 0;   // (si_mala_kernel_info reports THIS call)
  int32_t rc = grad_entry_check(ctx, who, itr > 0 && nchains > 0 && chain_id0 >= 0 && sigma_z > 0.0);
  if (rc != SI_OK) return rc;
  BIND(ctx);
  const int32_t C = nchains, M = ctx->iM;
  if (ctx->mala_cap < C) {
    SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->mala_cap = 0;
    const size_t mc = (size_t)M * (size_t)C;
    if (!ctx->d_mala_z.alloc(mc) || !ctx->d_mala_g.alloc(mc) || !ctx->d_mala_zp.alloc(mc) || !ctx->d_mala_gp.alloc(mc) ||
        !ctx->d_mala_lp.alloc((size_t)C) || !ctx->d_mala_lpp.alloc((size_t)C) || !ctx->d_mala_nacc.alloc((size_t)C))
      return fail(ctx, SI_ERR_NOMEM, std::string(who) + ": sampler state allocation failed");
    ctx->mala_cap = C;
  }
  const size_t zelems = (size_t)M * (size_t)itr * (size_t)C;
  if (!ctx->d_outZ.reserve(zelems) || !ctx->d_outlp.reserve((size_t)itr * C) || (G_out && !ctx->d_outG.reserve(zelems)))
    return fail(ctx, SI_ERR_NOMEM, std::string(who) + ": output allocation failed");
  double* const dG = G_out ? ctx->d_outG.get() : nullptr;
  int64_t G = 0, fit = 0;
  const int nb = vgrad_route(ctx, &G, &fit);
  const bool fused = fit >= 1;
  if (fused && (rc = vgrad_ensure(ctx, who, (int)std::min<int64_t>(fit, C), G)) != SI_OK) return rc;
  const int passes = fused ? (C + ctx->vg_cap - 1) / ctx->vg_cap : C;
  std::vector<double> hz, hlp, hg;   // the other route's host images of the proposals, their values and gradients
  if (!fused) {
    hz.resize((size_t)M * C);
    hlp.resize((size_t)C);
    hg.resize((size_t)M * C);
  }
  hipError_t e = hipSuccess;
  {
    ProfScope ps(ctx, SI_K_RWMH, 0, 0);
    launch_mala_propose(ctx->stream, ctx->d_mala_z, ctx->d_mala_g, ctx->d_mala_zp, M, C, sigma_z, seed, chain_id0, 0, true);
    e = hipGetLastError();
  }
  for (int64_t t = 0; t < itr && e == hipSuccess && rc == SI_OK; ++t) {
    if (fused) {
      for (int32_t p0 = 0; p0 < C; p0 += ctx->vg_cap)
        vgrad_pass(ctx, nb, G, ctx->d_mala_zp + (size_t)M * p0, std::min<int32_t>(ctx->vg_cap, C - p0), ctx->d_mala_lpp + p0,
                   ctx->d_mala_gp + (size_t)M * p0);
      e = hipGetLastError();
    } else {
      e = hipMemcpyAsync(hz.data(), ctx->d_mala_zp, hz.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // (also: the uploads of transition t - 1 have left hlp / hg)
      for (int32_t c = 0; c < C && e == hipSuccess && rc == SI_OK; ++c)
        rc = logdensity_grad_point(ctx, hz.data() + (size_t)M * c, hlp.data() + c, hg.data() + (size_t)M * c);
      if (rc != SI_OK) break;
      if (e == hipSuccess) e = hipMemcpyAsync(ctx->d_mala_lpp, hlp.data(), hlp.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
      if (e == hipSuccess) e = hipMemcpyAsync(ctx->d_mala_gp, hg.data(), hg.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    }
    if (e != hipSuccess) break;
    ProfScope ps(ctx, SI_K_RWMH, 0, 0);
    launch_mala_accept(ctx->stream, ctx->d_mala_z, ctx->d_mala_lp, ctx->d_mala_g, ctx->d_mala_zp, ctx->d_mala_lpp, ctx->d_mala_gp,
                       ctx->d_mala_nacc, M, C, sigma_z, seed, chain_id0, (uint64_t)t, ctx->d_outZ, ctx->d_outlp, dG, itr, t + 1 < itr);
    e = hipGetLastError();
  }
  // the common tail (the pattern of finish_chains, capi_sample.hip): the downloads, ONE synchronisation, the first error reported
  std::vector<int64_t> nacc((size_t)C);
  const bool ok = e == hipSuccess && rc == SI_OK;
  if (ok && Z_out) e = hipMemcpyAsync(Z_out, ctx->d_outZ, zelems * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
  if (ok && e == hipSuccess && lp_out)
    e = hipMemcpyAsync(lp_out, ctx->d_outlp, (size_t)itr * C * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
  if (ok && e == hipSuccess && G_out) e = hipMemcpyAsync(G_out, dG, zelems * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
  if (ok && e == hipSuccess)
    e = hipMemcpyAsync(nacc.data(), ctx->d_mala_nacc, (size_t)C * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t e2 = hipStreamSynchronize(ctx->stream);
  if (rc != SI_OK) return rc;
  if (e != hipSuccess) return fail(ctx, SI_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
  if (e2 != hipSuccess) return fail(ctx, SI_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e2));
  accept_rates(nacc, itr, accept_rate_out);
  ctx->last_mala_fused = fused ? 1 : 0;
  ctx->last_mala_passes = passes;
  return SI_OK;
}

int32_t si_mala_kernel_info(si_ctx* ctx, int32_t* fused_out, int32_t* passes_out) {
  CHECK_CTX(ctx);
  if (fused_out) *fused_out = ctx->last_mala_fused;
  if (passes_out) *passes_out = ctx->last_mala_passes;
  return SI_OK;
}

}  // extern "C"
