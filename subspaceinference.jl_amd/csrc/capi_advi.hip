// C ABI, ADVI (reference src/space_inference.jl:126-138): si_fit_advi, si_advi_kernel_info.  The step is defined once, in
// kernels_advi.hip (the contract: include/subspace_hip.h); this file queues it.  Host-side orchestration only; no CPU fallback
// anywhere in this file.
//
// Two routes, one definition, one audit (tests/advi_audit.py):
//   fused   chains of si_logdensity_grad_batch's fused class: per step the R S points go through vgrad_pass (launch_reconstruct,
//           launch_chain_vgrad, launch_chain_vgrad_reduce) once per pass of vg_cap points, outputs left on the device, then ONE
//           advi_update_kernel launch, which also forms the next step's points: 3 passes + 1 launches per step.  The state never
//           leaves the device, nothing is copied and nothing synchronises until the tail.  A launch-queued loop: no persistent
//           kernel, no grid barrier, nothing that can spin.
//   other   every other chain (Conv / MaxPool / flatten, SI_F32, the four later activations, wide layers): the same two kernels,
//           but the points come down to the host, their values and gradients are computed column by column by
//           si_logdensity_grad's own path and go back up before the update kernel.  SLOW AND SYNCHRONISING: one round trip per
//           point and step; it exists so that every chain the gradient covers has the device fit's definition.
#include "capi_common.h"

using namespace si;

extern "C" {

int32_t si_fit_advi(si_ctx* ctx, int64_t max_iters, int32_t samples_per_step, double sigma_z, double eta, double tau, int32_t window,
                    uint64_t seed, int32_t chain_id0, int32_t nruns, int64_t ndraws, double* theta_out, double* Z_out, double* elbo_out,
                    double* theta_trace_out, double* points_out) {
  CHECK_CTX(ctx);
  const char* who = "si_fit_advi";
  ctx->last_advi_fused = ctx->last_advi_passes = 0;   // (si_advi_kernel_info reports THIS call)
  const int64_t T = max_iters, D = ndraws;
  const int32_t S = samples_per_step, W = window, R = nruns;
  // (the comparisons are written so that a NaN refuses; S nblk < 2^24: the Philox block field of the step draws)
  const bool args_ok = T >= 1 && S >= 1 && W >= 1 && W <= 1024 && R >= 1 && chain_id0 >= 0 && sigma_z > 0.0 && tau > 0.0 && eta > 0.0 &&
                       D >= 0 && theta_out && (D == 0 || Z_out);
  int32_t rc = grad_entry_check(ctx, who, args_ok);
  if (rc != SI_OK) return rc;
  const int32_t M = ctx->iM;
  if ((int64_t)S * ((M + 1) / 2) >= ((int64_t)1 << 24) || (int64_t)R * S > INT32_MAX)
    return fail(ctx, SI_ERR_INVALID, std::string(who) + ": bad argument (samples_per_step * ceil(M / 2) must stay below 2^24)");
  BIND(ctx);
  const size_t m = (size_t)M, pts = m * (size_t)S * (size_t)R;
  const size_t trace_elems = 2 * m * (size_t)(T + 1) * (size_t)R, ptsout_elems = m * (size_t)S * (size_t)T * (size_t)R;
  const size_t z_elems = m * (size_t)D * (size_t)R;
  if (!ctx->d_advi_theta.reserve(2 * m * R) || !ctx->d_advi_ring.reserve((size_t)W * 2 * m * R) || !ctx->d_advi_eta.reserve(pts) ||
      !ctx->d_advi_z.reserve(pts) || !ctx->d_advi_g.reserve(pts) || !ctx->d_advi_lp.reserve((size_t)S * R))
    return fail(ctx, SI_ERR_NOMEM, std::string(who) + ": state allocation failed");
  if ((D > 0 && !ctx->d_outZ.reserve(z_elems)) || (elbo_out && !ctx->d_outlp.reserve((size_t)T * R)) ||
      (theta_trace_out && !ctx->d_advi_trace.reserve(trace_elems)) || (points_out && !ctx->d_advi_pts.reserve(ptsout_elems)))
    return fail(ctx, SI_ERR_NOMEM, std::string(who) + ": output allocation failed");
  double* const d_elbo = elbo_out ? ctx->d_outlp.get() : nullptr;
  AdviRun a;
  a.theta = ctx->d_advi_theta, a.ring = ctx->d_advi_ring, a.eta = ctx->d_advi_eta, a.z = ctx->d_advi_z;
  a.trace_out = theta_trace_out ? ctx->d_advi_trace.get() : nullptr;
  a.pts_out = points_out ? ctx->d_advi_pts.get() : nullptr;
  a.M = M, a.S = S, a.W = W, a.chain_id0 = chain_id0, a.T = T, a.seed = seed;
  const int32_t C = R * S;   // the points of one step, run by run
  int64_t G = 0, fit = 0;
  const int nb = vgrad_route(ctx, &G, &fit);
  const bool fused = fit >= 1;
  if (fused && (rc = vgrad_ensure(ctx, who, (int)std::min<int64_t>(fit, C), G)) != SI_OK) return rc;
  const int passes = fused ? (C + ctx->vg_cap - 1) / ctx->vg_cap : C;
  std::vector<double> hz, hlp, hg;   // the other route's host images of the points, their values and gradients
  if (!fused) {
    hz.resize(pts);
    hlp.resize((size_t)C);
    hg.resize(pts);
  }
  hipError_t e = hipSuccess;
  {
    ProfScope ps(ctx, SI_K_RWMH, 0, 0);
    launch_advi_draw(ctx->stream, a, R, sigma_z, true, false, nullptr, 0);
    e = hipGetLastError();
  }
  for (int64_t t = 0; t < T && e == hipSuccess && rc == SI_OK; ++t) {
    if (fused) {
      for (int32_t p0 = 0; p0 < C; p0 += ctx->vg_cap)
        vgrad_pass(ctx, nb, G, ctx->d_advi_z + m * p0, std::min<int32_t>(ctx->vg_cap, C - p0), ctx->d_advi_lp + p0, ctx->d_advi_g + m * p0);
      e = hipGetLastError();
    } else {
      e = hipMemcpyAsync(hz.data(), ctx->d_advi_z, pts * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // (also: the uploads of step t - 1 have left hlp / hg)
      for (int32_t c = 0; c < C && e == hipSuccess && rc == SI_OK; ++c)
        rc = logdensity_grad_point(ctx, hz.data() + m * c, hlp.data() + c, hg.data() + m * c);
      if (rc != SI_OK) break;
      if (e == hipSuccess) e = hipMemcpyAsync(ctx->d_advi_lp, hlp.data(), hlp.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
      if (e == hipSuccess) e = hipMemcpyAsync(ctx->d_advi_g, hg.data(), hg.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    }
    if (e != hipSuccess) break;
    ProfScope ps(ctx, SI_K_RWMH, 0, 0);
    launch_advi_update(ctx->stream, a, R, ctx->d_advi_lp, ctx->d_advi_g, eta, tau, t, d_elbo, t + 1 < T);
    e = hipGetLastError();
  }
  if (e == hipSuccess && rc == SI_OK && D > 0) {
    ProfScope ps(ctx, SI_K_RWMH, 0, 0);
    launch_advi_draw(ctx->stream, a, R, sigma_z, false, true, ctx->d_outZ, D);
    e = hipGetLastError();
  }
  // the common tail (the pattern of si_sample_mala): the downloads, ONE synchronisation, the first error reported
  const bool ok = e == hipSuccess && rc == SI_OK;
  auto down = [&](double* dst, const double* src, size_t n) {
    if (ok && e == hipSuccess && dst) e = hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
  };
  down(theta_out, ctx->d_advi_theta, 2 * m * R);
  if (D > 0) down(Z_out, ctx->d_outZ, z_elems);
  down(elbo_out, d_elbo, (size_t)T * R);
  down(theta_trace_out, a.trace_out, trace_elems);
  down(points_out, a.pts_out, ptsout_elems);
  const hipError_t e2 = hipStreamSynchronize(ctx->stream);
  if (rc != SI_OK) return rc;
  if (e != hipSuccess) return fail(ctx, SI_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
  if (e2 != hipSuccess) return fail(ctx, SI_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e2));
  ctx->last_advi_fused = fused ? 1 : 0;
  ctx->last_advi_passes = passes;
  return SI_OK;
}

int32_t si_advi_kernel_info(si_ctx* ctx, int32_t* fused_out, int32_t* passes_out) {
  CHECK_CTX(ctx);
  if (fused_out) *fused_out = ctx->last_advi_fused;
  if (passes_out) *passes_out = ctx->last_advi_passes;
  return SI_OK;
}

}  // extern "C"
