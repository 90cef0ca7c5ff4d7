// C ABI, ADVI (reference src/space_inference.jl:126-138): si_fit_advi, si_advi_kernel_info.  The step is defined once, in
// kernels_advi.hip (the contract: include/subspace_hip.h); this file queues it.  Host-side orchestration only; no CPU fallback
// anywhere in this file.
//
// One definition, one audit (tests/advi_audit.py), on the two routes of the stacked evaluator (StackedVgrad, capi_infer.hip): per
// step one evaluation at the R S points, then ONE advi_update_kernel launch, which also forms the next step's points.
#include "capi_common.h"

using namespace si;

extern "C" {

int32_t si_fit_advi(si_ctx* ctx, int64_t max_iters, int32_t samples_per_step, double sigma_z, double eta, double tau, int32_t window,
                    uint64_t seed, int32_t chain_id0, int32_t nruns, int64_t ndraws, double* theta_out, double* Z_out, double* elbo_out,
                    double* theta_trace_out, double* points_out) {
  CHECK_CTX(ctx);
  const char* who = "si_fit_advi";
  ctx->advi.info = CallInfo();   // (si_advi_kernel_info reports THIS call)
  const int64_t T = max_iters, D = ndraws;
  const int32_t S = samples_per_step, W = window, R = nruns;
  // (the comparisons are written so that a NaN refuses; S nblk < 2^24: the Philox block field of the step draws)
  const bool args_ok = T >= 1 && S >= 1 && W >= 1 && W <= 1024 && R >= 1 && chain_id0 >= 0 && sigma_z > 0.0 && tau > 0.0 && eta > 0.0 &&
                       D >= 0 && theta_out && (D == 0 || Z_out);
  int32_t rc = infer_entry_check(ctx, who, bad_if(!args_ok), SESSION_SHARED, true);
  if (rc != SI_OK) return rc;
  const int32_t M = ctx->setup.M;
  if ((int64_t)S * ((M + 1) / 2) >= ((int64_t)1 << 24) || (int64_t)R * S > INT32_MAX)
    return fail(ctx, SI_ERR_INVALID, std::string(who) + ": bad argument (samples_per_step * ceil(M / 2) must stay below 2^24)");
  BIND(ctx);
  const size_t m = (size_t)M, pts = m * (size_t)S * (size_t)R;
  const size_t trace_elems = 2 * m * (size_t)(T + 1) * (size_t)R, ptsout_elems = m * (size_t)S * (size_t)T * (size_t)R;
  const size_t z_elems = m * (size_t)D * (size_t)R;
  if (!ctx->advi.theta.reserve(2 * m * R) || !ctx->advi.ring.reserve((size_t)W * 2 * m * R) || !ctx->advi.eta.reserve(pts) ||
      !ctx->advi.z.reserve(pts) || !ctx->advi.g.reserve(pts) || !ctx->advi.lp.reserve((size_t)S * R))
    return fail(ctx, SI_ERR_NOMEM, std::string(who) + ": state allocation failed");
  if ((D > 0 && !ctx->chains.outZ.reserve(z_elems)) || (elbo_out && !ctx->chains.outlp.reserve((size_t)T * R)) ||
      (theta_trace_out && !ctx->advi.trace.reserve(trace_elems)) || (points_out && !ctx->advi.pts.reserve(ptsout_elems)))
    return fail(ctx, SI_ERR_NOMEM, std::string(who) + ": output allocation failed");
  double* const d_elbo = elbo_out ? ctx->chains.outlp.get() : nullptr;
  AdviRun a;
  a.theta = ctx->advi.theta, a.ring = ctx->advi.ring, a.eta = ctx->advi.eta, a.z = ctx->advi.z;
  a.trace_out = theta_trace_out ? ctx->advi.trace.get() : nullptr;
  a.pts_out = points_out ? ctx->advi.pts.get() : nullptr;
  a.M = M, a.S = S, a.W = W, a.chain_id0 = chain_id0, a.T = T, a.seed = seed;
  const int32_t C = R * S;   // the points of one step, run by run
  StackedVgrad vg;
  if ((rc = vg.open(ctx, who, C)) != SI_OK) return rc;
  hipError_t e = hipSuccess;
  {
    ProfScope ps(ctx, SI_K_RWMH, 0, 0);
    launch_advi_draw(ctx->stream, a, R, sigma_z, true, false, nullptr, 0);
    e = hipGetLastError();
  }
  for (int64_t t = 0; t < T && e == hipSuccess && rc == SI_OK; ++t) {
    vg.eval(ctx->advi.z, ctx->advi.lp, ctx->advi.g, e, rc);
    if (e != hipSuccess || rc != SI_OK) break;
    ProfScope ps(ctx, SI_K_RWMH, 0, 0);
    launch_advi_update(ctx->stream, a, R, ctx->advi.lp, ctx->advi.g, eta, tau, t, d_elbo, t + 1 < T);
    e = hipGetLastError();
  }
  if (e == hipSuccess && rc == SI_OK && D > 0) {
    ProfScope ps(ctx, SI_K_RWMH, 0, 0);
    launch_advi_draw(ctx->stream, a, R, sigma_z, false, true, ctx->chains.outZ, D);
    e = hipGetLastError();
  }
  const size_t f64 = sizeof(double);
  rc = finish_downloads(ctx, who, e, rc, {{theta_out, ctx->advi.theta, 2 * m * R * f64},
                                          {D > 0 ? Z_out : nullptr, ctx->chains.outZ, z_elems * f64},
                                          {elbo_out, d_elbo, (size_t)T * R * f64},
                                          {theta_trace_out, a.trace_out, trace_elems * f64},
                                          {points_out, a.pts_out, ptsout_elems * f64}});
  if (rc != SI_OK) return rc;
  ctx->advi.info = call_info(vg);
  return SI_OK;
}

int32_t si_advi_kernel_info(si_ctx* ctx, int32_t* fused_out, int32_t* passes_out) {
  CHECK_CTX(ctx);
  if (fused_out) *fused_out = ctx->advi.info.fused;
  if (passes_out) *passes_out = ctx->advi.info.passes;
  return SI_OK;
}

}  // extern "C"
