// C ABI, MALA (reference src/space_inference.jl:117-120): si_sample_mala, si_mala_kernel_info.  The transition is defined once, in
// kernels_mala.hip; this file queues it.  Host-side orchestration only; no CPU fallback anywhere in this file.
//
// One definition, one audit (tests/mala_audit.py), on the two routes of the stacked evaluator (StackedVgrad, capi_infer.hip): per
// transition one evaluation at the proposals, then mala_accept_kernel.
#include "capi_common.h"

using namespace si;

extern "C" {

int32_t si_sample_mala(si_ctx* ctx, int64_t itr, double sigma_z, uint64_t seed, int32_t chain_id0, int32_t nchains, double* Z_out,
                       double* lp_out, double* accept_rate_out, double* G_out) {
  CHECK_CTX(ctx);
  const char* who = "si_sample_mala";
  ctx->mala.info = CallInfo();   // (si_mala_kernel_info reports THIS call)
  int32_t rc = infer_entry_check(ctx, who, bad_if(!(itr > 0 && nchains > 0 && chain_id0 >= 0 && sigma_z > 0.0)), SESSION_SHARED, true);
  if (rc != SI_OK) return rc;
  BIND(ctx);
  const int32_t C = nchains, M = ctx->setup.M;
  if ((rc = reserve_chain_state(ctx, who, C)) != SI_OK) return rc;
  if ((rc = reserve_state(ctx, who, ctx->mala.cap, C, [&] { return ctx->mala.nacc.alloc((size_t)C); })) != SI_OK) return rc;
  const size_t zelems = (size_t)M * (size_t)itr * (size_t)C;
  if (!ctx->chains.outZ.reserve(zelems) || !ctx->chains.outlp.reserve((size_t)itr * C) || (G_out && !ctx->mala.outG.reserve(zelems)))
    return fail(ctx, SI_ERR_NOMEM, std::string(who) + ": output allocation failed");
  MalaRun a;
  chain_run_args(a, ctx, itr, sigma_z, seed, chain_id0, G_out != nullptr);
  a.nacc = ctx->mala.nacc;
  a.h = 0.5 * (sigma_z * sigma_z);
  StackedVgrad vg;
  if ((rc = vg.open(ctx, who, C)) != SI_OK) return rc;
  hipError_t e = hipSuccess;
  {
    ProfScope ps(ctx, SI_K_RWMH, 0, 0);
    launch_mala_propose(ctx->stream, a, C, 0, true);
    e = hipGetLastError();
  }
  for (int64_t t = 0; t < itr && e == hipSuccess && rc == SI_OK; ++t) {
    eval_pending(ctx, vg, e, rc);
    if (e != hipSuccess || rc != SI_OK) break;
    ProfScope ps(ctx, SI_K_RWMH, 0, 0);
    launch_mala_accept(ctx->stream, a, C, (uint64_t)t, t + 1 < itr);
    e = hipGetLastError();
  }
  std::vector<int64_t> nacc((size_t)C);
  rc = finish_downloads(ctx, who, e, rc, {{Z_out, ctx->chains.outZ, zelems * sizeof(double)},
                                          {lp_out, ctx->chains.outlp, (size_t)itr * C * sizeof(double)},
                                          {G_out, a.G_out, zelems * sizeof(double)},
                                          {nacc.data(), ctx->mala.nacc, (size_t)C * sizeof(int64_t)}});
  if (rc != SI_OK) return rc;
  accept_rates(nacc, itr, accept_rate_out);
  ctx->mala.info = call_info(vg);
  return SI_OK;
}

int32_t si_mala_kernel_info(si_ctx* ctx, int32_t* fused_out, int32_t* passes_out) {
  CHECK_CTX(ctx);
  if (fused_out) *fused_out = ctx->mala.info.fused;
  if (passes_out) *passes_out = ctx->mala.info.passes;
  return SI_OK;
}

}  // extern "C"
