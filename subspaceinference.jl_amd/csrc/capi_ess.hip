// C ABI, elliptical slice sampling (not in the reference): si_sample_ess, si_ess_kernel_info.  The transition is defined once, in
// kernels_ess.hip; this file queues it.  Host-side orchestration only; no CPU fallback anywhere in this file.
//
// The sampler needs values only, so it rides the stacked value path of the RWMH samplers -- eval_density_all on chains.zprop,
// fw.slots chains per pass of launches -- for every density the library evaluates: Conv chains, SI_F32, the decoder route, the
// categorical and Bernoulli likelihoods, a NeuralODE with or without si_node_set_grad.  The shrink loop of a transition is data
// dependent, so EVERY ROUND SYNCHRONISES (value_round, capi_common.h): one evaluation at the chains' pending points, a memset of
// the open word, ess_round_kernel and a 4-byte read-back of how many chains still shrink -- the pattern of a NUTS leaf, value only.
// Chains advance in lock-step within a transition: a chain that has kept a point waits for the others with that point in its slot,
// which is evaluated and ignored.  A transition takes at most max_evals rounds.
#include "capi_common.h"

using namespace si;

extern "C" {

int32_t si_sample_ess(si_ctx* ctx, int64_t itr, double sigma_z, int32_t max_evals, uint64_t seed, int32_t chain_id0, int32_t nchains,
                      double* Z_out, double* lp_out, int32_t* nev_out, double* theta_out) {
  CHECK_CTX(ctx);
  const char* who = "si_sample_ess";
  ctx->ess.passes = 0, ctx->ess.rounds = ctx->ess.evals = 0;   // (si_ess_kernel_info reports THIS call)
  // (every comparison is false for a NaN: refused.  max_evals: the block field of a Philox counter has 24 bits)
  int32_t rc = infer_entry_check(ctx, who, bad_if(!(itr > 0 && nchains > 0 && chain_id0 >= 0 && sigma_z > 0.0 && max_evals >= 1 && max_evals <= (1 << 24)),
                                                  "itr, nchains, sigma_z must be positive, max_evals in 1 .. 2^24"), SESSION_SHARED);
  if (rc != SI_OK) return rc;
  BIND(ctx);
  const int32_t C = nchains, M = ctx->setup.M;
  if ((rc = ensure_chains(ctx, C)) != SI_OK) return rc;
  EssState& s = ctx->ess;
  if ((rc = reserve_state(ctx, who, s.cap, C, [&] {
         const size_t c = (size_t)C;
         return s.nu.alloc((size_t)M * c) && s.logy.alloc(c) && s.theta.alloc(c) && s.lo.alloc(c) && s.hi.alloc(c) && s.k.alloc(c) && s.closed.alloc(c) &&
                s.open.alloc(1);
       })) != SI_OK)
    return rc;
  const size_t zelems = (size_t)M * (size_t)itr * (size_t)C, selems = (size_t)itr * (size_t)C;
  if (!ctx->chains.outZ.reserve(zelems) || !ctx->chains.outlp.reserve(selems) || !s.outnev.reserve(selems) || !s.outtheta.reserve(selems))
    return fail(ctx, SI_ERR_NOMEM, std::string(who) + ": output allocation failed");
  const double d = (double)ctx->setup.model.out_dim * (double)ctx->setup.B;
  const EssRun a{ctx->chains.zcur, ctx->chains.lpcur, ctx->chains.zprop, s.nu, ctx->chains.sse, ctx->setup.sigma_p > 0.0 ? ctx->chains.wsq.get() : nullptr,
                 s.logy, s.theta, s.lo, s.hi, s.k, s.closed, ctx->chains.outZ, ctx->chains.outlp, s.outtheta, s.outnev,
                 M, chain_id0, max_evals, itr, seed, sigma_z, lik_c0(ctx, d), lik_s2(ctx), prior_c0(ctx), prior_sp2(ctx)};
  hipError_t e = hipSuccess;
  int64_t rounds = 0;
  for (int64_t t = 0; t < itr && e == hipSuccess && rc == SI_OK; ++t) {
    {
      ProfScope ps(ctx, SI_K_RWMH, 0, 0);
      if (t == 0)
        launch_ess_init(ctx->stream, a, C);
      else
        launch_ess_begin(ctx->stream, a, C, (uint64_t)t);
      e = hipGetLastError();
    }
    int32_t open = 1;
    int64_t r = 0;
    while (open > 0 && r < max_evals &&
           value_round(ctx, C, open, e, rc, [&](int32_t* d_open) { launch_ess_round(ctx->stream, a, C, (uint64_t)t, d_open); }))
      ++r;
    if (t > 0) rounds += r;   // (the initial point's evaluation is not a transition's)
    if (e != hipSuccess || rc != SI_OK) break;
    if (open > 0) rc = fail(ctx, SI_ERR_STATE, std::string(who) + ": a transition did not end within max_evals rounds");
  }
  std::vector<int32_t> nev(selems);   // (always fetched: si_ess_kernel_info's evals)
  rc = finish_downloads(ctx, who, e, rc, {{Z_out, ctx->chains.outZ, zelems * sizeof(double)},
                                          {lp_out, ctx->chains.outlp, selems * sizeof(double)},
                                          {nev.data(), s.outnev, selems * sizeof(int32_t)},
                                          {theta_out, s.outtheta, selems * sizeof(double)}});
  if (rc != SI_OK) return rc;
  int64_t evals = 0;
  for (int32_t c = 0; c < C; ++c)
    for (int64_t t = 1; t < itr; ++t) evals += std::abs((int64_t)nev[(size_t)(t + itr * c)]);
  if (nev_out) std::memcpy(nev_out, nev.data(), selems * sizeof(int32_t));
  s.passes = (C + std::max(1, ctx->fw.slots) - 1) / std::max(1, ctx->fw.slots);
  s.rounds = rounds;
  s.evals = evals;
  return SI_OK;
}

int32_t si_ess_kernel_info(si_ctx* ctx, int32_t* passes_out, int64_t* rounds_out, int64_t* evals_out) {
  CHECK_CTX(ctx);
  if (passes_out) *passes_out = ctx->ess.passes;
  if (rounds_out) *rounds_out = ctx->ess.rounds;
  if (evals_out) *evals_out = ctx->ess.evals;
  return SI_OK;
}

}  // extern "C"
