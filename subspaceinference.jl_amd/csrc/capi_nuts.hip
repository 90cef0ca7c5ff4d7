// C ABI, NUTS (reference src/space_inference.jl:139-160): si_sample_nuts, si_nuts_kernel_info.  The transition is defined once, in
// kernels_nuts.hip; the initial point, the step-size search, the adaptor's phases and the chains' HMC state are si_sample_hmc's own
// functions (capi_hmc.hip, declared in capi_common.h).  Host-side orchestration only; no CPU fallback anywhere in this file.
//
// The trajectory of a transition is a data-dependent tree, so EVERY ROUND SYNCHRONISES, on both routes of the stacked evaluator: a
// round is one evaluation at the chains' pending points, a memset of the open word, nuts_leaf_kernel and a 4-byte read-back of how
// many chains are still building -- the pattern of the step-size search.  Chains advance in lock-step within a transition: a chain
// whose tree is finished waits for the others, its slot is evaluated and ignored.  A transition takes at most 2^max_depth - 1 rounds.
#include "capi_common.h"

using namespace si;

extern "C" {

int32_t si_sample_nuts(si_ctx* ctx, int64_t itr, int64_t n_adapts, double sigma_z, double delta, int32_t max_depth, double max_dh,
                       uint64_t seed, int32_t chain_id0, int32_t nchains, double* Z_out, double* lp_out, double* alpha_out,
                       double* eps_out, int32_t* depth_out, int32_t* nleaf_out, int32_t* sel_out, double* G_out, double* Minv_out,
                       double* leaf_out, int64_t leaf_cap) {
  CHECK_CTX(ctx);
  const char* who = "si_sample_nuts";
  ctx->nuts.info = CallInfo();   // (si_nuts_kernel_info reports THIS call)
  // (every comparison is false for a NaN: refused)
  int32_t rc = infer_entry_check(ctx, who, bad_if(!(itr > 0 && n_adapts >= 0 && n_adapts <= itr && nchains > 0 && chain_id0 >= 0 && sigma_z > 0.0 &&
                                                  delta > 0.0 && delta < 1.0 && max_depth >= 1 && max_depth <= NUTS_MAX_DEPTH && max_dh > 0.0 &&
                                                  (!leaf_out || leaf_cap >= 1))), SESSION_SHARED, true);
  if (rc != SI_OK) return rc;
  BIND(ctx);
  const int32_t C = nchains, M = ctx->setup.M;
  const int64_t cols = itr + 1;
  if ((rc = hmc_reserve_state(ctx, who, C, true)) != SI_OK) return rc;
  const size_t zelems = (size_t)M * (size_t)cols * (size_t)C, selems = (size_t)cols * (size_t)C;
  const size_t lelems = leaf_out ? (3 * (size_t)M + 1) * (size_t)leaf_cap * (size_t)C : 0;
  if (!ctx->chains.outZ.reserve(zelems) || !ctx->chains.outlp.reserve(selems) || !ctx->hmc.outalpha.reserve(selems) || !ctx->hmc.outeps.reserve(selems) ||
      !ctx->nuts.outdepth.reserve(selems) || !ctx->nuts.outnleaf.reserve(selems) || !ctx->nuts.outsel.reserve(selems) ||
      (G_out && !ctx->mala.outG.reserve(zelems)) || (Minv_out && !ctx->hmc.outMinv.reserve(zelems)) || (leaf_out && !ctx->nuts.outleaf.reserve(lelems)))
    return fail(ctx, SI_ERR_NOMEM, std::string(who) + ": output allocation failed");
  HmcPhases phases(n_adapts);
  const HmcRun a = hmc_run_args(ctx, itr, sigma_z, delta, seed, chain_id0, G_out != nullptr, Minv_out != nullptr);
  const NutsRun n{ctx->nuts.zm, ctx->nuts.rm, ctx->nuts.gm, ctx->nuts.zq, ctx->nuts.rq, ctx->nuts.gq, ctx->nuts.rho,
                  ctx->nuts.zc, ctx->nuts.gc, ctx->nuts.stack, ctx->nuts.tree, ctx->nuts.outdepth, ctx->nuts.outnleaf, ctx->nuts.outsel,
                  leaf_out ? ctx->nuts.outleaf.get() : nullptr, leaf_cap, max_depth, max_dh};
  StackedVgrad vg;
  if ((rc = vg.open(ctx, who, C)) != SI_OK) return rc;
  // (log slots that no leaf reaches read as NaN: all bits set)
  hipError_t e = leaf_out ? hipMemsetAsync(ctx->nuts.outleaf, 0xFF, lelems * sizeof(double), ctx->stream) : hipSuccess;
  const int search_rounds = e == hipSuccess ? hmc_preamble(ctx, who, a, vg, C, e, rc) : 0;
  const int64_t round_cap = ((int64_t)1 << max_depth) - 1;
  int64_t rounds = 0;
  for (int64_t t = 1; t <= itr && e == hipSuccess && rc == SI_OK; ++t) {
    {
      ProfScope ps(ctx, SI_K_RWMH, 0, 0);
      launch_nuts_begin(ctx->stream, a, n, C, (uint64_t)t, t == 1);
      e = hipGetLastError();
    }
    int32_t open = 1;
    int64_t r = 0;
    while (open > 0 && r < round_cap &&
           synced_round(ctx, vg, open, e, rc, [&](int32_t* d_open) { launch_nuts_leaf(ctx->stream, a, n, C, (uint64_t)t, d_open); }))
      ++r;
    rounds += r;
    if (e != hipSuccess || rc != SI_OK) break;
    if (open > 0) {
      rc = fail(ctx, SI_ERR_STATE, std::string(who) + ": a trajectory tree did not finish within 2^max_depth - 1 leaves");
      break;
    }
    bool adapting, in_window, window_close, last_adapt;
    phases.at(t, adapting, in_window, window_close, last_adapt);
    ProfScope ps(ctx, SI_K_RWMH, 0, 0);
    launch_nuts_end(ctx->stream, a, n, C, (uint64_t)t, adapting, in_window, window_close, last_adapt);
    e = hipGetLastError();
  }
  const size_t zbytes = zelems * sizeof(double), sbytes = selems * sizeof(double), ibytes = selems * sizeof(int32_t);
  std::vector<int32_t> nleaf(selems);   // (always fetched: si_nuts_kernel_info's leaves)
  rc = finish_downloads(ctx, who, e, rc, {{Z_out, ctx->chains.outZ, zbytes}, {lp_out, ctx->chains.outlp, sbytes}, {alpha_out, ctx->hmc.outalpha, sbytes},
                                          {eps_out, ctx->hmc.outeps, sbytes}, {depth_out, ctx->nuts.outdepth, ibytes},
                                          {nleaf.data(), ctx->nuts.outnleaf, ibytes}, {sel_out, ctx->nuts.outsel, ibytes},
                                          {G_out, a.G_out, zbytes}, {Minv_out, a.Minv_out, zbytes},
                                          {leaf_out, n.leaf_out, lelems * sizeof(double)}});
  if (rc != SI_OK) return rc;
  int64_t leaves = 0;
  for (int32_t v : nleaf) leaves += v;
  if (nleaf_out) std::memcpy(nleaf_out, nleaf.data(), ibytes);
  ctx->nuts.info = call_info(vg, search_rounds, rounds, leaves);
  return SI_OK;
}

int32_t si_nuts_kernel_info(si_ctx* ctx, int32_t* fused_out, int32_t* passes_out, int32_t* search_rounds_out, int64_t* rounds_out,
                            int64_t* leaves_out) {
  CHECK_CTX(ctx);
  const CallInfo& i = ctx->nuts.info;
  if (fused_out) *fused_out = i.fused;
  if (passes_out) *passes_out = i.passes;
  if (search_rounds_out) *search_rounds_out = i.search_rounds;
  if (rounds_out) *rounds_out = i.rounds;
  if (leaves_out) *leaves_out = i.leaves;
  return SI_OK;
}

}  // extern "C"
