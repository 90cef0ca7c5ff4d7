// C ABI, HMC (reference src/space_inference.jl:139-160): si_sample_hmc, si_hmc_kernel_info, si_host_hmc_windows.  The transition, the
// adaptor update and the step-size search are defined once, in kernels_hmc.hip; this file queues them.  Host-side orchestration
// only; no CPU fallback anywhere in this file.
//
// One definition, one audit (tests/hmc_audit.py), on the two routes of the stacked evaluator (StackedVgrad, capi_infer.hip): per
// transition one evaluation at the proposals, then hmc_accept_kernel; position, momentum, step size, metric and adaptor state
// never leave the device.
// The state's allocation, the preamble (hmc_init and the search) and the adaptation phases of a step are functions of namespace si
// here, declared in capi_common.h: si_sample_nuts (capi_nuts.hip) runs the same ones.
// THE PREAMBLE SYNCHRONISES on both routes: the step-size search is data dependent, so after every round (search kernel, value and
// gradient at the trial points) the host reads back ONE 4-byte count of the chains still searching.  It is a one-off before the
// first transition, bounded by the restatement's own limits (1 + 100 + 100 evaluations after the one at z_0), and the only place
// where the call reads back before its tail.
#include "capi_common.h"

using namespace si;

namespace si {

// samplers.StanAdaptor.__init__: init buffer 75, terminal buffer 50, windows doubling from 25 with the last one stretched to the end
// of the slow phase; 15 % / 75 % / 10 % when the three do not fit and n_adapts >= 20; below 20 no step is inside a window
int32_t hmc_windows(int64_t n_adapts, int64_t* window_start, int64_t* window_end, int64_t* splits, int32_t cap) {
  int64_t init_buffer = 75, term_buffer = 50, window_size = 25;
  if (init_buffer + window_size + term_buffer > n_adapts) {
    if (n_adapts >= 20) {
      init_buffer = (int64_t)(0.15 * (double)n_adapts);
      term_buffer = (int64_t)(0.1 * (double)n_adapts);
      window_size = n_adapts - init_buffer - term_buffer;
    } else {
      init_buffer = n_adapts + 1;
      term_buffer = 0;
      window_size = 1;
    }
  }
  if (window_start) *window_start = init_buffer + 1;
  const int64_t end = n_adapts - term_buffer;
  if (window_end) *window_end = end;
  int32_t count = 0;
  for (int64_t nxt = init_buffer + window_size; nxt <= end;) {
    if (nxt + 2 * window_size > end) nxt = end;
    if (splits && count < cap) splits[count] = nxt;
    ++count;
    window_size *= 2;
    nxt += window_size;
  }
  return count;
}

int32_t hmc_reserve_state(si_ctx* ctx, const char* who, int32_t C, bool nuts) {
  const size_t mc = (size_t)ctx->setup.M * (size_t)C;
  int32_t rc = reserve_chain_state(ctx, who, C);
  if (rc == SI_OK)
    rc = reserve_state(ctx, who, ctx->hmc.cap, C, [&] {
      return ctx->hmc.rh.alloc(mc) && ctx->hmc.minv.alloc(mc) && ctx->hmc.wmean.alloc(mc) && ctx->hmc.wm2.alloc(mc) &&
             ctx->hmc.chain.alloc((size_t)C) && ctx->hmc.open.alloc(1);
    });
  if (rc == SI_OK && nuts)
    rc = reserve_state(ctx, who, ctx->nuts.cap, C, [&] {
      for (DevBuf<double>* b : {&ctx->nuts.zm, &ctx->nuts.rm, &ctx->nuts.gm, &ctx->nuts.zq, &ctx->nuts.rq, &ctx->nuts.gq,
                                &ctx->nuts.rho, &ctx->nuts.zc, &ctx->nuts.gc})
        if (!b->alloc(mc)) return false;
      return ctx->nuts.stack.alloc(4 * mc * NUTS_MAX_DEPTH) && ctx->nuts.tree.alloc((size_t)C);
    });
  return rc;
}

HmcRun hmc_run_args(si_ctx* ctx, int64_t itr, double sigma_z, double delta, uint64_t seed, int32_t chain_id0, bool want_G, bool want_Minv) {
  HmcRun a;
  chain_run_args(a, ctx, itr, sigma_z, seed, chain_id0, want_G);
  a.rh = ctx->hmc.rh, a.minv = ctx->hmc.minv, a.wmean = ctx->hmc.wmean, a.wm2 = ctx->hmc.wm2, a.chain = ctx->hmc.chain;
  a.alpha_out = ctx->hmc.outalpha, a.eps_out = ctx->hmc.outeps, a.Minv_out = want_Minv ? ctx->hmc.outMinv.get() : nullptr;
  a.delta = delta;
  return a;
}

int hmc_preamble(si_ctx* ctx, const char* who, const HmcRun& a, StackedVgrad& vg, int32_t C, hipError_t& e, int32_t& rc) {
  {
    ProfScope ps(ctx, SI_K_RWMH, 0, 0);
    launch_hmc_init(ctx->stream, a, C);
    e = hipGetLastError();
  }
  // z_0's value and gradient, then the search, round by round (at most 1 + 1 + 100 + 100 rounds: the start, the direction, the
  // crossings, the bisections)
  int rounds = 0;
  int32_t open = 1;
  while (open > 0 && rounds < 2 * 100 + 3 &&
         synced_round(ctx, vg, open, e, rc, [&](int32_t* d_open) { launch_hmc_search(ctx->stream, a, C, d_open); }))
    ++rounds;
  if (e == hipSuccess && rc == SI_OK && open > 0) rc = fail(ctx, SI_ERR_STATE, std::string(who) + ": the step-size search did not finish within its own limits");
  return rounds;
}

HmcPhases::HmcPhases(int64_t n_adapts_) : n_adapts(n_adapts_), splits((size_t)std::max<int32_t>(1, hmc_windows(n_adapts_, nullptr, nullptr, nullptr, 0))) {
  nsplits = hmc_windows(n_adapts, &ws, &we, splits.data(), (int32_t)splits.size());
}

void HmcPhases::at(int64_t t, bool& adapting, bool& in_window, bool& window_close, bool& last_adapt) {
  adapting = t <= n_adapts, in_window = adapting && ws <= t && t <= we;
  while (next_split < (size_t)nsplits && splits[next_split] < t) ++next_split;
  window_close = in_window && next_split < (size_t)nsplits && splits[next_split] == t;
  last_adapt = t == n_adapts;
}

}  // namespace si

extern "C" {

int32_t si_host_hmc_windows(int64_t n_adapts, int64_t* window_start, int64_t* window_end, int64_t* splits, int32_t cap) {
  if (n_adapts < 0) return 0;
  return hmc_windows(n_adapts, window_start, window_end, splits, cap);
}

int32_t si_sample_hmc(si_ctx* ctx, int64_t itr, int64_t n_adapts, double sigma_z, double delta, uint64_t seed, int32_t chain_id0,
                      int32_t nchains, double* Z_out, double* lp_out, double* alpha_out, double* eps_out, double* G_out,
                      double* Minv_out) {
  CHECK_CTX(ctx);
  const char* who = "si_sample_hmc";
  ctx->hmc.info = CallInfo();   // (si_hmc_kernel_info reports THIS call)
  // (every comparison is false for a NaN: refused)
  int32_t rc = infer_entry_check(ctx, who, bad_if(!(itr > 0 && n_adapts >= 0 && n_adapts <= itr && nchains > 0 && chain_id0 >= 0 && sigma_z > 0.0 &&
                                                  delta > 0.0 && delta < 1.0)), SESSION_SHARED, true);
  if (rc != SI_OK) return rc;
  BIND(ctx);
  const int32_t C = nchains, M = ctx->setup.M;
  const int64_t cols = itr + 1;
  if ((rc = hmc_reserve_state(ctx, who, C, false)) != SI_OK) return rc;
  const size_t zelems = (size_t)M * (size_t)cols * (size_t)C, selems = (size_t)cols * (size_t)C;
  if (!ctx->chains.outZ.reserve(zelems) || !ctx->chains.outlp.reserve(selems) || !ctx->hmc.outalpha.reserve(selems) || !ctx->hmc.outeps.reserve(selems) ||
      (G_out && !ctx->mala.outG.reserve(zelems)) || (Minv_out && !ctx->hmc.outMinv.reserve(zelems)))
    return fail(ctx, SI_ERR_NOMEM, std::string(who) + ": output allocation failed");
  HmcPhases phases(n_adapts);
  const HmcRun a = hmc_run_args(ctx, itr, sigma_z, delta, seed, chain_id0, G_out != nullptr, Minv_out != nullptr);
  StackedVgrad vg;
  if ((rc = vg.open(ctx, who, C)) != SI_OK) return rc;
  hipError_t e = hipSuccess;
  const int rounds = hmc_preamble(ctx, who, a, vg, C, e, rc);
  if (e == hipSuccess && rc == SI_OK) {
    ProfScope ps(ctx, SI_K_RWMH, 0, 0);
    launch_hmc_propose(ctx->stream, a, C, 1);
    e = hipGetLastError();
  }
  for (int64_t t = 1; t <= itr && e == hipSuccess && rc == SI_OK; ++t) {
    eval_pending(ctx, vg, e, rc);
    if (e != hipSuccess || rc != SI_OK) break;
    bool adapting, in_window, window_close, last_adapt;
    phases.at(t, adapting, in_window, window_close, last_adapt);
    ProfScope ps(ctx, SI_K_RWMH, 0, 0);
    launch_hmc_accept(ctx->stream, a, C, (uint64_t)t, adapting, in_window, window_close, last_adapt, t < itr);
    e = hipGetLastError();
  }
  const size_t zbytes = zelems * sizeof(double), sbytes = selems * sizeof(double);
  rc = finish_downloads(ctx, who, e, rc, {{Z_out, ctx->chains.outZ, zbytes}, {lp_out, ctx->chains.outlp, sbytes}, {alpha_out, ctx->hmc.outalpha, sbytes},
                                          {eps_out, ctx->hmc.outeps, sbytes}, {G_out, a.G_out, zbytes}, {Minv_out, a.Minv_out, zbytes}});
  if (rc != SI_OK) return rc;
  ctx->hmc.info = call_info(vg, rounds);
  return SI_OK;
}

int32_t si_hmc_kernel_info(si_ctx* ctx, int32_t* fused_out, int32_t* passes_out, int32_t* search_rounds_out) {
  CHECK_CTX(ctx);
  if (fused_out) *fused_out = ctx->hmc.info.fused;
  if (passes_out) *passes_out = ctx->hmc.info.passes;
  if (search_rounds_out) *search_rounds_out = ctx->hmc.info.search_rounds;
  return SI_OK;
}

}  // extern "C"
