// Declarations shared by the translation units of the C ABI:
//   capi.hip         context + construction
//   capi_infer.hip   inference set-up, density, gradient, predictive forward, the stacked value-and-gradient evaluator
//   capi_sample.hip  the RWMH samplers and the output map
//   capi_mala.hip / capi_hmc.hip / capi_nuts.hip / capi_advi.hip   the MALA / HMC / NUTS samplers / the ADVI fit
// Nothing here is part of the public interface (include/subspace_hip.h).  Buffers are owned by the types of dev_buf.h (through
// si_internal.h): no file of the C ABI calls hipMalloc / hipFree / hipHostMalloc / hipHostFree or creates an event by hand.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "si_internal.h"

namespace si {

void free_infer(Ctx* c);   // capi.hip: everything si_infer_setup allocated
// the acceptance rates of a finished chain from its per-chain accept counts (one place for all sampler forms and si_rwmh_end)
inline void accept_rates(const std::vector<int64_t>& nacc, int64_t itr, double* out) {
  for (size_t c = 0; out && c < nacc.size(); ++c) out[c] = itr > 1 ? (double)nacc[c] / (double)(itr - 1) : 0.0;
}

}  // namespace si

#define CHECK_CTX(ctx) \
  if (!(ctx)) return SI_ERR_INVALID
#define BIND(ctx) SI_HIP(ctx, hipSetDevice((ctx)->device))

namespace si {

// What a density evaluation reads that depends on WHICH data set and WHICH workspace the call is for.  What belongs to the chain
// set up stays on the context: setup.model, fw.w / fw.w32 / fw.wpack*, chains.zprop, chains.sse, chains.wsq, the tile program.  setup_view is the view of the set-up's own data; si_predict builds one over its temporaries.
struct DensityView {
  const double *X, *Xc;           // Xc: X re-laid channel-fastest (spatial input), else null
  const float* X32;               // X rounded to fp32 (f32), else null
  const double* Y;
  int64_t B;
  const DevBuf<double>* act;      // the two ping-pong activation buffers, chain slots act_elems apart
  const DevBuf<float>* act32;     // (f32)
  double* ssepart;
  int sse_blocks;
  double *part, *yhat;            // partial products of the fused head; fp64 model outputs
  int64_t act_elems;
  bool f32;                       // the forward pass runs on fp32 operands
  bool defer_sse_final;           // the SSE block partials stay in ssepart (the RWMH tail kernel sums them)
  bool is_setup_data;             // X, Y, B are the set-up's: what the narrow chain's plan and tile program were built for
};
struct DensityOutputs { const double* p = nullptr; int64_t stride = 0; };   // the fp64 model outputs of one pass of eval_density: chain slot j at p + j * stride
// the narrow-head rule: a narrow last layer (regression heads: out = 1) of a Dense chain is folded into the epilogue of the layer
// before it (kernels_gemm.h carries the four MFMA-epilogue activations)
inline bool head_fused(const NetPlan& plan, const si_layer* layers, int L) {
  return !plan.has_conv && (L >= 2) && layers[L - 1].out <= SI_FUSE_MAX_OUT &&
         layers[L - 1].act < SI_ACT_LEAKYRELU && layers[L - 2].act < SI_ACT_LEAKYRELU;
}
// The ONE place a layer table becomes a ChainModel (capi.hip), for si_infer_setup* and si_train_setup* alike: net_plan, head_fused, the two kernels' slot
// counts, the main layer, the widest stored output.  node_d > 0: a NeuralODE's right-hand side d -> ... -> d (no fused head; out_dim = the trajectories' d*S rows)
int32_t chain_model_build(Ctx* ctx, const char* who, const si_layer* layers, int L, int64_t N, int32_t in_dim, int32_t out_dim, bool f32,
                          int32_t node_d, ChainModel& out);
// ---- the three value-and-gradient passes (dense_value_and_grad_f64 / _f32, net_value_and_grad) behind one workspace and one
// dispatch (capi.hip), for si_logdensity_grad and the training step.  sweep_ws_alloc is the ONE place that decides how large a
// reverse-sweep buffer is: the route follows from plan.has_conv and f32 (never both); on any failure ws is left empty.
bool sweep_ws_alloc(Ctx* ctx, SweepWs& ws, const ChainModel& m, int64_t Bmax);
// What differs between the callers of the pass.  chain_value_and_grad runs the route of `ws` on `st` (the context's stream) over
// B <= Bmax observations and, on the fp32 route, widens gw32 into gw behind it: gw holds the gradient, *sse the sum of squared
// errors (another cost: its numerator).
struct ChainValueGrad {
  const ChainModel* m;
  const double* w64;      // flat weights, and rounded to fp32 (DenseF32)
  const float* w32;
  const double *X, *Xc;   // input of layer 0; Xc: re-laid channel-fastest (a Conv chain on spatial input: net_input)
  const float* X32;       // (DenseF32)
  const double* Y;
  int64_t B;
  double* part;           // the forward pass's head partials (m->part_slots() feature slots)
  double *ssepart, *sse;
  int sse_blocks;
  double *gw, *wpack;     // wpack: packed conv weights (Conv)
  double scale;           // of Delta_L: -2 / d for the mse loss, 1 / sigma^2 for the log-density
  const CostTail* cost;   // training with another cost, else nullptr
  bool traffic;           // profile: DenseForward::traffic (DenseF64)
  double bwd_flops;       // profile: NetValueGrad::bwd_flops (Conv)
};
int32_t chain_value_and_grad(Ctx* ctx, hipStream_t st, SweepWs& ws, const ChainValueGrad& in);
// the cap on a stacked workspace: how many chains one pass of launches carries follows from it (batch_width, vgrad_route, the
// NeuralODE gradient's record)
constexpr double SI_BATCH_BYTES = 2.0 * 1024.0 * 1024.0 * 1024.0;
constexpr int32_t SI_NOT_TAKEN = INT32_MIN;   // a density route's or a sampler form's answer "does not apply": the next one is tried

}  // namespace si

extern "C" {   // (defined inside the extern "C" blocks of their translation units; not exported by include/subspace_hip.h)
// capi_infer.hip
int32_t ensure_chains(si_ctx* ctx, int32_t C);   // forward workspace + sampler state for C chains
si::DensityView setup_view(const si_ctx* ctx, bool defer_sse_final = false);
// chains.zprop[:, c0 .. c0+nc) -> chains.sse, nc <= the view's chain slots; eval_density_all: all C chains, fw.slots at a time
// (out: where the pass left the fp64 model outputs, decided by the route that produced them; nullptr: not asked for)
int32_t eval_density(si_ctx* ctx, const si::DensityView& v, int c0, int nc, si::DensityOutputs* out);
int32_t eval_density_all(si_ctx* ctx, const si::DensityView& v, int C);
// "form the weights of these points": w[:, c] = W_swa + P z_c (K4), or W_swa + decoder(z_c) while a decoder is set
// (si_infer_set_decoder), for the n points z_dev[M x n] (device).  The one place the C ABI forms weights outside a sampler
// kernel of its own.  w32: also rounded once to fp32 (P route only).  keep_y (decoder route, n = 1): decoder(z) stays in dec.y
// for pull_back_to_z.  Queued on the stream; an error only when the decoder's workspace cannot grow.
int32_t form_weights(si_ctx* ctx, const double* z_dev, int32_t n, double* w, int64_t ldw, float* w32 = nullptr, bool keep_y = false);
// "pull grad.gw back to z": gz = P' gw, or J_decoder(z)' gw at the point form_weights(.., keep_y = true) saw last
void pull_back_to_z(si_ctx* ctx, const double* gw, double* gz);
double mvnormal_c0(double d, double sigma);
double prior_c0(const si_ctx* ctx);
// the constants of lp = c0 - (sse / s2) / 2 [+ prior_c0 - (wsq / sp2) / 2] for the chain or NeuralODE set up
double lik_c0(const si_ctx* ctx, double d);
double lik_s2(const si_ctx* ctx);
double prior_sp2(const si_ctx* ctx);
// a categorical / Bernoulli likelihood is set (si_infer_set_likelihood): the ONE predicate by which every route that forms the
// SSE inside a kernel of its own steps aside (chain_loop_applies, rwmh_grid, density_fused, vgrad_route)
inline bool lik_on(const si_ctx* ctx) { return ctx->setup.lik != 0; }
// capi_node.hip: the NeuralODE route behind eval_density and si_predict (node.on), and the part of its set-up that
// infer_setup_common carries (capi_infer.hip)
int32_t node_density(si_ctx* ctx, const si::DensityView& v, int c0, int nc, si::DensityOutputs* out);
int32_t node_predict(si_ctx* ctx, const double* Z, int32_t C, const double* U0new, int64_t Bn, double* U_out);
int32_t infer_setup_node_base(si_ctx* ctx, const si_layer* layers, int32_t L, int64_t N, int32_t M, const double* W_swa, const double* P,
                              const double* U0, const double* Y, int32_t d, int32_t S, int64_t f);
// ... and its value-and-gradient route (si_node_set_grad): the workspace for min(C, what the budget allows) chains per pass; one
// pass of launches for n <= node.g_cap points on the device (queued: nothing is copied, nothing synchronises; P route only); one
// point from the host (either seam; synchronises); C points from the host, pass by pass (P route)
int32_t node_grad_ensure(si_ctx* ctx, const char* who, int32_t C);
int32_t node_value_and_grad(si_ctx* ctx, const double* z_dev, int32_t n, double* lp_dev, double* gz_dev);
int32_t node_grad_point(si_ctx* ctx, const double* z, double* lp_out, double* grad_out);
int32_t node_grad_batch(si_ctx* ctx, const double* Z, int32_t C, double* lp_out, double* grad_out);
// capi_train.hip: after NeuralODE training steps (si_train_setup_node) a synchronising call ends with this -- it synchronises the
// stream, reads the failure record back and returns SI_ERR_INVALID naming step, trajectory and status, once; SI_OK otherwise
int32_t train_node_report(si_ctx* ctx, const char* who);
void fused_fill_program(const si_ctx* ctx, si::ChainFusedPlan& fp);
// The state rules and error texts of the inference entry points, each sentence in one place.  need_setup: "call si_infer_setup first".
// no_session: no step-wise session may be open (SESSION_SHARED names the shared proposal / SSE buffers, SESSION_SETTING is the setters'
// shorter sentence, SESSION_ANY: not checked).  infer_entry_check is the sequence most entry points run: the set-up, with `grad` the gradient
// entries' NeuralODE rule, the arguments (bad_args: nullptr when fine, else the text behind "who: "), the session; another order: the pieces.
enum SessionRule { SESSION_ANY, SESSION_SHARED, SESSION_SETTING };
int32_t need_setup(si_ctx* ctx, const char* who);
int32_t no_session(si_ctx* ctx, const char* who, SessionRule rule);
int32_t infer_entry_check(si_ctx* ctx, const char* who, const char* bad_args, SessionRule rule = SESSION_SHARED, bool grad = false);
inline const char* bad_if(bool bad, const char* text = "bad argument") { return bad ? text : nullptr; }
}

namespace si {

// Value and gradient at C stacked points that live on the device, for the gradient-driven entry points (si_sample_mala,
// si_sample_hmc, si_fit_advi); defined in capi_infer.hip, where the two routes are described.
struct StackedVgrad {
  bool fused = false;   // the route of this call
  bool node = false;    // ... or the third: a NeuralODE set-up on the P route, node_value_and_grad pass by pass (capi_node.hip)
  int passes = 0;       // per evaluation: passes of launches (fused) / single-point evaluations (other)
  // once per call, after the caller's own allocations: the route, then the fused workspace or the other route's host images
  int32_t open(si_ctx* ctx, const char* who, int32_t C);
  // lp_dev[C], g_dev[M x C] at z_dev[M x C].  e and rc are the call's own, both fine on entry; it stops at the first failure of either
  void eval(const double* z_dev, double* lp_dev, double* g_dev, hipError_t& e, int32_t& rc);

 private:
  si_ctx* ctx = nullptr;
  int32_t C = 0;
  int nb = 0;
  int64_t G = 0;
  std::vector<double> hz, hlp, hg;   // the other route's host images of the points, their values and gradients
};

// The tail of such a call: the downloads (queued only while everything so far succeeded; a null dst is an output not asked
// for), ONE synchronisation -- also after a failure -- and the first error reported: rc, then e, then the synchronisation's.
struct Download { void* dst; const void* src; size_t bytes; };
int32_t finish_downloads(si_ctx* ctx, const char* who, hipError_t e, int32_t rc, std::initializer_list<Download> downs);

// What such a call took, for the context's CallInfo of its entry point (each entry point clears its own first: a refused call reports zeros)
inline CallInfo call_info(const StackedVgrad& vg, int search_rounds = 0, int64_t rounds = 0, int64_t leaves = 0) {
  return CallInfo{vg.fused ? 1 : 0, vg.passes, search_rounds, rounds, leaves};
}

// Per-chain sampler state that grows on demand, for every group of buffers that has a capacity: nothing is queued on the buffers
// while they are replaced, and a failed growth leaves the capacity at zero.  alloc() allocates the group for C chains.
template <class Alloc>
int32_t reserve_state(si_ctx* ctx, const char* who, int& cap, int32_t C, Alloc&& alloc) {
  if (cap >= C) return SI_OK;
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  cap = 0;
  if (!alloc()) return fail(ctx, SI_ERR_NOMEM, std::string(who) + ": sampler state allocation failed");
  cap = C;
  return SI_OK;
}
// the context's ChainState for C chains: what si_sample_mala, si_sample_hmc and si_sample_nuts reserve first
inline int32_t reserve_chain_state(si_ctx* ctx, const char* who, int32_t C) {
  ChainState& s = ctx->chain_state;
  const size_t mc = (size_t)ctx->setup.M * (size_t)C;
  return reserve_state(ctx, who, s.cap, C, [&] {
    return s.z.alloc(mc) && s.g.alloc(mc) && s.zp.alloc(mc) && s.gp.alloc(mc) && s.lp.alloc((size_t)C) && s.lpp.alloc((size_t)C);
  });
}
// ... and the part of their kernels' arguments that lies over it and over the sample arrays (reserved by the caller)
inline void chain_run_args(ChainRun& r, si_ctx* ctx, int64_t itr, double sigma_z, uint64_t seed, int32_t chain_id0, bool want_G) {
  ChainState& s = ctx->chain_state;
  r.z = s.z, r.lp = s.lp, r.g = s.g, r.zp = s.zp, r.lpp = s.lpp, r.gp = s.gp;
  r.Z_out = ctx->chains.outZ, r.lp_out = ctx->chains.outlp, r.G_out = want_G ? ctx->mala.outG.get() : nullptr;
  r.M = ctx->setup.M, r.chain_id0 = chain_id0, r.itr = itr, r.seed = seed, r.sigma_z = sigma_z;
}

// the value and gradient at the chains' proposals / pending points: (lpp, gp) at zp
inline void eval_pending(si_ctx* ctx, StackedVgrad& vg, hipError_t& e, int32_t& rc) {
  ChainState& s = ctx->chain_state;
  vg.eval(s.zp, s.lpp, s.gp, e, rc);
}

// One synchronised round of a data-dependent loop (the step-size search, a NUTS leaf): one evaluation at the chains' pending
// points, the open word cleared, launch(open word) -- the kernel counts the chains that go on into it -- a 4-byte read-back into
// `open` and a synchronisation.  e / rc as StackedVgrad::eval treats them; returns whether the round was completed.
// What follows the evaluation in either kind of round: the open word `d_open` cleared, launch(d_open), the read-back, the synchronisation
template <class Launch>
bool round_tail(si_ctx* ctx, int32_t* d_open, int32_t& open, hipError_t& e, Launch&& launch) {
  if ((e = hipMemsetAsync(d_open, 0, sizeof(int32_t), ctx->stream)) != hipSuccess) return false;
  {
    ProfScope ps(ctx, SI_K_RWMH, 0, 0);
    launch(d_open);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&open, d_open, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  return e == hipSuccess;
}
template <class Launch>
bool synced_round(si_ctx* ctx, StackedVgrad& vg, int32_t& open, hipError_t& e, int32_t& rc, Launch&& launch) {
  if (e == hipSuccess && rc == SI_OK) eval_pending(ctx, vg, e, rc);
  if (e != hipSuccess || rc != SI_OK) return false;
  return round_tail(ctx, ctx->hmc.open.get(), open, e, launch);
}
// The same round on values alone (an elliptical slice's shrink loop): the evaluation is eval_density_all at the C pending points in
// chains.zprop, fw.slots per pass of launches, and leaves the density's sums in chains.sse / chains.wsq; the open word is ess.open
template <class Launch>
bool value_round(si_ctx* ctx, int32_t C, int32_t& open, hipError_t& e, int32_t& rc, Launch&& launch) {
  if (e == hipSuccess && rc == SI_OK) rc = eval_density_all(ctx, setup_view(ctx), C);
  if (e != hipSuccess || rc != SI_OK) return false;
  return round_tail(ctx, ctx->ess.open.get(), open, e, launch);
}

// capi_hmc.hip: what si_sample_hmc and si_sample_nuts share.  The chains' state on top of ChainState (nuts: the tree's too); the
// kernels' shared arguments over the state and the output arrays (reserved by the caller); the preamble -- hmc_init, then the step-size search round by round -- returning its rounds, with
// e / rc as StackedVgrad::eval treats them; and the adaptation phase of every step t = 1, 2, ... in turn (the host's knowledge,
// handed to the kernels as flags).
int32_t hmc_reserve_state(si_ctx* ctx, const char* who, int32_t C, bool nuts);
HmcRun hmc_run_args(si_ctx* ctx, int64_t itr, double sigma_z, double delta, uint64_t seed, int32_t chain_id0, bool want_G, bool want_Minv);
int hmc_preamble(si_ctx* ctx, const char* who, const HmcRun& a, StackedVgrad& vg, int32_t C, hipError_t& e, int32_t& rc);
struct HmcPhases {
  explicit HmcPhases(int64_t n_adapts);
  void at(int64_t t, bool& adapting, bool& in_window, bool& window_close, bool& last_adapt);   // t must not decrease between calls

 private:
  int64_t n_adapts, ws = 0, we = 0;
  std::vector<int64_t> splits;
  int32_t nsplits = 0;
  size_t next_split = 0;
};

}  // namespace si
