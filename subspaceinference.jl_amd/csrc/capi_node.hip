// C ABI, NeuralODE models (reference src/space_inference.jl:96-101; model_re at src/libs.jl:36-54): si_infer_setup_node,
// si_node_solve, si_node_tableau, si_node_info, and the two routes eval_density and si_predict hand over while a node set-up is
// active.  Host-side orchestration only: the integrations run in kernels_node.hip, W_swa + P z (or the decoder) in form_weights,
// ||W||^2 in launch_sse as the prior term does.  No CPU fallback anywhere in this file.
#include "capi_common.h"
#include "node_tableau.h"

using namespace si;

namespace si {

const char* node_plan(const si_layer* layers, int32_t L, int64_t N, int32_t d, int32_t S, const double* ts, const si_node_opts* opts,
                      NodeArgs& a) {
  int32_t prev = d, widest = 1;
  for (int32_t l = 0; l < L; ++l) {
    const si_layer& ly = layers[l];
    if (ly.kind != SI_LAYER_DENSE) return "every layer of the right-hand side must be SI_LAYER_DENSE";
    if (ly.act < 0 || ly.act >= SI_ACT_COUNT) return "unknown activation";
    if (ly.in != prev) return "consecutive layer widths do not chain from d";
    if (ly.out < 1 || ly.out > SI_NODE_MAX_WIDTH) return "layer widths must be 1 to 256";
    const int64_t wn = (int64_t)ly.in * ly.out;
    if (ly.w_off < 0 || ly.w_off > N - wn || ly.b_off < 0 || ly.b_off > N - ly.out) return "a layer's offset range falls outside [0, N)";
    a.lay.in[l] = ly.in, a.lay.out[l] = ly.out, a.lay.act[l] = ly.act, a.lay.w_off[l] = (int32_t)ly.w_off, a.lay.b_off[l] = (int32_t)ly.b_off;
    prev = ly.out;
    widest = std::max(widest, ly.out);
  }
  if (prev != d) return "the right-hand side must map d to d";
  a.lay.n = L;
  if (!std::isfinite(opts->t0)) return "t0 must be finite";
  for (int32_t s = 0; s < S; ++s)
    if (!std::isfinite(ts[s]) || (s == 0 ? ts[0] < opts->t0 : !(ts[s] > ts[s - 1])))
      return "the save times must be finite, strictly ascending and not before t0";
  if (opts->pre_power != 1 && opts->pre_power != 3) return "pre_power must be 1 or 3";
  if (opts->max_steps < 0 || opts->max_steps > SI_NODE_MAX_STEPS) return "max_steps must be 1 to 1000000 (0: 100000)";
  if (opts->adaptive != 0 && opts->adaptive != 1) return "adaptive must be 0 or 1";
  if (opts->adaptive) {
    if (!(std::isfinite(opts->reltol) && opts->reltol > 0.0 && std::isfinite(opts->abstol) && opts->abstol > 0.0))
      return "reltol and abstol must be finite and positive in adaptive mode";
    if (!(std::isfinite(opts->dt) && opts->dt >= 0.0)) return "dt must be finite and >= 0 (0: the starting-step rule)";
  } else if (!(std::isfinite(opts->dt) && opts->dt > 0.0)) {
    return "dt must be finite and positive in fixed-step mode";
  }
  // G lanes per trajectory: the smallest power of two >= the widest layer, capped at 64 (a group never crosses a wave)
  a.G = 1, a.lgG = 0;
  while (a.G < widest && a.G < 64) a.G *= 2, a.lgG += 1;
  a.maxw = widest, a.d = d, a.S = S, a.N = (int32_t)N;
  a.t0 = opts->t0, a.reltol = opts->reltol, a.abstol = opts->abstol, a.dt = opts->dt;
  a.adaptive = opts->adaptive, a.max_steps = opts->max_steps == 0 ? 100000 : opts->max_steps, a.pre_power = opts->pre_power;
  return nullptr;
}

}  // namespace si

namespace {

// the kernel's arguments for `nc` chain slots whose weights lie in w: the set-up's constants plus this pass's data and outputs
NodeArgs node_args(const si_ctx* ctx, const double* w, const double* U0, const double* Y, int64_t f, double* sse_p, double* U_out,
                   int32_t* nacc, int32_t* nrej, int32_t* status) {
  NodeArgs a = ctx->node.args;
  a.w = w, a.ldw = pad_ld(ctx->setup.model.N);
  a.U0 = U0, a.Y = Y, a.f = f;
  a.ts = ctx->node.ts;
  a.sse_p = sse_p, a.U_out = U_out, a.nacc = nacc, a.nrej = nrej, a.status = status;
  return a;
}

// the per-trajectory sums (and, on request, the saved states) of one pass of launches; nothing is queued on a buffer that goes
int32_t node_reserve(si_ctx* ctx, size_t ssep, size_t uout) {
  NodeState& n = ctx->node;
  if (n.ssep.size() >= ssep && (uout == 0 || n.uout.size() >= uout)) return SI_OK;
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (!n.ssep.reserve(ssep) || (uout != 0 && !n.uout.reserve(uout))) return fail(ctx, SI_ERR_NOMEM, "NeuralODE density: workspace allocation failed");
  return SI_OK;
}

}  // namespace

extern "C" {

static int32_t need_node_setup(si_ctx* ctx, const char* who) {
  return ctx->setup.ready && ctx->node.on ? SI_OK : fail(ctx, SI_ERR_STATE, std::string(who) + ": call si_infer_setup_node first");
}
int32_t node_density(si_ctx* ctx, const DensityView& v, int c0, int nc, DensityOutputs* out) {
  const int64_t N = ctx->setup.model.N, ldw = pad_ld(N), f = v.B;
  const int32_t M = ctx->setup.M;
  const size_t traj = (size_t)ctx->node.d * (size_t)ctx->node.S * (size_t)f;
  int32_t rc = node_reserve(ctx, (size_t)f * (size_t)nc, out ? traj * (size_t)nc : 0);
  if (rc != SI_OK) return rc;
  {
    ProfScope ps(ctx, SI_K_RECON, 2.0 * (double)N * M * nc, (double)N * (M + 1 + nc) * 8.0);
    if ((rc = form_weights(ctx, ctx->chains.zprop + (size_t)c0 * M, nc, ctx->fw.w, ldw)) != SI_OK) return rc;
  }
  launch_sse(ctx->stream, ctx->fw.w, nullptr, N, ctx->fw.wsqpart, ctx->setup.wsq_blocks, ctx->chains.wsq + c0, nc, ldw);   // ||W||^2 per chain
  {
    ProfScope ps(ctx, SI_K_DENSE, 0.0, 0.0);
    const NodeArgs a = node_args(ctx, ctx->fw.w, v.X, v.Y, f, ctx->node.ssep, out ? ctx->node.uout.get() : nullptr, nullptr, nullptr, nullptr);
    SI_HIP(ctx, launch_node_solve(ctx->stream, a, nc));
    launch_node_sum(ctx->stream, ctx->node.ssep, f, ctx->chains.sse + c0, nc);
  }
  SI_HIP(ctx, hipGetLastError());
  if (out) *out = {ctx->node.uout, (int64_t)traj};
  return SI_OK;
}

int32_t si_infer_setup_node(si_ctx* ctx, const si_layer* layers, int32_t L, int64_t N, int32_t M, const double* W_swa, const double* P,
                            const double* U0, const double* Y, int32_t d, int32_t S, int64_t f, const double* ts, const void* opts_in) {
  CHECK_CTX(ctx);
  const si_node_opts* opts = static_cast<const si_node_opts*>(opts_in);
  auto bad = [&](const char* what) { return fail(ctx, SI_ERR_INVALID, std::string("si_infer_setup_node: ") + what); };
  if (!layers || !U0 || !Y || !ts || !opts || M <= 0 || f <= 0) return bad("bad argument");
  if (L < 1 || L > SI_NODE_MAX_LAYERS) return bad("a NeuralODE right-hand side has 1 to 8 Dense layers");
  if (d < 1 || d > SI_NODE_MAX_D) return bad("the state dimension d must be 1 to 8");
  if (N < 1 || N > SI_NODE_MAX_N) return bad("N must be 1 to 8192");
  if (S < 1 || S > SI_NODE_MAX_S) return bad("the number of save times S must be 1 to 4096");
  // (the per-chain sum walks its f per-trajectory values in the reference's order, one thread per chain: 2^20 is a millisecond of it)
  if (f > ((int64_t)1 << 20)) return bad("f must be at most 2^20 trajectories");
  NodeArgs a;
  if (const char* what = node_plan(layers, L, N, d, S, ts, opts, a)) return bad(what);
  int32_t rc = infer_setup_node_base(ctx, layers, L, N, M, W_swa, P, U0, Y, d, S, f);
  if (rc != SI_OK) return rc;
  NodeState& n = ctx->node;
  if (!n.ts.alloc((size_t)S) || hipMemcpy(n.ts, ts, (size_t)S * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
    free_infer(ctx);
    return fail(ctx, SI_ERR_NOMEM, "si_infer_setup_node: device allocation / upload failed");
  }
  n.args = a, n.d = d, n.S = S;
  ctx->setup.sigma_p = 1.0;   // "the prior term on": its constants are lik_c0 / lik_s2 / prior_c0 / prior_sp2 (capi_infer.hip)
  n.on = true;
  return SI_OK;
}

int32_t si_node_solve(si_ctx* ctx, const double* Z, int32_t C, double* U_out, double* sse_out, int32_t* naccept_out,
                      int32_t* nreject_out, int32_t* status_out) {
  CHECK_CTX(ctx);
  int32_t rc = need_node_setup(ctx, "si_node_solve");
  if (rc != SI_OK || (rc = infer_entry_check(ctx, "si_node_solve", bad_if(!Z || C <= 0))) != SI_OK) return rc;
  BIND(ctx);
  if ((rc = ensure_chains(ctx, C)) != SI_OK) return rc;
  const int64_t N = ctx->setup.model.N, ldw = pad_ld(N), f = ctx->setup.B;
  const int32_t M = ctx->setup.M;
  const size_t traj = (size_t)ctx->node.d * (size_t)ctx->node.S * (size_t)f;
  // an audit read-back, not a hot path: fw.slots chains per pass (at most 256 MB of saved states), one synchronisation per pass
  int wb = std::max(1, std::min<int>(ctx->fw.slots, C));
  if (U_out) wb = (int)std::max<size_t>(1, std::min<size_t>((size_t)wb, ((size_t)32 << 20) / traj));
  DevBuf<double> dU, dS;
  DevBuf<int32_t> dI;
  if ((U_out && !dU.alloc(traj * (size_t)wb)) || !dS.alloc((size_t)f * wb) || !dI.alloc((size_t)3 * (size_t)f * wb))
    return fail(ctx, SI_ERR_NOMEM, "si_node_solve: device allocation failed");
  SI_HIP(ctx, hipMemcpyAsync(ctx->chains.zprop, Z, (size_t)M * C * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  const size_t fw = (size_t)f * (size_t)wb;
  for (int c0 = 0; c0 < C; c0 += wb) {
    const int nc = std::min(wb, C - c0);
    const size_t fn = (size_t)f * (size_t)nc;
    if ((rc = form_weights(ctx, ctx->chains.zprop + (size_t)c0 * M, nc, ctx->fw.w, ldw)) != SI_OK) return rc;
    const NodeArgs a = node_args(ctx, ctx->fw.w, ctx->setup.X, ctx->setup.Y, f, dS, U_out ? dU.get() : nullptr, dI, dI + fw, dI + 2 * fw);
    SI_HIP(ctx, launch_node_solve(ctx->stream, a, nc));
    if (U_out) SI_HIP(ctx, hipMemcpyAsync(U_out + traj * (size_t)c0, dU, traj * (size_t)nc * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (sse_out) SI_HIP(ctx, hipMemcpyAsync(sse_out + (size_t)f * c0, dS, fn * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (naccept_out) SI_HIP(ctx, hipMemcpyAsync(naccept_out + (size_t)f * c0, dI, fn * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (nreject_out) SI_HIP(ctx, hipMemcpyAsync(nreject_out + (size_t)f * c0, dI + fw, fn * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (status_out) SI_HIP(ctx, hipMemcpyAsync(status_out + (size_t)f * c0, dI + 2 * fw, fn * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return SI_OK;
}

// si_predict in a node set-up: the saved states from new initial conditions U0new (d x Bn) at Z[:, c], d*S x Bn x C
int32_t node_predict(si_ctx* ctx, const double* Z, int32_t C, const double* U0new, int64_t Bn, double* U_out) {
  const int64_t N = ctx->setup.model.N, ldw = pad_ld(N);
  const int32_t M = ctx->setup.M, d = ctx->node.d;
  const size_t traj = (size_t)d * (size_t)ctx->node.S * (size_t)Bn;
  const int wb = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::min<int>(ctx->fw.slots, C), ((size_t)32 << 20) / traj));
  DevBuf<double> dX, dU, dS;
  if (!dX.alloc((size_t)d * (size_t)Bn) || !dU.alloc(traj * (size_t)wb) || !dS.alloc((size_t)Bn * wb))
    return fail(ctx, SI_ERR_NOMEM, "si_predict: device allocation failed");
  SI_HIP(ctx, hipMemcpyAsync(dX, U0new, (size_t)d * (size_t)Bn * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  SI_HIP(ctx, hipMemcpyAsync(ctx->chains.zprop, Z, (size_t)M * C * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  for (int c0 = 0; c0 < C; c0 += wb) {
    const int nc = std::min(wb, C - c0);
    const int32_t rc = form_weights(ctx, ctx->chains.zprop + (size_t)c0 * M, nc, ctx->fw.w, ldw);
    if (rc != SI_OK) return rc;
    const NodeArgs a = node_args(ctx, ctx->fw.w, dX, nullptr, Bn, dS, dU, nullptr, nullptr, nullptr);
    SI_HIP(ctx, launch_node_solve(ctx->stream, a, nc));
    SI_HIP(ctx, hipMemcpyAsync(U_out + traj * (size_t)c0, dU, traj * (size_t)nc * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return SI_OK;
}

// ---- the gradient through the solver (si_node_set_grad; node.py: logdensity_grad is the definition) ----------------------------
// the bytes one chain of a pass needs: its record (f * max_steps * (d + 2) doubles) and its per-trajectory gradient slices (f * N)
static double node_grad_chain_bytes(const si_ctx* ctx) {
  const NodeArgs& a = ctx->node.args;
  return 8.0 * (double)ctx->setup.B * ((double)a.max_steps * (double)(a.d + 2) + (double)ctx->setup.model.N);
}

static void node_grad_drop(NodeState& n) {
  for (DevBuf<double>* b : {&n.g_z, &n.g_w, &n.g_ssep, &n.g_sse, &n.g_wsq, &n.g_wsqpart, &n.g_rec, &n.g_slices, &n.g_gw, &n.g_lp, &n.g_gz}) b->reset();
  n.g_cnt.reset();
  n.g_cap = 0;
}

int32_t si_node_set_grad(si_ctx* ctx, int32_t on) {
  CHECK_CTX(ctx);
  int32_t rc0 = need_node_setup(ctx, "si_node_set_grad");
  if (rc0 != SI_OK || (rc0 = no_session(ctx, "si_node_set_grad", SESSION_SETTING)) != SI_OK) return rc0;
  if (on != 0 && on != 1) return fail(ctx, SI_ERR_INVALID, "si_node_set_grad: on must be 0 or 1");
  BIND(ctx);
  NodeState& n = ctx->node;
  if (!on) {
    SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    node_grad_drop(n);
    n.grad = false, n.g_fit = 0;
    return SI_OK;
  }
  if (n.args.maxw > 64)
    return fail(ctx, SI_ERR_INVALID, "si_node_set_grad: a layer is wider than 64 (the reverse kernel gives every lane of a trajectory's group one unit per layer)");
  const double fit = std::floor(SI_BATCH_BYTES / node_grad_chain_bytes(ctx));
  if (fit < 1.0)
    return fail(ctx, SI_ERR_INVALID, "si_node_set_grad: the record of one chain (f * max_steps * (d + 2) doubles) and its gradient slices (f * N) "
                                     "do not fit the 2 GiB workspace budget: lower max_steps");
  n.g_fit = (int)std::min(fit, 65535.0);   // (a launch carries its chains in grid.y)
  n.grad = true;
  return SI_OK;
}

int32_t si_node_grad_info(si_ctx* ctx, int32_t* on_out, int32_t* chains_per_pass_out) {
  CHECK_CTX(ctx);
  const bool on = ctx->setup.ready && ctx->node.on && ctx->node.grad;
  if (on_out) *on_out = on ? 1 : 0;
  if (chains_per_pass_out) *chains_per_pass_out = on ? ctx->node.g_fit : 0;
  return SI_OK;
}

int32_t node_grad_ensure(si_ctx* ctx, const char* who, int32_t C) {
  NodeState& n = ctx->node;
  const int cap = std::min<int>(n.g_fit, std::max(1, C));
  if (n.g_cap >= cap) return SI_OK;
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  node_grad_drop(n);
  const size_t S = (size_t)cap, f = (size_t)ctx->setup.B, N = (size_t)ctx->setup.model.N, ldw = (size_t)pad_ld(ctx->setup.model.N), M = (size_t)ctx->setup.M;
  const bool ok = n.g_z.alloc(S * M) && n.g_w.alloc(S * ldw) && n.g_ssep.alloc(S * f) && n.g_sse.alloc(S) && n.g_wsq.alloc(S) &&
                  n.g_wsqpart.alloc(S * (size_t)ctx->setup.wsq_blocks) && n.g_rec.alloc(S * f * (size_t)n.args.max_steps * (size_t)(n.d + 2)) &&
                  n.g_slices.alloc(S * f * N) && n.g_gw.alloc(S * ldw) && n.g_lp.alloc(S) && n.g_gz.alloc(S * M) && n.g_cnt.alloc(3 * S * f) &&
                  ctx->grad.ptgpart.reserve((size_t)ptg_blocks() * M);
  if (!ok) {
    node_grad_drop(n);
    return fail(ctx, SI_ERR_NOMEM, std::string(who) + ": workspace allocation failed (the NeuralODE gradient's record: lower max_steps)");
  }
  // (the padding rows of g_w / g_gw are written by no kernel and launch_prior_grad runs over whole columns: defined once, here)
  SI_HIP(ctx, hipMemset(n.g_w, 0, S * ldw * sizeof(double)));
  SI_HIP(ctx, hipMemset(n.g_gw, 0, S * ldw * sizeof(double)));
  n.g_cap = cap;
  return SI_OK;
}

// the weights are in g_w: ||W||^2, the forward with record, the reverse kernel, the sums (gw without the prior term, lp)
static int32_t node_grad_launches(si_ctx* ctx, int32_t nc, double* lp_dev) {
  NodeState& n = ctx->node;
  const int64_t N = ctx->setup.model.N, ldw = pad_ld(N), f = ctx->setup.B;
  const size_t fc = (size_t)f * (size_t)n.g_cap;
  launch_sse(ctx->stream, n.g_w, nullptr, N, n.g_wsqpart, ctx->setup.wsq_blocks, n.g_wsq, nc, ldw);
  SI_HIP(ctx, hipMemsetAsync(n.g_slices, 0, (size_t)nc * (size_t)f * (size_t)N * sizeof(double), ctx->stream));   // "from 0.0"
  NodeArgs a = node_args(ctx, n.g_w, ctx->setup.X, ctx->setup.Y, f, n.g_ssep, nullptr, n.g_cnt, n.g_cnt + fc, n.g_cnt + 2 * fc);
  a.rec = n.g_rec, a.gsl = n.g_slices;
  {
    ProfScope ps(ctx, SI_K_DENSE, 0.0, 0.0);
    SI_HIP(ctx, launch_node_solve(ctx->stream, a, nc));
    launch_node_sum(ctx->stream, n.g_ssep, f, n.g_sse, nc);
  }
  {
    ProfScope ps(ctx, SI_K_BACKWARD, 0.0, 0.0);
    SI_HIP(ctx, launch_node_grad(ctx->stream, a, nc));
    launch_node_grad_sum(ctx->stream, n.g_slices, f, N, n.g_gw, ldw, n.g_sse, n.g_wsq, lp_dev, nc);
  }
  launch_prior_grad(ctx->stream, n.g_gw, n.g_w, (int64_t)nc * ldw, 1.0 / prior_sp2(ctx), ctx->num_cu);   // - 2 W, every chain at once
  SI_HIP(ctx, hipGetLastError());
  return SI_OK;
}

int32_t node_value_and_grad(si_ctx* ctx, const double* z_dev, int32_t nc, double* lp_dev, double* gz_dev) {
  NodeState& n = ctx->node;
  const int64_t ldw = pad_ld(ctx->setup.model.N);
  int32_t rc;
  {
    ProfScope ps(ctx, SI_K_RECON, 2.0 * (double)ctx->setup.model.N * ctx->setup.M * nc, (double)ctx->setup.model.N * (ctx->setup.M + 1 + nc) * 8.0);
    if ((rc = form_weights(ctx, z_dev, nc, n.g_w, ldw, nullptr, /*keep_y=*/ctx->dec.on)) != SI_OK) return rc;
  }
  if ((rc = node_grad_launches(ctx, nc, lp_dev)) != SI_OK) return rc;
  for (int32_t c = 0; c < nc; ++c) pull_back_to_z(ctx, n.g_gw + (size_t)ldw * c, gz_dev + (size_t)ctx->setup.M * c);   // queued per point
  SI_HIP(ctx, hipGetLastError());
  return SI_OK;
}

int32_t node_grad_point(si_ctx* ctx, const double* z, double* lp_out, double* grad_out) {
  NodeState& n = ctx->node;
  const size_t M = (size_t)ctx->setup.M;
  int32_t rc = node_grad_ensure(ctx, "si_logdensity_grad", 1);
  if (rc != SI_OK) return rc;
  SI_HIP(ctx, hipMemcpyAsync(n.g_z, z, M * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if ((rc = node_value_and_grad(ctx, n.g_z, 1, n.g_lp, n.g_gz)) != SI_OK) return rc;
  SI_HIP(ctx, hipMemcpyAsync(lp_out, n.g_lp, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  SI_HIP(ctx, hipMemcpyAsync(grad_out, n.g_gz, M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SI_OK;
}

int32_t node_grad_batch(si_ctx* ctx, const double* Z, int32_t C, double* lp_out, double* grad_out) {
  NodeState& n = ctx->node;
  const size_t M = (size_t)ctx->setup.M;
  int32_t rc = node_grad_ensure(ctx, "si_logdensity_grad_batch", C);
  if (rc != SI_OK) return rc;
  for (int32_t c0 = 0; c0 < C; c0 += n.g_cap) {
    const int32_t nc = std::min<int32_t>(n.g_cap, C - c0);
    SI_HIP(ctx, hipMemcpyAsync(n.g_z, Z + M * c0, M * nc * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = node_value_and_grad(ctx, n.g_z, nc, n.g_lp, n.g_gz)) != SI_OK) return rc;
    SI_HIP(ctx, hipMemcpyAsync(lp_out + c0, n.g_lp, (size_t)nc * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SI_HIP(ctx, hipMemcpyAsync(grad_out + M * c0, n.g_gz, M * nc * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  }
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SI_OK;
}

// the audit read-back: lp (C), d lp / dW (N x C, the prior term included) and its pull-back (M x C) at Z[:, c]; either seam
int32_t si_node_grad(si_ctx* ctx, const double* Z, int32_t C, double* lp_out, double* gw_out, double* gz_out) {
  CHECK_CTX(ctx);
  int32_t rc = need_node_setup(ctx, "si_node_grad");
  if (rc != SI_OK) return rc;
  rc = infer_entry_check(ctx, "si_node_grad", bad_if(!Z || C < 1), SESSION_SHARED, true);
  if (rc != SI_OK) return rc;
  BIND(ctx);
  NodeState& n = ctx->node;
  const size_t M = (size_t)ctx->setup.M, N = (size_t)ctx->setup.model.N, ldw = (size_t)pad_ld(ctx->setup.model.N);
  const int32_t want = ctx->dec.on ? 1 : C;   // (the decoder's reverse holds one point: column by column)
  if ((rc = node_grad_ensure(ctx, "si_node_grad", want)) != SI_OK) return rc;
  const int32_t step = ctx->dec.on ? 1 : n.g_cap;
  for (int32_t c0 = 0; c0 < C; c0 += step) {
    const int32_t nc = std::min<int32_t>(step, C - c0);
    SI_HIP(ctx, hipMemcpyAsync(n.g_z, Z + M * c0, M * nc * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = node_value_and_grad(ctx, n.g_z, nc, n.g_lp, n.g_gz)) != SI_OK) return rc;
    if (lp_out) SI_HIP(ctx, hipMemcpyAsync(lp_out + c0, n.g_lp, (size_t)nc * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (gw_out)
      SI_HIP(ctx, hipMemcpy2DAsync(gw_out + N * c0, N * sizeof(double), n.g_gw, ldw * sizeof(double), N * sizeof(double), (size_t)nc,
                                   hipMemcpyDeviceToHost, ctx->stream));
    if (gz_out) SI_HIP(ctx, hipMemcpyAsync(gz_out + M * c0, n.g_gz, M * nc * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return SI_OK;
}

int32_t si_node_tableau(double* out) {
  if (!out) return SI_ERR_INVALID;
  int n = 0;
  for (double v : NODE_C) out[n++] = v;
  for (int i = 1; i < 7; ++i)
    for (int j = 0; j < i; ++j) out[n++] = NODE_A[i][j];
  for (double v : NODE_BT) out[n++] = v;
  for (double v : NODE_B1) out[n++] = v;
  for (double v : NODE_B2) out[n++] = v;
  for (double v : NODE_B3) out[n++] = v;
  for (double v : NODE_B4) out[n++] = v;
  for (double v : NODE_B5) out[n++] = v;
  for (double v : NODE_B6) out[n++] = v;
  for (double v : NODE_B7) out[n++] = v;
  static_assert(7 + 21 + 7 + 4 + 6 * 3 == NODE_TABLEAU_LEN, "si_node_tableau's length");
  return SI_OK;
}

int32_t si_node_info(si_ctx* ctx, int32_t* active_out, int32_t* d_out, int32_t* S_out, int64_t* f_out, int32_t* G_out) {
  CHECK_CTX(ctx);
  const bool on = ctx->setup.ready && ctx->node.on;
  if (active_out) *active_out = on ? 1 : 0;
  if (d_out) *d_out = on ? ctx->node.d : 0;
  if (S_out) *S_out = on ? ctx->node.S : 0;
  if (f_out) *f_out = on ? ctx->setup.B : 0;
  if (G_out) *G_out = on ? ctx->node.args.G : 0;
  return SI_OK;
}

}  // extern "C"
