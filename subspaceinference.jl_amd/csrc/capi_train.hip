// On-device training step for Dense chains with the mse cost.  Replaces the caller-side body of the
// reference's loop, src/subspace_construction.jl:39-43
//     gs = gradient(ps) do training_loss = cost(model, d...) end ;  Flux.update!(opt, ps, gs)
// for `cost = (m, x, y) -> Flux.Losses.mse(m(x), y)` and opt in {Descent, Momentum, ADAM} (Flux 0.11.2 semantics:
// Float32 parameters and Float32 optimiser state, Float64 arithmetic because the data are Float64).  The weights never
// leave the GPU: si_train_push feeds K1 from the device-resident Float32 vector.  The gradient is the value-and-gradient pass
// shared with si_logdensity_grad -- one workspace (SweepWs, sized by sweep_ws_alloc) and one dispatch (chain_value_and_grad,
// capi.hip) over dense_value_and_grad_f64, dense_value_and_grad_f32 (below) and net_value_and_grad (capi_net.hip) -- with the mse
// scale -2 / d or, after si_train_set_cost, with the tail of another cost (kernels_cost.hip) in place of its launch_delta_out; or
// a NeuralODE's (si_train_setup_node, below).  The step keeps the batch, the widened weights, net_input per batch and grad_ready.
// One step is: the batch (train_batch), the gradient by the set-up's route (TrainState::route: train_gradient, node_gradient), the
// update (optimiser_update.h: optimiser_kernel here, fused into the tail kernel on the NeuralODE route).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <optional>
#include <string>

#include "capi_common.h"
#include "optimiser_update.h"

namespace si {

template <class T>
__global__ __launch_bounds__(256) void gather_cols_kernel(const T* __restrict__ src, int rows, const int64_t* __restrict__ idx, int64_t nb,
                                                          T* __restrict__ dst) {
  const int64_t total = (int64_t)rows * nb;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const int64_t j = e / rows;
    const int r = (int)(e - j * rows);
    dst[e] = src[r + (int64_t)rows * idx[j]];
  }
}

// Float32 -> Float64 (exact) or Float64 -> Float32 (rounds once, as `Float32.(x)` would)
template <class S, class D>
__global__ __launch_bounds__(256) void convert_kernel(const S* __restrict__ src, int64_t n, D* __restrict__ dst) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = (D)src[i];
}

// the update rule (optimiser_update.h) on every element of the flat weight vector
__global__ __launch_bounds__(256) void optimiser_kernel(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
                                                        const double* __restrict__ g, int64_t n, int kind, double eta,
                                                        double p1, double p2, double bp1, double bp2, int g32) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    optimiser_update(w, m, v, i, g[i], kind, eta, p1, p2, bp1, bp2, g32 != 0);
}

static int grid_for(int64_t n, int num_cu) {
  int64_t b = (n + 255) / 256;
  if (b > (int64_t)num_cu * 8) b = (int64_t)num_cu * 8;
  return (int)(b < 1 ? 1 : b);
}

template <class T>
static void launch_gather_cols(hipStream_t st, const T* src, int rows, const int64_t* idx, int64_t nb, T* dst, int num_cu) {
  hipLaunchKernelGGL(gather_cols_kernel<T>, dim3(grid_for((int64_t)rows * nb, num_cu)), dim3(256), 0, st, src, rows, idx, nb, dst);
}
template <class S, class D>
static void launch_convert(hipStream_t st, const S* src, int64_t n, D* dst, int num_cu) {
  hipLaunchKernelGGL((convert_kernel<S, D>), dim3(grid_for(n, num_cu)), dim3(256), 0, st, src, n, dst);
}
void launch_widen_f32_to_f64(hipStream_t st, const float* src, int64_t n, double* dst, int num_cu) { launch_convert(st, src, n, dst, num_cu); }

void free_train(Ctx* c) {
  delete c->train;
  c->train = nullptr;
}
CtxCore::~CtxCore() { delete train; }

// what the cost's numerator is divided by for a batch of nb observations: out_dim * nb, SI_COST_LOGITCE: nb (agg = mean over the
// columns of a dims = 1 sum)
double train_denominator(const TrainState* t, int64_t nb) {
  return t->cost == SI_COST_LOGITCE ? (double)nb : (double)t->model.out_dim * (double)nb;
}

// ---- value and gradient in fp32 (dense_forward<float> + the fp32 reverse sweep), shared by the training step and si_logdensity_grad
int32_t dense_value_and_grad_f32(Ctx* ctx, hipStream_t st, const DenseSweepF32& s) {
  SweepF32Ws& ws = *s.ws;
  const si_layer* layers = s.m->lay();
  const bool fuse_tail = s.m->fuse_tail;
  const size_t nl = s.m->layers.size();
  const int64_t nb = s.B;
  const float* w = s.w32;
  const si_layer& ll = layers[nl - 1];
  const int64_t d = (int64_t)ll.out * nb;
  // (a fused head's own output lives in yhat64)
  const DenseForward<float> fw{s.m, w, s.w64, s.X32, s.Y, nb, ws.hs32.data(), {nullptr, nullptr}, ChainBatch(), s.m->fuse_slots32,
                               s.part, fuse_tail ? ws.yhat64.get() : nullptr, s.ssepart, s.sse_blocks, s.sse, false, false, false};
  const float* h = dense_forward(ctx, st, fw);
  double bflops = 0.0;
  for (size_t l = 0; l < nl; ++l) bflops += 4.0 * (double)layers[l].in * layers[l].out * (double)nb;
  ProfScope ps(ctx, SI_K_BACKWARD, bflops, 0.0);
  SI_HIP(ctx, hipMemsetAsync(ws.gw32, 0, (size_t)pad_ld(s.m->N) * sizeof(float), st));
  int cur = 0;
  if (s.cost)
    launch_cost_tail<float>(st, *s.cost, s.Y, fuse_tail ? ws.yhat64.get() : nullptr, fuse_tail ? nullptr : h, ll.out, nb, ll.act,
                            ws.delta32[cur].get(), s.sse);
  else
    launch_delta_out_f32(st, s.Y, fuse_tail ? ws.yhat64 : nullptr, fuse_tail ? nullptr : h, d, s.scale, ll.act, ws.delta32[cur]);
  size_t top = nl;
  bool have_db = false;   // db of layer top-1 already produced (by the pass that formed its Delta)
  if (fuse_tail) {
    const si_layer& lp = layers[nl - 2];
    launch_mul_dact_rowsum_f32(st, ws.delta32[cur], nullptr, ll.out, nb, SI_ACT_IDENTITY, nullptr, ws.rspart64, ws.gw32 + ll.b_off);
    launch_tail_bwd_f32(st, w + ll.w_off, ws.delta32[cur], ws.hs32[nl - 2], ll.out, ll.in, nb, lp.act, ws.delta32[cur ^ 1], ws.tailpart64,
                        ws.gw32 + ll.w_off, ws.gw32 + lp.b_off);
    cur ^= 1;
    top = nl - 1;
    have_db = true;
  }
  for (size_t li = top; li-- > 0;) {
    const si_layer& ly = layers[li];
    const float* hprev = li > 0 ? ws.hs32[li - 1] : s.X32;
    launch_backward_weight_f32(st, ws.delta32[cur], hprev, ws.part32, ly.out, ly.in, nb, ctx->num_cu, ws.gw32 + ly.w_off);
    if (!have_db)
      launch_mul_dact_rowsum_f32(st, ws.delta32[cur], nullptr, ly.out, nb, SI_ACT_IDENTITY, nullptr, ws.rspart64, ws.gw32 + ly.b_off);
    if (li > 0) {
      // Delta_{l-1} = (W_l' Delta_l) .* act'(H_{l-1}): the forward kernel on W_l' (out' = in, in' = out, zero bias) with the
      // multiply in its store, then the row sums (db of layer l-1); shapes the LDS-DMA kernel does not take: one elementwise pass
      // behind the GEMM does both
      const si_layer& lq = layers[li - 1];
      launch_transpose_f32(st, w + ly.w_off, ly.out, ly.in, ws.wt32);
      if (launch_dense_f32_dx(st, ws.wt32, ws.zero32, ws.delta32[cur], ws.delta32[cur ^ 1], ly.in, ly.out, nb, ws.hs32[li - 1], lq.act))
        launch_mul_dact_rowsum_f32(st, ws.delta32[cur ^ 1], nullptr, ly.in, nb, SI_ACT_IDENTITY, nullptr, ws.rspart64, ws.gw32 + lq.b_off);
      else
        launch_mul_dact_rowsum_f32(st, ws.delta32[cur ^ 1], ws.hs32[li - 1], ly.in, nb, lq.act, ws.delta32[cur ^ 1], ws.rspart64,
                                   ws.gw32 + lq.b_off);
      cur ^= 1;
      have_db = true;
    }
  }
  SI_HIP(ctx, hipGetLastError());
  return SI_OK;
}

}  // namespace si

using namespace si;

extern "C" {

static int32_t train_setup_failed(si_ctx* ctx, int32_t code, const std::string& msg) {
  free_train(ctx);
  return fail(ctx, code, msg);
}

// What every set-up does first: the stream drains, the old state goes, the new one gets its route, its sizes, the optimiser's
// parameters and the buffers every route has.  ok: those allocations succeeded (the caller adds its own and reports them together)
static int32_t train_setup_begin(si_ctx* ctx, TrainRoute route, ChainModel&& model, int64_t B_total, int64_t batch_max, int32_t opt_kind,
                                 double eta, double p1, double p2, bool& ok) {
  SI_HIP(ctx, hipSetDevice(ctx->device));
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  free_train(ctx);
  TrainState* t = ctx->train = new TrainState();
  TrainOpt& o = t->opt;
  TrainBatch& b = t->batch;
  t->route = route;
  t->model = std::move(model); t->Btot = B_total; t->Bmax = batch_max;
  const int64_t N = t->model.N;
  const int32_t in_dim = t->model.in_dim, out_dim = t->model.out_dim;
  o.kind = opt_kind; o.eta = eta; o.p1 = p1; o.p2 = p2; o.bp1 = p1; o.bp2 = p2;  // ADAM: beta powers start at beta
  const size_t bm = (size_t)batch_max, nx = (size_t)in_dim * (size_t)B_total;
  ok = (route == TrainRoute::DenseF32 ? t->X32.alloc(nx) && t->Xb32.alloc((size_t)in_dim * bm) : t->X.alloc(nx) && t->Xb.alloc((size_t)in_dim * bm)) &&
       t->Y.alloc((size_t)out_dim * (size_t)B_total) && t->Yb.alloc((size_t)out_dim * bm) && b.idx.alloc(bm) && b.pin[0].alloc(bm) &&
       b.pin[1].alloc(bm) && b.ev[0].create() && b.ev[1].create() && o.w32.alloc((size_t)N) && o.m32.alloc((size_t)N) &&
       o.v32.alloc((size_t)N) && o.w64.alloc((size_t)pad_ld(N)) && o.gw.alloc((size_t)pad_ld(N)) && t->sse.alloc(1);
  return SI_OK;
}

// ... and last, behind the route's own uploads: the weights, zero moments, a zero Float64 copy (queued)
static hipError_t train_setup_upload(si_ctx* ctx, const float* w0) {
  TrainOpt& o = ctx->train->opt;
  const size_t n = (size_t)ctx->train->model.N;
  hipError_t e = hipMemcpyAsync(o.w32, w0, n * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(o.m32, 0, n * sizeof(float), ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(o.v32, 0, n * sizeof(float), ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(o.w64, 0, (size_t)pad_ld(ctx->train->model.N) * sizeof(double), ctx->stream);
  return e;
}

static int32_t train_setup_impl(si_ctx* ctx, const si_layer* layers, int32_t L, int64_t N, const float* w0, const void* Xv,
                                const void* Yv, int32_t data_dtype, int32_t in_dim, int32_t out_dim, int64_t B_total, int64_t batch_max,
                                int32_t opt_kind, double eta, double p1, double p2, int32_t compute_dtype) {
  if (!ctx) return SI_ERR_INVALID;
  if (!layers || L <= 0 || N <= 0 || !w0 || !Xv || !Yv || in_dim <= 0 || out_dim <= 0 || B_total <= 0 || batch_max <= 0 ||
      batch_max > B_total || opt_kind < 0 || opt_kind > 2)
    return fail(ctx, SI_ERR_INVALID, "si_train_setup: bad argument");
  if ((data_dtype != SI_F32 && data_dtype != SI_F64) || (compute_dtype != SI_F32 && compute_dtype != SI_F64 && compute_dtype != SI_DTYPE_OF_DATA))
    return fail(ctx, SI_ERR_INVALID, "si_train_setup_ex: data_dtype is SI_F32 / SI_F64, compute_dtype SI_F32 / SI_F64 / SI_DTYPE_OF_DATA");
  const bool f32 = (compute_dtype == SI_DTYPE_OF_DATA ? data_dtype : compute_dtype) == SI_F32;
  ChainModel model;
  const int32_t prc = chain_model_build(ctx, "si_train_setup", layers, L, N, in_dim, out_dim, f32, 0, model);
  if (prc != SI_OK) return prc;
  const bool has_conv = model.plan.has_conv;
  if (f32 && has_conv)
    return fail(ctx, SI_ERR_INVALID, "si_train_setup_ex: compute_dtype = SI_F32 is implemented for Dense chains; Conv / MaxPool / flatten chains train in SI_F64");
  const TrainRoute route = has_conv ? TrainRoute::Conv : f32 ? TrainRoute::DenseF32 : TrainRoute::DenseF64;
  bool ok = false;
  const int32_t rcb = train_setup_begin(ctx, route, std::move(model), B_total, batch_max, opt_kind, eta, p1, p2, ok);
  if (rcb != SI_OK) return rcb;
  TrainState* t = ctx->train;
  const ChainModel& m = t->model;
  const NetPlan& plan = m.plan;
  t->sse_blocks = sse_num_blocks((int64_t)out_dim * batch_max, ctx->num_cu);
  ok = ok && t->ssepart.alloc((size_t)t->sse_blocks) && (!m.fuse_tail || t->part.alloc((size_t)m.part_slots() * out_dim * batch_max)) &&
       (!plan.has_conv || t->wpack.alloc(plan.wpack_elems)) && (!plan.input_spatial || t->Xc.alloc((size_t)plan.in_elems * batch_max)) &&
       sweep_ws_alloc(ctx, t->sweep, m, batch_max);
  if (!ok) return train_setup_failed(ctx, SI_ERR_NOMEM, "si_train_setup: device allocation failed");
  // the data in the element type the step computes in (X) / sums the loss in (Y: fp64 always); one conversion at set-up where
  // the caller's type differs (Float32 -> Float64 is exact; Float64 -> Float32 rounds once, as `Float32.(X)` would)
  const size_t nx = (size_t)in_dim * B_total, ny = (size_t)out_dim * B_total;
  const size_t esz = data_dtype == SI_F32 ? 4 : 8;
  DevBuf<char> stage;
  const bool x_conv = (data_dtype == SI_F32) != f32, y_conv = data_dtype == SI_F32;
  if ((x_conv || y_conv) && !stage.alloc(std::max(nx, ny) * esz))
    return train_setup_failed(ctx, SI_ERR_NOMEM, "si_train_setup: device allocation failed");
  hipStream_t st = ctx->stream;
  hipError_t e = hipMemcpyAsync(x_conv ? (void*)stage.get() : f32 ? (void*)t->X32.get() : (void*)t->X.get(), Xv, nx * esz, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && x_conv) {
    if (f32) launch_convert(st, reinterpret_cast<const double*>(stage.get()), (int64_t)nx, t->X32.get(), ctx->num_cu);
    else launch_widen_f32_to_f64(st, reinterpret_cast<const float*>(stage.get()), (int64_t)nx, t->X, ctx->num_cu);
  }
  if (e == hipSuccess && y_conv) e = hipStreamSynchronize(st);   // (the staging buffer is reused)
  if (e == hipSuccess) e = hipMemcpyAsync(y_conv ? (void*)stage.get() : (void*)t->Y.get(), Yv, ny * esz, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && y_conv) launch_widen_f32_to_f64(st, reinterpret_cast<const float*>(stage.get()), (int64_t)ny, t->Y, ctx->num_cu);
  if (e == hipSuccess) e = train_setup_upload(ctx, w0);
  const hipError_t e2 = hipStreamSynchronize(st);
  if (e != hipSuccess || e2 != hipSuccess)
    return train_setup_failed(ctx, SI_ERR_HIP, std::string("si_train_setup: ") + hipGetErrorString(e != hipSuccess ? e : e2));
  return SI_OK;
}

int32_t si_train_setup(si_ctx* ctx, const si_layer* layers, int32_t L, int64_t N, const float* w0, const double* X,
                       const double* Y, int32_t in_dim, int32_t out_dim, int64_t B_total, int64_t batch_max,
                       int32_t opt_kind, double eta, double p1, double p2) {
  return train_setup_impl(ctx, layers, L, N, w0, X, Y, SI_F64, in_dim, out_dim, B_total, batch_max, opt_kind, eta, p1, p2, SI_F64);
}

int32_t si_train_setup_ex(si_ctx* ctx, const si_layer* layers, int32_t L, int64_t N, const float* w0, const void* X, const void* Y,
                          int32_t data_dtype, int32_t in_dim, int32_t out_dim, int64_t B_total, int64_t batch_max, int32_t opt_kind,
                          double eta, double p1, double p2, int32_t compute_dtype) {
  return train_setup_impl(ctx, layers, L, N, w0, X, Y, data_dtype, in_dim, out_dim, B_total, batch_max, opt_kind, eta, p1, p2,
                          compute_dtype);
}

// The cost of the steps that follow (kernels_cost.hip).  Like si_infer_set_prior it follows its set-up, which starts with mse
int32_t si_train_set_cost(si_ctx* ctx, int32_t cost, double param) {
  if (!ctx) return SI_ERR_INVALID;
  TrainState* t = ctx->train;
  if (!t) return fail(ctx, SI_ERR_STATE, "si_train_set_cost: call si_train_setup first");
  if (t->route == TrainRoute::Node) return fail(ctx, SI_ERR_INVALID, "si_train_set_cost: not available for NeuralODE training");
  if (cost < SI_COST_MSE || cost > SI_COST_LOGITBCE)
    return fail(ctx, SI_ERR_INVALID, "si_train_set_cost: unknown cost " + std::to_string(cost) + " (0 mse, 1 mae, 2 huber_loss, 3 logitcrossentropy, 4 logitbinarycrossentropy)");
  if (cost == SI_COST_HUBER && !(std::isfinite(param) && param > 0.0))
    return fail(ctx, SI_ERR_INVALID, "si_train_set_cost: huber_loss needs a finite delta > 0");
  if (t->opt.grad_ready) return fail(ctx, SI_ERR_INVALID, "si_train_set_cost: a gradient is pending (si_train_apply first)");
  SI_HIP(ctx, hipSetDevice(ctx->device));
  if (cost != SI_COST_MSE && !t->costpart && !t->costpart.alloc((size_t)SI_COST_MAX_BLOCKS))
    return fail(ctx, SI_ERR_NOMEM, "si_train_set_cost: device allocation failed");
  t->cost = cost;
  t->cost_param = cost == SI_COST_HUBER ? param : 0.0;
  return SI_OK;
}

int32_t si_train_cost_info(si_ctx* ctx, int32_t* cost_out, double* param_out) {
  if (!ctx) return SI_ERR_INVALID;
  if (!ctx->train) return fail(ctx, SI_ERR_STATE, "si_train_cost_info: no training state");
  if (cost_out) *cost_out = ctx->train->cost;
  if (param_out) *param_out = ctx->train->cost_param;
  return SI_OK;
}

int32_t si_train_compute_dtype(si_ctx* ctx, int32_t* out) {
  if (!ctx) return SI_ERR_INVALID;
  if (!ctx->train || !out) return fail(ctx, SI_ERR_STATE, "si_train_compute_dtype: no training state / NULL output");
  *out = ctx->train->route == TrainRoute::DenseF32 ? SI_F32 : SI_F64;
  return SI_OK;
}

// ---- NeuralODE training (node.py: train_value_and_grad is the definition; flux.NodeSSE the cost) ----------------------------------
// loss = sum_{p in batch} ||sol_p(W) - Y_p||^2 + ||W||^2 / penalty_div; its gradient is the frozen-step discrete adjoint of
// si_node_set_grad (kernels_node.hip: the forward with record, then the reverse kernel, one chain, f = nb) plus the penalty's.
// The solver workspace is the training state's own (NodeTrain); only the launchers are the inference route's.
int32_t si_train_setup_node(si_ctx* ctx, const si_layer* layers, int32_t L, int64_t N, const float* w0, const double* U0, const double* Y,
                            int32_t d, int32_t S, int64_t f, const double* ts, const void* opts_in, int64_t batch_max, int32_t opt_kind,
                            double eta, double p1, double p2, double penalty_div) {
  if (!ctx) return SI_ERR_INVALID;
  const si_node_opts* opts = static_cast<const si_node_opts*>(opts_in);
  auto bad = [&](const char* what) { return fail(ctx, SI_ERR_INVALID, std::string("si_train_setup_node: ") + what); };
  if (!layers || !w0 || !U0 || !Y || !ts || !opts || f <= 0 || batch_max <= 0 || batch_max > f || opt_kind < 0 || opt_kind > 2 ||
      !(penalty_div >= 0.0) || !std::isfinite(penalty_div))
    return bad("bad argument");
  if (L < 1 || L > SI_NODE_MAX_LAYERS) return bad("a NeuralODE right-hand side has 1 to 8 Dense layers");
  if (d < 1 || d > SI_NODE_MAX_D) return bad("the state dimension d must be 1 to 8");
  if (N < 1 || N > SI_NODE_MAX_N) return bad("N must be 1 to 8192");
  if (S < 1 || S > SI_NODE_MAX_S) return bad("the number of save times S must be 1 to 4096");
  if (f > ((int64_t)1 << 20)) return bad("f must be at most 2^20 trajectories");
  NodeArgs a;
  if (const char* what = node_plan(layers, L, N, d, S, ts, opts, a)) return bad(what);
  if (a.maxw > 64) return bad("a layer is wider than 64 (the reverse kernel gives every lane of a trajectory's group one unit per layer)");
  // the step record (batch_max * max_steps * (d + 2) doubles) and the gradient slices (batch_max * N) within the workspace budget
  if (8.0 * (double)batch_max * ((double)a.max_steps * (double)(d + 2) + (double)N) > SI_BATCH_BYTES)
    return bad("the step record (batch_max * max_steps * (d + 2) doubles) and the gradient slices (batch_max * N) do not fit the "
               "2 GiB workspace budget: lower max_steps or the batch size");
  bool ok = false;
  ChainModel model;   // (a right-hand side is validated by node_plan above; it has no NetPlan and no fused head)
  model.layers.assign(layers, layers + L);
  model.N = N, model.in_dim = d, model.out_dim = d * S;
  const int32_t rcb = train_setup_begin(ctx, TrainRoute::Node, std::move(model), f, batch_max, opt_kind, eta, p1, p2, ok);
  if (rcb != SI_OK) return rcb;
  TrainState* t = ctx->train;
  NodeTrain* nt = &t->node;
  nt->args = a;
  nt->penalty_div = penalty_div;
  nt->wsq_blocks = sse_num_blocks(N, ctx->num_cu);
  const size_t bm = (size_t)batch_max;
  ok = ok && nt->ts.alloc((size_t)S) && nt->ssep.alloc(bm) && nt->rec.alloc(bm * (size_t)a.max_steps * (size_t)(d + 2)) &&
       nt->slices.alloc(bm * (size_t)N) && nt->cnt.alloc(3 * bm) && nt->wsq.alloc(1) && nt->wsqpart.alloc((size_t)nt->wsq_blocks) &&
       nt->fail.alloc(3);
  if (!ok)
    return train_setup_failed(ctx, SI_ERR_NOMEM, "si_train_setup_node: device allocation failed (the step record: lower max_steps or the batch size)");
  hipStream_t st = ctx->stream;
  hipError_t e = hipMemcpyAsync(t->X, U0, (size_t)d * (size_t)f * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(t->Y, Y, (size_t)t->model.out_dim * (size_t)f * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(nt->ts, ts, (size_t)S * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = train_setup_upload(ctx, w0);
  if (e == hipSuccess) e = hipMemsetAsync(t->opt.gw, 0, (size_t)pad_ld(N) * sizeof(double), st);
  if (e == hipSuccess) e = hipMemsetAsync(t->sse, 0, sizeof(double), st);
  if (e == hipSuccess) e = hipMemsetAsync(nt->fail, 0, 3 * sizeof(int64_t), st);
  if (e == hipSuccess) {
    launch_widen_f32_to_f64(st, t->opt.w32, N, t->opt.w64, ctx->num_cu);   // the first step's solve reads the Float64 copy
    e = hipGetLastError();
  }
  const hipError_t e2 = hipStreamSynchronize(st);
  if (e != hipSuccess || e2 != hipSuccess)
    return train_setup_failed(ctx, SI_ERR_HIP, std::string("si_train_setup_node: ") + hipGetErrorString(e != hipSuccess ? e : e2));
  return SI_OK;
}

static bool is_node(const si_ctx* ctx) { return ctx->train && ctx->train->route == TrainRoute::Node; }

// the NeuralODE route's failure record, read back (synchronises): [0] the 1-based step that failed first (0: none), [1] trajectory, [2] status
static int32_t node_fail_record(si_ctx* ctx, int64_t rec[3]) {
  SI_HIP(ctx, hipSetDevice(ctx->device));
  SI_HIP(ctx, hipMemcpyAsync(rec, ctx->train->node.fail, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SI_OK;
}

int32_t si_train_node_info(si_ctx* ctx, int32_t* active_out, int32_t* G_out, int64_t* failed_step_out, int64_t* failed_traj_out,
                           int32_t* failed_status_out) {
  if (!ctx) return SI_ERR_INVALID;
  const bool node = is_node(ctx);
  int64_t rec[3] = {0, 0, 0};
  if (node)
    if (const int32_t rc = node_fail_record(ctx, rec)) return rc;
  if (active_out) *active_out = node ? 1 : 0;
  if (G_out) *G_out = node ? ctx->train->node.args.G : 0;
  if (failed_step_out) *failed_step_out = rec[0] != 0 ? rec[0] : -1;
  if (failed_traj_out) *failed_traj_out = rec[0] != 0 ? rec[1] : -1;
  if (failed_status_out) *failed_status_out = rec[0] != 0 ? (int32_t)rec[2] : 0;
  return SI_OK;
}

// ADAM's beta powers after one more update: the running product, one multiplication per update
static void advance_beta_powers(TrainOpt& o) {
  if (o.kind == 2) o.bp1 *= o.p1, o.bp2 *= o.p2;
}

// after a synchronisation of the stream: a failure record the caller has not been told about yet -> SI_ERR_INVALID, once
int32_t train_node_report(si_ctx* ctx, const char* who) {
  if (!is_node(ctx)) return SI_OK;
  NodeTrain* nt = &ctx->train->node;
  if (nt->reported || nt->checked == nt->steps) return SI_OK;
  int64_t rec[3] = {0, 0, 0};
  if (const int32_t rc = node_fail_record(ctx, rec)) return rc;
  nt->checked = nt->steps;
  if (rec[0] == 0) return SI_OK;
  nt->reported = true;
  TrainOpt& o = ctx->train->opt;
  o.grad_ready = false;
  o.bp1 = o.p1, o.bp2 = o.p2;   // the beta powers as the last step that was taken left them
  for (int64_t k = 1; k < rec[0] && o.kind == 2; ++k) advance_beta_powers(o);
  return fail(ctx, SI_ERR_INVALID, std::string(who) + ": NeuralODE training step " + std::to_string(rec[0]) + ": trajectory " +
                                       std::to_string(rec[1]) + " of its batch ended with status " + std::to_string(rec[2]) +
                                       " (1: max_steps reached, 2: a non-finite state); that step and every later one left the "
                                       "weights and the optimiser state as they were");
}

// ---- the batch stage of every route: the observations idx[0..nb) of the set-up's data, in the route's element types
struct TrainBatchView {
  const double* X;
  const float* X32;
  const double* Y;
};
// idx is caller-owned: copied into a pinned buffer, shipped asynchronously; the buffer is free again once its event has
// passed (two steps later at the earliest) -- no synchronisation of the stream, the call returns while the GPU works.
// prof: a scope of class SI_K_SSE opened in front of the first launch and left open for the caller's launches behind it
static int32_t train_batch(si_ctx* ctx, const char* who, const int64_t* idx, int64_t nb, TrainBatchView& v,
                           std::optional<ProfScope>* prof = nullptr) {
  TrainState* t = ctx->train;
  TrainBatch& b = t->batch;
  if (!idx || nb <= 0 || nb > t->Bmax) return fail(ctx, SI_ERR_INVALID, std::string(who) + ": bad batch");
  bool in_order = true;   // idx = 0, 1, ..., nb-1 (a full batch of an unshuffled DataLoader): the data are used in place
  for (int64_t j = 0; j < nb; ++j) {
    if (idx[j] < 0 || idx[j] >= t->Btot)
      return fail(ctx, SI_ERR_INVALID, std::string(who) + ": BoundsError: batch index out of range");
    in_order = in_order && idx[j] == j;
  }
  SI_HIP(ctx, hipSetDevice(ctx->device));
  if (prof) prof->emplace(ctx, SI_K_SSE, 0.0, 0.0);
  v = TrainBatchView{t->X, t->X32, t->Y};
  if (in_order) return SI_OK;
  const int s = b.slot;
  b.slot ^= 1;
  if (b.busy[s]) SI_HIP(ctx, hipEventSynchronize(b.ev[s]));
  std::memcpy(b.pin[s], idx, (size_t)nb * sizeof(int64_t));
  SI_HIP(ctx, hipMemcpyAsync(b.idx, b.pin[s], (size_t)nb * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  SI_HIP(ctx, hipEventRecord(b.ev[s], ctx->stream));
  b.busy[s] = true;
  if (t->route == TrainRoute::DenseF32)
    launch_gather_cols(ctx->stream, t->X32.get(), t->model.in_dim, b.idx.get(), nb, t->Xb32.get(), ctx->num_cu);
  else
    launch_gather_cols(ctx->stream, t->X.get(), t->model.in_dim, b.idx.get(), nb, t->Xb.get(), ctx->num_cu);
  launch_gather_cols(ctx->stream, t->Y.get(), t->model.out_dim, b.idx.get(), nb, t->Yb.get(), ctx->num_cu);
  v = TrainBatchView{t->Xb, t->Xb32, t->Yb};
  return SI_OK;
}

// the NeuralODE route: the batch's columns, ||W||^2, the forward with record, the reverse kernel and the tail -- with `apply` the
// update is fused into it (si_train_step) -- all queued on the context's stream
static int32_t node_gradient(si_ctx* ctx, const char* who, const int64_t* idx, int64_t nb, bool apply) {
  TrainState* t = ctx->train;
  TrainOpt& o = t->opt;
  NodeTrain* nt = &t->node;
  // (a failure the caller has been told about: the set-up takes no further steps, the device's would be no-ops)
  if (nt->reported) return fail(ctx, SI_ERR_INVALID, std::string(who) + ": an earlier NeuralODE training step failed (si_train_node_info): set up again");
  hipStream_t st = ctx->stream;
  const int64_t N = t->model.N, Bmax = t->Bmax;
  TrainBatchView v;
  {
    std::optional<ProfScope> ps;
    const int32_t rcb = train_batch(ctx, who, idx, nb, v, &ps);
    if (rcb != SI_OK) return rcb;
    launch_sse(st, o.w64, nullptr, N, nt->wsqpart, nt->wsq_blocks, nt->wsq, 1, pad_ld(N));   // ||W||^2, as the density forms it
    SI_HIP(ctx, hipMemsetAsync(nt->slices, 0, (size_t)nb * (size_t)N * sizeof(double), st));     // "from 0.0"
  }
  NodeArgs a = nt->args;
  a.w = o.w64, a.ldw = pad_ld(N);
  a.U0 = v.X, a.Y = v.Y, a.f = nb, a.ts = nt->ts;
  a.sse_p = nt->ssep, a.U_out = nullptr;
  a.nacc = nt->cnt, a.nrej = nt->cnt + Bmax, a.status = nt->cnt + 2 * Bmax;
  a.rec = nt->rec, a.gsl = nt->slices;
  {
    ProfScope ps(ctx, SI_K_DENSE, 0.0, 0.0);
    SI_HIP(ctx, launch_node_solve(st, a, 1));
  }
  {
    ProfScope ps(ctx, SI_K_BACKWARD, 0.0, 0.0);
    SI_HIP(ctx, launch_node_grad(st, a, 1));
  }
  {
    ProfScope ps(ctx, SI_K_RECON, 0.0, 0.0);   // (the tail: gw, the loss, the update and the refreshed Float64 weights)
    const NodeTailArgs ta{nt->slices, nt->ssep, nt->wsq, a.status, nb, N, nt->steps + 1, nt->penalty_div, o.w32, o.m32, o.v32,
                          o.w64, o.gw, t->sse, nt->fail, o.kind, o.eta, o.p1, o.p2, o.bp1, o.bp2};
    launch_node_train_tail(st, ta, apply);
  }
  SI_HIP(ctx, hipGetLastError());
  nt->steps += 1;
  return SI_OK;
}

// The gradient of the route's cost on the observations idx[0..nb), left in opt.gw, the cost's numerator -- mse: the sum of squared
// errors (Node: the loss) -- in t->sse.  The Chain routes scale it as if the batch were part of d_total = train_denominator of the
// WHOLE batch.  A cost other than mse runs its tail (kernels_cost.hip) in place of the route's launch_delta_out*
static int32_t train_gradient(si_ctx* ctx, const char* who, const int64_t* idx, int64_t nb, double d_total, bool node_apply) {
  TrainState* t = ctx->train;
  if (!t) return fail(ctx, SI_ERR_STATE, std::string(who) + ": call si_train_setup first");
  if (t->route == TrainRoute::Node) return node_gradient(ctx, who, idx, nb, node_apply);
  TrainOpt& o = t->opt;
  TrainBatchView v;
  const int32_t rcb = train_batch(ctx, who, idx, nb, v);
  if (rcb != SI_OK) return rcb;
  hipStream_t st = ctx->stream;
  launch_widen_f32_to_f64(st, o.w32, t->model.N, o.w64, ctx->num_cu);
  const NetPlan& p = t->model.plan;
  if (p.input_spatial) net_input(ctx, p, v.X, t->Xc, nb);
  const CostTail tail{t->cost, t->cost_param, 1.0 / d_total, t->costpart};
  // (DenseF32: a Float32 model on Float32 data is a Float32 Zygote pass in the reference, src/subspace_construction.jl:39-43)
  const ChainValueGrad in{&t->model, o.w64, o.w32, v.X, t->Xc, v.X32, v.Y, nb, t->part, t->ssepart, t->sse,
                          sse_num_blocks((int64_t)t->model.out_dim * nb, ctx->num_cu), o.gw, t->wpack, -2.0 / d_total /* d mse / d yhat = 2 (yhat - y) / d */, t->cost != SI_COST_MSE ? &tail : nullptr,
                          false, 0.0};
  const int32_t rc = chain_value_and_grad(ctx, st, t->sweep, in);
  if (rc != SI_OK) return rc;
  SI_HIP(ctx, hipGetLastError());
  o.grad_ready = true;
  return SI_OK;
}

// Flux.update!(opt, ps, gs) from the gradient in opt.gw
static int32_t train_apply(si_ctx* ctx) {
  TrainState* t = ctx->train;
  TrainOpt& o = t->opt;
  hipLaunchKernelGGL(optimiser_kernel, dim3(grid_for(t->model.N, ctx->num_cu)), dim3(256), 0, ctx->stream, o.w32, o.m32, o.v32, o.gw, t->model.N,
                     o.kind, o.eta, o.p1, o.p2, o.bp1, o.bp2, t->route == TrainRoute::DenseF32 ? 1 : 0);
  SI_HIP(ctx, hipGetLastError());
  advance_beta_powers(o);
  o.grad_ready = false;
  return SI_OK;
}

// batch, gradient by route, update.  A NeuralODE's update is fused into its tail kernel: one pass of launches, and nothing
// synchronises unless the loss is asked for
int32_t si_train_step(si_ctx* ctx, const int64_t* idx, int64_t nb, double* loss_out) {
  if (!ctx) return SI_ERR_INVALID;
  TrainState* t = ctx->train;
  const bool node = is_node(ctx);
  const double d = t ? train_denominator(t, nb) : 1.0;
  int32_t rc = train_gradient(ctx, "si_train_step", idx, nb, d, /*node_apply=*/true);
  if (rc != SI_OK) return rc;
  if (node) {   // (a failed step does not advance the beta powers: train_node_report rewinds)
    advance_beta_powers(t->opt);
    t->opt.grad_ready = false;
  } else {
    ProfScope ps(ctx, SI_K_BACKWARD, 0.0, 0.0);
    if ((rc = train_apply(ctx)) != SI_OK) return rc;
  }
  if (loss_out) {
    double sse = 0.0;
    SI_HIP(ctx, hipMemcpyAsync(&sse, t->sse, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *loss_out = node ? sse : sse / d;  // the cost (mse by default) of the batch BEFORE the update, as Zygote's forward value (Node: the loss, penalty included)
    return train_node_report(ctx, "si_train_step");
  }
  return SI_OK;
}

// ---- data-parallel form of the same step ("add one gradient all-reduce per step"): every rank holds the
// same weights / optimiser state and its own share of the batch.  si_train_grad leaves d(mse over the WHOLE batch)/dw
// restricted to this rank's observations in a device buffer, the caller sums that buffer over the ranks IN PLACE
// (RCCL all-reduce on the pointer from si_train_grad_ptr; or _get/_set through the host), si_train_apply updates.
int32_t si_train_grad(si_ctx* ctx, const int64_t* idx, int64_t nb, int64_t nb_total, double* sse_local_out) {
  if (!ctx) return SI_ERR_INVALID;
  if (nb_total < nb) return fail(ctx, SI_ERR_INVALID, "si_train_grad: nb_total < nb");
  TrainState* t = ctx->train;
  const bool node = is_node(ctx);
  // a NeuralODE step is not data-parallel: the gradient of this batch alone (the tail kernel without the update);
  // sse_local_out receives the loss of the batch, penalty included
  if (node && nb_total != nb) return fail(ctx, SI_ERR_INVALID, "si_train_grad: a share of a batch is not available for NeuralODE training (nb_total must equal nb)");
  const double d_total = t ? train_denominator(t, nb_total) : 1.0;
  if (t && nb == 0 && nb_total > 0) {  // a rank without a share of a small batch contributes a zero gradient
    SI_HIP(ctx, hipSetDevice(ctx->device));
    SI_HIP(ctx, hipMemsetAsync(t->opt.gw, 0, (size_t)pad_ld(t->model.N) * sizeof(double), ctx->stream));
    SI_HIP(ctx, hipMemsetAsync(t->sse, 0, sizeof(double), ctx->stream));
    t->opt.grad_ready = true;
    if (sse_local_out) *sse_local_out = 0.0;
    SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SI_OK;
  }
  int32_t rc = train_gradient(ctx, "si_train_grad", idx, nb, d_total, /*node_apply=*/false);
  if (rc != SI_OK) return rc;
  if (sse_local_out) SI_HIP(ctx, hipMemcpyAsync(sse_local_out, t->sse, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the gradient is complete when the caller starts its collective
  if ((rc = train_node_report(ctx, "si_train_grad")) != SI_OK) return rc;
  t->opt.grad_ready = true;
  return SI_OK;
}

int32_t si_train_grad_ptr(si_ctx* ctx, double** grad_dev_out, int64_t* n_out) {
  if (!ctx) return SI_ERR_INVALID;
  if (!ctx->train || !grad_dev_out || !n_out) return fail(ctx, SI_ERR_STATE, "si_train_grad_ptr: no training state / NULL output");
  *grad_dev_out = ctx->train->opt.gw;
  *n_out = ctx->train->model.N;
  return SI_OK;
}

int32_t si_train_grad_get(si_ctx* ctx, double* g_out) {
  if (!ctx) return SI_ERR_INVALID;
  // (a NeuralODE step's tail kernel leaves its gradient in gw: it can be read after si_train_step too, for the audit)
  const bool node_gw = is_node(ctx) && ctx->train->node.steps > 0 && !ctx->train->node.reported;
  if (!ctx->train || !(ctx->train->opt.grad_ready || node_gw) || !g_out) return fail(ctx, SI_ERR_STATE, "si_train_grad_get: no gradient pending / NULL output");
  SI_HIP(ctx, hipSetDevice(ctx->device));
  SI_HIP(ctx, hipMemcpyAsync(g_out, ctx->train->opt.gw, (size_t)ctx->train->model.N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SI_OK;
}

int32_t si_train_grad_set(si_ctx* ctx, const double* g_in) {
  if (!ctx) return SI_ERR_INVALID;
  if (!ctx->train || !ctx->train->opt.grad_ready || !g_in) return fail(ctx, SI_ERR_STATE, "si_train_grad_set: no gradient pending / NULL input");
  SI_HIP(ctx, hipSetDevice(ctx->device));
  SI_HIP(ctx, hipMemcpyAsync(ctx->train->opt.gw, g_in, (size_t)ctx->train->model.N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SI_OK;
}

int32_t si_train_apply(si_ctx* ctx) {
  if (!ctx) return SI_ERR_INVALID;
  if (!ctx->train || !ctx->train->opt.grad_ready) return fail(ctx, SI_ERR_STATE, "si_train_apply: no gradient pending (call si_train_grad)");
  SI_HIP(ctx, hipSetDevice(ctx->device));
  const int32_t rc = train_apply(ctx);
  if (rc == SI_OK && is_node(ctx))   // the next step's solve reads the Float64 copy (si_train_step refreshes it in its tail kernel)
    launch_widen_f32_to_f64(ctx->stream, ctx->train->opt.w32, ctx->train->model.N, ctx->train->opt.w64, ctx->num_cu);
  return rc;
}

int32_t si_train_push(si_ctx* ctx, double n) {
  if (!ctx) return SI_ERR_INVALID;
  if (!ctx->train) return fail(ctx, SI_ERR_STATE, "si_train_push: call si_train_setup first");
  if (ctx->train->model.N != ctx->N) return fail(ctx, SI_ERR_INVALID, "si_train_push: construction and training sizes differ");
  return si_construct_push_dev(ctx, ctx->train->opt.w32, SI_F32, n);
}

int32_t si_train_get_weights(si_ctx* ctx, float* w_out) {
  if (!ctx) return SI_ERR_INVALID;
  if (!ctx->train || !w_out) return fail(ctx, SI_ERR_STATE, "si_train_get_weights: no training state / NULL output");
  SI_HIP(ctx, hipSetDevice(ctx->device));
  SI_HIP(ctx, hipMemcpyAsync(w_out, ctx->train->opt.w32, (size_t)ctx->train->model.N * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return train_node_report(ctx, "si_train_get_weights");
}

int32_t si_train_get_opt_state(si_ctx* ctx, float* m_out, float* v_out, double* beta_pows_out) {
  if (!ctx) return SI_ERR_INVALID;
  if (!ctx->train) return fail(ctx, SI_ERR_STATE, "si_train_get_opt_state: no training state");
  SI_HIP(ctx, hipSetDevice(ctx->device));
  TrainOpt& o = ctx->train->opt;
  const size_t nbytes = (size_t)ctx->train->model.N * sizeof(float);
  if (m_out && o.m32) SI_HIP(ctx, hipMemcpyAsync(m_out, o.m32, nbytes, hipMemcpyDeviceToHost, ctx->stream));
  if (v_out && o.v32) SI_HIP(ctx, hipMemcpyAsync(v_out, o.v32, nbytes, hipMemcpyDeviceToHost, ctx->stream));
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int32_t rcn = train_node_report(ctx, "si_train_get_opt_state");
  if (rcn != SI_OK) return rcn;
  if (beta_pows_out) {
    beta_pows_out[0] = o.bp1;
    beta_pows_out[1] = o.bp2;
  }
  return SI_OK;
}

}  // extern "C"
