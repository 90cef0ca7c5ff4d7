// si_ae_train_*: Chain(encoder, decoder) trained on the deviation columns on the device (reference
// src/subspace_construction.jl:125-140).  The state is its own object on the context (CtxCore::ae), independent of si_train_* and
// of an inference set-up; the kernels are kernels_ae_train.hip's, the definition is autoencoder.py: train_step.
#include "capi_common.h"

using namespace si;

extern "C" {

static int32_t ae_refuse(si_ctx* ctx, const std::string& msg) {
  ctx->ae.reset();
  return fail(ctx, SI_ERR_INVALID, "si_ae_train_setup: " + msg);
}

int32_t si_ae_train_setup(si_ctx* ctx, const si_layer* layers, int32_t L, int64_t n_params, const void* w0, int32_t w_dtype,
                          const double* X, int64_t N, int64_t K, int32_t batch_max, int32_t opt_kind, double eta, double p1, double p2,
                          int32_t penalty) {
  CHECK_CTX(ctx);
  BIND(ctx);
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->ae.reset();
  if (!layers || !w0) return ae_refuse(ctx, "layers and w0 must not be NULL");
  if (L < 2 || L > SI_AE_MAX_LAYERS) return ae_refuse(ctx, "E + D outside 2 .. 16 (an encoder and a decoder of 1 .. 8 Dense layers each)");
  if (w_dtype != SI_F32 && w_dtype != SI_F64) return ae_refuse(ctx, "w_dtype must be SI_F32 or SI_F64");
  if (batch_max < 1 || batch_max > SI_AE_MAX_BATCH) return ae_refuse(ctx, "batch_max outside 1 .. 8");
  if (opt_kind < 0 || opt_kind > 2) return ae_refuse(ctx, "opt_kind must be 0 (Descent), 1 (Momentum) or 2 (ADAM)");
  if (N < 1) return ae_refuse(ctx, "N must be positive");
  AeLayers lay;
  lay.n = L;
  int64_t off = 0;
  int32_t a_off = 0;
  for (int l = 0; l < L; ++l) {
    const si_layer& s = layers[l];
    if (s.kind != SI_LAYER_DENSE) return ae_refuse(ctx, "non-Dense layers: the encoder and the decoder must be Dense only");
    if (s.act < 0 || s.act >= SI_ACT_COUNT) return ae_refuse(ctx, "unknown activation");
    if (s.in < 1 || s.out < 1) return ae_refuse(ctx, "a layer without inputs or outputs");
    if (l == 0 && s.in != N) return ae_refuse(ctx, "the first layer's in differs from N");
    if (l == L - 1 && s.out != N) return ae_refuse(ctx, "the last layer's out differs from N");
    if (l > 0 && s.in != layers[l - 1].out) return ae_refuse(ctx, "consecutive widths do not chain");
    if (l < L - 1 && s.out > SI_AE_MAX_WIDTH) return ae_refuse(ctx, "a hidden width above 256");
    if (s.w_off != off || s.b_off != off + (int64_t)s.in * s.out)
      return ae_refuse(ctx, "the layers' offsets must be the packed flux.params order ([vec(W_l); b_l] per layer)");
    lay.in[l] = s.in, lay.out[l] = s.out, lay.act[l] = s.act, lay.w_off[l] = s.w_off, lay.b_off[l] = s.b_off;
    if (l < L - 1) {
      lay.a_off[l] = a_off;
      a_off += s.out * batch_max;
    }
    off += (int64_t)s.in * s.out + s.out;
  }
  if (off != n_params) return ae_refuse(ctx, "n_params differs from the layers' parameter count");
  std::unique_ptr<AeTrainState> t(new AeTrainState());
  AeArgs& a = t->args;
  a.lay = lay;
  if (!X) {   // the open construction's A, in place
    if (!ctx->c_active || ctx->a_pending || ctx->K < 1 || !ctx->d_A)
      return fail(ctx, SI_ERR_STATE, "si_ae_train_setup: X = NULL needs an open construction with pushed columns");
    if (ctx->max_cols > 0) return ae_refuse(ctx, "X = NULL with a construction that keeps a ring of max_cols columns");
    if (ctx->N != N) return ae_refuse(ctx, "N differs from the construction's");
    t->borrowed = true;
    t->K = ctx->K;
    t->a_dtype = ctx->a_dtype;
    a.A = ctx->d_A.get();
    a.ldA = ctx->ldA;
  } else {
    if (K < 1) return ae_refuse(ctx, "K must be positive");
    t->K = K;
    a.ldA = pad_ld(N);
    if (!t->X.alloc((size_t)a.ldA * (size_t)K)) return fail(ctx, SI_ERR_NOMEM, "si_ae_train_setup: device allocation of X failed");
    SI_HIP(ctx, hipMemcpy2DAsync(t->X, (size_t)a.ldA * sizeof(double), X, (size_t)N * sizeof(double), (size_t)N * sizeof(double), (size_t)K,
                                 hipMemcpyHostToDevice, ctx->stream));
    a.A = t->X.get();
  }
  a.N = N;
  a.nblk = (N + ae_rows() - 1) / ae_rows();
  a.G = (int32_t)std::min<int64_t>(a.nblk, ae_grid_cap());
  t->n_params = n_params, t->dtype = w_dtype, t->batch_max = batch_max;
  const size_t esz = w_dtype == SI_F32 ? 4 : 8, bytes = (size_t)n_params * esz;
  const size_t e1 = (size_t)lay.out[0], H = (size_t)lay.in[L - 1];
  if (!t->w.alloc(bytes) || !t->m.alloc(bytes) || !t->v.alloc(bytes) || !t->part1.alloc((size_t)a.G * (e1 * batch_max + 1)) ||
      !t->part2.alloc((size_t)a.G * (H * batch_max + 2)) || !t->acts.alloc((size_t)a_off) || !t->deltas.alloc((size_t)a_off) ||
      !t->loss.alloc(2))
    return fail(ctx, SI_ERR_NOMEM, "si_ae_train_setup: device allocation failed");
  SI_HIP(ctx, hipMemcpyAsync(t->w, w0, bytes, hipMemcpyHostToDevice, ctx->stream));
  SI_HIP(ctx, hipMemsetAsync(t->m, 0, bytes, ctx->stream));
  SI_HIP(ctx, hipMemsetAsync(t->v, 0, bytes, ctx->stream));
  SI_HIP(ctx, hipMemsetAsync(t->loss, 0, 2 * sizeof(double), ctx->stream));
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));   // w0 and X are the caller's
  a.w = t->w.get(), a.m = t->m.get(), a.v = t->v.get();
  a.part1 = t->part1, a.part2 = t->part2, a.acts = t->acts, a.deltas = t->deltas, a.loss = t->loss;
  a.kind = opt_kind, a.penalty = penalty ? 1 : 0;
  a.eta = eta, a.p1 = p1, a.p2 = p2;
  a.bp1 = p1, a.bp2 = p2;   // Flux's state (zero(x), zero(x), beta): the powers start at beta
  ctx->ae = std::move(t);
  return SI_OK;
}

static int32_t ae_batch(si_ctx* ctx, const char* who, AeTrainState* t, const int64_t* idx, int64_t nb) {
  if (!idx || nb < 1) return fail(ctx, SI_ERR_INVALID, std::string(who) + ": idx must hold at least one column index");
  if (nb > t->batch_max) return fail(ctx, SI_ERR_INVALID, std::string(who) + ": nb > batch_max");
  for (int64_t b = 0; b < nb; ++b)
    if (idx[b] < 0 || idx[b] >= t->K) return fail(ctx, SI_ERR_INVALID, std::string(who) + ": an index outside 0 .. K-1");
  for (int b = 0; b < SI_AE_MAX_BATCH; ++b) t->args.col[b] = b < nb ? idx[b] : 0;
  t->args.nb = (int32_t)nb;
  t->args.s = 2.0 / (double)(t->args.N * nb);
  return SI_OK;
}

// Profiling classes of a step: SI_K_DENSE the first layer's forward and the head; SI_K_DENSE_MAIN the pass over W_D with its
// fused update; SI_K_BACKWARD the head's reverse, the loss word and the updates of the small arrays and of W_1.
int32_t si_ae_train_step(si_ctx* ctx, const int64_t* idx, int64_t nb, double* loss_out) {
  CHECK_CTX(ctx);
  AeTrainState* t = ctx->ae.get();
  if (!t) return fail(ctx, SI_ERR_STATE, "si_ae_train_step: call si_ae_train_setup first");
  int32_t rc = ae_batch(ctx, "si_ae_train_step", t, idx, nb);
  if (rc != SI_OK) return rc;
  BIND(ctx);
  const AeArgs& a = t->args;
  const int L = a.lay.n;
  const double e1 = a.lay.out[0], H = a.lay.in[L - 1], N = (double)a.N, esz = t->dtype == SI_F32 ? 4 : 8,
               asz = t->a_dtype == SI_F32 ? 4 : 8, rw = a.kind == 2 ? 5 : a.kind == 1 ? 4 : 2;
  {
    ProfScope ps(ctx, SI_K_DENSE, 2.0 * N * e1 * nb, N * (e1 * esz + nb * asz));
    launch_ae_forward(ctx->stream, a, t->dtype, t->a_dtype);
  }
  {
    ProfScope ps(ctx, SI_K_DENSE_MAIN, 6.0 * N * H * nb, N * ((H + 1) * esz * rw + nb * asz));
    launch_ae_last(ctx->stream, a, t->dtype, t->a_dtype, true);
  }
  {
    ProfScope ps(ctx, SI_K_BACKWARD, 2.0 * N * e1 * nb, N * e1 * (esz * rw + nb * asz / e1));
    launch_ae_reverse(ctx->stream, a, t->dtype, t->a_dtype, ctx->num_cu);
  }
  SI_HIP(ctx, hipGetLastError());
  if (a.kind == 2) t->args.bp1 *= a.p1, t->args.bp2 *= a.p2;
  if (loss_out) {
    SI_HIP(ctx, hipMemcpyAsync(loss_out, t->loss, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return SI_OK;
}

// autoloss(re_weight) (reference :129,137): forward only, batch_max columns at a time; the chunks' sums of r^2 are added in
// ascending order and divided once by N K
int32_t si_ae_train_loss(si_ctx* ctx, double* loss_out) {
  CHECK_CTX(ctx);
  AeTrainState* t = ctx->ae.get();
  if (!t) return fail(ctx, SI_ERR_STATE, "si_ae_train_loss: call si_ae_train_setup first");
  if (!loss_out) return fail(ctx, SI_ERR_INVALID, "si_ae_train_loss: loss_out is NULL");
  BIND(ctx);
  SI_HIP(ctx, hipMemsetAsync(t->loss + 1, 0, sizeof(double), ctx->stream));
  int64_t idx[SI_AE_MAX_BATCH];
  for (int64_t k0 = 0; k0 < t->K; k0 += t->batch_max) {
    const int64_t nb = std::min<int64_t>(t->batch_max, t->K - k0);
    for (int64_t b = 0; b < nb; ++b) idx[b] = k0 + b;
    const int32_t rc = ae_batch(ctx, "si_ae_train_loss", t, idx, nb);
    if (rc != SI_OK) return rc;
    ProfScope ps(ctx, SI_K_SSE, 0.0, 0.0);
    launch_ae_forward(ctx->stream, t->args, t->dtype, t->a_dtype);
    launch_ae_last(ctx->stream, t->args, t->dtype, t->a_dtype, false);
    launch_ae_loss_chunk(ctx->stream, t->args, t->dtype, k0 + nb >= t->K, (double)(t->args.N * t->K));
  }
  SI_HIP(ctx, hipGetLastError());
  SI_HIP(ctx, hipMemcpyAsync(loss_out, t->loss, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SI_OK;
}

int32_t si_ae_train_get_params(si_ctx* ctx, void* w_out) {
  CHECK_CTX(ctx);
  AeTrainState* t = ctx->ae.get();
  if (!t) return fail(ctx, SI_ERR_STATE, "si_ae_train_get_params: call si_ae_train_setup first");
  if (!w_out) return fail(ctx, SI_ERR_INVALID, "si_ae_train_get_params: w_out is NULL");
  BIND(ctx);
  SI_HIP(ctx, hipMemcpyAsync(w_out, t->w, (size_t)t->n_params * (t->dtype == SI_F32 ? 4 : 8), hipMemcpyDeviceToHost, ctx->stream));
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SI_OK;
}

int32_t si_ae_train_get_opt_state(si_ctx* ctx, void* m_out, void* v_out, double* beta_pows_out) {
  CHECK_CTX(ctx);
  AeTrainState* t = ctx->ae.get();
  if (!t) return fail(ctx, SI_ERR_STATE, "si_ae_train_get_opt_state: call si_ae_train_setup first");
  BIND(ctx);
  const size_t bytes = (size_t)t->n_params * (t->dtype == SI_F32 ? 4 : 8);
  if (m_out) SI_HIP(ctx, hipMemcpyAsync(m_out, t->m, bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (v_out) SI_HIP(ctx, hipMemcpyAsync(v_out, t->v, bytes, hipMemcpyDeviceToHost, ctx->stream));
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (beta_pows_out) beta_pows_out[0] = t->args.bp1, beta_pows_out[1] = t->args.bp2;
  return SI_OK;
}

int32_t si_ae_train_info(si_ctx* ctx, int32_t* active_out, int64_t* N_out, int64_t* K_out, int64_t* n_params_out, int32_t* fused_out) {
  CHECK_CTX(ctx);
  const AeTrainState* t = ctx->ae.get();
  if (active_out) *active_out = t ? 1 : 0;
  if (N_out) *N_out = t ? t->args.N : 0;
  if (K_out) *K_out = t ? t->K : 0;
  if (n_params_out) *n_params_out = t ? t->n_params : 0;
  if (fused_out) *fused_out = t ? 1 : 0;   // the last layer's update runs inside the pass over W_D
  return SI_OK;
}

int32_t si_ae_train_free(si_ctx* ctx) {
  CHECK_CTX(ctx);
  BIND(ctx);
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->ae.reset();
  return SI_OK;
}

}  // extern "C"
