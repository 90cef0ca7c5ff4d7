// Training Chain(encoder, decoder) on the deviation columns (si_ae_train_*; reference src/subspace_construction.jl:125-140).
// gfx950, fp64 sums, no atomics, plain launches; every loop bound is a kernel argument.  Compiled without contraction of
// a*b+c: subspaceinference.jl_amd/autoencoder.py (train_value_and_grad, train_step) rounds every product and every sum.
// T is the parameters' element type, TA the storage type of A; widening is exact.
//
// The autoencoder is N -> e_1 -> ... -> H -> N.  W_1 (e_1 x N, Flux's out x in) has the e_1 values of input row n contiguous;
// W_D (N x H) has row n at stride N.  Both are N-parallel and memory-bound, so both big layers run as ROW kernels: a thread owns
// row n of a row block of AE_ROWS rows, a workgroup takes the row blocks rb = blockIdx.x, + G, ... (G = min(row blocks, AE_GRID)).
//
// The three N-long sums (first layer's forward, the pull-back W_D' dt, sum r^2; with the penalty the rows' shares of sum w^2) have
// ONE order, a function of N alone (autoencoder._nsum(.., "blocked") restates it): per row block a shuffle-down tree over each
// wave's 64 rows, then (w0 + w1) + (w2 + w3); a workgroup adds its row blocks in ascending order from 0.0 (in LDS, one owner
// thread per sum); the G workgroup sums are added in ascending order from 0.0 by the thread that needs them.
//
//   ae_first_fwd_kernel     streams W_1 once against the nb columns of A read IN PLACE: G x (e_1 nb + 1) workgroup sums
//   ae_head_fwd_kernel      one workgroup per column: a_1 = act(sum + b_1), then the middle layers; keeps every a_l
//   ae_last_kernel<UPD>     one pass over W_D: y = act(W_D[n,:] h + b[n]), r, the row's r^2, dt; with UPD the row's share of
//                           W_D' dt (G x (H nb + 2) workgroup sums) and then -- the row is this thread's alone, so W_D[n,:] is
//                           still the pre-update value -- g = s sum_b dt[n,b] h[:,b] (+ 2w) and optimiser_update on W_D[n,:],
//                           b_D[n] in place: dW_D is never written
//   ae_head_rev_kernel      one workgroup per column: dt_l of the middle layers and of layer 1 through the transposed layers
//   ae_loss_kernel          the loss word
//   ae_mid_update_kernel    b_1 and the middle arrays: g = s sum_b dt_l[j,b] a_{l-1}[i,b] (+ 2w), optimiser_update
//   ae_first_update_kernel  a linear stream over W_1, m, v: g = s sum_b dt_1[j,b] X[n,b] (+ 2w), optimiser_update
#include "kernels_gemm.h"
#include "optimiser_update.h"

namespace si {

constexpr int AE_ROWS = 256;     // rows of a row block = threads of a workgroup
constexpr int AE_GRID = 1024;    // most workgroups of a row kernel
constexpr int AE_BP = SI_AE_MAX_BATCH;                                  // column pitch of the LDS copies of h and dt_1
constexpr int AE_MAX_SLOTS = SI_AE_MAX_WIDTH * SI_AE_MAX_BATCH + 2;     // sums a row kernel carries

int ae_rows() { return AE_ROWS; }
int ae_grid_cap() { return AE_GRID; }

__device__ __forceinline__ double ae_wave_tree(double s) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  return s;
}

// sum k of this row block: the waves' trees into red; after every 256 sums (and after the last, k == nslots - 1) their owner
// threads add (w0 + w1) + (w2 + w3) to the workgroup's running sums.  Called by all threads with the same k.
__device__ __forceinline__ void ae_put(double c, int k, int nslots, double* red, double* acc) {
  const double s = ae_wave_tree(c);
  if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * AE_ROWS + (k & (AE_ROWS - 1))] = s;
  if ((k & (AE_ROWS - 1)) == AE_ROWS - 1 || k == nslots - 1) {
    __syncthreads();
    const int base = k & ~(AE_ROWS - 1);
    const int t = threadIdx.x;
    if (base + t <= k) acc[base + t] += (red[t] + red[AE_ROWS + t]) + (red[2 * AE_ROWS + t] + red[3 * AE_ROWS + t]);
    __syncthreads();
  }
}

template <typename T, typename TA>
__global__ __launch_bounds__(AE_ROWS) void ae_first_fwd_kernel(AeArgs a) {
  __shared__ double red[4 * AE_ROWS], acc[AE_MAX_SLOTS];
  const int e1 = a.lay.out[0], nb = a.nb, nslots = e1 * nb + 1;
  const T* W = static_cast<const T*>(a.w) + a.lay.w_off[0];
  const TA* A = static_cast<const TA*>(a.A);
  for (int k = threadIdx.x; k < nslots; k += AE_ROWS) acc[k] = 0.0;
  __syncthreads();
  for (int64_t rb = blockIdx.x; rb < a.nblk; rb += a.G) {
    const int64_t n = rb * AE_ROWS + threadIdx.x;
    const bool live = n < a.N;
    double x[SI_AE_MAX_BATCH];
#pragma unroll
    for (int b = 0; b < SI_AE_MAX_BATCH; ++b) x[b] = (live && b < nb) ? (double)A[n + a.col[b] * a.ldA] : 0.0;
    const T* Wn = W + (int64_t)e1 * (live ? n : 0);
    int k = 0;
    double q = 0.0;
    for (int j = 0; j < e1; ++j) {
      const double wv = live ? (double)Wn[j] : 0.0;
      q += wv * wv;
#pragma unroll
      for (int b = 0; b < SI_AE_MAX_BATCH; ++b)
        if (b < nb) ae_put(wv * x[b], k++, nslots, red, acc);
    }
    ae_put(q, k, nslots, red, acc);   // the row's share of sum w^2 (read with the penalty only)
  }
  for (int k = threadIdx.x; k < nslots; k += AE_ROWS) a.part1[(int64_t)blockIdx.x * nslots + k] = acc[k];
}

template <typename T>
__global__ __launch_bounds__(256) void ae_head_fwd_kernel(AeArgs a) {
  __shared__ double buf[2][SI_AE_MAX_WIDTH];
  const int b = blockIdx.x, nb = a.nb, e1 = a.lay.out[0], nslots = e1 * nb + 1;
  const T* w = static_cast<const T*>(a.w);
  for (int j = threadIdx.x; j < e1; j += 256) {
    double u = 0.0;
    for (int g = 0; g < a.G; ++g) u += a.part1[(int64_t)g * nslots + j * nb + b];
    u += (double)w[a.lay.b_off[0] + j];
    const double av = act_full(u, a.lay.act[0]);
    buf[0][j] = av;
    a.acts[a.lay.a_off[0] + b * e1 + j] = av;
  }
  __syncthreads();
  int cur = 0;
  for (int l = 1; l < a.lay.n - 1; ++l) {
    const int in = a.lay.in[l], out = a.lay.out[l], act = a.lay.act[l];
    const T* W = w + a.lay.w_off[l];
    const T* bias = w + a.lay.b_off[l];
    for (int j = threadIdx.x; j < out; j += 256) {
      double u = 0.0;
      for (int i = 0; i < in; ++i) u += (double)W[j + (int64_t)out * i] * buf[cur][i];
      u += (double)bias[j];
      const double av = act_full(u, act);
      buf[cur ^ 1][j] = av;
      a.acts[a.lay.a_off[l] + b * out + j] = av;
    }
    __syncthreads();
    cur ^= 1;
  }
}

// Algorithmic bytes per row with UPD: sizeof(T) * (H + 1) * 5 (w, m, v read; w, m, v written -- Descent 2, Momentum 4 of the 5) +
// sizeof(TA) * nb; the second read of W_D[n,:] comes from the cache.  Without UPD: sizeof(T) * (H + 1) + sizeof(TA) * nb.
template <typename T, typename TA, bool UPD>
__global__ __launch_bounds__(AE_ROWS) void ae_last_kernel(AeArgs a) {
  __shared__ double red[4 * AE_ROWS], acc[AE_MAX_SLOTS], hs[SI_AE_MAX_WIDTH * AE_BP];
  const int L = a.lay.n, H = a.lay.in[L - 1], act = a.lay.act[L - 1], nb = a.nb;
  const int nslots = UPD ? H * nb + 2 : 2;
  T* w = static_cast<T*>(a.w);
  T* m = static_cast<T*>(a.m);
  T* v = static_cast<T*>(a.v);
  const int64_t wo = a.lay.w_off[L - 1], bo = a.lay.b_off[L - 1], N = a.N;
  const TA* A = static_cast<const TA*>(a.A);
  for (int k = threadIdx.x; k < nslots; k += AE_ROWS) acc[k] = 0.0;
  for (int i = threadIdx.x; i < H * AE_BP; i += AE_ROWS) {
    const int h = i / AE_BP, b = i - h * AE_BP;
    hs[i] = b < nb ? a.acts[a.lay.a_off[L - 2] + b * H + h] : 0.0;
  }
  __syncthreads();
  for (int64_t rb = blockIdx.x; rb < a.nblk; rb += a.G) {
    const int64_t n = rb * AE_ROWS + threadIdx.x;
    const bool live = n < N;
    const int64_t nn = live ? n : 0;
    double x[SI_AE_MAX_BATCH], y[SI_AE_MAX_BATCH];
#pragma unroll
    for (int b = 0; b < SI_AE_MAX_BATCH; ++b) {
      x[b] = (live && b < nb) ? (double)A[n + a.col[b] * a.ldA] : 0.0;
      y[b] = 0.0;
    }
    double pen = 0.0;
    for (int h = 0; h < H; ++h) {
      const double wv = live ? (double)w[wo + nn + N * h] : 0.0;
      pen += wv * wv;
#pragma unroll
      for (int b = 0; b < SI_AE_MAX_BATCH; ++b) y[b] += wv * hs[h * AE_BP + b];
    }
    const double bias = live ? (double)w[bo + nn] : 0.0;
    pen += bias * bias;
    double sq = 0.0, gb = 0.0;
#pragma unroll
    for (int b = 0; b < SI_AE_MAX_BATCH; ++b) {   // y[b] becomes dt[n, b]
      const double yv = act_full(y[b] + bias, act);
      const double r = (live && b < nb) ? yv - x[b] : 0.0;
      sq += r * r;
      y[b] = r * dact_full(yv, act);
      gb += y[b];
    }
    if (UPD) {
      int k = 0;
      for (int h = 0; h < H; ++h) {
        const int64_t i = wo + nn + N * h;
        const double wv = live ? (double)w[i] : 0.0;   // still the value the forward read: the update below comes after
#pragma unroll
        for (int b = 0; b < SI_AE_MAX_BATCH; ++b)
          if (b < nb) ae_put(wv * y[b], k++, nslots, red, acc);
        if (live) {
          double Gs = 0.0;
#pragma unroll
          for (int b = 0; b < SI_AE_MAX_BATCH; ++b) Gs += y[b] * hs[h * AE_BP + b];   // (columns >= nb add 0.0 * 0.0)
          double g = a.s * Gs;
          if (a.penalty) g += 2.0 * wv;
          optimiser_update(w, m, v, i, g, a.kind, a.eta, a.p1, a.p2, a.bp1, a.bp2, false);
        }
      }
      if (live) {
        double g = a.s * gb;
        if (a.penalty) g += 2.0 * bias;
        optimiser_update(w, m, v, bo + n, g, a.kind, a.eta, a.p1, a.p2, a.bp1, a.bp2, false);
      }
      ae_put(sq, k++, nslots, red, acc);
      ae_put(pen, k, nslots, red, acc);
    } else {
      ae_put(sq, 0, nslots, red, acc);
      ae_put(pen, 1, nslots, red, acc);
    }
  }
  for (int k = threadIdx.x; k < nslots; k += AE_ROWS) a.part2[(int64_t)blockIdx.x * nslots + k] = acc[k];
}

template <typename T>
__global__ __launch_bounds__(256) void ae_head_rev_kernel(AeArgs a) {
  __shared__ double g[SI_AE_MAX_WIDTH], dl[SI_AE_MAX_WIDTH];
  const int b = blockIdx.x, nb = a.nb, L = a.lay.n, H = a.lay.in[L - 1], nslots = H * nb + 2;
  const T* w = static_cast<const T*>(a.w);
  for (int i = threadIdx.x; i < H; i += 256) {
    double s = 0.0;
    for (int gi = 0; gi < a.G; ++gi) s += a.part2[(int64_t)gi * nslots + i * nb + b];
    g[i] = s;
  }
  __syncthreads();
  for (int l = L - 2; l >= 0; --l) {
    const int in = a.lay.in[l], out = a.lay.out[l], act = a.lay.act[l];
    for (int j = threadIdx.x; j < out; j += 256) {
      const double d = g[j] * dact_full(a.acts[a.lay.a_off[l] + b * out + j], act);
      dl[j] = d;
      a.deltas[a.lay.a_off[l] + b * out + j] = d;
    }
    __syncthreads();
    if (l > 0) {
      const T* W = w + a.lay.w_off[l];
      for (int i = threadIdx.x; i < in; i += 256) {
        double s = 0.0;
        for (int j = 0; j < out; ++j) s += (double)W[j + (int64_t)out * i] * dl[j];
        g[i] = s;
      }
    }
    __syncthreads();
  }
}

// mode 0: a step's loss = sum r^2 / denom (+ penalty).  mode 1 / 2: a chunk of si_ae_train_loss -- loss[1] += the chunk's
// sum r^2; mode 2 (the last chunk) then loss[0] = loss[1] / denom (+ penalty).  One workgroup.
template <typename T>
__global__ __launch_bounds__(256) void ae_loss_kernel(AeArgs a, int mode, double denom) {
  __shared__ double red[4];
  const int L = a.lay.n, nb = a.nb, e1 = a.lay.out[0], H = a.lay.in[L - 1];
  const int ns1 = e1 * nb + 1, ns2 = mode == 0 ? H * nb + 2 : 2;
  const T* w = static_cast<const T*>(a.w);
  double pm = 0.0;
  if (a.penalty && mode != 1) {   // b_1 and the middle arrays: one contiguous range of the flat vector
    for (int64_t i = a.lay.b_off[0] + threadIdx.x; i < a.lay.w_off[L - 1]; i += 256) pm += (double)w[i] * (double)w[i];
    pm = ae_wave_tree(pm);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = pm;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double ssq = 0.0;
  for (int g = 0; g < a.G; ++g) ssq += a.part2[(int64_t)g * ns2 + ns2 - 2];
  if (mode != 0) {
    ssq = a.loss[1] + ssq;
    a.loss[1] = ssq;
    if (mode == 1) return;
  }
  double loss = ssq / denom;
  if (a.penalty) {
    double pf = 0.0, pl = 0.0;
    for (int g = 0; g < a.G; ++g) pf += a.part1[(int64_t)g * ns1 + ns1 - 1];
    for (int g = 0; g < a.G; ++g) pl += a.part2[(int64_t)g * ns2 + ns2 - 1];
    loss += (pf + ((red[0] + red[1]) + (red[2] + red[3]))) + pl;
  }
  a.loss[0] = loss;
}

template <typename T>
__global__ __launch_bounds__(256) void ae_mid_update_kernel(AeArgs a) {
  const int L = a.lay.n, nb = a.nb;
  T* w = static_cast<T*>(a.w);
  T* m = static_cast<T*>(a.m);
  T* v = static_cast<T*>(a.v);
  const int64_t hi = a.lay.w_off[L - 1];
  for (int64_t i = a.lay.b_off[0] + (int64_t)blockIdx.x * 256 + threadIdx.x; i < hi; i += (int64_t)gridDim.x * 256) {
    double Gs = 0.0;
    for (int l = 0; l < L - 1; ++l) {
      const int in = a.lay.in[l], out = a.lay.out[l];
      const int64_t bo = a.lay.b_off[l];
      if (i >= bo && i < bo + out) {
        const int j = (int)(i - bo);
        for (int b = 0; b < nb; ++b) Gs += a.deltas[a.lay.a_off[l] + b * out + j];
        break;
      }
      const int64_t wo = a.lay.w_off[l];
      if (l > 0 && i >= wo && i < bo) {
        const int64_t e = i - wo;
        const int ii = (int)(e / out), j = (int)(e - (int64_t)ii * out);
        for (int b = 0; b < nb; ++b) Gs += a.deltas[a.lay.a_off[l] + b * out + j] * a.acts[a.lay.a_off[l - 1] + b * in + ii];
        break;
      }
    }
    double g = a.s * Gs;
    if (a.penalty) g += 2.0 * (double)w[i];
    optimiser_update(w, m, v, i, g, a.kind, a.eta, a.p1, a.p2, a.bp1, a.bp2, false);
  }
}

// Algorithmic bytes per element: 5 * sizeof(T) (ADAM) + sizeof(TA) * nb / e_1 -- fully coalesced over W_1, m, v
template <typename T, typename TA>
__global__ __launch_bounds__(256) void ae_first_update_kernel(AeArgs a) {
  __shared__ double d1[SI_AE_MAX_WIDTH * AE_BP];
  const int e1 = a.lay.out[0], nb = a.nb;
  T* w = static_cast<T*>(a.w);
  T* m = static_cast<T*>(a.m);
  T* v = static_cast<T*>(a.v);
  const TA* A = static_cast<const TA*>(a.A);
  for (int i = threadIdx.x; i < e1 * AE_BP; i += 256) {
    const int j = i / AE_BP, b = i - j * AE_BP;
    d1[i] = b < nb ? a.deltas[a.lay.a_off[0] + b * e1 + j] : 0.0;
  }
  __syncthreads();
  const int64_t total = (int64_t)e1 * a.N, wo = a.lay.w_off[0];
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t n = e / e1;
    const int j = (int)(e - n * e1);
    double Gs = 0.0;
#pragma unroll
    for (int b = 0; b < SI_AE_MAX_BATCH; ++b)
      if (b < nb) Gs += d1[j * AE_BP + b] * (double)A[n + a.col[b] * a.ldA];
    double g = a.s * Gs;
    if (a.penalty) g += 2.0 * (double)w[wo + e];
    optimiser_update(w, m, v, wo + e, g, a.kind, a.eta, a.p1, a.p2, a.bp1, a.bp2, false);
  }
}

static int ae_linear_grid(int64_t items, int num_cu) {
  int64_t blocks = (items + 255) / 256;
  const int64_t cap = (int64_t)num_cu * 8;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

template <typename T, typename TA>
static void ae_forward_t(hipStream_t st, const AeArgs& a) {
  hipLaunchKernelGGL((ae_first_fwd_kernel<T, TA>), dim3(a.G), dim3(AE_ROWS), 0, st, a);
  hipLaunchKernelGGL((ae_head_fwd_kernel<T>), dim3(a.nb), dim3(256), 0, st, a);
}
template <typename T, typename TA>
static void ae_last_t(hipStream_t st, const AeArgs& a, bool update) {
  if (update)
    hipLaunchKernelGGL((ae_last_kernel<T, TA, true>), dim3(a.G), dim3(AE_ROWS), 0, st, a);
  else
    hipLaunchKernelGGL((ae_last_kernel<T, TA, false>), dim3(a.G), dim3(AE_ROWS), 0, st, a);
}
template <typename T, typename TA>
static void ae_reverse_t(hipStream_t st, const AeArgs& a, int num_cu) {
  hipLaunchKernelGGL((ae_head_rev_kernel<T>), dim3(a.nb), dim3(256), 0, st, a);
  hipLaunchKernelGGL((ae_loss_kernel<T>), dim3(1), dim3(256), 0, st, a, 0, (double)(a.N * a.nb));
  const int L = a.lay.n;
  hipLaunchKernelGGL((ae_mid_update_kernel<T>), dim3(ae_linear_grid(a.lay.w_off[L - 1] - a.lay.b_off[0], num_cu)), dim3(256), 0, st, a);
  hipLaunchKernelGGL((ae_first_update_kernel<T, TA>), dim3(ae_linear_grid((int64_t)a.lay.out[0] * a.N, num_cu)), dim3(256), 0, st, a);
}

#define AE_DISPATCH(fn, ...)                                      \
  do {                                                            \
    if (dtype == SI_F32) {                                        \
      if (a_dtype == SI_F32) fn<float, float>(__VA_ARGS__);       \
      else fn<float, double>(__VA_ARGS__);                        \
    } else {                                                      \
      if (a_dtype == SI_F32) fn<double, float>(__VA_ARGS__);      \
      else fn<double, double>(__VA_ARGS__);                       \
    }                                                             \
  } while (0)

void launch_ae_forward(hipStream_t st, const AeArgs& a, int32_t dtype, int32_t a_dtype) { AE_DISPATCH(ae_forward_t, st, a); }
void launch_ae_last(hipStream_t st, const AeArgs& a, int32_t dtype, int32_t a_dtype, bool update) { AE_DISPATCH(ae_last_t, st, a, update); }
void launch_ae_reverse(hipStream_t st, const AeArgs& a, int32_t dtype, int32_t a_dtype, int num_cu) { AE_DISPATCH(ae_reverse_t, st, a, num_cu); }
void launch_ae_loss_chunk(hipStream_t st, const AeArgs& a, int32_t dtype, bool last, double denom) {
  if (dtype == SI_F32)
    hipLaunchKernelGGL((ae_loss_kernel<float>), dim3(1), dim3(256), 0, st, a, last ? 2 : 1, denom);
  else
    hipLaunchKernelGGL((ae_loss_kernel<double>), dim3(1), dim3(256), 0, st, a, last ? 2 : 1, denom);
}

}  // namespace si
