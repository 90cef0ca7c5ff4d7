// The autoencoder route's kernels (si_infer_set_decoder; reference src/space_inference.jl:247,278: W_swa + decoder(z)).
// gfx950, fp64 sums, no atomics.  Every sum has a fixed order that depends on the decoder's shapes only -- never on the number
// of points, on a point's column or on the run.  Compiled without contraction of a*b+c: the definition
// (subspaceinference.jl_amd/autoencoder.py) rounds every product and every sum, and with W_D = P the last layer reproduces
// K4 (kernels_stream.hip, compiled the same way) bit for bit.  T is the parameters' element type; widening is exact.
//   head forward   layers 1 .. D-1, one workgroup per point, activations in LDS, every layer's output kept for the reverse
//   last forward   K4's access pattern: a thread owns two consecutive rows, 16-byte (fp32: 8-byte) loads down each column of
//                  W_D, the layer input wave-uniform; y = act(acc + b), w = swa + y
//   last reverse   launch_ptg's scheme: fixed row blocks, thread-strided sums, shuffle-down tree, wave sums in order, then a
//                  final kernel over the block partials
//   head reverse   one workgroup per point: ga -> gz through the transposed head layers, act' from the kept outputs
#include "kernels_gemm.h"

namespace si {

constexpr int DEC_MAXW = 1024;   // M and every hidden width (si_infer_set_decoder refuses wider ones)

template <typename T>
__global__ __launch_bounds__(256) void decoder_head_fwd_kernel(DecoderHead hd, const T* __restrict__ params,
                                                               const double* __restrict__ Z, int M, double* __restrict__ hid,
                                                               int SH) {
  __shared__ double buf[2][DEC_MAXW];
  const int64_t p = blockIdx.x;
  for (int i = threadIdx.x; i < M; i += 256) buf[0][i] = Z[p * M + i];
  __syncthreads();
  int cur = 0;
  for (int l = 0; l < hd.n; ++l) {
    const int in = hd.in[l], out = hd.out[l], act = hd.act[l];
    const T* W = params + hd.w_off[l];
    const T* b = params + hd.b_off[l];
    for (int j = threadIdx.x; j < out; j += 256) {
      double u = 0.0;
      for (int i = 0; i < in; ++i) u += (double)W[j + (int64_t)out * i] * buf[cur][i];
      u += (double)b[j];
      const double a = act_full(u, act);
      buf[cur ^ 1][j] = a;
      hid[p * SH + hd.hid_off[l] + j] = a;
    }
    __syncthreads();
    cur ^= 1;
  }
}

template <typename T>
struct Pair;
template <>
struct Pair<double> {
  static __device__ __forceinline__ double2 load(const double* p) { return *reinterpret_cast<const double2*>(p); }
};
template <>
struct Pair<float> {
  static __device__ __forceinline__ double2 load(const float* p) {
    const float2 v = *reinterpret_cast<const float2*>(p);
    return make_double2((double)v.x, (double)v.y);
  }
};

// Algorithmic bytes per row: sizeof(T) * (H + 1) + 8 read, 8 * CB (w) [+ 8 * CB (y)] written; W_D is read ONCE for up to CB points.
template <typename T, int CB>
__global__ __launch_bounds__(256) void decoder_last_fwd_kernel(const double* __restrict__ swa, const T* __restrict__ Wd, int64_t ldD,
                                                               const T* __restrict__ bd, int64_t N, int32_t H, int32_t act,
                                                               const double* __restrict__ A, int64_t lda, double* __restrict__ w,
                                                               int64_t ldw, double* __restrict__ y, int64_t ldy) {
  const int64_t npair = (N + 1) >> 1;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (blockIdx.y != 0) {   // point groups of CB stacked in grid.y: one launch for all of them
    const int64_t cg = (int64_t)blockIdx.y * CB;
    A += cg * lda;
    if (w != nullptr) w += cg * ldw;
    if (y != nullptr) y += cg * ldy;
  }
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npair; p += stride) {
    const int64_t r = p << 1;
    double2 acc[CB];
#pragma unroll
    for (int c = 0; c < CB; ++c) acc[c] = make_double2(0.0, 0.0);
    for (int h = 0; h < H; ++h) {
      const double2 wv = Pair<T>::load(Wd + r + (int64_t)h * ldD);
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        const double a = A[h + c * lda];
        acc[c].x += wv.x * a;
        acc[c].y += wv.y * a;
      }
    }
    const double2 bv = Pair<T>::load(bd + r);
    double2 sv = make_double2(0.0, 0.0);
    if (w != nullptr) sv = *reinterpret_cast<const double2*>(swa + r);
    const bool both = r + 1 < N;
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      const double y0 = act_full(acc[c].x + bv.x, act), y1 = act_full(acc[c].y + bv.y, act);
      if (w != nullptr) {
        double* dst = w + (int64_t)c * ldw + r;
        if (both && (ldw & 1) == 0) {
          *reinterpret_cast<double2*>(dst) = make_double2(sv.x + y0, sv.y + y1);
        } else {
          dst[0] = sv.x + y0;
          if (both) dst[1] = sv.y + y1;
        }
      }
      if (y != nullptr) {
        double* dst = y + (int64_t)c * ldy + r;
        if (both && (ldy & 1) == 0) {
          *reinterpret_cast<double2*>(dst) = make_double2(y0, y1);
        } else {
          dst[0] = y0;
          if (both) dst[1] = y1;
        }
      }
    }
  }
}

// ga[h] = sum_r W_D[r + ldD * h] * (g[r] * act'(y[r]))   (HBM-bound: W_D is read once)
constexpr int DEC_REV_BLOCKS = 1024;
constexpr int DEC_REV_HT = 4;
template <typename T>
__global__ __launch_bounds__(256) void decoder_last_rev_partial_kernel(const T* __restrict__ Wd, int64_t ldD, int64_t N, int H, int act,
                                                                       const double* __restrict__ g, const double* __restrict__ y,
                                                                       double* __restrict__ part) {
  __shared__ double red[4][DEC_REV_HT];
  const int64_t per = ((N + DEC_REV_BLOCKS - 1) / DEC_REV_BLOCKS + 1) / 2 * 2;
  const int64_t r0 = (int64_t)blockIdx.x * per;
  int64_t r1 = r0 + per;
  if (r1 > N) r1 = N;
  for (int h0 = 0; h0 < H; h0 += DEC_REV_HT) {
    double s[DEC_REV_HT];
#pragma unroll
    for (int j = 0; j < DEC_REV_HT; ++j) s[j] = 0.0;
    for (int64_t r = r0 + threadIdx.x; r < r1; r += 256) {
      const double gv = g[r] * dact_full(y[r], act);
#pragma unroll
      for (int j = 0; j < DEC_REV_HT; ++j)
        if (h0 + j < H) s[j] += (double)Wd[r + ldD * (h0 + j)] * gv;
    }
#pragma unroll
    for (int j = 0; j < DEC_REV_HT; ++j) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) s[j] += __shfl_down(s[j], off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int j = 0; j < DEC_REV_HT; ++j) red[threadIdx.x >> 6][j] = s[j];
    }
    __syncthreads();
    if (threadIdx.x < DEC_REV_HT && h0 + threadIdx.x < H)
      part[(int64_t)blockIdx.x * H + h0 + threadIdx.x] =
          (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    __syncthreads();
  }
}
// one workgroup per h: 256 threads stride over the block partials, fixed tree
__global__ __launch_bounds__(256) void decoder_last_rev_final_kernel(const double* __restrict__ part, int H, double* __restrict__ ga) {
  __shared__ double red[4];
  const int h = blockIdx.x;
  double s = 0.0;
  for (int b = threadIdx.x; b < DEC_REV_BLOCKS; b += 256) s += part[(int64_t)b * H + h];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) ga[h] = (red[0] + red[1]) + (red[2] + red[3]);
}

// per layer l = D-1 .. 1: delta = g .* act'(a_l) (a_l from hid), g <- W_l' delta with the sum over the output index ascending
// from 0.0; gz = the g that leaves layer 1
template <typename T>
__global__ __launch_bounds__(256) void decoder_head_rev_kernel(DecoderHead hd, const T* __restrict__ params,
                                                               const double* __restrict__ ga, int H, const double* __restrict__ hid,
                                                               int SH, double* __restrict__ gz, int M) {
  __shared__ double gbuf[DEC_MAXW], delta[DEC_MAXW];
  const int64_t p = blockIdx.x;
  for (int i = threadIdx.x; i < H; i += 256) gbuf[i] = ga[p * H + i];
  __syncthreads();
  for (int l = hd.n - 1; l >= 0; --l) {
    const int in = hd.in[l], out = hd.out[l], act = hd.act[l];
    const T* W = params + hd.w_off[l];
    for (int j = threadIdx.x; j < out; j += 256) delta[j] = gbuf[j] * dact_full(hid[p * SH + hd.hid_off[l] + j], act);
    __syncthreads();
    for (int i = threadIdx.x; i < in; i += 256) {
      double s = 0.0;
      for (int j = 0; j < out; ++j) s += (double)W[j + (int64_t)out * i] * delta[j];
      gbuf[i] = s;
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < M; i += 256) gz[p * M + i] = gbuf[i];
}

static int decoder_stream_grid(int64_t work_items, int num_cu) {   // (kernels_stream.hip's stream_grid)
  int64_t blocks = (work_items + 255) / 256;
  const int64_t cap = (int64_t)num_cu * 8;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

void launch_decoder_head_fwd(hipStream_t st, const DecoderHead& hd, const void* params, int32_t dtype, const double* Z, int32_t M,
                             double* hid, int32_t SH, int32_t npoints) {
  if (hd.n == 0 || npoints <= 0) return;   // D = 1: a = z, nothing to run
  if (dtype == SI_F32)
    hipLaunchKernelGGL((decoder_head_fwd_kernel<float>), dim3(npoints), dim3(256), 0, st, hd, static_cast<const float*>(params), Z, M, hid, SH);
  else
    hipLaunchKernelGGL((decoder_head_fwd_kernel<double>), dim3(npoints), dim3(256), 0, st, hd, static_cast<const double*>(params), Z, M, hid, SH);
}

template <typename T>
static void launch_decoder_last_fwd_t(hipStream_t st, const double* swa, const T* Wd, int64_t ldD, const T* bd, int64_t N, int32_t H,
                                      int32_t act, const double* A, int64_t lda, int32_t C, double* w, int64_t ldw, double* y,
                                      int64_t ldy, int num_cu) {
  const int grid = decoder_stream_grid((N + 1) >> 1, num_cu);
  int c0 = 0;
  if (C >= 8) {   // many stacked points: every group of four in one launch, as K4 stacks its chains
    const int n4 = C / 4;
    hipLaunchKernelGGL((decoder_last_fwd_kernel<T, 4>), dim3(grid, n4), dim3(256), 0, st, swa, Wd, ldD, bd, N, H, act, A, lda, w, ldw, y, ldy);
    c0 = 4 * n4;
  }
  while (c0 < C) {
    const int rem = C - c0;
    const double* Ac = A + (int64_t)c0 * lda;
    double* wc = w ? w + (int64_t)c0 * ldw : nullptr;
    double* yc = y ? y + (int64_t)c0 * ldy : nullptr;
    if (rem >= 4) {
      hipLaunchKernelGGL((decoder_last_fwd_kernel<T, 4>), dim3(grid), dim3(256), 0, st, swa, Wd, ldD, bd, N, H, act, Ac, lda, wc, ldw, yc, ldy);
      c0 += 4;
    } else if (rem >= 2) {
      hipLaunchKernelGGL((decoder_last_fwd_kernel<T, 2>), dim3(grid), dim3(256), 0, st, swa, Wd, ldD, bd, N, H, act, Ac, lda, wc, ldw, yc, ldy);
      c0 += 2;
    } else {
      hipLaunchKernelGGL((decoder_last_fwd_kernel<T, 1>), dim3(grid), dim3(256), 0, st, swa, Wd, ldD, bd, N, H, act, Ac, lda, wc, ldw, yc, ldy);
      c0 += 1;
    }
  }
}

void launch_decoder_last_fwd(hipStream_t st, const double* swa, const void* Wd, int64_t ldD, const void* bd, int32_t dtype, int64_t N,
                             int32_t H, int32_t act, const double* A, int64_t lda, int32_t C, double* w, int64_t ldw, double* y,
                             int64_t ldy, int num_cu) {
  if (dtype == SI_F32)
    launch_decoder_last_fwd_t<float>(st, swa, static_cast<const float*>(Wd), ldD, static_cast<const float*>(bd), N, H, act, A, lda, C, w,
                                     ldw, y, ldy, num_cu);
  else
    launch_decoder_last_fwd_t<double>(st, swa, static_cast<const double*>(Wd), ldD, static_cast<const double*>(bd), N, H, act, A, lda, C,
                                      w, ldw, y, ldy, num_cu);
}

int decoder_rev_blocks() { return DEC_REV_BLOCKS; }

void launch_decoder_last_rev(hipStream_t st, const void* Wd, int64_t ldD, int32_t dtype, int64_t N, int32_t H, int32_t act,
                             const double* g, const double* y, double* part, double* ga) {
  if (dtype == SI_F32)
    hipLaunchKernelGGL((decoder_last_rev_partial_kernel<float>), dim3(DEC_REV_BLOCKS), dim3(256), 0, st, static_cast<const float*>(Wd), ldD,
                       N, H, act, g, y, part);
  else
    hipLaunchKernelGGL((decoder_last_rev_partial_kernel<double>), dim3(DEC_REV_BLOCKS), dim3(256), 0, st, static_cast<const double*>(Wd),
                       ldD, N, H, act, g, y, part);
  hipLaunchKernelGGL(decoder_last_rev_final_kernel, dim3(H), dim3(256), 0, st, part, H, ga);
}

void launch_decoder_head_rev(hipStream_t st, const DecoderHead& hd, const void* params, int32_t dtype, const double* ga, int32_t H,
                             const double* hid, int32_t SH, double* gz, int32_t M, int32_t npoints) {
  if (npoints <= 0) return;
  if (dtype == SI_F32)
    hipLaunchKernelGGL((decoder_head_rev_kernel<float>), dim3(npoints), dim3(256), 0, st, hd, static_cast<const float*>(params), ga, H, hid,
                       SH, gz, M);
  else
    hipLaunchKernelGGL((decoder_head_rev_kernel<double>), dim3(npoints), dim3(256), 0, st, hd, static_cast<const double*>(params), ga, H,
                       hid, SH, gz, M);
}

}  // namespace si
