// Kernels of si_construct_finish_diffmap: the diffusion map of the reference's `diffusion_subspace`
// (src/subspace_construction.jl:202-206, `fit(DiffMap, A', maxoutdim = M)` of ManifoldLearning 0.6.2).  The definition is
// restated in diffmap.py  [upstream, from memory, unverifiable offline];  every unverified point is a kernel argument (eps, alpha,
// kernel_sign, rescale).  With X = A' (K x N, column i = the K deviations of weight i):
//   1. dm_minmax / dm_rescale   Xr[k, i] = (X[k, i] - mn_k) * (1 / (mx_k - mn_k)), NaN -> 0 (three rounded operations: this file is
//                               compiled with -ffp-contract=off, Xr is bit-equal to the NumPy restatement); s_i = sum_k Xr[k, i]^2
//   2. dm_pairwise              S = Xr' Xr on v_mfma_f64_16x16x4_f64, and in the epilogue d_ij = (s_i + s_j) - 2 S_ij,
//                               Kmat_ij = exp(kernel_sign * d_ij / eps), the store and the tile's row sums
//   3. dm_scale_rows x 2        Kmat_ij /= (p_i p_j)^alpha with the row sums of the new entries, then Kn_ij = Kmat_ij / (q_i q_j)
//   4. dm_deflate, dm_colnorm, dm_finish: the streaming kernels of the block subspace iteration (capi_diffmap.hip)
//
// The pairwise matrix has a short reduction (K = tens to a few hundred) and a large output (N x N): the opposite of the
// tall-skinny Gram kernel.  One 4-wave workgroup owns a 64 x 64 tile (I, J) with J >= I of the UPPER block triangle and writes
// both Kmat[I, J] and its mirror Kmat[J, I] from the same registers, so Kmat is exactly symmetric by construction and half the
// matrix products are never formed.  Wave w owns rows 16w .. 16w+15 of the tile and its four 16-column tiles; the operands
// come straight from Xr (K x N, a column is contiguous; the whole matrix is cache-resident), lane (q, c) holding
// Xr[4 step + q][i0 + c].  Every 16 x 16 result goes through the wave's own LDS patch once so that both stores run along the
// contiguous direction of Kmat (128-byte segments).
// Row sums: tile (I, J) writes part[J][rows of I] (sums over its 64 columns) and, off the diagonal, part[I][rows of J] (sums
// over its 64 rows); p_i = sum over the block index in ascending order.  Every partial is written by exactly one workgroup,
// in a fixed order inside it: the bits depend on N and K alone, not on the grid, the run or the order workgroups finish in.
#include "si_internal.h"

namespace si {

typedef double d4 __attribute__((ext_vector_type(4)));
constexpr int DM_T = 64;   // tile edge of the pairwise kernel and column chunk of the scaling passes

template <typename AT>
__device__ __forceinline__ double dm_load(const void* A, int64_t idx) {
  return (double)static_cast<const AT*>(A)[idx];
}

// mm[2k], mm[2k + 1] = min / max of column k of A over its N rows (min and max are exact: any order gives the same bits)
template <typename AT>
__global__ __launch_bounds__(256) void dm_minmax_kernel(const void* __restrict__ A, int64_t ldA, int64_t N, double* __restrict__ mm) {
  __shared__ double smn[256], smx[256];
  const int k = blockIdx.x, t = threadIdx.x;
  double mn = INFINITY, mx = -INFINITY;
  for (int64_t i = t; i < N; i += 256) {
    const double v = dm_load<AT>(A, i + (int64_t)k * ldA);
    mn = v < mn ? v : mn;
    mx = v > mx ? v : mx;
  }
  smn[t] = mn, smx[t] = mx;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      smn[t] = smn[t + s] < smn[t] ? smn[t + s] : smn[t];
      smx[t] = smx[t + s] > smx[t] ? smx[t + s] : smx[t];
    }
    __syncthreads();
  }
  if (t == 0) mm[2 * k] = smn[0], mm[2 * k + 1] = smx[0];
}

// Xr (Kp x Npad, column i contiguous; rows [K, Kp) and columns [N, Npad) stay zero) and s_i, one thread per weight i
template <typename AT>
__global__ __launch_bounds__(256) void dm_rescale_kernel(const void* __restrict__ A, int64_t ldA, int64_t N, int K, int Kp,
                                                         const double* __restrict__ mm, int rescale, double* __restrict__ Xr,
                                                         double* __restrict__ s) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  double acc = 0.0;
  for (int k = 0; k < K; ++k) {
    double v = dm_load<AT>(A, i + (int64_t)k * ldA);
    if (rescale) {
      const double mn = mm[2 * k], sc = 1.0 / (mm[2 * k + 1] - mn);
      v = (v - mn) * sc;
      if (v != v) v = 0.0;
    }
    Xr[(int64_t)k + (int64_t)Kp * i] = v;
    acc = acc + v * v;
  }
  s[i] = acc;
}

// grid = the nb (nb + 1) / 2 tiles of the upper block triangle; part: nb x ldn; flag: raised on a non-finite entry
__global__ __launch_bounds__(256) void dm_pairwise_kernel(const double* __restrict__ Xr, int Kp, const double* __restrict__ s,
                                                          int64_t N, int nb, double sign_over_one, double eps,
                                                          double* __restrict__ Kmat, int64_t ldn, double* __restrict__ part,
                                                          int* __restrict__ flag) {
  __shared__ double patch[4][16 * 17];
  __shared__ double colpart[4][DM_T];
  // tile (I, J), J >= I, from the linear index: row I of the triangle starts at I nb - I (I - 1) / 2
  int I = 0, rem = (int)blockIdx.x;
  while (rem >= nb - I) rem -= nb - I, ++I;
  const int J = I + rem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, c = lane & 15;
  const int64_t i0 = (int64_t)I * DM_T + 16 * wave, j0 = (int64_t)J * DM_T;
  const double* xa = Xr + (int64_t)Kp * (i0 + c) + q;
  const double* xb = Xr + (int64_t)Kp * (j0 + c) + q;
  d4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = (d4){0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < Kp; k0 += 4) {   // ascending k for every entry, (i, j) and (j, i) being ONE accumulator
    const double a = xa[k0];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, xb[k0 + (int64_t)Kp * 16 * t], acc[t], 0, 0, 0);
  }
  // a lane holds S[i = i0 + q + 4 r][j = j0 + 16 t + c]
  double si[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) si[r] = s[i0 + q + 4 * r];   // (s has Npad entries, zero past N)
  double rows[4] = {0.0, 0.0, 0.0, 0.0}, cols[4];
  bool bad = false;
  double* pt = patch[wave];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int64_t j = j0 + 16 * t + c;
    const double sj = s[j];
    double csum = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t i = i0 + q + 4 * r;
      const double d = (si[r] + sj) - 2.0 * acc[t][r];
      double v = exp(sign_over_one * d / eps);
      const bool valid = i < N && j < N;
      v = valid ? v : 0.0;
      bad = bad || (valid && !(fabs(v) <= 1.79769313486231570815e308));
      acc[t][r] = v;
      rows[r] = rows[r] + v;
      csum = csum + v;
    }
    // column sums over the wave's 16 rows: the 4 r in the lane, then the 4 q (lanes 16 and 32 apart)
    csum = csum + __shfl_xor(csum, 16);
    csum = csum + __shfl_xor(csum, 32);
    cols[t] = csum;
    // mirror store Kmat[j, i]: lanes along c are consecutive rows j
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t i = i0 + q + 4 * r;
      if (I != J && i < N && j < N) Kmat[j + ldn * i] = acc[t][r];
    }
    // Kmat[i, j] through the wave's patch, so that lanes along c become consecutive rows i
#pragma unroll
    for (int r = 0; r < 4; ++r) pt[(q + 4 * r) * 17 + c] = acc[t][r];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double v = pt[c * 17 + (q + 4 * r)];   // S[i = i0 + c][j = j0 + 16 t + q + 4 r]
      const int64_t i = i0 + c, jj = j0 + 16 * t + q + 4 * r;
      if (i < N && jj < N && (I != J || i <= jj)) {
        Kmat[i + ldn * jj] = v;
        if (I == J) Kmat[jj + ldn * i] = v;   // diagonal tile: the upper triangle mirrored, as the Gram kernel does
      }
    }
    __syncthreads();
  }
  // row sums over the tile's 64 columns: the 4 t in the lane (above), then the 16 c of the lane's row group
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double v = rows[r];
    v = v + __shfl_xor(v, 8, 16);
    v = v + __shfl_xor(v, 4, 16);
    v = v + __shfl_xor(v, 2, 16);
    v = v + __shfl_xor(v, 1, 16);
    const int64_t i = i0 + q + 4 * r;
    if (c == 0 && i < N) part[(int64_t)J * ldn + i] = v;
  }
  if (I != J) {   // the mirror's row sums: column sums of this tile over its 4 waves, in wave order
    if (q == 0) {
#pragma unroll
      for (int t = 0; t < 4; ++t) colpart[wave][16 * t + c] = cols[t];
    }
    __syncthreads();
    if (tid < DM_T) {
      const double v = ((colpart[0][tid] + colpart[1][tid]) + colpart[2][tid]) + colpart[3][tid];
      const int64_t j = j0 + tid;
      if (j < N) part[(int64_t)I * ldn + j] = v;
    }
  }
  if (bad) atomicOr(flag, 1);
}

// out[i] = sum_b part[b][i], b ascending;  mode 1: its square root
__global__ __launch_bounds__(256) void dm_sum_parts_kernel(const double* __restrict__ part, int nb, int64_t ldn, int64_t N, int mode,
                                                           double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  double t = 0.0;
  for (int b = 0; b < nb; ++b) t = t + part[(int64_t)b * ldn + i];
  out[i] = mode == 1 ? sqrt(t) : t;
}

// Kmat_ij /= w(v_i v_j) for the 64 columns of chunk blockIdx.y, one thread per row: w = x^alpha (mode 0; alpha == 1 is x itself)
// with part[chunk][i] = the new entries' sum over the chunk's columns in ascending order, or w = x (mode 1, no sums)
__global__ __launch_bounds__(256) void dm_scale_rows_kernel(double* __restrict__ Kmat, int64_t ldn, int64_t N, const double* __restrict__ v,
                                                            double alpha, int mode, double* __restrict__ part) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int64_t j0 = (int64_t)blockIdx.y * DM_T;
  const int64_t j1 = j0 + DM_T < N ? j0 + DM_T : N;
  const double vi = v[i];
  double t = 0.0;
  for (int64_t j = j0; j < j1; ++j) {
    double w = vi * v[j];
    if (mode == 0 && alpha != 1.0) w = pow(w, alpha);
    const double x = Kmat[i + ldn * j] / w;
    Kmat[i + ldn * j] = x;
    t = t + x;
  }
  if (mode == 0) part[(int64_t)blockIdx.y * ldn + i] = t;
}

// block tree sum of 256 values in a fixed order (every thread returns the total)
__device__ __forceinline__ double dm_block_sum(double v, double* sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) sh[t] = sh[t] + sh[t + s];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// u_1 = q / ||q||  (one workgroup)
__global__ __launch_bounds__(256) void dm_unit_kernel(const double* __restrict__ q, int64_t N, double* __restrict__ u1) {
  __shared__ double sh[256];
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < N; i += 256) a = a + q[i] * q[i];
  const double nrm = sqrt(dm_block_sum(a, sh));
  for (int64_t i = threadIdx.x; i < N; i += 256) u1[i] = q[i] / nrm;
}

// deflation V[:, j] -= u_1 (u_1' V[:, j]), one workgroup per column
__global__ __launch_bounds__(256) void dm_deflate_kernel(double* __restrict__ V, int64_t ldv, int64_t N, const double* __restrict__ u1) {
  __shared__ double sh[256];
  double* col = V + (int64_t)blockIdx.x * ldv;
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < N; i += 256) a = a + u1[i] * col[i];
  const double dot = dm_block_sum(a, sh);
  for (int64_t i = threadIdx.x; i < N; i += 256) col[i] = col[i] - u1[i] * dot;
}

// out[j] = ||R[:, j]||, one workgroup per column
__global__ __launch_bounds__(256) void dm_colnorm_kernel(const double* __restrict__ R, int64_t ldr, int64_t N, double* __restrict__ out) {
  __shared__ double sh[256];
  const double* col = R + (int64_t)blockIdx.x * ldr;
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < N; i += 256) a = a + col[i] * col[i];
  const double t = dm_block_sum(a, sh);
  if (threadIdx.x == 0) out[blockIdx.x] = sqrt(t);
}

// P[:, j] = sign_j * U[:, j] ./ u_1 with sign_j making the entry of largest magnitude positive (lowest index on a tie), one
// workgroup per column (reference :205-206: transform(diff_M), returned transposed)
__global__ __launch_bounds__(256) void dm_finish_kernel(const double* __restrict__ U, int64_t ldu, int64_t N, const double* __restrict__ u1,
                                                        double* __restrict__ P, int64_t ldp) {
  __shared__ double sv[256];
  __shared__ long long sidx[256];
  const int t = threadIdx.x;
  const double* col = U + (int64_t)blockIdx.x * ldu;
  double best = -1.0;
  long long bi = 0;
  for (int64_t i = t; i < N; i += 256) {   // ascending i inside a thread: a strict > keeps the lowest index
    const double a = fabs(col[i] / u1[i]);
    if (a > best) best = a, bi = i;
  }
  sv[t] = best, sidx[t] = bi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s && (sv[t + s] > sv[t] || (sv[t + s] == sv[t] && sidx[t + s] < sidx[t]))) sv[t] = sv[t + s], sidx[t] = sidx[t + s];
    __syncthreads();
  }
  const double sgn = col[sidx[0]] / u1[sidx[0]] < 0.0 ? -1.0 : 1.0;
  double* out = P + (int64_t)blockIdx.x * ldp;
  for (int64_t i = t; i < N; i += 256) out[i] = sgn * (col[i] / u1[i]);
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
void launch_dm_rescale(hipStream_t st, const void* A, int32_t a_dtype, int64_t ldA, int64_t N, int K, int Kp, int rescale, double* mm,
                       double* Xr, double* s) {
  const unsigned nblk = (unsigned)((N + 255) / 256);
  if (a_dtype == SI_F32) {
    if (rescale) hipLaunchKernelGGL(dm_minmax_kernel<float>, dim3((unsigned)K), dim3(256), 0, st, A, ldA, N, mm);
    hipLaunchKernelGGL(dm_rescale_kernel<float>, dim3(nblk), dim3(256), 0, st, A, ldA, N, K, Kp, mm, rescale, Xr, s);
  } else {
    if (rescale) hipLaunchKernelGGL(dm_minmax_kernel<double>, dim3((unsigned)K), dim3(256), 0, st, A, ldA, N, mm);
    hipLaunchKernelGGL(dm_rescale_kernel<double>, dim3(nblk), dim3(256), 0, st, A, ldA, N, K, Kp, mm, rescale, Xr, s);
  }
}

int dm_blocks(int64_t N) { return (int)((N + DM_T - 1) / DM_T); }

void launch_dm_pairwise(hipStream_t st, const double* Xr, int Kp, const double* s, int64_t N, int kernel_sign, double eps, double* Kmat,
                        int64_t ldn, double* part, int* flag) {
  const int nb = dm_blocks(N);
  const unsigned tiles = (unsigned)((int64_t)nb * (nb + 1) / 2);
  hipLaunchKernelGGL(dm_pairwise_kernel, dim3(tiles), dim3(256), 0, st, Xr, Kp, s, N, nb, (double)kernel_sign, eps, Kmat, ldn, part, flag);
}

void launch_dm_sum_parts(hipStream_t st, const double* part, int64_t ldn, int64_t N, bool root, double* out) {
  hipLaunchKernelGGL(dm_sum_parts_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, part, dm_blocks(N), ldn, N, root ? 1 : 0, out);
}

void launch_dm_scale_rows(hipStream_t st, double* Kmat, int64_t ldn, int64_t N, const double* v, double alpha, bool with_sums, double* part) {
  hipLaunchKernelGGL(dm_scale_rows_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)dm_blocks(N)), dim3(256), 0, st, Kmat, ldn, N, v, alpha,
                     with_sums ? 0 : 1, part);
}

void launch_dm_unit(hipStream_t st, const double* q, int64_t N, double* u1) {
  hipLaunchKernelGGL(dm_unit_kernel, dim3(1), dim3(256), 0, st, q, N, u1);
}
void launch_dm_deflate(hipStream_t st, double* V, int64_t ldv, int64_t N, int ncol, const double* u1) {
  hipLaunchKernelGGL(dm_deflate_kernel, dim3((unsigned)ncol), dim3(256), 0, st, V, ldv, N, u1);
}
void launch_dm_colnorm(hipStream_t st, const double* R, int64_t ldr, int64_t N, int ncol, double* out) {
  hipLaunchKernelGGL(dm_colnorm_kernel, dim3((unsigned)ncol), dim3(256), 0, st, R, ldr, N, out);
}
void launch_dm_finish(hipStream_t st, const double* U, int64_t ldu, int64_t N, int M, const double* u1, double* P, int64_t ldp) {
  hipLaunchKernelGGL(dm_finish_kernel, dim3((unsigned)M), dim3(256), 0, st, U, ldu, N, u1, P, ldp);
}

}  // namespace si
