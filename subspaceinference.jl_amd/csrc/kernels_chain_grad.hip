// Value AND gradient of the log-density of a NARROW Dense chain for many points at once (si_logdensity_grad_batch): the class
// of kernels_chain_grid.hip (docs/src/nn_example.md:112-118, 2-200-50-50-50-1 on 1000 observations), reference
// src/space_inference.jl:107 `l_pi_grad` as it is used by :117-120 (:mala) and :139-160 (:hmc).
//
//   chain_vgrad_kernel<NB>       grid (ceil(B / (16 NB)), points).  A workgroup owns 16 NB observations of ONE point: forward
//                                through every layer with EVERY layer's activation kept in LDS, the output delta
//                                (y - yhat) / sigma^2 .* act', then per layer from the last: db = rowsum(Delta),
//                                dW = Delta * H', Delta_prev = (W' Delta) .* act'.  The reverse sweep rebuilds act' from the stored
//                                outputs (dact_from_output of kernels_bwd.hip).  All three matrix products of a layer run on
//                                v_mfma_f64_16x16x4_f64 with the fragment conventions of chain_tile / cg_tile:
//                                  lane (q, c) = (lane >> 4, lane & 15) hands over A[i = c][k = q] and B[k = q][j = c] and
//                                  receives D[i = q + 4 r][j = c] in element r.
//                                The workgroup writes ITS partial of grad_w (N doubles) and of the sum of squared errors.
//   chain_vgrad_reduce_kernel    one workgroup per point: the partials of the point's workgroups summed in index order, the
//                                prior's term (prior_grad_kernel: g -= w / sigma_p^2), grad_z = P' g (thread-strided sums, a
//                                shuffle-down tree, the wave sums in order: ptg_partial_kernel's scheme), lp.
//
// The weights W_swa + P z of every point come from ONE stacked launch_reconstruct in front (K4's own kernel).
//
// No floating-point atomics: every sum has a fixed order that depends on the chain and on B only, so a point's result does not
// depend on how many points the call carries, on its column, or on the run.  Every wave meets every barrier (all loops around
// a barrier run over workgroup-uniform bounds; nothing returns early).  Columns b >= B of a ragged last workgroup have Delta = 0
// AND stored activations = 0: they add exact zeros to every partial.  Compiled with -ffp-contract=off.
#include <algorithm>

#include "chain_common.h"

namespace si {

typedef double vg4 __attribute__((ext_vector_type(4)));

extern __shared__ __attribute__((aligned(16))) double vg_lds[];

constexpr int VG_NT = 256;   // 4 waves: the 16-wide tiles of a layer are dealt over them
constexpr int VG_NW = VG_NT / 64;
constexpr int VG_KC = 8;     // k steps whose operands are requested together

__device__ __forceinline__ double vg_dact(double h, int act) {   // (dact_from_output of kernels_bwd.hip)
  switch (act) {
    case SI_ACT_RELU: return h > 0.0 ? 1.0 : 0.0;
    case SI_ACT_TANH: return 1.0 - h * h;
    case SI_ACT_SIGMOID: return h * (1.0 - h);
    default: return 1.0;
  }
}
__device__ __attribute__((noinline)) double vg_act_slow(double v, int act) { return chain_act(v, act); }
__device__ __forceinline__ double vg_act(double v, int act) {
  if (act == SI_ACT_RELU) return v > 0.0 ? v : 0.0;
  if (act == SI_ACT_IDENTITY) return v;
  return vg_act_slow(v, act);
}

// acc[nb] += sum over k < klen of  LDS[abase + k + lda * (16 nb + c)] * G[gbase(k)]  -- the two products whose B operand streams
// from the weights: the forward layer (k = input feature, G = W[row + out k]) and W' Delta (k = output feature, G = W[k + out col]).
// gk = element stride of k in G, g0 = the lane's offset at k = 0.  k steps of 4 in ascending order, VG_KC at a time; a step past
// klen hands zeros to both operands.  The LDS image has rows up to a multiple of 4 (zero).
template <int NB>
__device__ __forceinline__ void vg_stream_tile(int abase, int lda, const double* __restrict__ G, int64_t g0, int64_t gk, int klen,
                                               int q, int c, vg4 (&acc)[NB]) {
  const int nst = (klen + 3) >> 2;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) acc[nb] = (vg4){0.0, 0.0, 0.0, 0.0};
  for (int s0 = 0; s0 < nst; s0 += VG_KC) {
    double f[VG_KC], a[VG_KC][NB];
#pragma unroll
    for (int s = 0; s < VG_KC; ++s) {
      const int k = 4 * (s0 + s) + q;
      const int kc = k < klen ? k : klen - 1;   // (always a valid element; the value is dropped)
      const double v = G[g0 + gk * kc];
      f[s] = k < klen ? v : 0.0;
    }
#pragma unroll
    for (int s = 0; s < VG_KC; ++s) {
      const bool live = s0 + s < nst;
      const int k = live ? 4 * (s0 + s) + q : q;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const double v = vg_lds[abase + k + lda * (16 * nb + c)];
        a[s][nb] = live ? v : 0.0;
      }
    }
#pragma unroll
    for (int s = 0; s < VG_KC; ++s)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s][nb], f[s], acc[nb], 0, 0, 0);
  }
}

// the workgroup's sum of v over its threads, on thread 0: shuffle-down wave sums, then (r0 + r1) + (r2 + r3)
__device__ __forceinline__ double vg_block_sum4(double v, int o_red) {
  v = chain_wave_sum(v);
  if ((threadIdx.x & 63) == 0) vg_lds[o_red + (threadIdx.x >> 6)] = v;
  __syncthreads();
  return (vg_lds[o_red] + vg_lds[o_red + 1]) + (vg_lds[o_red + 2] + vg_lds[o_red + 3]);
}

template <int NB>
__global__ __launch_bounds__(VG_NT) void chain_vgrad_kernel(ChainVgradPlan p, const double* __restrict__ w, int64_t w_stride,
                                                           const double* __restrict__ X, const double* __restrict__ Y, double inv_s2,
                                                           double* __restrict__ part, int64_t part_stride,
                                                           double* __restrict__ ssepart) {
  constexpr int BT = 16 * NB;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (scalar: the tile loops branch uniformly)
  const int q = lane >> 4, c = lane & 15;
  const int L = p.L, B = p.B;
  const int64_t wg = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  const int64_t b0 = (int64_t)blockIdx.x * BT;
  w += (int64_t)blockIdx.y * w_stride;
  part += wg * part_stride;

  // ---- the X tile as image 0: rows k >= in (up to a multiple of 4) and columns b >= B are zero
  {
    const int in0 = p.lay[0].in, inp = (in0 + 3) & ~3, ld0 = p.ld[0];
    for (int e = tid; e < inp * BT; e += VG_NT) {
      const int k = e % inp, b = e / inp;
      vg_lds[p.o_img[0] + k + ld0 * b] = (k < in0 && b0 + b < B) ? X[k + (int64_t)in0 * (b0 + b)] : 0.0;
    }
  }
  __syncthreads();

  // ---- forward: image l + 1 = act(W_l * image l + b_l), every image kept
  for (int l = 0; l < L; ++l) {
    const int in = p.lay[l].in, out = p.lay[l].out, act = p.lay[l].act;
    const double* W = w + p.lay[l].w_off;
    const double* bias = w + p.lay[l].b_off;
    const int hi = p.o_img[l], ldi = p.ld[l], ho = p.o_img[l + 1], ldo = p.ld[l + 1];
    const int ntm = (out + 15) >> 4, outp = (out + 3) & ~3;
    for (int mt = wave; mt < ntm; mt += VG_NW) {
      const int gi = 16 * mt + c, row = gi < out ? gi : out - 1;   // (rows past `out` only feed outputs that are never stored)
      vg4 acc[NB];
      vg_stream_tile<NB>(hi + 0, ldi, W, row, out, in, q, c, acc);
      const double bv = bias[row];
      if (gi < outp) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int b = 16 * nb + q + 4 * r;
            vg_lds[ho + gi + ldo * b] = (gi < out && b0 + b < B) ? vg_act(acc[nb][r] + bv, act) : 0.0;
          }
      }
    }
    __syncthreads();
  }

  // ---- Delta_L = (y - yhat) / sigma^2 .* act_L'(yhat) (delta_out_kernel) and this workgroup's squared errors
  {
    const int outL = p.lay[L - 1].out, outp = (outL + 3) & ~3, actL = p.lay[L - 1].act;
    const int ho = p.o_img[L], ldo = p.ld[L], D = p.o_delta[(L - 1) & 1];
    double sq = 0.0;
    for (int e = tid; e < outp * BT; e += VG_NT) {
      const int o = e % outp, b = e / outp;
      double dv = 0.0;
      if (o < outL && b0 + b < B) {
        const double yh = vg_lds[ho + o + ldo * b];
        const double r = Y[o + (int64_t)outL * (b0 + b)] - yh;
        sq += r * r;
        dv = inv_s2 * r * vg_dact(yh, actL);
      }
      vg_lds[D + o + ldo * b] = dv;
    }
    const double s = vg_block_sum4(sq, p.o_red);   // (its barrier also publishes Delta_L)
    if (tid == 0) ssepart[wg] = s;
  }

  // ---- reverse sweep
  for (int l = L - 1; l >= 0; --l) {
    const int in = p.lay[l].in, out = p.lay[l].out;
    const double* W = w + p.lay[l].w_off;
    const int D = p.o_delta[l & 1], ldd = p.ld[l + 1], hi = p.o_img[l], ldi = p.ld[l];
    // db_l = rowsum(Delta_l): the workgroup's columns in order
    for (int o = tid; o < out; o += VG_NT) {
      double s = 0.0;
      for (int b = 0; b < BT; ++b) s += vg_lds[D + o + ldd * b];
      part[p.lay[l].b_off + o] = s;
    }
    // dW_l = Delta_l * H_l' contracted over the workgroup's observations: D[i = input feature][j = output feature]
    {
      const int nti = (in + 15) >> 4, nto = (out + 15) >> 4;
      double* dW = part + p.lay[l].w_off;
      for (int t = wave; t < nti * nto; t += VG_NW) {
        const int it = t % nti, ot = t / nti;
        const int ri = 16 * it + c < in ? 16 * it + c : in - 1;      // (a clamped row / column only feeds results that are not stored)
        const int ro = 16 * ot + c < out ? 16 * ot + c : out - 1;
        double a[4 * NB], f[4 * NB];
#pragma unroll
        for (int s = 0; s < 4 * NB; ++s) {
          a[s] = vg_lds[hi + ri + ldi * (4 * s + q)];
          f[s] = vg_lds[D + ro + ldd * (4 * s + q)];
        }
        vg4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 4 * NB; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], f[s], acc, 0, 0, 0);
        const int o = 16 * ot + c;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 16 * it + q + 4 * r;
          if (i < in && o < out) dW[o + (int64_t)out * i] = acc[r];
        }
      }
    }
    // Delta_{l-1} = (W_l' Delta_l) .* act_{l-1}'(H_l): D[i = observation][j = input feature], contracted over the output features
    if (l > 0) {
      const int actp = p.lay[l - 1].act, Dn = p.o_delta[(l - 1) & 1];
      const int nti = (in + 15) >> 4, inp = (in + 3) & ~3;
      for (int it = wave; it < nti; it += VG_NW) {
        const int gi = 16 * it + c, col = gi < in ? gi : in - 1;
        vg4 acc[NB];
        vg_stream_tile<NB>(D, ldd, W, (int64_t)out * col, 1, out, q, c, acc);
        if (gi < inp) {
#pragma unroll
          for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int b = 16 * nb + q + 4 * r;
              const double h = vg_lds[hi + gi + ldi * b];
              vg_lds[Dn + gi + ldi * b] = (gi < in && b0 + b < B) ? acc[nb][r] * vg_dact(h, actp) : 0.0;
            }
        }
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// one workgroup per point
constexpr int VR_NT = 1024;
constexpr int VR_MT = 4;     // columns of P per sweep (PTG_MT of kernels_bwd.hip)

// the workgroup's sum on every thread: shuffle-down wave sums, the 16 wave sums added in order
__device__ __forceinline__ double vr_block_sum(double v, double* red) {
  v = chain_wave_sum(v);
  __syncthreads();   // (the last round's readers are done)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int i = 1; i < VR_NT / 64; ++i) s += red[i];
  return s;
}

__global__ __launch_bounds__(VR_NT) void chain_vgrad_reduce_kernel(const double* __restrict__ part, int G, int64_t N, int64_t part_stride,
                                                                  const double* __restrict__ ssepart, const double* __restrict__ w,
                                                                  int64_t w_stride, const double* __restrict__ P, int64_t ldP, int M,
                                                                  int prior, double inv_sp2, double sigma_p2, double c0p, double c0,
                                                                  double sigma2, double* __restrict__ gw, double* __restrict__ lp_out,
                                                                  double* __restrict__ gz_out) {
  __shared__ double red[VR_NT / 64];
  const int tid = threadIdx.x;
  const int64_t pt = blockIdx.x;
  part += pt * G * part_stride;
  ssepart += pt * G;
  w += pt * w_stride;
  gw += pt * part_stride;
  // grad_w[r] = the point's workgroup partials in index order (eight requested together, added in order), then the prior's term
  double wsq = 0.0;
  for (int64_t r = tid; r < N; r += VR_NT) {
    double s = 0.0;
    int g = 0;
    for (; g + 8 <= G; g += 8) {
      double v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = part[(int64_t)(g + j) * part_stride + r];
#pragma unroll
      for (int j = 0; j < 8; ++j) s += v[j];
    }
    for (; g < G; ++g) s += part[(int64_t)g * part_stride + r];
    if (prior) {
      const double wv = w[r];
      s -= wv * inv_sp2;   // (prior_grad_kernel)
      wsq += wv * wv;
    }
    gw[r] = s;   // (read back below by the thread that wrote it)
  }
  double sq = 0.0;
  for (int g = tid; g < G; g += VR_NT) sq += ssepart[g];
  const double sse = vr_block_sum(sq, red);
  const double wsum = prior ? vr_block_sum(wsq, red) : 0.0;
  if (tid == 0) {
    double lp = c0 - (sse / sigma2) / 2.0;
    if (prior) lp += c0p - (wsum / sigma_p2) / 2.0;
    lp_out[pt] = lp;
  }
  // grad_z = P' grad_w
  for (int m0 = 0; m0 < M; m0 += VR_MT) {
    double s[VR_MT];
#pragma unroll
    for (int j = 0; j < VR_MT; ++j) s[j] = 0.0;
    for (int64_t r = tid; r < N; r += VR_NT) {
      const double gv = gw[r];
#pragma unroll
      for (int j = 0; j < VR_MT; ++j)
        if (m0 + j < M) s[j] += P[r + ldP * (m0 + j)] * gv;
    }
#pragma unroll
    for (int j = 0; j < VR_MT; ++j) {
      const double t = vr_block_sum(s[j], red);
      if (tid == 0 && m0 + j < M) gz_out[pt * M + m0 + j] = t;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// host: the LDS plan.  Image l (the input of layer l; image L = the model outputs) is [k + ld * b] with ld = ceil4(width) + 2, as
// in chain_fused_plan (conflict-free ds_read_b64 fragments along k; rows up to a multiple of 4 exist and are zero); EVERY image is
// kept.  Two Delta buffers of the widest image (Delta_l has the pitch of image l + 1), four doubles of wave sums.
// Returns the bytes of dynamic LDS for batch tiles of 16 NB observations, or 0 when the chain is not of this class / does not fit.
size_t chain_vgrad_plan(ChainVgradPlan& p, const si_layer* layers, int L, int64_t B, int NB) {
  if (L < 1 || L > SI_CHAIN_MAX_LAYERS || B < 1 || B > (1 << 30)) return 0;
  const int BT = 16 * NB;
  p.L = L;
  p.B = (int)B;
  for (int l = 0; l < L; ++l) {
    if (layers[l].kind != SI_LAYER_DENSE || layers[l].act >= SI_ACT_LEAKYRELU || layers[l].in < 1 || layers[l].out < 1) return 0;
    if (l > 0 && layers[l].in != layers[l - 1].out) return 0;
    p.lay[l] = layers[l];
    p.ld[l] = ((layers[l].in + 3) & ~3) + 2;
  }
  p.ld[L] = ((layers[L - 1].out + 3) & ~3) + 2;
  int64_t off = 0, maxd = 0;
  for (int l = 0; l <= L; ++l) {
    p.o_img[l] = (int)off;
    off += (int64_t)p.ld[l] * BT;
    if (l > 0) maxd = std::max<int64_t>(maxd, (int64_t)p.ld[l] * BT);
    if (off > (1 << 24)) return 0;
  }
  p.o_delta[0] = (int)off;
  off += maxd;
  p.o_delta[1] = (int)off;
  off += maxd;
  p.o_red = (int)off;
  off += 4;
  p.lds_doubles = (int)off;
  if (off > (int64_t)(160 * 1024) / 8) return 0;
  return (size_t)off * sizeof(double);
}

template <int NB>
static void launch_vgrad_nb(hipStream_t st, const ChainVgradPlan& p, size_t lds, const double* w, int64_t w_stride, const double* X,
                            const double* Y, double inv_s2, double* part, int64_t part_stride, double* ssepart, int npoints) {
  static LdsOptIn optin;
  optin.ensure(reinterpret_cast<const void*>(chain_vgrad_kernel<NB>), lds);
  const unsigned G = (unsigned)((p.B + 16 * NB - 1) / (16 * NB));
  hipLaunchKernelGGL((chain_vgrad_kernel<NB>), dim3(G, (unsigned)npoints), dim3(VG_NT), lds, st, p, w, w_stride, X, Y, inv_s2, part,
                     part_stride, ssepart);
}

// npoints <= 65535 (grid.y): the caller walks its points in groups
void launch_chain_vgrad(hipStream_t st, const ChainVgradPlan& p, int NB, size_t lds, const double* w, int64_t w_stride, const double* X,
                        const double* Y, double inv_s2, double* part, int64_t part_stride, double* ssepart, int npoints) {
  if (NB == 2)
    launch_vgrad_nb<2>(st, p, lds, w, w_stride, X, Y, inv_s2, part, part_stride, ssepart, npoints);
  else
    launch_vgrad_nb<1>(st, p, lds, w, w_stride, X, Y, inv_s2, part, part_stride, ssepart, npoints);
}

void launch_chain_vgrad_reduce(hipStream_t st, const double* part, int G, int64_t N, int64_t part_stride, const double* ssepart,
                               const double* w, int64_t w_stride, const double* P, int64_t ldP, int M, double sigma_p, double c0p,
                               double c0, double sigma2, double* gw, double* lp_out, double* gz_out, int npoints) {
  const bool prior = sigma_p > 0.0;
  const double sp2 = prior ? sigma_p * sigma_p : 1.0;
  hipLaunchKernelGGL(chain_vgrad_reduce_kernel, dim3((unsigned)npoints), dim3(VR_NT), 0, st, part, G, N, part_stride, ssepart, w,
                     w_stride, P, ldP, M, prior ? 1 : 0, 1.0 / sp2, sp2, c0p, c0, sigma2, gw, lp_out, gz_out);
}

}  // namespace si
