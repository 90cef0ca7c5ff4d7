// MALA (reference src/space_inference.jl:117-120, AdvancedMH 0.6.2 `MALA(x -> MvNormal((sigma_z^2 / 2) .* x, sigma_z))`) with the
// chain state on the device: the transition of samplers.mala, defined once, on the Philox stream of philox.h.
//
//   chain c draws from Philox chain chain_id0 + c: purpose 0 at step t = the M normals n_t, purpose 1 at step t = e_t;  h = sigma_z^2 / 2
//   t = 0    z = sigma_z n_0;  (lp, g) = value and gradient at z
//   t >= 1   zp = z + h g + sigma_z n_t;  (lpp, gp) = value and gradient at zp
//            fwd = zp - z - h g;  bwd = z - zp - h gp;  logq = -(bwd.bwd - fwd.fwd) / (2 sigma_z^2)
//            accept iff -e_t < lpp - lp + logq   (a NaN anywhere makes the comparison false: reject)
//            accept: (z, lp, g) = (zp, lpp, gp);  sample t = (z, lp, g)
//
// Two kernels, one workgroup per chain.  The value and gradient at the proposals come from the caller's launches between them
// (si_sample_mala, capi_mala.hip).  Every sum over m has a fixed order that depends on M alone: thread i adds its components
// 2j, 2j + 1 for j = i, i + 256, ... in that order, the wave sums are chain_wave_sum's, the four wave sums are added as
// (r0 + r1) + (r2 + r3) -- so a chain's bits do not depend on the number of chains, on its column or on the run.  The file is
// compiled without contraction of a * b + c, like K1: every product and sum here is rounded by itself, as the host restatement's.
#include "chain_common.h"
#include "philox.h"
#include "si_internal.h"

namespace si {

static constexpr int MALA_NT = 256;

// zprop[:, c] = z[:, c] + h g[:, c] + sigma_z n_step  (first: z = sigma_z n_0, nothing is read)
__device__ __forceinline__ void mala_propose_chain(const double* __restrict__ z, const double* __restrict__ g, double* __restrict__ zprop,
                                                   int32_t M, double sigma_z, double h, uint64_t seed, uint32_t chain, uint64_t step,
                                                   bool first) {
  const int nblk = (M + 1) >> 1;
  for (int j = threadIdx.x; j < nblk; j += MALA_NT) {
    double n[2];
    philox_normal2(seed, chain, step, (uint32_t)j, n[0], n[1]);
    for (int k = 0; k < 2; ++k) {
      const int m = 2 * j + k;
      if (m < M) zprop[m] = first ? sigma_z * n[k] : (z[m] + h * g[m]) + sigma_z * n[k];
    }
  }
}

__global__ __launch_bounds__(MALA_NT) void mala_propose_kernel(const double* __restrict__ z, const double* __restrict__ g,
                                                               double* __restrict__ zprop, int32_t M, double sigma_z, double h,
                                                               uint64_t seed, int32_t chain_id0, uint64_t step, int first) {
  const int64_t c = blockIdx.x;
  mala_propose_chain(z + c * M, g + c * M, zprop + c * M, M, sigma_z, h, seed, (uint32_t)(chain_id0 + (int32_t)c), step, first != 0);
}

// Transition `step` of every chain, given (lpp, gp) at zprop: logq, the decision, the next state, sample `step` of Z / lp / G,
// the accept count, and -- in the same launch -- the proposal of transition step + 1 from the state just chosen.
__global__ __launch_bounds__(MALA_NT) void mala_accept_kernel(double* __restrict__ z, double* __restrict__ lp, double* __restrict__ g,
                                                              double* __restrict__ zprop, const double* __restrict__ lpp,
                                                              const double* __restrict__ gp, int64_t* __restrict__ nacc, int32_t M,
                                                              double sigma_z, double h, uint64_t seed, int32_t chain_id0, uint64_t step,
                                                              double* __restrict__ Z_out, double* __restrict__ lp_out,
                                                              double* __restrict__ G_out, int64_t itr, int propose_next) {
  __shared__ double red[2][MALA_NT / 64];
  __shared__ int accept_s;
  const int64_t c = blockIdx.x;
  const int tid = threadIdx.x;
  const uint32_t chain = (uint32_t)(chain_id0 + (int32_t)c);
  z += c * M;
  g += c * M;
  zprop += c * M;
  gp += c * M;
  const int nblk = (M + 1) >> 1;
  if (step > 0) {
    double ff = 0.0, bb = 0.0;
    for (int j = tid; j < nblk; j += MALA_NT) {
      for (int k = 0; k < 2; ++k) {
        const int m = 2 * j + k;
        if (m < M) {
          const double zv = z[m], zpv = zprop[m];
          const double fwd = (zpv - zv) - h * g[m];
          const double bwd = (zv - zpv) - h * gp[m];
          ff += fwd * fwd;
          bb += bwd * bwd;
        }
      }
    }
    ff = chain_wave_sum(ff);
    bb = chain_wave_sum(bb);
    if ((tid & 63) == 0) {
      red[0][tid >> 6] = ff;
      red[1][tid >> 6] = bb;
    }
  }
  __syncthreads();
  if (tid == 0) {
    bool accept = true;
    const double lp_new = lpp[c];
    if (step > 0) {
      const double fsum = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
      const double bsum = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
      const double logq = -(bsum - fsum) / (2.0 * (sigma_z * sigma_z));
      const double e = philox_randexp(seed, chain, step);
      accept = (-e < (lp_new - lp[c]) + logq);   // NaN compares false => reject
    }
    const double lp_keep = accept ? lp_new : lp[c];
    lp[c] = lp_keep;
    lp_out[(int64_t)step + itr * c] = lp_keep;
    if (step == 0)
      nacc[c] = 0;
    else if (accept)
      nacc[c] += 1;
    accept_s = accept ? 1 : 0;
  }
  __syncthreads();
  const bool accept = accept_s != 0;
  const int64_t obase = (int64_t)M * ((int64_t)step + itr * c);
  // (thread i owns the components 2j, 2j + 1 of its j in every phase: nothing below reads what another thread writes)
  for (int j = tid; j < nblk; j += MALA_NT) {
    for (int k = 0; k < 2; ++k) {
      const int m = 2 * j + k;
      if (m < M) {
        const double zv = accept ? zprop[m] : z[m];
        const double gv = accept ? gp[m] : g[m];
        z[m] = zv;
        g[m] = gv;
        Z_out[obase + m] = zv;
        if (G_out) G_out[obase + m] = gv;
      }
    }
  }
  if (propose_next) mala_propose_chain(z, g, zprop, M, sigma_z, h, seed, chain, step + 1, false);
}

void launch_mala_propose(hipStream_t st, const double* z, const double* g, double* zprop, int32_t M, int32_t C, double sigma_z,
                         uint64_t seed, int32_t chain_id0, uint64_t step, bool first) {
  hipLaunchKernelGGL(mala_propose_kernel, dim3((unsigned)C), dim3(MALA_NT), 0, st, z, g, zprop, M, sigma_z, 0.5 * (sigma_z * sigma_z),
                     seed, chain_id0, step, first ? 1 : 0);
}

void launch_mala_accept(hipStream_t st, double* z, double* lp, double* g, double* zprop, const double* lpp, const double* gp,
                        int64_t* nacc, int32_t M, int32_t C, double sigma_z, uint64_t seed, int32_t chain_id0, uint64_t step,
                        double* Z_out, double* lp_out, double* G_out, int64_t itr, bool propose_next) {
  hipLaunchKernelGGL(mala_accept_kernel, dim3((unsigned)C), dim3(MALA_NT), 0, st, z, lp, g, zprop, lpp, gp, nacc, M, sigma_z,
                     0.5 * (sigma_z * sigma_z), seed, chain_id0, step, Z_out, lp_out, G_out, itr, propose_next ? 1 : 0);
}

}  // namespace si
