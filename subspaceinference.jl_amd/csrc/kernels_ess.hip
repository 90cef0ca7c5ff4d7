// Elliptical slice sampling (Murray, Adams, MacKay 2010; the sampler of Izmailov et al., "Subspace Inference for Bayesian Deep
// Learning") under the prior z ~ N(0, sigma_z^2 I), with the chain state on the device: the transition of samplers.ess_iter, defined
// once, on the Philox stream of philox.h.  NOT IN THE REFERENCE, whose sub_inference has no such sampler.
//
//   target   p(z) ~ exp(density(z)) N(z; 0, sigma_z^2 I): sigma_z is the PRIOR's standard deviation on z here, not a step size
//   chain c draws from Philox chain chain_id0 + c: purpose 0 at step 0 = the M normals n_0; purpose 1 at step t = e_t (Exp(1));
//   purpose 9 at step t = the M normals n_t; purpose 10 at step t, block j = v_j = u53(x1, x0)
//   t = 0    z = sigma_z n_0;  lp = density(z);  nev = 1, theta = 0
//   t >= 1   nu = sigma_z n_t;  logy = lp - e_t;  theta = 2 pi v_0;  lo = theta - 2 pi;  hi = theta;  k = 0
//            repeat:  zp = z cos theta + nu sin theta;  lpp = density(zp);  k += 1
//                     lpp > logy (a NaN compares false)  -> (z, lp) = (zp, lpp);  nev[t] = k;  theta[t] = theta;  stop
//                     k == max_evals                     -> state kept;  nev[t] = -max_evals;  theta[t] = 0;  stop
//                     theta < 0 ? lo = theta : hi = theta;   theta = lo + (hi - lo) v_k
//            column t = (z, lp)
//
// Three kernels, one workgroup per chain.  The density's sums at the pending points come from the caller's launches between them
// (si_sample_ess, capi_ess.hip: eval_density_all on chains.zprop); lpp is formed from them with rwmh_accept_kernel's expression.
// Component ownership is sampler_device.h's, so a chain's bits do not depend on the number of chains, on its column or on the run.
// Every angle is plain IEEE arithmetic on exact uniforms and the file is compiled without contraction of a * b + c: the host
// restatement forms the same angles bit for bit while its decisions are the device's.  No atomics except the count of open chains.
#include "sampler_device.h"

namespace si {

static constexpr uint32_t ESS_P_NU = 9u, ESS_P_SHRINK = 10u;
static constexpr double ESS_TWO_PI = 2.0 * 3.14159265358979323846;

__device__ __forceinline__ double ess_uniform(const EssRun& a, int64_t c, uint64_t step, uint32_t block) {
  const Philox4 x = philox_draw(a.seed, (uint32_t)(a.chain_id0 + (int32_t)c), step, ESS_P_SHRINK, block);
  return u53(x.v[1], x.v[0]);
}

// zp = z cos theta + nu sin theta for the chain of this workgroup: two products and a sum, each rounded by itself
__device__ __forceinline__ void ess_point(const EssRun& a, int64_t c, double theta) {
  const double *z = a.z + c * a.M, *nu = a.nu + c * a.M;
  double* zp = a.zp + c * a.M;
  const double cs = cos(theta), sn = sin(theta);
  for_owned(a.M, [&](int m) { zp[m] = z[m] * cs + nu[m] * sn; });
}

// z_0 = sigma_z n_0 into zp; the chain is open with no evaluation counted
__global__ __launch_bounds__(SAMPLER_NT) void ess_init_kernel(EssRun a) {
  const int64_t c = blockIdx.x;
  double* zp = a.zp + c * a.M;
  for_owned_normal(a.M, a.seed, (uint32_t)(a.chain_id0 + (int32_t)c), 0, 0u, [&](int m, double n) { zp[m] = a.sigma_z * n; });
  if (threadIdx.x == 0) {
    a.k[c] = 0;
    a.closed[c] = 0;
  }
}

// Transition `step` >= 1 begins: nu, logy, the first angle, the full bracket, the first point; every chain open.  The scalars are
// computed by every thread from the same inputs; thread 0 writes them.
__global__ __launch_bounds__(SAMPLER_NT) void ess_begin_kernel(EssRun a, uint64_t step) {
  const int64_t c = blockIdx.x;
  double* nu = a.nu + c * a.M;
  for_owned_normal(a.M, a.seed, (uint32_t)(a.chain_id0 + (int32_t)c), step, ESS_P_NU, [&](int m, double n) { nu[m] = a.sigma_z * n; });
  const double e = philox_randexp(a.seed, (uint32_t)(a.chain_id0 + (int32_t)c), step);
  const double theta = ESS_TWO_PI * ess_uniform(a, c, step, 0u);
  if (threadIdx.x == 0) {
    a.logy[c] = a.lp[c] - e;
    a.theta[c] = theta;
    a.lo[c] = theta - ESS_TWO_PI;
    a.hi[c] = theta;
    a.k[c] = 0;
    a.closed[c] = 0;
  }
  ess_point(a, c, theta);   // (every thread reads only the nu it wrote itself)
}

// One round of transition `step` given the density's sums at zp, for every open chain: lpp, then a keep (the state, column `step`,
// the chain closed), the cap (column `step` from the state, the chain closed, the state back in zp) or a shrink (the bracket, the
// next angle and point, the chain counted into *open).  step 0: the initial point is kept whatever its value.
// The chain's scalars are read by every thread BEFORE the barrier; thread 0 writes them after it.
__global__ __launch_bounds__(SAMPLER_NT) void ess_round_kernel(EssRun a, uint64_t step, int32_t* __restrict__ open) {
  const int64_t c = blockIdx.x;
  const int32_t M = a.M;
  if (a.closed[c]) return;   // (uniform over the workgroup: written by thread 0 of an earlier launch)
  // Distributions.logpdf(MvNormal(mu, sigma), y) = c0 - (sse / sigma^2) / 2 [+ the prior term]: rwmh_accept_kernel's expression
  double lpp = a.c0 - (a.sse[c] / a.s2) / 2.0;
  if (a.wsq) lpp += a.c0p - (a.wsq[c] / a.sp2) / 2.0;
  const double lp_old = a.lp[c], logy = a.logy[c], theta = step == 0 ? 0.0 : a.theta[c];
  double lo = a.lo[c], hi = a.hi[c];
  const int32_t k = a.k[c] + 1;
  __syncthreads();
  const int64_t col = (int64_t)step + a.itr * c;
  double *z = a.z + c * M, *zp = a.zp + c * M, *Z_col = a.Z_out + M * col;
  if (step == 0 || lpp > logy) {   // NaN compares false => shrink
    for_owned(M, [&](int m) {
      const double zv = zp[m];
      z[m] = zv;
      Z_col[m] = zv;
    });
    if (threadIdx.x == 0) {
      a.lp[c] = lpp;
      a.lp_out[col] = lpp;
      a.nev_out[col] = k;
      a.theta_out[col] = theta;
      a.k[c] = k;
      a.closed[c] = 1;
    }
  } else if (k >= a.max_evals) {
    for_owned(M, [&](int m) {
      const double zv = z[m];
      zp[m] = zv;
      Z_col[m] = zv;
    });
    if (threadIdx.x == 0) {
      a.lp_out[col] = lp_old;
      a.nev_out[col] = -a.max_evals;
      a.theta_out[col] = 0.0;
      a.k[c] = k;
      a.closed[c] = 1;
    }
  } else {
    if (theta < 0.0)
      lo = theta;
    else
      hi = theta;
    const double next = lo + (hi - lo) * ess_uniform(a, c, step, (uint32_t)k);
    if (threadIdx.x == 0) {
      a.lo[c] = lo;
      a.hi[c] = hi;
      a.theta[c] = next;
      a.k[c] = k;
      atomicAdd(open, 1);
    }
    ess_point(a, c, next);
  }
}

void launch_ess_init(hipStream_t st, const EssRun& a, int32_t C) {
  hipLaunchKernelGGL(ess_init_kernel, dim3((unsigned)C), dim3(SAMPLER_NT), 0, st, a);
}

void launch_ess_begin(hipStream_t st, const EssRun& a, int32_t C, uint64_t step) {
  hipLaunchKernelGGL(ess_begin_kernel, dim3((unsigned)C), dim3(SAMPLER_NT), 0, st, a, step);
}

void launch_ess_round(hipStream_t st, const EssRun& a, int32_t C, uint64_t step, int32_t* open) {
  hipLaunchKernelGGL(ess_round_kernel, dim3((unsigned)C), dim3(SAMPLER_NT), 0, st, a, step, open);
}

}  // namespace si
