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
// (si_sample_mala, capi_mala.hip).  Component ownership and the fixed order of every sum over m are sampler_device.h's -- so a
// chain's bits do not depend on the number of chains, on its column or on the run.  The file is compiled without contraction of
// a * b + c, like K1: every product and sum here is rounded by itself, as the host restatement's.
#include "sampler_device.h"

namespace si {

// zp = z + h g + sigma_z n_step for the chain of this workgroup  (first: z = sigma_z n_0, nothing is read)
__device__ __forceinline__ void mala_propose_chain(const MalaRun& a, int64_t c, uint64_t step, bool first) {
  const double *z = a.z + c * a.M, *g = a.g + c * a.M;
  double* zp = a.zp + c * a.M;
  for_owned_normal(a.M, a.seed, (uint32_t)(a.chain_id0 + (int32_t)c), step, 0u, [&](int m, double n) {
    zp[m] = first ? a.sigma_z * n : (z[m] + a.h * g[m]) + a.sigma_z * n;
  });
}

__global__ __launch_bounds__(SAMPLER_NT) void mala_propose_kernel(MalaRun a, uint64_t step, int first) {
  mala_propose_chain(a, blockIdx.x, step, first != 0);
}

// Transition `step` of every chain, given (lpp, gp) at zp: logq, the decision, the next state, sample `step` of Z / lp / G,
// the accept count, and -- in the same launch -- the proposal of transition step + 1 from the state just chosen.
// The decision's scalars are computed by every thread from the same inputs (the sums are broadcast by block_sum); thread 0 writes
// them.  lp[c] is read BEFORE the barriers of the sums: thread 0 writes it after them.
__global__ __launch_bounds__(SAMPLER_NT) void mala_accept_kernel(MalaRun a, uint64_t step, int propose_next) {
  __shared__ double red[2 * SAMPLER_WAVES];
  const int64_t c = blockIdx.x;
  const int32_t M = a.M;
  double *z = a.z + c * M, *g = a.g + c * M;
  const double *zp = a.zp + c * M, *gp = a.gp + c * M;
  const double lp_new = a.lpp[c];
  bool accept = true;
  if (step > 0) {   // (uniform over the workgroup)
    const double lp_old = a.lp[c];
    double s[2] = {0.0, 0.0};   // fwd.fwd, bwd.bwd
    for_owned(M, [&](int m) {
      const double zv = z[m], zpv = zp[m];
      const double fwd = (zpv - zv) - a.h * g[m];
      const double bwd = (zv - zpv) - a.h * gp[m];
      s[0] += fwd * fwd;
      s[1] += bwd * bwd;
    });
    block_sum(s, red);
    const double logq = -(s[1] - s[0]) / (2.0 * (a.sigma_z * a.sigma_z));
    const double e = philox_randexp(a.seed, (uint32_t)(a.chain_id0 + (int32_t)c), step);
    accept = (-e < (lp_new - lp_old) + logq);   // NaN compares false => reject
  }
  const int64_t col = (int64_t)step + a.itr * c;
  if (threadIdx.x == 0) {
    const double lp_keep = accept ? lp_new : a.lp[c];
    a.lp[c] = lp_keep;
    a.lp_out[col] = lp_keep;
    if (step == 0)
      a.nacc[c] = 0;
    else if (accept)
      a.nacc[c] += 1;
  }
  keep_and_record(M, accept ? zp : z, accept ? gp : g, z, g, a.Z_out + M * col, a.G_out ? a.G_out + M * col : nullptr);
  if (propose_next) mala_propose_chain(a, c, step + 1, false);
}

void launch_mala_propose(hipStream_t st, const MalaRun& a, int32_t C, uint64_t step, bool first) {
  hipLaunchKernelGGL(mala_propose_kernel, dim3((unsigned)C), dim3(SAMPLER_NT), 0, st, a, step, first ? 1 : 0);
}

void launch_mala_accept(hipStream_t st, const MalaRun& a, int32_t C, uint64_t step, bool propose_next) {
  hipLaunchKernelGGL(mala_accept_kernel, dim3((unsigned)C), dim3(SAMPLER_NT), 0, st, a, step, propose_next ? 1 : 0);
}

}  // namespace si
