// ADVI (reference src/space_inference.jl:126-138, AdvancedVI 0.1.3 `vi(density, ADVI(S, T), q, theta_0)` then `rand(q, D)`) with the
// variational state on the device: the step of si_fit_advi (include/subspace_hip.h holds the contract), defined once, on the
// Philox stream of philox.h.  The optimiser is that version's default TruncatedADAGrad(0.1, 1.0, 100) and the ELBO is the mean of
// the density at S draws plus the entropy of the diagonal normal [upstream, from memory, unverifiable offline].
//
//   run r draws from Philox chain chain_id0 + r: purpose 2 = the initial point, 3 = the step draws, 4 = the final draws
//   theta = [mu; omega];  theta_0 = sigma_z n (2M normals, blocks 0 .. M-1 of purpose 2, step 0)
//   step t:  sigma = exp(omega);  eta_k = block k nblk + j of (purpose 3, step t);  z_k = mu + sigma eta_k;  (lp_k, g_k) at z_k
//            H = M (log 2 pi + 1) / 2 + sum_m omega_m;  elbo_t = (((lp_0 / S + H) + lp_1 / S) + ...) + lp_{S-1} / S
//            dmu_m = -(sum_k g_k[m]) / S;  domega_m = -(sum_k (g_k[m] eta_k[m]) sigma_m) / S - 1
//            ring slot t mod W of component p = d_p^2;  s_p = the W slots in slot order;  theta_p -= d_p (eta_opt / (tau + sqrt(s_p)))
//   draws    z_i = mu_T + exp(omega_T) n_i, n_i = (purpose 4, step i)
//
// Two kernels, one workgroup of SAMPLER_NT threads per run.  The values and gradients at the points come from the caller's launches
// between them (si_fit_advi, capi_advi.hip).  Thread i owns the components m of mu AND of omega that sampler_device.h's for_owned
// gives it, in every phase after theta_0: the sums over k and over the ring's slots are sequential inside one thread, and nothing
// but sum_m omega_m crosses threads -- that sum is sampler_device.h's block_sum.  Two loops keep their own block index and are
// written out: the step draws (block k nblk + j) and theta_0 (M full blocks over 2M components).
// eta_k stays in a device buffer between the two kernels: the update uses the bits the points were made from.  The file is
// compiled without contraction of a * b + c: every product, sum and quotient is rounded by itself, as the host restatement's.
#include "sampler_device.h"

namespace si {

static constexpr double ADVI_LOG_2PI = 1.8378770664093453;   // (a literal: the host restatement must not depend on a libm's log)

// the points of `step` from theta as it stands, for the components this thread owns: eta, z = mu + exp(omega) eta, the trace copy
__device__ __forceinline__ void advi_form_points(const AdviRun& a, int64_t r, uint32_t chain, uint64_t step) {
  const int M = a.M, S = a.S, nblk = (M + 1) >> 1;
  const double* theta = a.theta + 2 * (int64_t)M * r;
  double* eta = a.eta + (int64_t)M * S * r;
  double* z = a.z + (int64_t)M * S * r;
  double* pts = a.pts_out ? a.pts_out + (int64_t)M * S * ((int64_t)step + a.T * r) : nullptr;
  // (for_owned's ownership written out: draw k of the components 2j, 2j + 1 is block k nblk + j, and exp(omega) is formed once per j)
  for (int j = threadIdx.x; j < nblk; j += SAMPLER_NT) {
    double mu[2] = {0.0, 0.0}, sg[2] = {0.0, 0.0};
    for (int c = 0; c < 2; ++c) {
      const int m = 2 * j + c;
      if (m < M) {
        mu[c] = theta[m];
        sg[c] = exp(theta[M + m]);
      }
    }
    for (int k = 0; k < S; ++k) {
      double n[2];
      philox_normal2_purpose(a.seed, chain, step, 3u, (uint32_t)(k * nblk + j), n[0], n[1]);
      for (int c = 0; c < 2; ++c) {
        const int m = 2 * j + c;
        if (m < M) {
          const double zv = mu[c] + sg[c] * n[c];
          eta[(int64_t)M * k + m] = n[c];
          z[(int64_t)M * k + m] = zv;
          if (pts) pts[(int64_t)M * k + m] = zv;
        }
      }
    }
  }
}

// first: theta_0 = sigma_z n, the ring cleared, trace column 0, the points of step 0.  final: Z_out[:, i, r] for the i of this
// workgroup's blockIdx.y.  (grid: R x 1 with first, R x min(D, 128) with final)
__global__ __launch_bounds__(SAMPLER_NT) void advi_draw_kernel(AdviRun a, double sigma_z, int first, int final, double* __restrict__ Z_out,
                                                            int64_t D) {
  const int64_t r = blockIdx.x;
  const int tid = threadIdx.x;
  const int M = a.M;
  const uint32_t chain = (uint32_t)(a.chain_id0 + (int32_t)r);
  double* theta = a.theta + 2 * (int64_t)M * r;
  if (first) {
    double* trace = a.trace_out ? a.trace_out + 2 * (int64_t)M * (a.T + 1) * r : nullptr;
    for (int j = tid; j < M; j += SAMPLER_NT) {   // (not for_owned: 2M components in M full blocks, none ragged, block by block)
      double n[2];
      philox_normal2_purpose(a.seed, chain, 0, 2u, (uint32_t)j, n[0], n[1]);
      for (int c = 0; c < 2; ++c) {
        const double v = sigma_z * n[c];
        theta[2 * j + c] = v;
        if (trace) trace[2 * j + c] = v;
      }
    }
    double* ring = a.ring + (int64_t)a.W * 2 * M * r;
    for (int64_t i = tid; i < (int64_t)a.W * 2 * M; i += SAMPLER_NT) ring[i] = 0.0;
    __syncthreads();   // (theta_0 was written block by block, the points read it component by component)
    advi_form_points(a, r, chain, 0);
  }
  if (final) {
    for (int64_t i = blockIdx.y; i < D; i += gridDim.y) {
      double* zo = Z_out + (int64_t)M * (i + D * r);
      for_owned_normal(M, a.seed, chain, (uint64_t)i, 4u, [&](int m, double n) { zo[m] = theta[m] + exp(theta[M + m]) * n; });
    }
  }
}

// Step t of every run, given (lp_k, g_k) at its points: elbo_t, d, the ring write, s, theta_{t+1}, the trace column t + 1 and --
// in the same launch -- the points of step t + 1 from the state just written.
__global__ __launch_bounds__(SAMPLER_NT) void advi_update_kernel(AdviRun a, const double* __restrict__ lp, const double* __restrict__ g,
                                                              double eta_opt, double tau, int64_t t, double* __restrict__ elbo_out,
                                                              int form_next) {
  __shared__ double red[SAMPLER_WAVES];
  const int64_t r = blockIdx.x;
  const int M = a.M, S = a.S, W = a.W;
  const uint32_t chain = (uint32_t)(a.chain_id0 + (int32_t)r);
  double* theta = a.theta + 2 * (int64_t)M * r;
  const double* eta = a.eta + (int64_t)M * S * r;
  g += (int64_t)M * S * r;
  lp += (int64_t)S * r;
  const double Sd = (double)S;
  if (elbo_out) {
    double so = 0.0;
    for_owned(M, [&](int m) { so += theta[M + m]; });
    so = block_sum<true>(so, red);   // (elbo_out is a kernel argument: the whole workgroup reaches the barrier or none of it does)
    if (threadIdx.x == 0) {
      const double H = ((double)M * (ADVI_LOG_2PI + 1.0)) / 2.0 + so;
      double e = lp[0] / Sd + H;
      for (int k = 1; k < S; ++k) e += lp[k] / Sd;
      elbo_out[t + a.T * r] = e;
    }
    // (no barrier before omega is overwritten below: every thread added its own components only)
  }
  double* ring = a.ring + (int64_t)W * 2 * M * r;
  double* trace = a.trace_out ? a.trace_out + 2 * (int64_t)M * ((t + 1) + (a.T + 1) * r) : nullptr;
  const int slot = (int)(t % W);
  for_owned(M, [&](int m) {
    const double sg = exp(theta[M + m]);
    double sm = 0.0, sw = 0.0;
    for (int k = 0; k < S; ++k) {
      const double gv = g[(int64_t)M * k + m];
      sm += gv;
      sw += (gv * eta[(int64_t)M * k + m]) * sg;
    }
    const double d[2] = {-(sm / Sd), -(sw / Sd) - 1.0};
    for (int h = 0; h < 2; ++h) {
      const int p = h * M + m;
      ring[(int64_t)slot * 2 * M + p] = d[h] * d[h];
      double s = 0.0;
      for (int w = 0; w < W; ++w) s += ring[(int64_t)w * 2 * M + p];
      const double v = theta[p] - d[h] * (eta_opt / (tau + sqrt(s)));
      theta[p] = v;
      if (trace) trace[p] = v;
    }
  });
  // (the thread that wrote mu_m and omega_m is the one that reads them here: no barrier)
  if (form_next) advi_form_points(a, r, chain, (uint64_t)(t + 1));
}

void launch_advi_draw(hipStream_t st, const AdviRun& a, int32_t R, double sigma_z, bool first, bool final, double* Z_out, int64_t D) {
  // (first writes theta: one workgroup per run; the draws only read it and are spread over grid.y)
  const unsigned gy = final && !first ? (unsigned)std::min<int64_t>(std::max<int64_t>(D, 1), 128) : 1u;
  hipLaunchKernelGGL(advi_draw_kernel, dim3((unsigned)R, gy), dim3(SAMPLER_NT), 0, st, a, sigma_z, first ? 1 : 0, final ? 1 : 0, Z_out, D);
}

void launch_advi_update(hipStream_t st, const AdviRun& a, int32_t R, const double* lp, const double* g, double eta_opt, double tau,
                        int64_t t, double* elbo_out, bool form_next) {
  hipLaunchKernelGGL(advi_update_kernel, dim3((unsigned)R), dim3(SAMPLER_NT), 0, st, a, lp, g, eta_opt, tau, t, elbo_out, form_next ? 1 : 0);
}

}  // namespace si
