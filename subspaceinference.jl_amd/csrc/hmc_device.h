// Device functions that kernels_hmc.hip and kernels_nuts.hip share: the fixed-order sum over a chain's components, the half kick and
// drift of a leapfrog step, and the Stan adaptor's update after a transition (samplers.StanAdaptor.adapt) -- each defined once, so
// that the two samplers cannot drift apart.  Compiled without contraction of a * b + c by both translation units.
#pragma once
#include "chain_common.h"
#include "si_internal.h"

namespace si {

static constexpr int HMC_NT = 256;
static constexpr uint32_t HMC_P_MOMENTUM = 5u, HMC_P_SEARCH = 6u;

// the sum of every thread's v in the fixed order; every thread gets it.  (Two barriers: red may be reused right after.)
__device__ __forceinline__ double hmc_block_sum(double v, double* red) {
  v = chain_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// rh = r + (e / 2) g,  zp = z + e (minv rh)  for the thread's components; returns its share of 1/2-less sum (minv r) r
__device__ __forceinline__ double hmc_kick_drift(int m, double r, double e, double mi, const double* __restrict__ z,
                                                 const double* __restrict__ g, double* __restrict__ rh, double* __restrict__ zp) {
  const double h = r + (0.5 * e) * g[m];
  rh[m] = h;
  zp[m] = z[m] + e * (mi * h);
  return (mi * r) * r;
}

// The adaptor's scalars after a transition with acceptance statistic alpha at step size eps (ONE thread of the chain's workgroup):
// the dual averaging, the window's count, the restart at a window's close, the averaged step size after the last adaptation step.
// e_next: the step size of the next transition;  wn: the window's count INCLUDING this step.
__device__ __forceinline__ void hmc_adapt_scalars(HmcChain* ch, double delta, double alpha, double eps, int adapting, int in_window,
                                                  int window_close, int last_adapt, double& e_next_out, int64_t& wn_out) {
  double e_next = eps;
  int64_t wn = ch->wn;
  if (adapting) {
    // Nesterov dual averaging of log eps towards the acceptance delta
    const double gamma = 0.05, t0 = 10.0, kappa = 0.75;
    const int64_t t = ++ch->da_t;
    const double acc = alpha < 1.0 ? alpha : 1.0;
    const double td = (double)t;
    ch->hbar = (1.0 - 1.0 / (td + t0)) * ch->hbar + (delta - acc) / (td + t0);
    const double log_eps = ch->mu - sqrt(td) / gamma * ch->hbar;
    const double eta = pow(td, -kappa);
    ch->log_eps_bar = eta * log_eps + (1.0 - eta) * ch->log_eps_bar;
    e_next = exp(700.0 < log_eps ? 700.0 : log_eps);   // (min(log_eps, 700) as the host forms it: a NaN stays)
    if (in_window) {
      wn += 1;
      if (window_close) {   // (the restart: at the eps just set)
        ch->mu = log(10.0 * e_next);
        ch->hbar = 0.0;
        ch->log_eps_bar = 0.0;
        ch->da_t = 0;
      }
    }
    if (last_adapt && ch->da_t > 0) e_next = exp(700.0 < ch->log_eps_bar ? 700.0 : ch->log_eps_bar);
    ch->eps = e_next;
    ch->wn = (in_window && window_close) ? 0 : wn;
  }
  e_next_out = e_next;
  wn_out = wn;
}

// Component m of the metric's window after a transition that kept zv (the thread that owns m; only inside a window): the Welford
// update, and at the window's close the regularised variance into minv and the window emptied
__device__ __forceinline__ void hmc_adapt_component(int m, double zv, double wn, int window_close, double* __restrict__ minv,
                                                    double* __restrict__ wmean, double* __restrict__ wm2) {
  const double dlt = zv - wmean[m];
  const double mean = wmean[m] + dlt / wn;
  const double m2 = wm2[m] + dlt * (zv - mean);
  if (window_close) {
    if (wn >= 2.0) minv[m] = (wn / (wn + 5.0)) * (m2 / (wn - 1.0)) + 1e-3 * (5.0 / (wn + 5.0));
    wmean[m] = 0.0;
    wm2[m] = 0.0;
  } else {
    wmean[m] = mean;
    wm2[m] = m2;
  }
}

}  // namespace si
