// Device functions that kernels_mala.hip, kernels_hmc.hip, kernels_nuts.hip and kernels_advi.hip share, each defined once so that
// the four samplers cannot drift apart: which thread owns which component of a chain, the fixed-order sum over a chain's components,
// the state a transition keeps written as the chain's state and as a column of the outputs, the half kick and drift of a leapfrog
// step, and the Stan adaptor's update after a transition (samplers.StanAdaptor.adapt).
//
// THE CONTRACT every audit and every "a chain's bits do not depend on the call" test rests on: one workgroup of SAMPLER_NT threads
// per chain; thread i owns the components 2j, 2j + 1 of its Philox blocks j = i, i + SAMPLER_NT, ... and visits them in that order
// (for_owned, for_owned_normal); a sum over m adds each thread's components in that order, the wave sums are chain_wave_sum's and
// the four wave sums are added as (r0 + r1) + (r2 + r3) (block_sum) -- so a chain's bits depend on M alone, not on the number of
// chains, its column, the pass or the run.  Compiled without contraction of a * b + c by all four translation units.
#pragma once
#include "chain_common.h"
#include "philox.h"
#include "si_internal.h"

namespace si {

static constexpr int SAMPLER_NT = 256;
static constexpr int SAMPLER_WAVES = SAMPLER_NT / 64;
static_assert(SAMPLER_WAVES == 4, "block_sum adds four wave sums as (r0 + r1) + (r2 + r3)");
static constexpr uint32_t HMC_P_MOMENTUM = 5u, HMC_P_SEARCH = 6u;

// f(m) for every component m < M that this thread owns: j ascending, 2j then 2j + 1.  (The pair is unrolled by request: left to
// itself the compiler keeps a loop of two around a large body -- advi_update_kernel's -- where the written-out loop had two copies,
// and a step of si_fit_advi at M = 20 took 435 us instead of 432.5.)
template <class F>
__device__ __forceinline__ void for_owned(int32_t M, F&& f) {
  const int nblk = (M + 1) >> 1;
  for (int j = threadIdx.x; j < nblk; j += SAMPLER_NT) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int m = 2 * j + k;
      if (m < M) f(m);
    }
  }
}

// f(m, n) likewise, n = the normal of component m: element m & 1 of block m >> 1 of (seed, chain, step, purpose), drawn once per block
template <class F>
__device__ __forceinline__ void for_owned_normal(int32_t M, uint64_t seed, uint32_t chain, uint64_t step, uint32_t purpose, F&& f) {
  const int nblk = (M + 1) >> 1;
  for (int j = threadIdx.x; j < nblk; j += SAMPLER_NT) {
    double n[2];
    philox_normal2_purpose(seed, chain, step, purpose, (uint32_t)j, n[0], n[1]);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int m = 2 * j + k;
      if (m < M) f(m, n[k]);
    }
  }
}

// v[i] = the sum of every thread's v[i] in the fixed order, for N = 1 or 2 values at once; every thread gets it.  red: N *
// SAMPLER_WAVES doubles of LDS.  Two barriers whatever N, both reached by every thread of the workgroup: red may be reused right
// after, and what a thread read before the call was read before any thread goes on.  RED_UNUSED: nothing in this launch has read
// red yet, so the first barrier is left out (advi_update_kernel's one sum: its step is short enough for a barrier to show).
template <int N, bool RED_UNUSED = false>
__device__ __forceinline__ void block_sum(double (&v)[N], double* red) {
  static_assert(N == 1 || N == 2, "one sum, or a pair behind one pair of barriers");
  for (int i = 0; i < N; ++i) v[i] = chain_wave_sum(v[i]);
  if (!RED_UNUSED) __syncthreads();
  if ((threadIdx.x & 63) == 0)
    for (int i = 0; i < N; ++i) red[SAMPLER_WAVES * i + (threadIdx.x >> 6)] = v[i];
  __syncthreads();
  for (int i = 0; i < N; ++i) {
    const double* r = red + SAMPLER_WAVES * i;
    v[i] = (r[0] + r[1]) + (r[2] + r[3]);
  }
}

template <bool RED_UNUSED = false>
__device__ __forceinline__ double block_sum(double v, double* red) {
  double a[1] = {v};
  block_sum<1, RED_UNUSED>(a, red);
  return a[0];
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

// The metric's window of a chain after a transition, for keep_and_record: null minv = the sampler has no metric (MALA)
struct AdaptWindow {
  double *minv = nullptr, *wmean = nullptr, *wm2 = nullptr;   // the chain's M each
  bool update = false;                                        // the step is inside a window: hmc_adapt_component with the kept z
  double wn = 0.0;                                            // the window's count INCLUDING this step
  int window_close = 0;
};

// The point (zk, gk) a transition keeps -- the proposal, the state itself or NUTS's candidate -- becomes the chain's state (z, g) and
// the column of the outputs that starts at Z_col / G_col / Minv_col (G_col, Minv_col may be null); Minv_col gets the metric the
// transition USED, then the window takes the kept z.  Every thread touches its own components only: no barrier.
__device__ __forceinline__ void keep_and_record(int32_t M, const double* zk, const double* gk, double* z, double* g, double* Z_col,
                                                double* G_col, double* Minv_col = nullptr, const AdaptWindow& w = AdaptWindow()) {
  for_owned(M, [&](int m) {
    const double zv = zk[m], gv = gk[m];
    z[m] = zv;
    g[m] = gv;
    Z_col[m] = zv;
    if (G_col) G_col[m] = gv;
    if (Minv_col) Minv_col[m] = w.minv[m];
    if (w.update) hmc_adapt_component(m, zv, w.wn, w.window_close, w.minv, w.wmean, w.wm2);
  });
}

// the same for column `col` of the outputs of chain c of an HMC / NUTS run; update: the step is inside a window of the metric
__device__ __forceinline__ void keep_and_record(const HmcRun& a, int64_t c, int64_t col, const double* zk, const double* gk,
                                                bool update = false, double wn = 0.0, int window_close = 0) {
  const int64_t s = c * a.M, o = (int64_t)a.M * col;
  keep_and_record(a.M, zk, gk, a.z + s, a.g + s, a.Z_out + o, a.G_out ? a.G_out + o : nullptr, a.Minv_out ? a.Minv_out + o : nullptr,
                  AdaptWindow{a.minv + s, a.wmean + s, a.wm2 + s, update, wn, window_close});
}

}  // namespace si
