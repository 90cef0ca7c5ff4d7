// HMC (reference src/space_inference.jl:139-160: AdvancedHMC 0.2.27 `StaticTrajectory(Leapfrog(eps), 1)` under `StanHMCAdaptor`) with
// the chain's position, momentum, step size, metric and adaptor state on the device: samplers.hmc + samplers.StanAdaptor +
// samplers.find_good_stepsize as they stand [upstream, unverifiable offline], defined once, on the Philox stream of philox.h.
//
//   chain c draws from Philox chain chain_id0 + c:  purpose 0, step 0 = the initial point's normals (MALA's z_0);  purpose 1, step t,
//   block 0 = u_t = u53(x1, x0) (the draw whose -log is MALA's e_t);  purpose 5, step t = the momentum normals n_t;  purpose 6,
//   step 0 = the momentum rho of the step-size search.
//
//   z_0 = sigma_z n(p0, 0);  (lp_0, g_0) at z_0;  Minv = 1
//   search   h0 = lp_0 - 1/2 rho.rho;  dH(e) = lpp - 1/2 rp.rp - h0 after one leapfrog step of size e from (z_0, rho)
//            eps = 0.1;  direction = dH(eps) > log 0.5 ? +1 : -1
//            crossing, at most 100 times:  eps' = direction > 0 ? 2 eps : eps / 2;  d = dH(eps)  (at the OLD eps, as upstream)
//                      stop when d is no longer on the starting side of log 0.5 (a NaN stops), else eps = eps'
//            (lo, hi) = (eps, eps') sorted;  bisection, at most 100 times:  mid = (lo + hi) / 2;  a = exp(dH(mid))
//                      a > 0.75: lo = mid;  a < 0.25: hi = mid;  else lo = mid and stop (a NaN lands here)
//            eps_0 = lo;  the adaptor starts with mu = log(10 eps_0), hbar = log_eps_bar = 0, count 0, empty window
//   t >= 1   with the adaptor's current (eps, Minv):
//            r = n_t / sqrt(Minv);  K0 = 1/2 sum (Minv r) r
//            rh = r + (eps / 2) g;  zp = z + eps (Minv rh);  (lpp, gp) at zp;  rp = rh + (eps / 2) gp;  K1 = 1/2 sum (Minv rp) rp
//            dH = (lpp - K1) - (lp - K0);  a = 0 if lpp - K1 is not finite, 1 if dH >= 0, else exp(dH)
//            accept iff u_t < a: (z, lp, g) = (zp, lpp, gp)
//            column t of Z / lp / G = the state;  alpha[t] = a;  eps[t] = eps;  Minv_out[:, t] = Minv  (those USED by transition t)
//            t <= n_adapts: the adaptor's update with (z, a) -- dual averaging (gamma 0.05, t0 10, kappa 0.75) on every step; inside a
//            window the Welford update with the KEPT state; at a window's close Minv = n / (n + 5) var + 1e-3 5 / (n + 5) (n >= 2),
//            the window emptied and the dual averaging restarted at the current eps; after step n_adapts eps = exp(log_eps_bar)
//
// Kernels: one workgroup of SAMPLER_NT threads per chain; the value and gradient at the trial points and proposals come from the
// caller's launches between them (si_sample_hmc, capi_hmc.hip).  Component ownership, the fixed order of every sum over m, the
// keep-and-record step, the half kick and drift and the adaptor's update are sampler_device.h's, shared with the other samplers -- a
// chain's bits depend on M alone, not on the number of chains, its column, the pass or the run.  Which phase of the adaptation a step
// is in is the host's knowledge and arrives as kernel arguments; there is no schedule on the device.  Compiled without contraction
// of a * b + c, like kernels_mala.hip.
#include "sampler_device.h"

namespace si {

static constexpr int HMC_MAX_ITER = 100;
enum { HMC_S_START = 0, HMC_S_DIRECTION = 1, HMC_S_CROSS = 2, HMC_S_BISECT = 3 };

// the proposal of transition `step` from the chain's state: r, K0 (into ch->k0 by thread 0), rh, zp
__device__ __forceinline__ void hmc_propose_chain(const double* __restrict__ z, const double* __restrict__ g, double* __restrict__ zp,
                                                  double* __restrict__ rh, const double* __restrict__ minv, HmcChain* ch, double eps,
                                                  int32_t M, uint64_t seed, uint32_t chain, uint64_t step, double* red) {
  double kk = 0.0;
  for_owned_normal(M, seed, chain, step, HMC_P_MOMENTUM, [&](int m, double n) {
    const double mi = minv[m];
    kk += hmc_kick_drift(m, n / sqrt(mi), eps, mi, z, g, rh, zp);
  });
  const double ksum = block_sum(kk, red);
  if (threadIdx.x == 0) ch->k0 = 0.5 * ksum;
}

// 1/2 sum (minv rp) rp with rp = rh + (e / 2) gp
__device__ __forceinline__ double hmc_kinetic_after(const double* __restrict__ rh, const double* __restrict__ gp,
                                                    const double* __restrict__ minv, double e, int32_t M, double* red) {
  double kk = 0.0;
  for_owned(M, [&](int m) {
    const double rp = rh[m] + (0.5 * e) * gp[m];
    kk += (minv[m] * rp) * rp;
  });
  return 0.5 * block_sum(kk, red);
}

__global__ __launch_bounds__(SAMPLER_NT) void hmc_init_kernel(HmcRun a) {
  const int64_t c = blockIdx.x;
  double* zp = a.zp + c * a.M;
  for_owned_normal(a.M, a.seed, (uint32_t)(a.chain_id0 + (int32_t)c), 0, 0u, [&](int m, double n) { zp[m] = a.sigma_z * n; });
  if (threadIdx.x == 0) {
    HmcChain& ch = a.chain[c];
    ch.s_phase = HMC_S_START;
    ch.s_done = 0;
    ch.s_iter = 0;
    ch.s_dir = 0;
  }
}

// One round of the step-size search of every chain: the state machine consumes (lpp, gp) at the last trial point and forms the next
// trial point in zp.  A finished chain returns at once and keeps its last point.
__global__ __launch_bounds__(SAMPLER_NT) void hmc_search_kernel(HmcRun a, int32_t* __restrict__ open) {
  __shared__ double red[SAMPLER_WAVES];
  __shared__ double trial_s;
  __shared__ int done_s;
  const int64_t c = blockIdx.x;
  const int tid = threadIdx.x;
  const int32_t M = a.M;
  const uint32_t chain = (uint32_t)(a.chain_id0 + (int32_t)c);
  HmcChain* ch = a.chain + c;
  if (ch->s_done) return;   // (uniform over the workgroup: written by thread 0 of an earlier launch)
  double *z = a.z + c * M, *g = a.g + c * M, *zp = a.zp + c * M, *rh = a.rh + c * M, *minv = a.minv + c * M;
  const double* gp = a.gp + c * M;
  const int phase = ch->s_phase;
  const double lpp = a.lpp[c];
  if (phase == HMC_S_START) {
    // (lpp, gp) are the value and gradient at z_0 = zp: the chain's state, column 0 of the outputs, H at (z_0, rho)
    double rr = 0.0;
    for_owned_normal(M, a.seed, chain, 0, HMC_P_SEARCH, [&](int m, double n) {
      minv[m] = 1.0;
      a.wmean[c * M + m] = 0.0;
      a.wm2[c * M + m] = 0.0;
      rr += n * n;
    });
    keep_and_record(a, c, (a.itr + 1) * c, zp, gp);
    const double rsum = block_sum(rr, red);
    if (tid == 0) {
      a.lp[c] = lpp;
      a.lp_out[(a.itr + 1) * c] = lpp;
      a.alpha_out[(a.itr + 1) * c] = 0.0;
      ch->s_h0 = lpp - 0.5 * rsum;
      ch->s_eps = 0.1;
      ch->s_next = 0.1;
      ch->s_phase = HMC_S_DIRECTION;
      trial_s = 0.1;
      done_s = 0;
    }
  } else {
    // dH of the trial just evaluated: rh holds rho + (e / 2) g_0 for the trial's e
    const double k1 = hmc_kinetic_after(rh, gp, minv, ch->s_trial, M, red);
    if (tid == 0) {
      const double d = (lpp - k1) - ch->s_h0;
      const double log_cross = -0.6931471805599453;   // log 0.5
      double eps = ch->s_eps, nxt = ch->s_next, lo = ch->s_lo, hi = ch->s_hi;
      int ph = phase, dir = ch->s_dir, it = ch->s_iter, done = 0;
      double trial = eps;
      bool bracket = false;
      if (ph == HMC_S_DIRECTION) {
        dir = d > log_cross ? 1 : -1;
        it = 0;
        nxt = dir == 1 ? 2.0 * eps : 0.5 * eps;
        ph = HMC_S_CROSS;
        trial = eps;
      } else if (ph == HMC_S_CROSS) {
        ++it;
        if ((dir == 1 && !(d > log_cross)) || (dir == -1 && !(d < log_cross))) {
          bracket = true;
        } else {
          eps = nxt;
          if (it >= HMC_MAX_ITER) {
            bracket = true;
          } else {
            nxt = dir == 1 ? 2.0 * eps : 0.5 * eps;
            trial = eps;
          }
        }
        if (bracket) {
          if (eps < nxt) {
            lo = eps;
            hi = nxt;
          } else {
            lo = nxt;
            hi = eps;
          }
          it = 0;
          ph = HMC_S_BISECT;
          trial = 0.5 * (lo + hi);
        }
      } else {   // HMC_S_BISECT: the trial was mid = (lo + hi) / 2
        const double mid = ch->s_trial;
        const double acc = exp(d);
        ++it;
        if (acc > 0.75) {
          lo = mid;
        } else if (acc < 0.25) {
          hi = mid;
        } else {
          lo = mid;
          done = 1;
        }
        if (it >= HMC_MAX_ITER) done = 1;
        trial = 0.5 * (lo + hi);
      }
      ch->s_eps = eps;
      ch->s_next = nxt;
      ch->s_lo = lo;
      ch->s_hi = hi;
      ch->s_phase = ph;
      ch->s_dir = dir;
      ch->s_iter = it;
      if (done) {
        ch->s_done = 1;
        ch->eps = lo;
        ch->mu = log(10.0 * lo);
        ch->hbar = 0.0;
        ch->log_eps_bar = 0.0;
        ch->da_t = 0;
        ch->wn = 0;
        a.eps_out[(a.itr + 1) * c] = lo;
      }
      trial_s = trial;
      done_s = done;
    }
  }
  __syncthreads();
  if (done_s) return;
  const double e = trial_s;
  for_owned_normal(M, a.seed, chain, 0, HMC_P_SEARCH, [&](int m, double n) { (void)hmc_kick_drift(m, n, e, 1.0, z, g, rh, zp); });
  if (tid == 0) {
    ch->s_trial = e;
    atomicAdd(open, 1);
  }
}

__global__ __launch_bounds__(SAMPLER_NT) void hmc_propose_kernel(HmcRun a, uint64_t step) {
  __shared__ double red[SAMPLER_WAVES];
  const int64_t c = blockIdx.x;
  const int32_t M = a.M;
  HmcChain* ch = a.chain + c;
  hmc_propose_chain(a.z + c * M, a.g + c * M, a.zp + c * M, a.rh + c * M, a.minv + c * M, ch, ch->eps, M, a.seed,
                    (uint32_t)(a.chain_id0 + (int32_t)c), step, red);
}

// Transition `step` of every chain given (lpp, gp) at zp: K1, a, the decision, the next state, column `step` of the outputs, the
// adaptor's update and -- in the same launch -- the proposal of transition step + 1 from the state and the (eps, Minv) just set.
__global__ __launch_bounds__(SAMPLER_NT) void hmc_accept_kernel(HmcRun a, uint64_t step, int adapting, int in_window, int window_close,
                                                            int last_adapt, int propose_next) {
  __shared__ double red[SAMPLER_WAVES];
  __shared__ int accept_s;
  __shared__ double eps_next_s, wn_s;
  const int64_t c = blockIdx.x;
  const int tid = threadIdx.x;
  const int32_t M = a.M;
  const uint32_t chain = (uint32_t)(a.chain_id0 + (int32_t)c);
  HmcChain* ch = a.chain + c;
  double *z = a.z + c * M, *g = a.g + c * M, *zp = a.zp + c * M, *rh = a.rh + c * M, *minv = a.minv + c * M;
  const double* gp = a.gp + c * M;
  const double eps = ch->eps;
  const int64_t col = (int64_t)step + (a.itr + 1) * c;
  const double k1 = hmc_kinetic_after(rh, gp, minv, eps, M, red);
  if (tid == 0) {
    const double lp_new = a.lpp[c], lp_old = a.lp[c];
    const double h1 = lp_new - k1, h0 = lp_old - ch->k0;
    const double dh = h1 - h0;
    const double alpha = isfinite(h1) ? (dh >= 0.0 ? 1.0 : exp(dh)) : 0.0;
    const Philox4 x = philox_draw(a.seed, chain, step, 1u, 0u);
    const bool accept = u53(x.v[1], x.v[0]) < alpha;   // (a NaN alpha compares false: reject)
    const double lp_keep = accept ? lp_new : lp_old;
    a.lp[c] = lp_keep;
    a.lp_out[col] = lp_keep;
    a.alpha_out[col] = alpha;
    a.eps_out[col] = eps;
    accept_s = accept ? 1 : 0;
    double e_next;
    int64_t wn;
    hmc_adapt_scalars(ch, a.delta, alpha, eps, adapting, in_window, window_close, last_adapt, e_next, wn);
    eps_next_s = e_next;
    wn_s = (double)wn;
  }
  __syncthreads();
  const bool accept = accept_s != 0;
  // (thread i owns the same components in every phase: nothing below reads what another thread writes)
  keep_and_record(a, c, col, accept ? zp : z, accept ? gp : g, adapting && in_window, wn_s /* INCLUDING this step */, window_close);
  if (propose_next) hmc_propose_chain(z, g, zp, rh, minv, ch, eps_next_s, M, a.seed, chain, step + 1, red);
}

void launch_hmc_init(hipStream_t st, const HmcRun& a, int32_t C) {
  hipLaunchKernelGGL(hmc_init_kernel, dim3((unsigned)C), dim3(SAMPLER_NT), 0, st, a);
}

void launch_hmc_search(hipStream_t st, const HmcRun& a, int32_t C, int32_t* open) {
  hipLaunchKernelGGL(hmc_search_kernel, dim3((unsigned)C), dim3(SAMPLER_NT), 0, st, a, open);
}

void launch_hmc_propose(hipStream_t st, const HmcRun& a, int32_t C, uint64_t step) {
  hipLaunchKernelGGL(hmc_propose_kernel, dim3((unsigned)C), dim3(SAMPLER_NT), 0, st, a, step);
}

void launch_hmc_accept(hipStream_t st, const HmcRun& a, int32_t C, uint64_t step, bool adapting, bool in_window, bool window_close,
                       bool last_adapt, bool propose_next) {
  hipLaunchKernelGGL(hmc_accept_kernel, dim3((unsigned)C), dim3(SAMPLER_NT), 0, st, a, step, adapting ? 1 : 0, in_window ? 1 : 0,
                     window_close ? 1 : 0, last_adapt ? 1 : 0, propose_next ? 1 : 0);
}

}  // namespace si
