// NUTS (reference src/space_inference.jl:139-160: AdvancedHMC 0.2.27 `NUTS{MultinomialTS, GeneralisedNoUTurn}(Leapfrog(eps))` under
// `StanHMCAdaptor`) with the trajectory tree, the step size, the metric and the adaptor state on the device: samplers.nuts_iter --
// the leaf-by-leaf restatement of samplers.nuts [upstream, unverifiable offline] -- on the Philox stream of philox.h.  Column 0, the
// step-size search and the adaptor are si_sample_hmc's (kernels_hmc.hip, sampler_device.h), shared, not copied.
//
//   chain c draws from Philox chain chain_id0 + c:  purposes 0, 5, 6 as si_sample_hmc;  purpose 7, step t, block j = the doubling at
//   depth j: direction +1 iff u53(x1, x0) < 0.5, progressive pick with u53(x3, x2);  purpose 8, step t, block 16 leaf + level = the
//   pick of the merge at `level` after leaf `leaf` (the running leaf count of the transition), u53(x1, x0).
//
//   begin    r0 = n_t / sqrt(Minv);  h0 = lp - 1/2 sum (Minv r0) r0;  both ends = (z, r0, g);  rho = r0;  logw = 0;  candidate = state
//   doubling at depth j = 0, 1, ...: direction v; 2^j leaves from the tree's end on the side of v, each one leapfrog step of size v eps:
//            rh = r + (v eps / 2) g;  z1 = z + v eps (Minv rh);  (lp1, g1) at z1;  r1 = rh + (v eps / 2) g1
//            h1 = lp1 - 1/2 sum (Minv r1) r1, -inf if not finite;  dh = h1 - h0;  alpha = 1 unless dh < 0, then min(1, exp(dh))
//            the leaf is pushed as a sub-tree (first r = r1, rho = r1, proposal = the leaf, logw = dh, alpha, n = 1)
//            divergent ((-dh) > max_dh): stop.  Else for every trailing zero bit of the leaf's number k within the doubling, at
//            level 1, 2, ...: the top two entries a (below), b (top) merge: logw = logaddexp(a.logw, b.logw);  the proposal becomes
//            b's iff log u < b.logw - logw;  rho = a.rho + b.rho;  alpha, n add;  stop iff rho . (Minv r-) <= 0 or rho . (Minv r+) <= 0
//            with r-/r+ = the sub-tree's ends (a's first r and the leaf just made, ordered by v)
//            on a stop the entries under the stopped one fold into it from the top down (alpha = below + top, n likewise)
//   end of a doubling (k = 2^j, one entry `sub`):  alpha_sum += sub.alpha;  n_alpha += sub.n;  candidate = sub's proposal iff
//            log u < sub.logw - logw;  rho += sub.rho;  logw = logaddexp(logw, sub.logw);  the transition ends iff the tree's ends
//            make a U-turn or j + 1 = max_depth.  A stop inside the doubling ends it after alpha_sum / n_alpha took the folded entry.
//   end      state = candidate;  a = alpha_sum / max(1, n_alpha);  column t of the outputs;  the adaptor's update with (z, a)
//
// Where things live: the tree's ends, rho, the candidate and the stack's vectors (4 M doubles per entry) are in global memory, M x C
// arrays that stay in L2 between the rounds -- at M = 513 one chain's stack alone is 164 KB, more than a workgroup's LDS, and every
// round is a separate launch anyway, so nothing could stay in LDS or registers from one leaf to the next.  Thread i owns the
// same components in every phase (sampler_device.h's ownership: for_owned), so no vector element is read by a thread other
// than the one that wrote it: merges are component-parallel and need no barrier apart from block_sum's.  Every
// scalar of the tree is computed redundantly by every thread from the same inputs (the sums are broadcast by block_sum) and kept
// in registers through the launch; thread 0 writes them back.  Entries below the top were written by earlier launches.
// Compiled without contraction of a * b + c, like kernels_hmc.hip.
#include "sampler_device.h"

namespace si {

static constexpr uint32_t NUTS_P_DOUBLING = 7u, NUTS_P_MERGE = 8u;

// max + log1p(exp(-|a - b|)); -inf when both are
__device__ __forceinline__ double nuts_logaddexp(double a, double b) {
  const double mx = a > b ? a : b;
  if (mx == -INFINITY) return mx;
  return mx + log1p(exp(-fabs(a - b)));
}

__device__ __forceinline__ int nuts_direction(uint64_t seed, uint32_t chain, uint64_t step, int depth) {
  const Philox4 x = philox_draw(seed, chain, step, NUTS_P_DOUBLING, (uint32_t)depth);
  return u53(x.v[1], x.v[0]) < 0.5 ? 1 : -1;
}

struct NutsPtrs {
  double *zm, *rm, *gm, *zq, *rq, *gq, *rho, *zc, *gc, *stack;
};

__device__ __forceinline__ NutsPtrs nuts_ptrs(const NutsRun& n, int64_t c, int32_t M) {
  return NutsPtrs{n.zm + c * M, n.rm + c * M, n.gm + c * M, n.zq + c * M, n.rq + c * M, n.gq + c * M, n.rho + c * M,
                  n.zc + c * M, n.gc + c * M, n.stack + c * (4 * (int64_t)M * NUTS_MAX_DEPTH)};
}

// the pending point of the next leaf: half kick and drift of size v eps from the tree's end on the side of v
__device__ __forceinline__ void nuts_next_point(const NutsPtrs& p, int dir, double eps, const double* __restrict__ minv,
                                                double* __restrict__ rh, double* __restrict__ zp, int32_t M) {
  const double* ez = dir > 0 ? p.zq : p.zm;
  const double* er = dir > 0 ? p.rq : p.rm;
  const double* eg = dir > 0 ? p.gq : p.gm;
  const double ve = (double)dir * eps;
  for_owned(M, [&](int m) { (void)hmc_kick_drift(m, er[m], ve, minv[m], ez, eg, rh, zp); });
}

__global__ __launch_bounds__(SAMPLER_NT) void nuts_begin_kernel(HmcRun a, NutsRun n, uint64_t step, int first) {
  __shared__ double red[SAMPLER_WAVES];
  const int64_t c = blockIdx.x;
  const int32_t M = a.M;
  const uint32_t chain = (uint32_t)(a.chain_id0 + (int32_t)c);
  const HmcChain* ch = a.chain + c;
  NutsChain* tr = n.tree + c;
  const NutsPtrs p = nuts_ptrs(n, c, M);
  const double *z = a.z + c * M, *g = a.g + c * M, *minv = a.minv + c * M;
  double kk = 0.0;
  for_owned_normal(M, a.seed, chain, step, HMC_P_MOMENTUM, [&](int m, double nn) {
    const double mi = minv[m], r = nn / sqrt(mi), zv = z[m], gv = g[m];
    kk += (mi * r) * r;
    p.zm[m] = zv, p.zq[m] = zv, p.zc[m] = zv;
    p.gm[m] = gv, p.gq[m] = gv, p.gc[m] = gv;
    p.rm[m] = r, p.rq[m] = r, p.rho[m] = r;
  });
  const double ksum = block_sum(kk, red);
  const int dir = nuts_direction(a.seed, chain, step, 0);
  if (threadIdx.x == 0) {
    const double lp = a.lp[c];
    tr->h0 = lp - 0.5 * ksum;
    tr->logw = 0.0;
    tr->lpc = lp;
    tr->alpha_sum = 0.0;
    tr->n_alpha = 0;
    tr->depth = 0;
    tr->ndoub = 1;
    tr->dir = dir;
    tr->k = 0;
    tr->sp = 0;
    tr->nleaf = 0;
    tr->selc = 0;
    tr->open = 1;
    if (first) {
      tr->nlog = 0;
      const int64_t col0 = (a.itr + 1) * c;
      n.depth_out[col0] = 0;
      n.nleaf_out[col0] = 0;
      n.sel_out[col0] = 0;
    }
  }
  nuts_next_point(p, dir, ch->eps, minv, a.rh + c * M, a.zp + c * M, M);
}

__global__ __launch_bounds__(SAMPLER_NT) void nuts_leaf_kernel(HmcRun a, NutsRun n, uint64_t step, int32_t* __restrict__ open) {
  __shared__ double red[2 * SAMPLER_WAVES];
  const int64_t c = blockIdx.x;
  const int tid = threadIdx.x;
  const int32_t M = a.M;
  const uint32_t chain = (uint32_t)(a.chain_id0 + (int32_t)c);
  NutsChain* tr = n.tree + c;
  if (!tr->open) return;   // (uniform over the workgroup: written by thread 0 of an earlier launch)
  const NutsPtrs p = nuts_ptrs(n, c, M);
  const double *minv = a.minv + c * M, *gp = a.gp + c * M;
  double *zp = a.zp + c * M, *rh = a.rh + c * M;
  const double eps = a.chain[c].eps;
  // the tree's scalars, in every thread's registers through the launch
  const double h0 = tr->h0;
  double logw = tr->logw, lpc = tr->lpc, alpha_sum = tr->alpha_sum;
  int n_alpha = tr->n_alpha, depth = tr->depth, ndoub = tr->ndoub, dir = tr->dir, k = tr->k, sp = tr->sp, nleaf = tr->nleaf,
      selc = tr->selc;
  const int64_t nlog = tr->nlog;
  int still = 1;
  // the leaf: second half kick, onto the tree's end on the side of dir, pushed as a one-leaf sub-tree, logged
  double *ez = dir > 0 ? p.zq : p.zm, *er = dir > 0 ? p.rq : p.rm, *eg = dir > 0 ? p.gq : p.gm;
  const double ve = (double)dir * eps;
  const double lp1 = a.lpp[c];
  double* top = p.stack + (int64_t)sp * 4 * M;   // [first r | rho | z of the proposal | g of the proposal]
  const bool log_it = n.leaf_out && nlog < n.leaf_cap;
  double* lg = log_it ? n.leaf_out + (3 * (int64_t)M + 1) * (nlog + n.leaf_cap * c) : nullptr;
  double kk = 0.0;
  for_owned(M, [&](int m) {
    const double zv = zp[m], gv = gp[m];
    const double r1 = rh[m] + (0.5 * ve) * gv;
    kk += (minv[m] * r1) * r1;
    ez[m] = zv, er[m] = r1, eg[m] = gv;
    top[m] = r1, top[M + m] = r1, top[2 * M + m] = zv, top[3 * M + m] = gv;
    if (log_it) lg[m] = zv, lg[M + m] = r1, lg[2 * M + 1 + m] = gv;
  });
  const double k1 = 0.5 * block_sum(kk, red);
  if (log_it && tid == 0) lg[2 * M] = lp1;
  double h1 = lp1 - k1;
  if (!isfinite(h1)) h1 = -INFINITY;
  const double dh = h1 - h0;
  ++nleaf;
  ++k;
  ++sp;
  // the top entry's scalars
  double t_lp = lp1, t_logw = dh, t_alpha = 1.0;
  if (dh < 0.0) {
    const double ex = exp(dh);
    t_alpha = ex < 1.0 ? ex : 1.0;
  }
  int t_n = 1, t_sel = nleaf;
  bool stop = (-dh) > n.max_dh;
  if (!stop) {
    for (int level = 1; ((k >> (level - 1)) & 1) == 0; ++level) {   // one merge per trailing zero bit of k
      const int ai = sp - 2;   // (k's trailing zeros count the complete sub-trees under the top: ai >= 0)
      double* sa = p.stack + (int64_t)ai * 4 * M;
      const double* sb = sa + 4 * M;
      // (a's scalars are read BEFORE the barriers of the sums below: thread 0 writes this slot at the end of the launch)
      const double a_logw = tr->s_logw[ai], a_lp = tr->s_lp[ai], a_alpha = tr->s_alpha[ai];
      const int a_n = tr->s_n[ai], a_sel = tr->s_sel[ai];
      const double lw = nuts_logaddexp(a_logw, t_logw);
      const Philox4 x = philox_draw(a.seed, chain, step, NUTS_P_MERGE, (uint32_t)(16 * nleaf + level));
      const bool pick = log(u53(x.v[1], x.v[0])) < t_logw - lw;
      double d[2] = {0.0, 0.0};   // rho . (Minv r-), rho . (Minv r+)
      for_owned(M, [&](int m) {
        const double rho = sa[M + m] + sb[M + m];
        sa[M + m] = rho;
        if (pick) sa[2 * M + m] = sb[2 * M + m], sa[3 * M + m] = sb[3 * M + m];
        const double rs = sa[m], re = er[m], mi = minv[m];
        d[0] += rho * (mi * (dir > 0 ? rs : re));
        d[1] += rho * (mi * (dir > 0 ? re : rs));
      });
      block_sum(d, red);
      if (!pick) t_lp = a_lp, t_sel = a_sel;
      t_logw = lw;
      t_alpha = a_alpha + t_alpha;
      t_n = a_n + t_n;
      --sp;
      if (d[0] <= 0.0 || d[1] <= 0.0) {
        stop = true;
        break;
      }
    }
  }
  if (stop) {
    for (int i = sp - 2; i >= 0; --i) {   // the entries under the stopped sub-tree fold into it, top to bottom
      t_alpha = tr->s_alpha[i] + t_alpha;
      t_n = tr->s_n[i] + t_n;
    }
    alpha_sum += t_alpha;
    n_alpha += t_n;
    still = 0;
  } else if (k == (1 << depth)) {
    // the doubling is complete: one entry, the stack's slot 0
    const double* sub = p.stack;
    alpha_sum += t_alpha;
    n_alpha += t_n;
    const Philox4 x = philox_draw(a.seed, chain, step, NUTS_P_DOUBLING, (uint32_t)depth);
    const bool pick = log(u53(x.v[3], x.v[2])) < t_logw - logw;
    double d[2] = {0.0, 0.0};   // rho . (Minv r-), rho . (Minv r+) of the whole tree
    for_owned(M, [&](int m) {
      if (pick) p.zc[m] = sub[2 * M + m], p.gc[m] = sub[3 * M + m];
      const double rho = p.rho[m] + sub[M + m], mi = minv[m];
      p.rho[m] = rho;
      d[0] += rho * (mi * p.rm[m]);
      d[1] += rho * (mi * p.rq[m]);
    });
    block_sum(d, red);
    if (pick) lpc = t_lp, selc = t_sel;
    logw = nuts_logaddexp(logw, t_logw);
    ++depth;
    if (d[0] <= 0.0 || d[1] <= 0.0 || depth >= n.max_depth) {
      still = 0;
    } else {
      dir = nuts_direction(a.seed, chain, step, depth);
      ++ndoub;
      k = 0;
      sp = 0;
    }
  }
  if (still) nuts_next_point(p, dir, eps, minv, rh, zp, M);
  if (tid == 0) {
    tr->logw = logw, tr->lpc = lpc, tr->alpha_sum = alpha_sum;
    tr->n_alpha = n_alpha, tr->depth = depth, tr->ndoub = ndoub, tr->dir = dir, tr->k = k, tr->sp = sp, tr->nleaf = nleaf,
    tr->selc = selc, tr->open = still;
    tr->nlog = nlog + 1;
    if (still && sp > 0) {
      tr->s_lp[sp - 1] = t_lp, tr->s_logw[sp - 1] = t_logw, tr->s_alpha[sp - 1] = t_alpha;
      tr->s_n[sp - 1] = t_n, tr->s_sel[sp - 1] = t_sel;
    }
    if (still) atomicAdd(open, 1);
  }
}

__global__ __launch_bounds__(SAMPLER_NT) void nuts_end_kernel(HmcRun a, NutsRun n, uint64_t step, int adapting, int in_window,
                                                          int window_close, int last_adapt) {
  __shared__ double wn_s;
  const int64_t c = blockIdx.x;
  const int tid = threadIdx.x;
  const int32_t M = a.M;
  HmcChain* ch = a.chain + c;
  const NutsChain* tr = n.tree + c;
  const NutsPtrs p = nuts_ptrs(n, c, M);
  const int64_t col = (int64_t)step + (a.itr + 1) * c;
  if (tid == 0) {
    const double eps = ch->eps;
    const int na = tr->n_alpha;
    const double alpha = tr->alpha_sum / (double)(na > 1 ? na : 1);
    a.lp[c] = tr->lpc;
    a.lp_out[col] = tr->lpc;
    a.alpha_out[col] = alpha;
    a.eps_out[col] = eps;
    n.depth_out[col] = tr->ndoub;
    n.nleaf_out[col] = tr->nleaf;
    n.sel_out[col] = tr->selc;
    double e_next;
    int64_t wn;
    hmc_adapt_scalars(ch, a.delta, alpha, eps, adapting, in_window, window_close, last_adapt, e_next, wn);
    wn_s = (double)wn;
  }
  __syncthreads();
  keep_and_record(a, c, col, p.zc, p.gc, adapting && in_window, wn_s /* the window's count INCLUDING this step */, window_close);
}

void launch_nuts_begin(hipStream_t st, const HmcRun& a, const NutsRun& n, int32_t C, uint64_t step, bool first) {
  hipLaunchKernelGGL(nuts_begin_kernel, dim3((unsigned)C), dim3(SAMPLER_NT), 0, st, a, n, step, first ? 1 : 0);
}

void launch_nuts_leaf(hipStream_t st, const HmcRun& a, const NutsRun& n, int32_t C, uint64_t step, int32_t* open) {
  hipLaunchKernelGGL(nuts_leaf_kernel, dim3((unsigned)C), dim3(SAMPLER_NT), 0, st, a, n, step, open);
}

void launch_nuts_end(hipStream_t st, const HmcRun& a, const NutsRun& n, int32_t C, uint64_t step, bool adapting, bool in_window,
                     bool window_close, bool last_adapt) {
  hipLaunchKernelGGL(nuts_end_kernel, dim3((unsigned)C), dim3(SAMPLER_NT), 0, st, a, n, step, adapting ? 1 : 0, in_window ? 1 : 0,
                     window_close ? 1 : 0, last_adapt ? 1 : 0);
}

}  // namespace si
