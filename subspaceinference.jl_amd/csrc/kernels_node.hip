// The NeuralODE density's kernel (si_infer_setup_node; reference src/space_inference.jl:96-101): f x C independent initial-value
// problems, each a strictly sequential adaptive Tsit5 integration whose right-hand side is a small Dense chain.  gfx950, fp64, no
// atomics.  Compiled without contraction of a*b+c: the definition (subspaceinference.jl_amd/node.py) rounds every product and
// every sum, and every expression here is written in its order.
//
// Layout: a group of G lanes (a power of two <= 64, so a group never crosses a wave) per trajectory, 256 / G trajectories per
// workgroup, grid.y = chain slot; the chain's N weights sit in LDS.  Lane j of a group owns the output units j, j + G, ... of
// every layer and evaluates their activation (where the time goes); a layer's outputs are exchanged through the group's own
// LDS slice.  LDS is in order per wave and the lanes of a group take identical branches (t, h, the RK state and the controller
// are replicated in each of them), so the exchange needs no workgroup barrier: a wavefront fence keeps the compiler's order.
// Groups of one wave take different numbers of steps; a group that is done simply leaves -- no operation spans groups.
// Every sum is sequential over the input index and owned by one lane: a trajectory's bits do not depend on G, f, C, its column,
// its chain slot or the run.  Every loop is bounded: the step loop by max_steps (accepted + rejected), the save loop by S.
#include "kernels_gemm.h"
#include "node_tableau.h"

namespace si {

__device__ __noinline__ double node_act(double v, int act) { return act_full(v, act); }

__device__ __forceinline__ void node_group_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ bool node_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }   // (false for NaN)

// out = f(u): a_0 = u or (u*u)*u, then the Dense layers; layer l writes the slice's buffer l & 1
template <int D>
__device__ __forceinline__ void node_rhs(const NodeArgs& a, const double* __restrict__ wl, double* ex, int lane, const double (&u)[D],
                                         double (&out)[D]) {
  double a0[D];
#pragma unroll
  for (int i = 0; i < D; ++i) a0[i] = a.pre_power == 3 ? (u[i] * u[i]) * u[i] : u[i];
  const int G = a.G;
  for (int l = 0; l < a.lay.n; ++l) {
    const int in = a.lay.in[l], on = a.lay.out[l], act = a.lay.act[l];
    const double* W = wl + a.lay.w_off[l];
    const double* b = wl + a.lay.b_off[l];
    const double* src = ex + ((l & 1) ? 0 : a.maxw);
    double* dst = ex + ((l & 1) ? a.maxw : 0);
    for (int j0 = 0; j0 < on; j0 += G) {   // (the trip count is the group's, not the lane's)
      const int j = j0 + lane;
      if (j < on) {
        double acc = 0.0;
        if (l == 0) {
#pragma unroll
          for (int i = 0; i < D; ++i) acc = acc + W[j + on * i] * a0[i];
        } else {
          for (int i = 0; i < in; ++i) acc = acc + W[j + on * i] * src[i];
        }
        acc = acc + b[j];
        dst[j] = node_act(acc, act);
      }
    }
    node_group_sync();
  }
  const double* res = ex + (((a.lay.n - 1) & 1) ? a.maxw : 0);
#pragma unroll
  for (int i = 0; i < D; ++i) out[i] = res[i];
  node_group_sync();
}

// c_1 k_1 + c_2 k_2 + ... + c_n k_n, terms ascending
template <int D, int NK>
__device__ __forceinline__ double node_comb(const double (&c)[NK], const double (&k)[7][D], int n, int i) {
  double s = c[0] * k[0][i];
#pragma unroll
  for (int j = 1; j < NK; ++j)
    if (j < n) s = s + c[j] * k[j][i];
  return s;
}

// RECORD: the same body once more, writing (t_n, hs_n, u_n) of every accepted step for the reverse kernel below (a.rec, sized by
// max_steps: accepted + rejected steps stay below it, so the record cannot overflow).  Nothing else differs: sums, counts and
// statuses are the unrecorded kernel's bits.
template <int D, bool RECORD>
__global__ __launch_bounds__(256) void node_solve_kernel(NodeArgs a) {
  extern __shared__ double node_lds[];
  const int G = a.G;
  const int grp = (int)threadIdx.x >> a.lgG, lane = (int)threadIdx.x & (G - 1);
  double* wl = node_lds;
  double* ex = node_lds + ((a.N + 1) & ~1) + (size_t)grp * 2 * (size_t)a.maxw;
  {
    const double* wg = a.w + (int64_t)blockIdx.y * a.ldw;
    for (int i = threadIdx.x; i < a.N; i += 256) wl[i] = wg[i];
  }
  __syncthreads();   // the only workgroup barrier: before any group can leave
  const int64_t p = (int64_t)blockIdx.x * (256 >> a.lgG) + grp;
  if (p >= a.f) return;
  const bool lead = lane == 0;
  const int S = a.S;
  const int64_t tr = (int64_t)blockIdx.y * a.f + p;   // the trajectory's slot in the per-trajectory outputs
  const double* Yp = a.Y ? a.Y + p * (int64_t)(D * S) : nullptr;
  double* Up = a.U_out ? a.U_out + tr * (int64_t)(D * S) : nullptr;
  const bool adaptive = a.adaptive != 0;
  const double tend = a.ts[S - 1];

  double u[D], un[D], k[7][D];
  double t = a.t0, h, qold = NODE_QOLD0, sse = 0.0;
  int s = 0, nacc = 0, nrej = 0, status = 0;
#pragma unroll
  for (int i = 0; i < D; ++i) u[i] = a.U0[p * D + i];

  auto save = [&](int ss, const double (&us)[D]) {   // the lead lane's: state i at save time ss, and its squared errors
#pragma unroll
    for (int i = 0; i < D; ++i) {
      if (Up) Up[(int64_t)i * S + ss] = us[i];
      if (Yp) {
        const double r = us[i] - Yp[(int64_t)i * S + ss];
        sse = sse + r * r;
      }
    }
  };

  node_rhs<D>(a, wl, ex, lane, u, k[0]);
  if (a.ts[0] == a.t0) {
    if (lead) save(0, u);
    s = 1;
  }
  bool live = s < S;
  // ---- the starting step (Hairer, Norsett, Wanner II.4, order 5), or the caller's dt
  if (adaptive && !(a.dt > 0.0)) {
    double sk[D], acc0 = 0.0, acc1 = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      sk[i] = a.abstol + a.reltol * fabs(u[i]);
      const double v0 = u[i] / sk[i], v1 = k[0][i] / sk[i];
      acc0 = acc0 + v0 * v0;
      acc1 = acc1 + v1 * v1;
    }
    const double d0 = sqrt(acc0 / (double)D), d1 = sqrt(acc1 / (double)D);
    double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * (d0 / d1);
    {
      const double span = tend - t;
      h0 = h0 < span ? h0 : span;
    }
#pragma unroll
    for (int i = 0; i < D; ++i) un[i] = u[i] + h0 * k[0][i];
    node_rhs<D>(a, wl, ex, lane, un, k[1]);
    double acc2 = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const double v = (k[1][i] - k[0][i]) / sk[i];
      acc2 = acc2 + v * v;
    }
    const double d2 = sqrt(acc2 / (double)D) / h0;
    const double dm = d1 > d2 ? d1 : d2;
    double h1;
    if (dm <= 1e-15) {
      const double hm = h0 * 1e-3;
      h1 = 1e-6 > hm ? 1e-6 : hm;
    } else {
      h1 = pow(0.01 / dm, 1.0 / 6.0);
    }
    const double h100 = 100.0 * h0;
    h = h100 < h1 ? h100 : h1;
  } else {
    h = a.dt;
  }
  if (live) {
    bool ok = node_finite(h);
#pragma unroll
    for (int i = 0; i < D; ++i) ok = ok && node_finite(k[0][i]);
    if (!ok) {
      status = 2;
      live = false;
    }
  }

  while (live) {
    if (nacc + nrej >= a.max_steps) {
      status = 1;
      break;
    }
    const bool last = t + h >= tend;
    const double hs = last ? tend - t : h;
    if (t + hs == t) {
      status = 2;
      break;
    }
    double arg[D];
#pragma unroll
    for (int st = 1; st < 6; ++st) {
#pragma unroll
      for (int i = 0; i < D; ++i) arg[i] = u[i] + hs * node_comb<D, 6>(NODE_A[st], k, st, i);
      node_rhs<D>(a, wl, ex, lane, arg, k[st]);
    }
#pragma unroll
    for (int i = 0; i < D; ++i) un[i] = u[i] + hs * node_comb<D, 6>(NODE_A[6], k, 6, i);
    node_rhs<D>(a, wl, ex, lane, un, k[6]);
    bool fine = true;
#pragma unroll
    for (int i = 0; i < D; ++i) fine = fine && node_finite(un[i]);
    bool accept = fine;
    double hnew = h;
    if (adaptive) {
      double acc = 0.0;
#pragma unroll
      for (int i = 0; i < D; ++i) {
        const double e = hs * node_comb<D, 7>(NODE_BT, k, 7, i);
        const double au = fabs(u[i]), an = fabs(un[i]);
        const double v = e / (a.abstol + a.reltol * (au > an ? au : an));
        acc = acc + v * v;
      }
      const double err = sqrt(acc / (double)D);
      fine = fine && node_finite(err);
      accept = fine && err <= 1.0;
      if (fine) {
        const double q11 = pow(err, NODE_BETA1);
        if (accept) {
          double q = (q11 / pow(qold, NODE_BETA2)) / NODE_GAMMA;
          q = NODE_QMIN_INV < q ? NODE_QMIN_INV : q;
          q = NODE_QMAX_INV > q ? NODE_QMAX_INV : q;
          hnew = hs / q;
          qold = err > 1e-4 ? err : 1e-4;
        } else {
          const double qr = q11 / NODE_GAMMA;
          hnew = hs / (NODE_QMIN_INV < qr ? NODE_QMIN_INV : qr);
        }
      }
    }
    if (!fine) {
      status = 2;
      break;
    }
    if (!accept) {
      nrej += 1;
      h = hnew;
      continue;
    }
    if constexpr (RECORD) {
      if (lead) {
        double* r = a.rec + (tr * a.max_steps + nacc) * (int64_t)(D + 2);
        r[0] = t, r[1] = hs;
#pragma unroll
        for (int i = 0; i < D; ++i) r[2 + i] = u[i];
      }
    }
    nacc += 1;
    const double tn = last ? tend : t + hs;
    while (s < S) {   // (saveat without tstops: the step never stops at a save time)
      const double tss = a.ts[s];
      if (!(tss <= tn)) break;
      if (lead) {
        if (tss == tn) {
          save(s, un);
        } else {
          const double th = (tss - t) / hs, th2 = th * th;
          const double bw[7] = {NODE_B1[0] * th * (th - NODE_B1[1]) * (th2 - NODE_B1[2] * th + NODE_B1[3]),
                                NODE_B2[0] * th2 * (th2 - NODE_B2[1] * th + NODE_B2[2]),
                                NODE_B3[0] * th2 * (th2 - NODE_B3[1] * th + NODE_B3[2]),
                                NODE_B4[0] * (th - NODE_B4[1]) * (th - NODE_B4[2]) * th2,
                                NODE_B5[0] * (th - NODE_B5[1]) * (th - NODE_B5[2]) * th2,
                                NODE_B6[0] * (th - NODE_B6[1]) * (th - NODE_B6[2]) * th2,
                                NODE_B7[0] * (th - NODE_B7[1]) * (th - NODE_B7[2]) * th2};
          double us[D];
#pragma unroll
          for (int i = 0; i < D; ++i) us[i] = u[i] + hs * node_comb<D, 7>(bw, k, 7, i);
          save(s, us);
        }
      }
      s += 1;
    }
    t = tn;
    h = hnew;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      u[i] = un[i];
      k[0][i] = k[6][i];
    }
    live = s < S;
  }

  if (lead) {
    if (status != 0) {   // a failed trajectory: +Inf, and NaN where it saved nothing
      sse = __longlong_as_double(0x7ff0000000000000LL);
      if (Up)
        for (int ss = s; ss < S; ++ss)
          for (int i = 0; i < D; ++i) Up[(int64_t)i * S + ss] = __longlong_as_double(0x7ff8000000000000LL);
    }
    a.sse_p[tr] = sse;
    if (a.nacc) a.nacc[tr] = nacc;
    if (a.nrej) a.nrej[tr] = nrej;
    if (a.status) a.status[tr] = status;
  }
}

// sse[c] = the per-trajectory sums of chain slot c in ascending p, from 0.0 (the reference's loop order): one thread per slot
__global__ __launch_bounds__(64) void node_sum_kernel(const double* __restrict__ sse_p, int64_t f, double* __restrict__ sse, int nchains) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= nchains) return;
  const double* v = sse_p + (int64_t)c * f;
  double acc = 0.0;
  for (int64_t p = 0; p < f; ++p) acc = acc + v[p];
  sse[c] = acc;
}

// ---- the gradient through the solver (si_node_set_grad; node.py: grad_slices is the definition) ---------------------------------
// The discrete adjoint over the recorded accepted steps, hs_n and every theta frozen.  The forward kernel's layout: G lanes per
// trajectory, 256 / G trajectories per workgroup, the chain's weights in LDS; every layer is at most 64 wide (si_node_set_grad), so
// lane j owns unit j -- row j of W and b_j -- of every layer.  Per step, descending, the seven stages are recomputed from the
// recorded u_n with node_rhs itself (k_1 = f(u_n) has the bits of the forward's FSAL value); then per stage in reverse node_vjp
// recomputes that stage's layer outputs, one value per lane and layer kept in the group's LDS slice, and back-propagates: the
// transposed product is lane i's own ascending sum over the exchanged delta, and lane j adds delta_j * a_in[i] into the
// trajectory's own N-slice in global memory with plain loads and stores (one lane per element and stage; the stream zeroed it).
// No atomics; the lanes of a group take identical branches (t, hs, the RK state and the adjoints are replicated in each);
// wavefront fences only after the one weight-load barrier; the step loop is bounded by the recorded count, the save loop by S.
// A trajectory's bits depend on its inputs alone: not on G, f, C, its column, its chain slot or the run.

// node_comb over stage values kept in LDS (kl[j * D + i] = k_{j+1}[i]): the same terms in the same order
template <int D, int NK>
__device__ __forceinline__ double node_comb_lds(const double (&c)[NK], const double* kl, int n, int i) {
  double s = c[0] * kl[i];
#pragma unroll
  for (int j = 1; j < NK; ++j)
    if (j < n) s = s + c[j] * kl[j * D + i];
  return s;
}

// g = J_u' kb of f at x; J_W' kb goes into the slice gs.  ac: the group's n x maxw layer outputs, dx: its two delta buffers.
template <int D>
__device__ __forceinline__ void node_vjp(const NodeArgs& a, const double* __restrict__ wl, double* ac, double* dx, int lane,
                                         const double (&x)[D], const double (&kb)[D], double (&g)[D], double* __restrict__ gs) {
  double a0[D];
#pragma unroll
  for (int i = 0; i < D; ++i) a0[i] = a.pre_power == 3 ? (x[i] * x[i]) * x[i] : x[i];
  const int mw = a.maxw;
  for (int l = 0; l < a.lay.n; ++l) {   // the forward's own sums, every layer's outputs kept
    const int in = a.lay.in[l], on = a.lay.out[l];
    const double* W = wl + a.lay.w_off[l];
    const double* src = l > 0 ? ac + (l - 1) * mw : ac;   // (layer 0 reads a0)
    if (lane < on) {
      double acc = 0.0;
      if (l == 0) {
#pragma unroll
        for (int i = 0; i < D; ++i) acc = acc + W[lane + on * i] * a0[i];
      } else {
        for (int i = 0; i < in; ++i) acc = acc + W[lane + on * i] * src[i];
      }
      acc = acc + wl[a.lay.b_off[l] + lane];
      ac[l * mw + lane] = node_act(acc, a.lay.act[l]);
    }
    node_group_sync();
  }
  double* dout = dx;
  double* din = dx + mw;
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < D; ++i) din[i] = kb[i];
  }
  node_group_sync();
  for (int l = a.lay.n - 1; l >= 0; --l) {
    const int in = a.lay.in[l], on = a.lay.out[l];
    const double* W = wl + a.lay.w_off[l];
    const double* src = l > 0 ? ac + (l - 1) * mw : ac;
    if (lane < on) {
      const double delta = din[lane] * dact_full(ac[l * mw + lane], a.lay.act[l]);
      dout[lane] = delta;
      double* gb = gs + a.lay.b_off[l] + lane;
      *gb = *gb + delta;
      double* gw = gs + a.lay.w_off[l] + lane;
      if (l == 0) {
#pragma unroll
        for (int i = 0; i < D; ++i) gw[on * i] = gw[on * i] + delta * a0[i];
      } else {
        for (int i = 0; i < in; ++i) gw[on * i] = gw[on * i] + delta * src[i];
      }
    }
    node_group_sync();
    if (lane < in) {
      double acc = 0.0;
      for (int j = 0; j < on; ++j) acc = acc + W[j + on * lane] * dout[j];
      din[lane] = acc;
    }
    node_group_sync();
  }
#pragma unroll
  for (int i = 0; i < D; ++i) g[i] = a.pre_power == 3 ? (3.0 * (x[i] * x[i])) * din[i] : din[i];
  node_group_sync();
}

template <int D>
__global__ __launch_bounds__(256) void node_grad_kernel(NodeArgs a) {
  extern __shared__ double node_lds[];
  const int G = a.G;
  const int grp = (int)threadIdx.x >> a.lgG, lane = (int)threadIdx.x & (G - 1);
  double* wl = node_lds;
  double* ex = node_lds + ((a.N + 1) & ~1) + (size_t)grp * (size_t)(4 + a.lay.n) * (size_t)a.maxw;   // node_rhs's two buffers,
  double* dx = ex + 2 * a.maxw;                                                                       // two delta buffers,
  double* ac = dx + 2 * a.maxw;                                                                       // the layer outputs
  // the step's seven stage values, per group (registers hold the adjoints: 7 d of those, u, u_{n+1}, lambda and u-bar)
  double* kl = node_lds + ((a.N + 1) & ~1) + (size_t)(256 >> a.lgG) * (size_t)(4 + a.lay.n) * (size_t)a.maxw + (size_t)grp * (7 * D);
  {
    const double* wg = a.w + (int64_t)blockIdx.y * a.ldw;
    for (int i = threadIdx.x; i < a.N; i += 256) wl[i] = wg[i];
  }
  __syncthreads();   // the only workgroup barrier: before any group can leave
  const int64_t p = (int64_t)blockIdx.x * (256 >> a.lgG) + grp;
  if (p >= a.f) return;
  const int S = a.S;
  const int64_t tr = (int64_t)blockIdx.y * a.f + p;
  const double* Yp = a.Y + p * (int64_t)(D * S);
  double* gs = a.gsl + tr * (int64_t)a.N;
  if (a.status[tr] != 0) {   // a failed trajectory: NaN in every component
    for (int i = lane; i < a.N; i += G) gs[i] = __longlong_as_double(0x7ff8000000000000LL);
    return;
  }
  int nst = a.nacc[tr];
  nst = nst < a.max_steps ? nst : a.max_steps;   // (the record's size, whatever the count says)
  const double* rc = a.rec + tr * (int64_t)a.max_steps * (int64_t)(D + 2);
  const double tend = a.ts[S - 1];

  double u[D], un[D], lam[D], ub[D], kb[7][D], g[D], arg[D];
#pragma unroll
  for (int i = 0; i < D; ++i) lam[i] = 0.0;
  auto stage = [&](int st, const double (&x)[D]) {   // k_{st+1} = f(x), left in the group's LDS slice
    node_rhs<D>(a, wl, ex, lane, x, g);
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < D; ++i) kl[st * D + i] = g[i];
    }
    node_group_sync();
  };
  int s = S - 1;
  for (int n = nst - 1; n >= 0; --n) {
    const double* r = rc + (int64_t)n * (D + 2);
    const double t = r[0], hs = r[1];
    const double tn = n + 1 < nst ? r[D + 2] : tend;
#pragma unroll
    for (int i = 0; i < D; ++i) u[i] = r[2 + i];
    stage(0, u);
#pragma unroll
    for (int st = 1; st < 6; ++st) {
#pragma unroll
      for (int i = 0; i < D; ++i) arg[i] = u[i] + hs * node_comb_lds<D, 6>(NODE_A[st], kl, st, i);
      stage(st, arg);
    }
#pragma unroll
    for (int i = 0; i < D; ++i) un[i] = u[i] + hs * node_comb_lds<D, 6>(NODE_A[6], kl, 6, i);
    stage(6, un);
#pragma unroll
    for (int i = 0; i < D; ++i) {
      ub[i] = 0.0;
#pragma unroll
      for (int j = 0; j < 7; ++j) kb[j][i] = 0.0;
    }
    while (s >= 0) {   // 1. the saves of the step, descending (a save at t0 belongs to no step)
      const double tss = a.ts[s];
      if (!(tss > t)) break;
      if (tss == tn) {
#pragma unroll
        for (int i = 0; i < D; ++i) lam[i] = lam[i] + -2.0 * (un[i] - Yp[(int64_t)i * S + s]);
      } else {
        const double th = (tss - t) / hs, th2 = th * th;
        const double bw[7] = {NODE_B1[0] * th * (th - NODE_B1[1]) * (th2 - NODE_B1[2] * th + NODE_B1[3]),
                              NODE_B2[0] * th2 * (th2 - NODE_B2[1] * th + NODE_B2[2]),
                              NODE_B3[0] * th2 * (th2 - NODE_B3[1] * th + NODE_B3[2]),
                              NODE_B4[0] * (th - NODE_B4[1]) * (th - NODE_B4[2]) * th2,
                              NODE_B5[0] * (th - NODE_B5[1]) * (th - NODE_B5[2]) * th2,
                              NODE_B6[0] * (th - NODE_B6[1]) * (th - NODE_B6[2]) * th2,
                              NODE_B7[0] * (th - NODE_B7[1]) * (th - NODE_B7[2]) * th2};
#pragma unroll
        for (int i = 0; i < D; ++i) {
          const double us = u[i] + hs * node_comb_lds<D, 7>(bw, kl, 7, i);
          const double res = -2.0 * (us - Yp[(int64_t)i * S + s]);
          ub[i] = ub[i] + res;
#pragma unroll
          for (int j = 0; j < 7; ++j) kb[j][i] = kb[j][i] + (hs * bw[j]) * res;
        }
      }
      s -= 1;
    }
    node_vjp<D>(a, wl, ac, dx, lane, un, kb[6], g, gs);   // 2. k_7 = f(u_{n+1})
#pragma unroll
    for (int i = 0; i < D; ++i) {
      lam[i] = lam[i] + g[i];
      ub[i] = ub[i] + lam[i];   // 3. u_{n+1} = u_n + hs sum_j a_7j k_j
#pragma unroll
      for (int j = 0; j < 6; ++j) kb[j][i] = kb[j][i] + (hs * NODE_A[6][j]) * lam[i];
    }
#pragma unroll
    for (int st = 5; st >= 1; --st) {   // 4. the stages 6 .. 2
#pragma unroll
      for (int i = 0; i < D; ++i) arg[i] = u[i] + hs * node_comb_lds<D, 6>(NODE_A[st], kl, st, i);
      node_vjp<D>(a, wl, ac, dx, lane, arg, kb[st], g, gs);
#pragma unroll
      for (int i = 0; i < D; ++i) {
        ub[i] = ub[i] + g[i];
#pragma unroll
        for (int j = 0; j < 6; ++j)
          if (j < st) kb[j][i] = kb[j][i] + (hs * NODE_A[st][j]) * g[i];
      }
    }
    node_vjp<D>(a, wl, ac, dx, lane, u, kb[0], g, gs);   // 5. k_1 = f(u_n)
#pragma unroll
    for (int i = 0; i < D; ++i) lam[i] = ub[i] + g[i];   // 6.
  }
}

// gw[:, c] = sum_p slice_p in ascending p from 0.0, one thread per element; thread 0 of the chain's first block forms lp[c] from
// the chain's sums exactly as the host does (lp_from_sums with the NeuralODE constants)
__global__ __launch_bounds__(256) void node_grad_sum_kernel(const double* __restrict__ gsl, int64_t f, int64_t N, double* __restrict__ gw,
                                                             int64_t ldg, const double* __restrict__ sse, const double* __restrict__ wsq,
                                                             double* __restrict__ lp) {
  const int c = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) {
    double v = 0.0 - (sse[c] / 0.5) / 2.0;
    v += 0.0 - (wsq[c] / 0.5) / 2.0;
    lp[c] = v;
  }
  if (i >= N) return;
  const double* v = gsl + (int64_t)c * f * N + i;
  double acc = 0.0;
  for (int64_t p = 0; p < f; ++p) acc = acc + v[p * N];
  gw[(int64_t)c * ldg + i] = acc;
}

size_t node_grad_lds_bytes(const NodeArgs& a) {
  return ((size_t)((a.N + 1) & ~1) + (size_t)(256 >> a.lgG) * ((size_t)(4 + a.lay.n) * (size_t)a.maxw + (size_t)7 * a.d)) * sizeof(double);
}

template <int D>
static hipError_t node_grad_launch_d(hipStream_t st, const NodeArgs& a, dim3 grid, size_t lds) {
  static LdsOptIn opt;
  if (lds > (size_t)48 * 1024) opt.ensure(reinterpret_cast<const void*>(&node_grad_kernel<D>), lds);
  hipLaunchKernelGGL(node_grad_kernel<D>, grid, dim3(256), lds, st, a);
  return hipGetLastError();
}

hipError_t launch_node_grad(hipStream_t st, const NodeArgs& a, int nchains) {
  if (!a.rec || !a.gsl || !a.nacc || !a.status || !a.Y || a.maxw > 64) return hipErrorInvalidValue;
  const int gpb = 256 >> a.lgG;
  const dim3 grid((unsigned)((a.f + gpb - 1) / gpb), (unsigned)nchains);
  const size_t lds = node_grad_lds_bytes(a);
  switch (a.d) {
    case 1: return node_grad_launch_d<1>(st, a, grid, lds);
    case 2: return node_grad_launch_d<2>(st, a, grid, lds);
    case 3: return node_grad_launch_d<3>(st, a, grid, lds);
    case 4: return node_grad_launch_d<4>(st, a, grid, lds);
    case 5: return node_grad_launch_d<5>(st, a, grid, lds);
    case 6: return node_grad_launch_d<6>(st, a, grid, lds);
    case 7: return node_grad_launch_d<7>(st, a, grid, lds);
    case 8: return node_grad_launch_d<8>(st, a, grid, lds);
    default: return hipErrorInvalidValue;
  }
}

void launch_node_grad_sum(hipStream_t st, const double* gsl, int64_t f, int64_t N, double* gw, int64_t ldg, const double* sse,
                          const double* wsq, double* lp, int nchains) {
  hipLaunchKernelGGL(node_grad_sum_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)nchains), dim3(256), 0, st, gsl, f, N, gw, ldg,
                     sse, wsq, lp);
}

size_t node_lds_bytes(const NodeArgs& a) {
  return ((size_t)((a.N + 1) & ~1) + (size_t)(256 >> a.lgG) * 2 * (size_t)a.maxw) * sizeof(double);
}

template <int D>
static hipError_t node_launch_d(hipStream_t st, const NodeArgs& a, dim3 grid, size_t lds) {
  static LdsOptIn opt, opt_rec;
  if (a.rec) {
    if (lds > (size_t)48 * 1024) opt_rec.ensure(reinterpret_cast<const void*>(&node_solve_kernel<D, true>), lds);
    hipLaunchKernelGGL((node_solve_kernel<D, true>), grid, dim3(256), lds, st, a);
  } else {
    if (lds > (size_t)48 * 1024) opt.ensure(reinterpret_cast<const void*>(&node_solve_kernel<D, false>), lds);
    hipLaunchKernelGGL((node_solve_kernel<D, false>), grid, dim3(256), lds, st, a);
  }
  return hipGetLastError();
}

hipError_t launch_node_solve(hipStream_t st, const NodeArgs& a, int nchains) {
  const int gpb = 256 >> a.lgG;
  const dim3 grid((unsigned)((a.f + gpb - 1) / gpb), (unsigned)nchains);
  const size_t lds = node_lds_bytes(a);
  switch (a.d) {
    case 1: return node_launch_d<1>(st, a, grid, lds);
    case 2: return node_launch_d<2>(st, a, grid, lds);
    case 3: return node_launch_d<3>(st, a, grid, lds);
    case 4: return node_launch_d<4>(st, a, grid, lds);
    case 5: return node_launch_d<5>(st, a, grid, lds);
    case 6: return node_launch_d<6>(st, a, grid, lds);
    case 7: return node_launch_d<7>(st, a, grid, lds);
    case 8: return node_launch_d<8>(st, a, grid, lds);
    default: return hipErrorInvalidValue;
  }
}

void launch_node_sum(hipStream_t st, const double* sse_p, int64_t f, double* sse, int nchains) {
  hipLaunchKernelGGL(node_sum_kernel, dim3((unsigned)((nchains + 63) / 64)), dim3(64), 0, st, sse_p, f, sse, nchains);
}

}  // namespace si
