// The costs of the training step other than mse (si_train_set_cost; costs.py is the definition): Flux 0.11.2's mae, huber_loss,
// logitcrossentropy (dims = 1) and logitbinarycrossentropy with agg = mean [upstream src/losses/functions.jl and NNlib's
// logsoftmax / logsigmoid, restated from memory, unverifiable offline].  A cost sits at the seam of the three training routes:
// behind the forward pass, which has left yhat (out x B, columns contiguous) in a device buffer, it produces
//     the numerator of the loss   -> the route's one-word loss buffer (replacing the SSE the forward's epilogue wrote there)
//     Delta_L = dL/dyhat .* act_L'(yhat)  -> the seed of the reverse sweep, in place of launch_delta_out*
// All arithmetic is fp64; yhat is read as the route holds it (TY = double / float), Delta is stored as the route's sweep reads it
// (TD = double / float, rounded once).  The loss is summed without atomics: every workgroup reduces its summands in a fixed order
// into one partial, cost_final_kernel adds the partials in ascending order.  Every loop bound is a kernel argument: the same
// inputs give the same bits.
#include <algorithm>

#include "cost_reduce.h"
#include "kernels_gemm.h"

namespace si {

// kinds 1, 2, 4: elementwise summand l(yhat, y) and its derivative
template <class TY, class TD>
__global__ __launch_bounds__(256) void cost_elem_kernel(const double* __restrict__ Y, const TY* __restrict__ Yhat, int64_t d, int kind,
                                                        double hdelta, double inv_denom, int act, TD* __restrict__ Delta,
                                                        double* __restrict__ part) {
  __shared__ double red[4];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double acc = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < d; e += stride) {
    const double yh = (double)Yhat[e], y = Y[e];
    double l, g;
    if (kind == SI_COST_LOGITBCE) {
      // (1 - y) yhat + softplus(-yhat), softplus(-x) = max(-x, 0) + log1p(exp(-|x|)); sigmoid through t = exp(-|x|) in (0, 1]
      const double t = exp(-fabs(yh));
      l = (1.0 - y) * yh + (yh < 0.0 ? -yh : 0.0) + log1p(t);
      g = (yh >= 0.0 ? 1.0 / (1.0 + t) : t / (1.0 + t)) - y;
    } else {
      const double r = yh - y, a = fabs(r);
      const double sg = r > 0.0 ? 1.0 : (r < 0.0 ? -1.0 : 0.0);   // sign(0) = 0
      if (kind == SI_COST_MAE) {
        l = a;
        g = sg;
      } else if (a < hdelta) {   // (strict: |r| = delta takes the linear branch)
        l = 0.5 * r * r;
        g = r;
      } else {
        l = hdelta * (a - 0.5 * hdelta);
        g = hdelta * sg;
      }
    }
    acc += l;
    Delta[e] = (TD)(g * inv_denom * dact_full(yh, act));
  }
  acc = cost_block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// kind 3: a wave64 owns 64 / seg columns at a time; seg = next_pow2(out) for out <= 32 (a 10-class head: four columns per wave),
// 64 otherwise, the lanes striding over i for out > 64.  Per column: max, sum exp, then sum Y and sum Y (yhat - lse), then Delta
// in a last sweep over the column, which the cache still holds.  (Measured and not kept: the four sweeps unrolled four times --
// 4 us faster of 258 at out = 1000, 6 us slower of 207 at out = 10)
template <class TY, class TD>
__global__ __launch_bounds__(256) void cost_logitce_kernel(const double* __restrict__ Y, const TY* __restrict__ Yhat, int out, int64_t nb,
                                                           int seg, double inv_nb, int act, TD* __restrict__ Delta,
                                                           double* __restrict__ part) {
  __shared__ double red[4];
  const int lane = threadIdx.x & 63;
  const int cpw = 64 / seg, sidx = lane / seg, pos = lane - sidx * seg;
  const int64_t nwaves = (int64_t)gridDim.x * 4, ngroups = (nb + cpw - 1) / cpw;
  double acc = 0.0;
  for (int64_t grp = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); grp < ngroups; grp += nwaves) {   // (wave-uniform)
    const int64_t b = grp * cpw + sidx;
    const bool valid = b < nb;
    const int iend = valid ? out : 0;
    const TY* __restrict__ yh = Yhat + b * out;
    const double* __restrict__ y = Y + b * out;
    double m = -__builtin_inf();
    for (int i = pos; i < iend; i += seg) m = fmax(m, (double)yh[i]);
    m = seg_max(m, seg);
    double se = 0.0;
    for (int i = pos; i < iend; i += seg) se += exp((double)yh[i] - m);
    se = seg_sum(se, seg);
    const double lse = m + log(se);
    double sy = 0.0, t = 0.0;
    for (int i = pos; i < iend; i += seg) {
      const double yi = y[i];
      sy += yi;
      t += yi * ((double)yh[i] - lse);
    }
    sy = seg_sum(sy, seg);
    t = seg_sum(t, seg);
    if (valid && pos == 0) acc -= t;
    TD* __restrict__ dl = Delta + b * out;
    for (int i = pos; i < iend; i += seg) {
      const double v = (double)yh[i];
      const double p = exp(v - m) / se;
      dl[i] = (TD)((sy * p - y[i]) * inv_nb * dact_full(v, act));
    }
  }
  acc = cost_block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// second stage: the workgroup partials in ascending order into the loss word
// (n <= SI_COST_MAX_BLOCKS: the launcher's grid.  The partials are fetched side by side into LDS and added from there by one
// thread: one thread reading them from global memory one after the other took 8 us longer at 160 partials)
__global__ __launch_bounds__(256) void cost_final_kernel(const double* __restrict__ part, int n, double* __restrict__ loss) {
  __shared__ double sh[SI_COST_MAX_BLOCKS];
  for (int i = threadIdx.x; i < n && i < SI_COST_MAX_BLOCKS; i += 256) sh[i] = part[i];
  __syncthreads();
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int i = 0; i < n && i < SI_COST_MAX_BLOCKS; ++i) s += sh[i];
  *loss = s;
}

template <class TY, class TD>
static void launch_cost_tail_t(hipStream_t st, const CostTail& c, const double* Y, const TY* Yhat, int32_t out, int64_t B, int act,
                               TD* delta, double* loss) {
  int64_t blocks;
  if (c.kind == SI_COST_LOGITCE) {
    int seg = 64;
    if (out <= 32)
      for (seg = 1; seg < out; seg <<= 1) {}
    const int64_t cpw = 64 / seg, ngroups = (B + cpw - 1) / cpw;
    blocks = std::min<int64_t>((ngroups + 3) / 4, SI_COST_MAX_BLOCKS);
    hipLaunchKernelGGL((cost_logitce_kernel<TY, TD>), dim3((unsigned)blocks), dim3(256), 0, st, Y, Yhat, out, B, seg, c.inv_denom, act,
                       delta, c.part);
  } else {
    const int64_t d = (int64_t)out * B;
    blocks = std::min<int64_t>((d + 255) / 256, SI_COST_MAX_BLOCKS);
    hipLaunchKernelGGL((cost_elem_kernel<TY, TD>), dim3((unsigned)blocks), dim3(256), 0, st, Y, Yhat, d, c.kind, c.param, c.inv_denom, act,
                       delta, c.part);
  }
  hipLaunchKernelGGL(cost_final_kernel, dim3(1), dim3(256), 0, st, c.part, (int)blocks, loss);
}

template <class TD>
void launch_cost_tail(hipStream_t st, const CostTail& c, const double* Y, const double* Yhat64, const float* Yhat32, int32_t out, int64_t B,
                      int act, TD* delta, double* loss) {
  if (Yhat64)
    launch_cost_tail_t(st, c, Y, Yhat64, out, B, act, delta, loss);
  else
    launch_cost_tail_t(st, c, Y, Yhat32, out, B, act, delta, loss);
}
template void launch_cost_tail<double>(hipStream_t, const CostTail&, const double*, const double*, const float*, int32_t, int64_t, int,
                                       double*, double*);
template void launch_cost_tail<float>(hipStream_t, const CostTail&, const double*, const double*, const float*, int32_t, int64_t, int,
                                      float*, double*);

}  // namespace si
