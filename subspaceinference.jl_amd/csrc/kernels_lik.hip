// The likelihood of a classifier behind the forward pass of the density (si_infer_set_likelihood; costs.py is the definition):
// the summed negative log-likelihood of the model outputs yhat (out x B, columns contiguous, fp64) of nc stacked chain slots in
// ONE launch, grid.y = chain slot.  Forward only: no Delta is written (the gradient goes through kernels_cost.hip's tail).
//     kind 1 categorical   nll = -sum_b sum_i Y_ib (yhat_ib - lse_b)          the numerator of SI_COST_LOGITCE
//     kind 2 Bernoulli     nll =  sum ((1 - Y) yhat + softplus(-yhat))        the numerator of SI_COST_LOGITBCE
// with the arithmetic of cost_logitce_kernel / cost_elem_kernel, summand for summand.  The partials of slot j go to
// part[j * gridDim.x + block], launch_sse's layout: gridDim.x is the view's sse_blocks, a workgroup that owns no column writes 0.0,
// and launch_sse_final / rwmh_tail_kernel add them as they add the squared errors'.  Every reduction has a fixed order (butterfly
// within a wave, the four wave sums ascending, the partials in sse_final_kernel's order) and every loop bound is a kernel argument
// that does not depend on nc: a slot's bits depend neither on nc nor on the call it arrives in.
#include <algorithm>

#include "cost_reduce.h"
#include "si_internal.h"

namespace si {

// a wave64 owns 64 / seg columns at a time; seg = next_pow2(out) for out <= 32, 64 otherwise with the lanes striding over i
// (cost_logitce_kernel's assignment: the lanes of a segment read consecutive words of one column).  Per column: max, sum exp,
// then sum Y (yhat - lse).
__global__ __launch_bounds__(256) void lik_logitce_kernel(const double* __restrict__ Y, const double* __restrict__ Yhat, int64_t yhat_stride,
                                                          int out, int64_t nb, int seg, double* __restrict__ part) {
  __shared__ double red[4];
  const int lane = threadIdx.x & 63;
  const int cpw = 64 / seg, sidx = lane / seg, pos = lane - sidx * seg;
  const int64_t nwaves = (int64_t)gridDim.x * 4, ngroups = (nb + cpw - 1) / cpw;
  Yhat += (int64_t)blockIdx.y * yhat_stride;   // chain slot
  part += (int64_t)blockIdx.y * gridDim.x;
  double acc = 0.0;
  for (int64_t grp = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); grp < ngroups; grp += nwaves) {   // (wave-uniform)
    const int64_t b = grp * cpw + sidx;
    const bool valid = b < nb;
    const int iend = valid ? out : 0;   // (a column past the batch is never read)
    const double* __restrict__ yh = Yhat + b * out;
    const double* __restrict__ y = Y + b * out;
    double m = -__builtin_inf();
    for (int i = pos; i < iend; i += seg) m = fmax(m, yh[i]);
    m = seg_max(m, seg);
    double se = 0.0;
    for (int i = pos; i < iend; i += seg) se += exp(yh[i] - m);
    se = seg_sum(se, seg);
    const double lse = m + log(se);
    double t = 0.0;
    for (int i = pos; i < iend; i += seg) t += y[i] * (yh[i] - lse);
    t = seg_sum(t, seg);
    if (valid && pos == 0) acc -= t;
  }
  acc = cost_block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// the elementwise likelihood (kind 2): one summand per element, a grid-stride sweep per workgroup
__global__ __launch_bounds__(256) void lik_elem_kernel(const double* __restrict__ Y, const double* __restrict__ Yhat, int64_t yhat_stride,
                                                       int64_t d, double* __restrict__ part) {
  __shared__ double red[4];
  Yhat += (int64_t)blockIdx.y * yhat_stride;   // chain slot
  part += (int64_t)blockIdx.y * gridDim.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double acc = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < d; e += stride) {
    const double yh = Yhat[e], y = Y[e];
    // (1 - y) yhat + softplus(-yhat), softplus(-x) = max(-x, 0) + log1p(exp(-|x|))
    const double t = exp(-fabs(yh));
    acc += (1.0 - y) * yh + (yh < 0.0 ? -yh : 0.0) + log1p(t);
  }
  acc = cost_block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

void launch_lik(hipStream_t st, int kind, const double* Y, const double* Yhat, int64_t yhat_stride, int32_t out, int64_t B, double* part,
                int nparts, double* nll_out, int nc, bool with_final) {
  const dim3 grid((unsigned)nparts, (unsigned)nc);
  if (kind == 1) {
    int seg = 64;
    if (out <= 32)
      for (seg = 1; seg < out; seg <<= 1) {}
    hipLaunchKernelGGL(lik_logitce_kernel, grid, dim3(256), 0, st, Y, Yhat, yhat_stride, out, B, seg, part);
  } else {
    hipLaunchKernelGGL(lik_elem_kernel, grid, dim3(256), 0, st, Y, Yhat, yhat_stride, (int64_t)out * B, part);
  }
  if (with_final) launch_sse_final(st, part, nparts, nll_out, nc);
}

}  // namespace si
