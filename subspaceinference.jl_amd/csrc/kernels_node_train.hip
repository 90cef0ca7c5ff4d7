// The tail of a NeuralODE training step (si_train_setup_node; node.py: train_value_and_grad is the definition): what follows the
// forward with record and the reverse kernel of kernels_node.hip.  One launch instead of four (the sum of the batch's gradient
// slices, the penalty, the update and the Float32 -> Float64 copy of capi_train.hip); the update is optimiser_update
// (optimiser_update.h), the function optimiser_kernel calls.  gfx950, fp64, compiled without contraction of a*b+c: every product
// and sum is rounded on its own, in the written order.
//
// One thread per weight element, 256-thread blocks, ceil(N / 256) blocks.  No atomics, no spinning, no workgroup barrier, plain
// loads and stores; every loop is bounded by nb.  Every thread first reads the nb status words of the batch and the sticky failure
// word, so the branch that follows is uniform across the grid: on a failure NOTHING is stored -- not gw, not the loss, not w, m,
// v or the Float64 copy -- except the failure record, which thread 0 of block 0 writes once (the first failing step wins: a set
// record is never overwritten).  (A thread that reads the record while thread 0 writes it leaves either way.)
#include "optimiser_update.h"
#include "si_internal.h"

namespace si {

template <bool APPLY>
__global__ __launch_bounds__(256) void node_train_tail_kernel(NodeTailArgs a) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool stuck = a.fail[0] != 0;
  int64_t bad_p = -1;
  int32_t bad_s = 0;
  for (int64_t p = 0; p < a.nb; ++p) {
    const int32_t s = a.status[p];
    if (s != 0 && bad_p < 0) bad_p = p, bad_s = s;
  }
  if (stuck || bad_p >= 0) {
    if (i == 0 && !stuck) a.fail[0] = a.step, a.fail[1] = bad_p, a.fail[2] = (int64_t)bad_s;
    return;
  }
  if (i == 0) {   // the loss of the batch before the update: the sums in ascending batch order from 0.0, then the penalty
    double sse = 0.0;
    for (int64_t p = 0; p < a.nb; ++p) sse = sse + a.ssep[p];
    *a.loss = a.penalty_div != 0.0 ? sse + a.wsq[0] / a.penalty_div : sse;
  }
  if (i >= a.N) return;
  double acc = 0.0;
  for (int64_t p = 0; p < a.nb; ++p) acc = acc + a.slices[p * a.N + i];
  const double gi = a.penalty_div != 0.0 ? (a.w64[i] * 2.0) / a.penalty_div - acc : 0.0 - acc;
  a.gw[i] = gi;
  if constexpr (APPLY) {   // the update with a Float64 gradient, and the copy the next step's solve reads
    a.w64[i] = (double)optimiser_update(a.w32, a.m32, a.v32, i, gi, a.kind, a.eta, a.p1, a.p2, a.bp1, a.bp2, /*g32=*/false);
  }
}

void launch_node_train_tail(hipStream_t st, const NodeTailArgs& a, bool apply) {
  const dim3 grid((unsigned)((a.N + 255) / 256));
  if (apply)
    hipLaunchKernelGGL(node_train_tail_kernel<true>, grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(node_train_tail_kernel<false>, grid, dim3(256), 0, st, a);
}

}  // namespace si
