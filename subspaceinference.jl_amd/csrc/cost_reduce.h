// The fixed-order reductions that the cost kernels (kernels_cost.hip) and the likelihood kernels (kernels_lik.hip) share: both
// translation units are compiled with -ffp-contract=off, and a sum formed through these has the same bits in either.
#pragma once
#include <hip/hip_runtime.h>

namespace si {

// the block's 256 values, summed in a fixed order: a butterfly within each wave (every lane ends with the same bits), then the
// four wave sums in ascending order
__device__ __forceinline__ double cost_block_sum(double v, double* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// reductions over the `seg` lanes of a column's segment (seg a power of two <= 64; segments are aligned): every lane of the
// segment ends with the same bits
__device__ __forceinline__ double seg_sum(double v, int seg) {
  for (int off = seg >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ double seg_max(double v, int seg) {
  for (int off = seg >> 1; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

}  // namespace si
