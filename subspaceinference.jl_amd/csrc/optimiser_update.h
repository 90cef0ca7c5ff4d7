// The update rule of the on-device training step, written once: optimiser_kernel (capi_train.hip) and node_train_tail_kernel<true>
// (kernels_node_train.hip) both call it, tests/test_gpu_optimiser_audit.py and tests/test_gpu_node_train.py pin it bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace si {

// Flux 0.11.2 apply! + update! on element i:  x .-= apply!(opt, x, g), state zero(x) (Float32), arithmetic in Float64; returns
// the new w[i].  Descent touches neither m nor v, Momentum not v.  No product is contracted with a sum, whatever the flags of
// the file that includes this.
// g32: the gradient arrays are Float32 (compute_dtype = SI_F32: g holds Float32 values) -- then `apply!` writes its step back
// into the Float32 array `delta` (rounded) and `x .-= delta` is a Float32 subtraction; with a Float64 gradient the step stays
// Float64 and x - step is rounded once on the store into x
__device__ __forceinline__ float optimiser_update(float* w, float* m, float* v, int64_t i, double gi, int kind, double eta, double p1,
                                                  double p2, double bp1, double bp2, bool g32) {
#pragma clang fp contract(off)
  double step;
  if (kind == 0) {  // Descent: delta .*= eta
    step = gi * eta;
  } else if (kind == 1) {  // Momentum: v = rho*v - eta*delta; delta = -v
    const float vn = (float)(p1 * (double)m[i] - eta * gi);
    m[i] = vn;
    step = -(double)vn;
  } else {  // ADAM
    const float mt = (float)(p1 * (double)m[i] + (1.0 - p1) * gi);
    const float vt = (float)(p2 * (double)v[i] + (1.0 - p2) * (gi * gi));
    m[i] = mt;
    v[i] = vt;
    step = (double)mt / (1.0 - bp1) / (sqrt((double)vt / (1.0 - bp2)) + 1e-8) * eta;
  }
  const float wn = g32 ? w[i] - (float)step : (float)((double)w[i] - step);
  w[i] = wn;
  return wn;
}

// the same rule on Float64 parameters (si_ae_train_setup with SI_F64): Flux keeps zero(x) as state, so m and v are Float64 and
// nothing is rounded to Float32 -- every expression as above
__device__ __forceinline__ double optimiser_update(double* w, double* m, double* v, int64_t i, double gi, int kind, double eta, double p1,
                                                   double p2, double bp1, double bp2, bool /*g32: a Float64 array has no Float32 gradient*/) {
#pragma clang fp contract(off)
  double step;
  if (kind == 0) {
    step = gi * eta;
  } else if (kind == 1) {
    const double vn = p1 * m[i] - eta * gi;
    m[i] = vn;
    step = -vn;
  } else {
    const double mt = p1 * m[i] + (1.0 - p1) * gi;
    const double vt = p2 * v[i] + (1.0 - p2) * (gi * gi);
    m[i] = mt;
    v[i] = vt;
    const double c1 = 1.0 - bp1, c2 = 1.0 - bp2;   // (the bias corrections' denominators, as above)
    step = mt / c1 / (sqrt(vt / c2) + 1e-8) * eta;
  }
  const double wn = w[i] - step;
  w[i] = wn;
  return wn;
}

}  // namespace si
