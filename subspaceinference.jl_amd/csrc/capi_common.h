// Declarations shared by the translation units of the C ABI (capi.hip: context + construction; capi_infer.hip: inference set-up,
// density, gradient, predictive forward; capi_sample.hip: the RWMH samplers and the output map; capi_mala.hip: the MALA sampler; capi_hmc.hip: the HMC sampler; capi_advi.hip: the ADVI fit).  Nothing here is part of the
// public interface (include/subspace_hip.h).  Buffers are owned by the types of dev_buf.h (through si_internal.h): no file of
// the C ABI calls hipMalloc / hipFree / hipHostMalloc / hipHostFree or creates an event by hand.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "si_internal.h"

namespace si {

void free_infer(Ctx* c);   // capi.hip: everything si_infer_setup allocated
// the acceptance rates of a finished chain from its per-chain accept counts (one place for all sampler forms and si_rwmh_end)
inline void accept_rates(const std::vector<int64_t>& nacc, int64_t itr, double* out) {
  for (size_t c = 0; out && c < nacc.size(); ++c) out[c] = itr > 1 ? (double)nacc[c] / (double)(itr - 1) : 0.0;
}

}  // namespace si

#define CHECK_CTX(ctx) \
  if (!(ctx)) return SI_ERR_INVALID
#define BIND(ctx) SI_HIP(ctx, hipSetDevice((ctx)->device))

extern "C" {   // (defined inside the extern "C" blocks of their translation units; not exported by include/subspace_hip.h)
// capi_infer.hip
int32_t ensure_chains(si_ctx* ctx, int32_t C);   // forward workspace + sampler state for C chains
int32_t eval_density(si_ctx* ctx, int c0, int nc, const double** yhat_out);   // d_zprop[:, c0 .. c0+nc) -> d_sse
int32_t eval_density_all(si_ctx* ctx, int C);
double mvnormal_c0(double d, double sigma);
double prior_c0(const si_ctx* ctx);
void fused_fill_program(const si_ctx* ctx, si::ChainFusedPlan& fp);
// the gradient entry points' state rules; value and gradient at one point through the per-layer launches (synchronises); the fused
// route of si_logdensity_grad_batch: its class / workgroups per point / points per pass, its workspace, one queued pass
int32_t grad_entry_check(si_ctx* ctx, const char* who, bool args_ok);
int32_t logdensity_grad_point(si_ctx* ctx, const double* z, double* lp_out, double* grad_out);
int vgrad_route(si_ctx* ctx, int64_t* G_out, int64_t* fit_out);
int32_t vgrad_ensure(si_ctx* ctx, const char* who, int cap, int64_t G);
void vgrad_pass(si_ctx* ctx, int nb, int64_t G, const double* z_dev, int n, double* lp_dev, double* gz_dev);
}
