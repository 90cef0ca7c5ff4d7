// C ABI of method = :diffusion (include/subspace_hip.h): si_construct_finish_diffmap replaces the reference's
// `fit(DiffMap, A', maxoutdim = M); transform` (src/subspace_construction.jl:202-206).  The definition
// [upstream, from memory, unverifiable offline] is in the header and restated in diffmap.py; the kernels are kernels_diffmap.hip.
// Host-side orchestration only, plus the small dense algebra of the eigensolver (matrices of the block width).
//
// The reference takes a full SVD of the N x N matrix Kn.  Here only the M + 1 leading vectors are computed:
//   * u_1 = q / ||q|| (lambda_1 = 1) is known analytically and deflated, never iterated for;
//   * the rest by block subspace iteration with b = min(N - 1, 2M + 16) columns.  Per iteration
//       W = Kn V                      K3 (launch_project; its right factor is V', one transpose kernel), then W -= u_1 (u_1' W)
//       G = [V W]' [V W]              one K2 launch on the stacked N x 2b block: V'V, V'W and W'W together
//       host: Rayleigh-Ritz           V'V = L L', H = L^-1 sym(V'W) L^-T (si_host_sym_eig), Ritz pairs (theta, y) by |theta|.
//                                     The GENERALISED problem: the block need not be orthonormal, only well conditioned.
//       next block = [V W] T          one K3 launch.  Column j is W y_j / theta_j (a power step of Ritz vector j) while
//                                     |theta_j| >= 1e-6 |theta_1|, else the Ritz vector V y_j itself (a power step of it would be
//                                     rounding noise); T also orthonormalises the columns (Cholesky of the PREDICTED Gram
//                                     matrix T0' G T0, a column whose pivot collapses falling back to its Ritz vector).  What the
//                                     prediction misses -- Cholesky-style orthonormalisation loses cond^2 * eps -- the next
//                                     iteration's V'V measures on the vectors themselves and the generalised problem takes
//                                     into account: that second factorisation is the second orthonormalisation.
//     One synchronisation per iteration (the download of G).
//   * residuals: r_j^2 = c' G c with c = [-theta_j y_j; y_j] comes from the same Gram entries, but as a difference of O(1)
//     numbers it bottoms out near 1e-8.  It is the SCREEN: once every leading r_j is below 1e-6 the residual vectors
//     [V W] c are formed (one K3 launch on M columns) and their norms summed in a fixed order; the iteration stops when every
//     one is <= tol.  Those iterations synchronise twice.
#include <chrono>
#include <cstdio>

#include "capi_common.h"

using namespace si;

namespace {

constexpr int64_t DM_MAX_N = 65536;

// column-major n x n helpers of the block width
inline double& at(std::vector<double>& a, int n, int i, int j) { return a[(size_t)i + (size_t)n * j]; }
inline double at(const std::vector<double>& a, int n, int i, int j) { return a[(size_t)i + (size_t)n * j]; }

// a = L L' (lower, in place; the upper triangle is left alone); false when a pivot is not positive
bool chol_lower(int n, std::vector<double>& a) {
  for (int j = 0; j < n; ++j) {
    double d = at(a, n, j, j);
    for (int k = 0; k < j; ++k) d -= at(a, n, j, k) * at(a, n, j, k);
    if (!(d > 0.0)) return false;
    d = std::sqrt(d);
    at(a, n, j, j) = d;
    for (int i = j + 1; i < n; ++i) {
      double s = at(a, n, i, j);
      for (int k = 0; k < j; ++k) s -= at(a, n, i, k) * at(a, n, j, k);
      at(a, n, i, j) = s / d;
    }
  }
  return true;
}
void solve_lower(int n, const std::vector<double>& L, double* x) {   // x <- L^-1 x
  for (int i = 0; i < n; ++i) {
    double s = x[i];
    for (int k = 0; k < i; ++k) s -= at(L, n, i, k) * x[k];
    x[i] = s / at(L, n, i, i);
  }
}
void solve_lower_t(int n, const std::vector<double>& L, double* x) {   // x <- L^-T x
  for (int i = n - 1; i >= 0; --i) {
    double s = x[i];
    for (int k = i + 1; k < n; ++k) s -= at(L, n, k, i) * x[k];
    x[i] = s / at(L, n, i, i);
  }
}

struct Ritz {
  std::vector<double> theta;   // b, |.| descending
  std::vector<double> Y;       // b x b, column j = coefficients of Ritz vector j in V (y' V'V y = 1)
  std::vector<double> screen;  // b: the residual of pair j as the Gram entries give it
};

// Rayleigh-Ritz of the stacked Gram matrix G (2b x 2b).  false: V'V is not positive definite or the eigensolver failed.
bool rayleigh_ritz(int b, const std::vector<double>& G, Ritz& out) {
  const int n2 = 2 * b;
  std::vector<double> L((size_t)b * b), Hs((size_t)b * b), H((size_t)b * b);
  for (int j = 0; j < b; ++j)
    for (int i = 0; i < b; ++i) {
      at(L, b, i, j) = at(G, n2, i, j);
      at(Hs, b, i, j) = 0.5 * (at(G, n2, i, b + j) + at(G, n2, j, b + i));
    }
  if (!chol_lower(b, L)) return false;
  // H = L^-1 Hs L^-T: T1 = L^-1 Hs by columns, then H' = L^-1 T1'
  std::vector<double> T1 = Hs, col((size_t)b);
  for (int j = 0; j < b; ++j) solve_lower(b, L, T1.data() + (size_t)j * b);
  for (int i = 0; i < b; ++i) {
    for (int j = 0; j < b; ++j) col[(size_t)j] = at(T1, b, i, j);
    solve_lower(b, L, col.data());
    for (int j = 0; j < b; ++j) at(H, b, i, j) = col[(size_t)j];
  }
  for (int j = 0; j < b; ++j)
    for (int i = 0; i < j; ++i) at(H, b, i, j) = at(H, b, j, i) = 0.5 * (at(H, b, i, j) + at(H, b, j, i));
  std::vector<double> w((size_t)b);
  if (sym_eig(b, H.data(), w.data()) != 0) return false;
  std::vector<int> idx((size_t)b);
  for (int i = 0; i < b; ++i) idx[(size_t)i] = i;
  for (int i = 1; i < b; ++i)   // insertion sort by |w| descending (stable)
    for (int k = i; k > 0 && std::fabs(w[(size_t)idx[(size_t)k]]) > std::fabs(w[(size_t)idx[(size_t)k - 1]]); --k)
      std::swap(idx[(size_t)k], idx[(size_t)k - 1]);
  out.theta.assign((size_t)b, 0.0);
  out.Y.assign((size_t)b * b, 0.0);
  out.screen.assign((size_t)b, 0.0);
  for (int j = 0; j < b; ++j) {
    const double th = w[(size_t)idx[(size_t)j]];
    double* y = out.Y.data() + (size_t)j * b;
    std::copy(H.begin() + (size_t)idx[(size_t)j] * b, H.begin() + (size_t)(idx[(size_t)j] + 1) * b, y);
    solve_lower_t(b, L, y);
    out.theta[(size_t)j] = th;
    double yWWy = 0.0, yHy = 0.0;
    for (int c = 0; c < b; ++c) {
      double sw = 0.0, sh = 0.0;
      for (int r = 0; r < b; ++r) sw += at(G, n2, b + r, b + c) * y[r], sh += at(Hs, b, r, c) * y[r];
      yWWy += sw * y[c], yHy += sh * y[c];
    }
    const double r2 = yWWy - 2.0 * th * yHy + th * th;
    out.screen[(size_t)j] = r2 > 0.0 ? std::sqrt(r2) : 0.0;
  }
  return true;
}

// T (2b x b): the next block is [V W] T (see the header comment)
void next_block(int b, const std::vector<double>& G, const Ritz& rz, std::vector<double>& T) {
  const int n2 = 2 * b;
  std::vector<double> C((size_t)n2 * b, 0.0), GC((size_t)n2 * b), R((size_t)b * b, 0.0), g((size_t)b);
  const double floor_theta = 1e-6 * std::fabs(rz.theta[0]);
  auto set_col = [&](int j, bool power) {
    double* c = C.data() + (size_t)j * n2;
    std::fill(c, c + n2, 0.0);
    const double* y = rz.Y.data() + (size_t)j * b;
    for (int r = 0; r < b; ++r) c[(power ? b : 0) + r] = power ? y[r] / rz.theta[(size_t)j] : y[r];
    double* gc = GC.data() + (size_t)j * n2;
    for (int i = 0; i < n2; ++i) {
      double s = 0.0;
      for (int k = 0; k < n2; ++k) s += at(G, n2, i, k) * c[k];
      gc[i] = s;
    }
  };
  for (int j = 0; j < b; ++j) {
    bool power = std::fabs(rz.theta[(size_t)j]) >= floor_theta && rz.theta[(size_t)j] != 0.0;
    for (;;) {
      set_col(j, power);
      const double* gc = GC.data() + (size_t)j * n2;
      for (int i = 0; i <= j; ++i) {   // g_i = c_i' G c_j
        const double* ci = C.data() + (size_t)i * n2;
        double s = 0.0;
        for (int k = 0; k < n2; ++k) s += ci[k] * gc[k];
        g[(size_t)i] = s;
      }
      double piv = g[(size_t)j];
      for (int i = 0; i < j; ++i) {
        double s = g[(size_t)i];
        for (int k = 0; k < i; ++k) s -= at(R, b, k, i) * at(R, b, k, j);
        at(R, b, i, j) = s / at(R, b, i, i);
        piv -= at(R, b, i, j) * at(R, b, i, j);
      }
      const double least = 1e-6 * std::fabs(g[(size_t)j]);
      if (piv >= least && piv > 0.0) {
        at(R, b, j, j) = std::sqrt(piv);
        break;
      }
      if (power) {
        power = false;   // its power step has nothing new in it: keep the Ritz vector
        continue;
      }
      at(R, b, j, j) = std::sqrt(least > 0.0 ? least : 1.0);   // (the next iteration's V'V is the judge of this block)
      break;
    }
  }
  // T R = C
  T.assign((size_t)n2 * b, 0.0);
  for (int j = 0; j < b; ++j) {
    double* t = T.data() + (size_t)j * n2;
    std::copy(C.begin() + (size_t)j * n2, C.begin() + (size_t)(j + 1) * n2, t);
    for (int k = 0; k < j; ++k) {
      const double r = at(R, b, k, j);
      const double* tk = T.data() + (size_t)k * n2;
      for (int i = 0; i < n2; ++i) t[i] -= tk[i] * r;
    }
    const double d = at(R, b, j, j);
    for (int i = 0; i < n2; ++i) t[i] /= d;
  }
}

uint64_t splitmix(uint64_t& s) {
  uint64_t z = (s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// cols (rows x ncol, column-major host) -> the right factor of launch_project: dst[k * Mpad + m], zero padded
void to_right_factor(const double* cols, int rows, int ncol, int Mpad, double* dst) {
  std::fill(dst, dst + (size_t)rows * Mpad, 0.0);
  for (int m = 0; m < ncol; ++m)
    for (int k = 0; k < rows; ++k) dst[(size_t)k * Mpad + m] = cols[(size_t)m * rows + k];
}

int32_t zero_alloc(si_ctx* ctx, DevBuf<double>& buf, size_t elems, const char* what) {
  if (buf.size() >= elems && buf != nullptr) return SI_OK;
  if (!buf.alloc(elems)) return fail(ctx, SI_ERR_NOMEM, std::string("si_construct_finish_diffmap: allocation of ") + what + " failed");
  SI_HIP(ctx, hipMemsetAsync(buf, 0, elems * sizeof(double), ctx->stream));
  return SI_OK;
}

}  // namespace

extern "C" {

int32_t si_construct_finish_diffmap(si_ctx* ctx, int32_t M, double eps, double alpha, int32_t kernel_sign, int32_t rescale, double tol,
                                    int32_t max_iters, double* W_swa_out, double* P_out, double* lambda_out, int64_t* K_out) {
  CHECK_CTX(ctx);
  const char* who = "si_construct_finish_diffmap: ";
  DiffmapState& dm = ctx->dm;
  dm.iters = 0, dm.residual = 0.0;
  if (!ctx->c_active || ctx->K <= 0) return fail(ctx, SI_ERR_STATE, std::string(who) + "nothing pushed");
  if (M < 1) return fail(ctx, SI_ERR_INVALID, std::string(who) + "M must be positive");
  if (!std::isfinite(eps) || !std::isfinite(alpha) || !(eps > 0.0))
    return fail(ctx, SI_ERR_INVALID, std::string(who) + "eps must be positive and finite, alpha finite");
  if (kernel_sign != 1 && kernel_sign != -1) return fail(ctx, SI_ERR_INVALID, std::string(who) + "kernel_sign must be +1 or -1");
  const int64_t N = ctx->N, K = ctx->K, ldn = ctx->ldA;
  if (K_out) *K_out = K;
  if (N > DM_MAX_N)
    return fail(ctx, SI_ERR_INVALID, std::string(who) + "N = " + std::to_string(N) + " > 65536: the dense N x N fp64 kernel matrix is 34 GB at "
                "that size (a matrix-free variant is not part of this build)");
  if ((int64_t)M + 1 > N - 1) return fail(ctx, SI_ERR_BOUNDS, "BoundsError: the diffusion map needs M + 1 <= N - 1 non-trivial vectors");
  if (!(tol > 0.0)) tol = 1e-12;
  if (max_iters <= 0) max_iters = 500;
  BIND(ctx);
  if (const int32_t rcn = train_node_report(ctx, "si_construct_finish_diffmap")) return rcn;   // (queued NeuralODE training steps: a failed one)
  hipStream_t st = ctx->stream;
  int32_t rc;
  dm.N = 0;  // the read-back is valid again once this call has built its kernel matrix
  const int b = (int)std::min<int64_t>(N - 1, 2 * (int64_t)M + 16), n2 = 2 * b;
  const int Kp = (int)((K + 3) / 4 * 4), nb = dm_blocks(N);
  const int64_t Npad = (int64_t)nb * 64, ldt = pad_ld(b);
  const int Mpad_b = project_mpad(b), Mpad_m = project_mpad(M);
  SI_HIP(ctx, hipStreamSynchronize(st));
  // ---- buffers (kept for the next call of this construction).  Everything a kernel reads beyond what is written is zero.
  if (dm.Kn.size() < (size_t)ldn * N) {
    if (!dm.Kn.alloc((size_t)ldn * N)) return fail(ctx, SI_ERR_NOMEM, std::string(who) + "allocation of the N x N kernel matrix failed");
    if (ldn > N)   // the padding rows [N, ldn) of every column, once: the kernels write rows < N only
      SI_HIP(ctx, hipMemset2DAsync(dm.Kn + N, (size_t)ldn * sizeof(double), 0, (size_t)(ldn - N) * sizeof(double), (size_t)N, st));
  }
  dm.Xr.reset();   // K differs between calls of one construction: rows [K, Kp) and columns [N, Npad) must be zero
  if ((rc = zero_alloc(ctx, dm.Xr, (size_t)Kp * Npad, "Xr")) != SI_OK) return rc;
  dm.s.reset();
  if ((rc = zero_alloc(ctx, dm.s, (size_t)Npad, "s")) != SI_OK) return rc;
  if (!dm.mm.reserve((size_t)2 * K) || !dm.part.reserve((size_t)nb * ldn) || !dm.p.reserve((size_t)ldn) || !dm.q.reserve((size_t)ldn) ||
      !dm.u1.reserve((size_t)ldn) || !dm.flag.reserve(1) || !dm.res.reserve((size_t)M) || !dm.G.reserve((size_t)n2 * n2) ||
      !dm.coef.reserve((size_t)n2 * std::max(Mpad_b, Mpad_m)))
    return fail(ctx, SI_ERR_NOMEM, std::string(who) + "allocation of the work vectors failed");
  dm.Z[0].reset(), dm.Z[1].reset(), dm.R.reset(), dm.Vt.reset();   // (b depends on M: sized and zeroed per call)
  if ((rc = zero_alloc(ctx, dm.Z[0], (size_t)ldn * n2, "the block")) != SI_OK) return rc;
  if ((rc = zero_alloc(ctx, dm.Z[1], (size_t)ldn * n2, "the block")) != SI_OK) return rc;
  if ((rc = zero_alloc(ctx, dm.R, (size_t)ldn * M, "the residual vectors")) != SI_OK) return rc;
  if ((rc = zero_alloc(ctx, dm.Vt, (size_t)ldt * N, "V'")) != SI_OK) return rc;
  const size_t gneed = launch_gram(st, dm.Z[0], ldn, N, n2, nullptr, nullptr, ctx->num_cu, nullptr);
  if (!dm.Gpart.reserve(gneed / sizeof(double) + 1)) return fail(ctx, SI_ERR_NOMEM, std::string(who) + "partial-slab allocation failed");
  const size_t pin_elems = (size_t)n2 * n2 + (size_t)n2 * std::max(Mpad_b, Mpad_m) + (size_t)M + 8;
  if (ctx->h_pin.size() < pin_elems && !ctx->h_pin.reserve(pin_elems))
    return fail(ctx, SI_ERR_NOMEM, std::string(who) + "pinned staging allocation failed");
  double* const hG = ctx->h_pin;
  double* const hcoef = hG + (size_t)n2 * n2;
  double* const hres = hcoef + (size_t)n2 * std::max(Mpad_b, Mpad_m);

  // ---- steps 1-3: Xr, Kmat, the two normalisations, u_1
  SI_HIP(ctx, hipMemsetAsync(dm.flag, 0, sizeof(int), st));
  {
    ProfScope ps(ctx, SI_K_PUSH, 0.0, (double)N * (double)K * (ctx->a_dtype == SI_F32 ? 4.0 : 8.0) * (rescale ? 2.0 : 1.0) + (double)N * Kp * 8.0);
    launch_dm_rescale(st, ctx->d_A, ctx->a_dtype, ldn, N, (int)K, Kp, rescale ? 1 : 0, dm.mm, dm.Xr, dm.s);
  }
  {
    ProfScope ps(ctx, SI_K_GRAM, (double)N * (double)N * (double)Kp, (double)N * (double)N * 8.0);   // half the products: the upper triangle
    launch_dm_pairwise(st, dm.Xr, Kp, dm.s, N, kernel_sign, eps, dm.Kn, ldn, dm.part, dm.flag);
  }
  {
    ProfScope ps(ctx, SI_K_GRAM_RED, 0.0, 4.0 * (double)N * (double)N * 8.0);   // two read-modify-write passes over Kmat
    launch_dm_sum_parts(st, dm.part, ldn, N, false, dm.p);
    launch_dm_scale_rows(st, dm.Kn, ldn, N, dm.p, alpha, true, dm.part);
    launch_dm_sum_parts(st, dm.part, ldn, N, true, dm.q);
    launch_dm_scale_rows(st, dm.Kn, ldn, N, dm.q, 1.0, false, nullptr);
    launch_dm_unit(st, dm.q, N, dm.u1);
  }
  SI_HIP(ctx, hipGetLastError());
  int hflag = 0;
  SI_HIP(ctx, hipMemcpyAsync(&hflag, dm.flag, sizeof(int), hipMemcpyDeviceToHost, st));
  // ---- the start block: fixed pseudo-random columns (the same for every call), u_1 deflated
  {
    std::vector<double> v0((size_t)N * b);
    uint64_t seed = 0x5bd1e995ull;
    for (double& x : v0) x = (double)(splitmix(seed) >> 11) * (1.0 / 9007199254740992.0) - 0.5;
    SI_HIP(ctx, hipMemcpy2DAsync(dm.Z[0], (size_t)ldn * sizeof(double), v0.data(), (size_t)N * sizeof(double), (size_t)N * sizeof(double),
                                 (size_t)b, hipMemcpyHostToDevice, st));
    SI_HIP(ctx, hipStreamSynchronize(st));   // (v0 is released; the flag has arrived)
  }
  if (hflag != 0)
    return fail(ctx, SI_ERR_INVALID, std::string(who) + "the kernel matrix has a non-finite entry (exp(kernel_sign * d / eps) overflows: "
                "kernel_sign = +1 with squared distances / eps beyond 709)");
  dm.N = N;   // Kn and u_1 are what the audit read-back returns, whether or not the iteration below converges
  launch_dm_deflate(st, dm.Z[0], ldn, N, b, dm.u1);

  // ---- block subspace iteration
  std::vector<double> G((size_t)n2 * n2), T;
  Ritz rz;
  int cur = 0;
  bool converged = false;
  double last_res = INFINITY;
  int it = 0;
  for (it = 1; it <= max_iters; ++it) {
    double* Z = dm.Z[cur];
    launch_transpose(st, Z, SI_F64, ldn, N, b, dm.Vt, ldt);
    {
      ProfScope ps(ctx, SI_K_PROJECT, 2.0 * (double)N * (double)N * (double)b, (double)N * (double)N * 8.0 + 2.0 * (double)N * b * 8.0);
      launch_project(st, dm.Kn, ldn, N, N, dm.Vt, b, (int32_t)ldt, Z + (size_t)b * ldn, ldn, ctx->num_cu);
    }
    launch_dm_deflate(st, Z + (size_t)b * ldn, ldn, N, b, dm.u1);
    launch_gram(st, Z, ldn, N, n2, dm.Gpart, dm.G, ctx->num_cu, nullptr);
    SI_HIP(ctx, hipGetLastError());
    SI_HIP(ctx, hipMemcpyAsync(hG, dm.G, (size_t)n2 * n2 * sizeof(double), hipMemcpyDeviceToHost, st));
    SI_HIP(ctx, hipStreamSynchronize(st));
    std::copy(hG, hG + (size_t)n2 * n2, G.begin());
    const auto t0 = std::chrono::steady_clock::now();
    const bool ok = rayleigh_ritz(b, G, rz);
    if (ok) next_block(b, G, rz, T);
    ctx->stats.ms[SI_K_EIG_HOST] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    ctx->stats.launches[SI_K_EIG_HOST] += 1;
    dm.iters = it;
    if (!ok)
      return fail(ctx, SI_ERR_INVALID, std::string(who) + "the block lost its rank at iteration " + std::to_string(it) +
                  " (V'V is not positive definite, or the host eigensolver did not converge)");
    double screen = 0.0;
    for (int j = 0; j < M; ++j) screen = std::max(screen, rz.screen[(size_t)j]);
    if (!(screen > std::max(1e-6, tol))) {
      // the residual vectors themselves: R[:, j] = W y_j - theta_j V y_j
      std::vector<double> cres((size_t)n2 * M, 0.0);
      for (int j = 0; j < M; ++j)
        for (int r = 0; r < b; ++r) {
          const double y = rz.Y[(size_t)j * b + r];
          cres[(size_t)j * n2 + r] = -rz.theta[(size_t)j] * y;
          cres[(size_t)j * n2 + b + r] = y;
        }
      to_right_factor(cres.data(), n2, M, Mpad_m, hcoef);
      SI_HIP(ctx, hipMemcpyAsync(dm.coef, hcoef, (size_t)n2 * Mpad_m * sizeof(double), hipMemcpyHostToDevice, st));
      {
        ProfScope ps(ctx, SI_K_PROJECT, 2.0 * (double)N * n2 * M, (double)N * (n2 + M) * 8.0);
        launch_project(st, Z, ldn, N, n2, dm.coef, M, Mpad_m, dm.R, ldn, ctx->num_cu);
      }
      launch_dm_colnorm(st, dm.R, ldn, N, M, dm.res);
      SI_HIP(ctx, hipGetLastError());
      SI_HIP(ctx, hipMemcpyAsync(hres, dm.res, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, st));
      SI_HIP(ctx, hipStreamSynchronize(st));
      last_res = 0.0;
      for (int j = 0; j < M; ++j) last_res = std::max(last_res, hres[j]);
      if (!(last_res == last_res)) last_res = INFINITY;
      dm.residual = last_res;
      if (last_res <= tol) {
        converged = true;
        break;
      }
    } else {
      dm.residual = last_res = screen;
    }
    to_right_factor(T.data(), n2, b, Mpad_b, hcoef);
    SI_HIP(ctx, hipMemcpyAsync(dm.coef, hcoef, (size_t)n2 * Mpad_b * sizeof(double), hipMemcpyHostToDevice, st));
    {
      ProfScope ps(ctx, SI_K_PROJECT, 2.0 * (double)N * n2 * b, (double)N * (n2 + b) * 8.0);
      launch_project(st, Z, ldn, N, n2, dm.coef, b, Mpad_b, dm.Z[cur ^ 1], ldn, ctx->num_cu);
    }
    SI_HIP(ctx, hipGetLastError());
    cur ^= 1;   // (the pinned coefficients are next written after the next iteration's synchronisation, which this upload precedes)
  }
  if (!converged) {
    char msg[256];
    snprintf(msg, sizeof msg, "%snot converged after %d iterations: largest leading residual %.3e > tol %.3e (the leading spectrum is not "
             "separated from the rest; the reference's full SVD has no such limit)", who, dm.iters, last_res, tol);
    return fail(ctx, SI_ERR_INVALID, msg);
  }
  // ---- step 5: u_{j+1} = V y_j, P[:, j] = sign_j u_{j+1} ./ u_1
  double* const U = dm.Z[cur ^ 1];
  to_right_factor(rz.Y.data(), b, M, Mpad_m, hcoef);
  SI_HIP(ctx, hipMemcpyAsync(dm.coef, hcoef, (size_t)b * Mpad_m * sizeof(double), hipMemcpyHostToDevice, st));
  {
    ProfScope ps(ctx, SI_K_PROJECT, 2.0 * (double)N * b * M, (double)N * (b + M) * 8.0);
    launch_project(st, dm.Z[cur], ldn, N, b, dm.coef, M, Mpad_m, U, ldn, ctx->num_cu);
  }
  if ((rc = construct_alloc_P(ctx, M)) != SI_OK) return rc;
  launch_dm_finish(st, U, ldn, N, M, dm.u1, ctx->d_P, ldn);
  SI_HIP(ctx, hipGetLastError());
  ctx->svals.assign((size_t)M, 0.0);
  for (int j = 0; j < M; ++j) ctx->svals[(size_t)j] = std::fabs(rz.theta[(size_t)j]);
  if (lambda_out) {
    lambda_out[0] = 1.0;
    for (int j = 0; j < M; ++j) lambda_out[j + 1] = rz.theta[(size_t)j];
  }
  if (W_swa_out) SI_HIP(ctx, hipMemcpyAsync(W_swa_out, ctx->d_swa, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
  if (P_out)
    SI_HIP(ctx, hipMemcpy2DAsync(P_out, (size_t)N * sizeof(double), ctx->d_P, (size_t)ldn * sizeof(double), (size_t)N * sizeof(double),
                                 (size_t)M, hipMemcpyDeviceToHost, st));
  SI_HIP(ctx, hipStreamSynchronize(st));
  ctx->M_built = M;
  ctx->c_finished = true;
  return SI_OK;
}

int32_t si_diffmap_info(si_ctx* ctx, int32_t* iters_out, double* residual_out) {
  CHECK_CTX(ctx);
  if (iters_out) *iters_out = ctx->dm.iters;
  if (residual_out) *residual_out = ctx->dm.residual;
  return SI_OK;
}

int32_t si_diffmap_get_kernel(si_ctx* ctx, double* Kn_out, double* u1_out) {
  CHECK_CTX(ctx);
  const int64_t N = ctx->dm.N;
  if (N <= 0 || N != ctx->N) return fail(ctx, SI_ERR_STATE, "si_diffmap_get_kernel: no successful si_construct_finish_diffmap on this construction");
  BIND(ctx);
  if (Kn_out)
    SI_HIP(ctx, hipMemcpy2DAsync(Kn_out, (size_t)N * sizeof(double), ctx->dm.Kn, (size_t)ctx->ldA * sizeof(double), (size_t)N * sizeof(double),
                                 (size_t)N, hipMemcpyDeviceToHost, ctx->stream));
  if (u1_out) SI_HIP(ctx, hipMemcpyAsync(u1_out, ctx->dm.u1, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  SI_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SI_OK;
}

}  // extern "C"
