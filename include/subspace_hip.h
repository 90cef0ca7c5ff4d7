/* subspace_hip.h -- C ABI of libsubspace_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the ONE hot path of efmanu/SubspaceInference.jl: subspace construction
 * (SWA mean -> deviation matrix -> tall-skinny Gram/eigen -> projection P) and subspace sampling
 * (W_swa + P*z -> Dense-chain forward -> Gaussian log-likelihood -> random-walk Metropolis).
 *
 * The reference is inline Julia with no FFI seam of its own; each entry point below cites the
 * reference expression it replaces (paths relative to the reference repository root).  A Julia
 * `ccall` wrapper and a Python `ctypes` binding over exactly these symbols are shown in
 * INTEGRATION.md.
 *
 * Conventions
 *   - every function returns int32 status: 0 = SI_OK, negative = error; si_last_error(ctx) gives the
 *     message (owned by the library, valid until the next call on that ctx).  The host wrappers turn a
 *     non-zero status into the reference's error convention, `throw(::String)`.
 *   - host pointers are caller-owned, contiguous, COLUMN-MAJOR (Julia layout); they are only read or
 *     written during the call and never retained.  "_dev" variants take device pointers instead.
 *   - device memory is owned by the opaque si_ctx and released by si_destroy.
 *   - one ctx drives ONE GPU (one process per GPU); a ctx is used by one host thread at a time.  More than one GPU =
 *     one process (and ctx) per GPU joined by an RCCL communicator: the si_comm_* section below.
 *   - there is NO CPU backend: si_create fails when no gfx950 device is usable.
 */
#ifndef SUBSPACE_HIP_H
#define SUBSPACE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct si_ctx si_ctx;

enum {
  SI_OK = 0,
  SI_ERR_INVALID = -1,  /* bad argument                                         */
  SI_ERR_STATE = -2,    /* call out of order (e.g. push before begin)           */
  SI_ERR_HIP = -3,      /* HIP runtime error, message has the hipError string   */
  SI_ERR_NOMEM = -4,    /* device or host allocation failed                     */
  SI_ERR_BOUNDS = -5,   /* M > rank(A): the reference's BoundsError at U[:,1:M] */
  SI_ERR_NODEVICE = -6, /* no usable GPU                                        */
  SI_ERR_COMM = -7      /* RCCL error / RCCL not loadable, message has the detail */
};

enum { SI_F32 = 0, SI_F64 = 1 };                 /* dtype of a weight snapshot; compute_dtype of si_infer_setup */
/* Flux 0.11.2 / NNlib 0.7.23 definitions [upstream]: leakyrelu(x) = max(0.01 x, x); elu(x) = x >= 0 ? x : exp(x) - 1;
 * softplus(x) = log(1 + exp(x)); selu(x) = 1.0507009873554805 * (x > 0 ? x : 1.6732632423543772 * (exp(x) - 1)).
 * (gelu / swish are not monotone: their derivative cannot be rebuilt from the stored output, so they are not offered.) */
enum { SI_ACT_IDENTITY = 0, SI_ACT_RELU = 1, SI_ACT_TANH = 2, SI_ACT_SIGMOID = 3, SI_ACT_LEAKYRELU = 4, SI_ACT_ELU = 5,
       SI_ACT_SOFTPLUS = 6, SI_ACT_SELU = 7, SI_ACT_COUNT = 8 };
enum { SI_LAYER_DENSE = 0, SI_LAYER_CONV = 1, SI_LAYER_MAXPOOL = 2, SI_LAYER_FLATTEN = 3 };

/* One layer of a Flux Chain.  Layout contract of the whole path inside the flat weight vector (src/libs.jl:19-22
 * extract_params, src/libs.jl:55-57 Flux.destructure/re -- `model_re` restructures ANY Chain):
 *   Dense  [vec(W) (out x in, column-major); b]          Conv  [vec(weight) (kw x kh x cin x cout, column-major); bias]
 * in the order of the layers; MaxPool and flatten own no parameters.  Activations between layers are (features x B)
 * matrices whose feature index runs in Julia's (W, H, C) column-major order -- the (W, H, C, N) arrays of Flux.
 *   SI_LAYER_DENSE    in, out, act, w_off, b_off                                  (geometry fields unused: 0)
 *   SI_LAYER_CONV     Flux 0.11.2 Conv((kw, kh), cin => cout, act; stride, pad, dilation) with NNlib's default TRUE
 *                     convolution (flipped kernel); in = wi*hi*cin, out = wo*ho*cout,
 *                     wo = (wi + 2*pw - dw*(kw-1) - 1) / sw + 1
 *   SI_LAYER_MAXPOOL  MaxPool((kw, kh); stride = (sw, sh), pad = 0); cin == cout channels
 *   SI_LAYER_FLATTEN  (W, H, C, N) -> (W*H*C, N); in == out                                                          */
typedef struct {
  int32_t kind;  /* SI_LAYER_*      */
  int32_t in;    /* input features  */
  int32_t out;   /* output features */
  int32_t act;   /* SI_ACT_*        */
  int64_t w_off; /* offset of vec(W) / vec(weight) in the flat vector (elements) */
  int64_t b_off; /* offset of the bias                                           */
  int32_t kw, kh;         /* Conv kernel / MaxPool window                         */
  int32_t cin, cout;      /* channels                                             */
  int32_t wi, hi;         /* input width, height                                  */
  int32_t sw, sh;         /* stride                                               */
  int32_t pw, ph;         /* Conv zero padding (each side)                        */
  int32_t dw, dh;         /* Conv dilation                                        */
} si_layer;

/* kernel classes timed by the library's own hipEvents (si_set_profiling) */
enum {
  SI_K_PUSH = 0,     /* K1 swa_dev_push                       */
  SI_K_GRAM = 1,     /* K2 gram A'A partials (MFMA f64)       */
  SI_K_GRAM_RED = 2, /* K2 partial-slab reduction             */
  SI_K_PROJECT = 3,  /* K3 P = A*V_M                          */
  SI_K_RECON = 4,    /* K4 w = W_swa + P*z                    */
  SI_K_DENSE = 5,    /* K5 dense layer GEMM (MFMA f64), all layers */
  SI_K_SSE = 6,      /* K5 sum of squared errors              */
  SI_K_RWMH = 7,     /* K6 propose / accept kernels           */
  SI_K_DENSE_MAIN = 8, /* K5 the largest layer only (dominant kernel) */
  SI_K_EIG_HOST = 9,   /* H1 K x K symmetric eigensolve: HOST wall time, not a device kernel */
  SI_K_BACKWARD = 10,  /* reverse sweep of si_logdensity_grad: delta, dW (split-K MFMA), W'delta, P'g */
  SI_K_CONV = 11,      /* K5 Conv layer: implicit-GEMM convolution (MFMA f64), forward                */
  SI_K_CONV_AUX = 12,  /* K5 Conv stacks: weight re-pack, MaxPool, layout changes (HBM-bound)         */
  SI_K_COUNT = 13
};

typedef struct {
  double ms[SI_K_COUNT];        /* accumulated device time per class (hipEvent), milliseconds */
  int64_t launches[SI_K_COUNT]; /* launches per class                                          */
  double flops[SI_K_COUNT];     /* accumulated ALGORITHMIC flops per class                     */
  double bytes[SI_K_COUNT];     /* accumulated ALGORITHMIC HBM bytes per class                 */
} si_stats;

int32_t si_version(void); /* 500: + narrow-chain fused density / grid loop (specialised at run time), si_train_setup_ex, SI_F32 on Conv chains; 400: + compute_dtype = SI_F32 (300: RCCL communicator, streamed output map, pipelined host push) */

/* ---- context ------------------------------------------------------------------------------- */
int32_t si_create(si_ctx** out, int32_t device_id);
int32_t si_destroy(si_ctx* ctx);
const char* si_last_error(si_ctx* ctx); /* ctx may be NULL: message of the last failed si_create */
/* run on a caller-provided hipStream_t (e.g. torch's current stream); NULL = the ctx's own stream */
int32_t si_set_stream(si_ctx* ctx, void* hip_stream);
int32_t si_synchronize(si_ctx* ctx);
int32_t si_set_profiling(si_ctx* ctx, int32_t on); /* hipEvent pair around every kernel launch */
/* restrict the event pairs to the classes whose bit (1u << SI_K_*) is set (default: all); launches / flops / bytes are
 * counted for every class regardless.  An event pair costs ~5 us of stream time: a timed region that wants the duration
 * of one kernel class only should say so. */
int32_t si_set_profiling_classes(si_ctx* ctx, uint32_t class_mask);
int32_t si_get_stats(si_ctx* ctx, si_stats* out);  /* synchronizes; resolves pending events   */
int32_t si_reset_stats(si_ctx* ctx);
int32_t si_device_name(si_ctx* ctx, char* buf, int32_t buflen);

/* ---- subspace construction: replaces src/subspace_construction.jl:31-33,45-52,61-65 ---------- */
/* :31-33  W_swa = zeros(N) (Float64), A = empty.  K_capacity = number of pushes that will follow.
 * max_cols = 0 keeps every deviation column (the reference's behaviour: the shift at :48-50 is
 * commented out); max_cols = M keeps only the newest M columns (the paper's column shift).        */
int32_t si_construct_begin(si_ctx* ctx, int64_t N, int64_t K_capacity, int32_t max_cols);
/* NON-DEFAULT option: start the running mean at the given weights instead of zeros -- what the
 * reference's docs describe ("Initialize ... W_swa = W_0", docs/src/nn_example.md:44) but its code does not do (:31).
 * Call right after si_construct_begin.                                                                             */
int32_t si_construct_set_mean(si_ctx* ctx, const void* w_host, int32_t w_dtype);
/* NON-DEFAULT option: store the deviation matrix in fp32.  The reference keeps A in Float64
 * (src/subspace_construction.jl:33,51-52); with a_dtype = SI_F32 every column w - W_swa is still FORMED in fp64 and rounded
 * once on the way to memory, while W_swa, the Gram matrix, its eigen-decomposition and P stay fp64.  Halves the memory of A
 * (BASELINE cfg5: 52 -> 26 GB) and the bytes the Gram / projection kernels stream.  Measured against the fp64 oracle
 * (tests/test_gpu_a32.py): W_swa bit-exact, singular values rtol 1e-6, P up to sign 1e-5 of its scale (north_star: 1e-4).
 * Call right after si_construct_begin, before the first push; si_construct_get_A returns the stored (rounded) columns.   */
int32_t si_construct_set_storage(si_ctx* ctx, int32_t a_dtype);
/* :45-52  W = extract_params(ps); n = i/c; W_swa = (n.*W_swa + W)./(n+1); W_dev = W - W_swa;
 * append!(A, W_dev).  `n` is supplied by the caller (it is the EPOCH counter i/c, repeated for every
 * batch of the epoch).  w has N elements of w_dtype.
 * si_construct_push (host snapshot, pageable is fine) is PIPELINED: the call copies w into one of two pinned staging
 * buffers (host threads, SI_HOST_COPY_THREADS), queues H2D + K1 on the ctx's stream and returns -- w_host may be reused
 * at once, the transfer and the kernel overlap the caller's next gradient / update!.  Errors of the queued work surface
 * at the next synchronising call (si_construct_finish, si_synchronize).                                              */
int32_t si_construct_push(si_ctx* ctx, const void* w_host, int32_t w_dtype, double n);
int32_t si_construct_push_dev(si_ctx* ctx, const void* w_dev, int32_t w_dtype, double n);
/* `count` pushes in one pass over snapshots already on the device: snapshot j starts at w_dev + j*ld elements and is
 * pushed with n_host[j].  Bit-identical to `count` calls of si_construct_push_dev, with W_swa held in registers
 * (count*(s_w+8)+16 bytes per element instead of count*(s_w+24)) and one launch instead of `count`.               */
int32_t si_construct_push_batch_dev(si_ctx* ctx, const void* w_dev, int32_t w_dtype, int64_t ld, int32_t count,
                                    const double* n_host);
/* Gram matrix G = A'A (K x K, fp64) of the columns pushed so far, computed on the device.
 * get/set exist so that a row-sharded construction (each rank holds a row block of w, W_swa, A, P) can
 * all-reduce G across ranks (RCCL via the host wrapper) before si_construct_finish.                  */
int32_t si_construct_gram(si_ctx* ctx);
int32_t si_construct_gram_get(si_ctx* ctx, double* G_host /* K*K */, int64_t* K_out);
int32_t si_construct_gram_set(si_ctx* ctx, const double* G_host /* K*K */);
/* The same hook without the host: device address of G (K x K fp64, contiguous, valid until the next si_construct_gram /
 * si_construct_begin).  A row-sharded construction all-reduces it IN PLACE over RCCL (stream-ordered after
 * si_construct_gram when the caller runs the collective on the stream given to si_set_stream) and then calls
 * si_construct_finish: no D2H / H2D of G, no extra synchronisation.                                                   */
int32_t si_construct_gram_ptr(si_ctx* ctx, double** G_dev_out, int64_t* K_out);
/* Ill-conditioned deviation matrices (s_M below ~3e-5 s_1, where A'A no longer resolves the trailing singular values;
 * psvd at src/subspace_construction.jl:63 resolves them down to 5 eps): si_construct_finish switches by itself to a
 * two-stage route -- B = A*V_full on the device, second Gram matrix G2 = B'B, scaled-criterion Jacobi on the host,
 * P = B*W_M.  A ROW-SHARDED construction has to all-reduce G2 as well, so the stage is exposed:
 *     si_construct_gram; all-reduce G;  si_construct_needs_refine(M, &flag)   -- same G => same flag on every rank
 *     if flag:  si_construct_refine  (leaves G2 where G was: si_construct_gram_ptr / _get / _set now address G2);
 *               all-reduce G2;
 *     si_construct_finish(M, ...).
 * After a refine, si_construct_gram_get returns G2 until the next si_construct_gram.                              */
int32_t si_construct_needs_refine(si_ctx* ctx, int32_t M, int32_t* flag_out);
int32_t si_construct_refine(si_ctx* ctx);
/* :61-65  A = reshape(A, N, :); U,s,V = psvd(A); P = U[:,1:M]*Diagonal(s[1:M])  ==  A*V[:,1:M].
 * Outputs may be NULL (results stay on the device for si_infer_setup).  s_out receives the M largest
 * singular values.  Column signs of P are fixed so that the entry of largest magnitude in each column
 * of V is positive (deterministic; the reference's signs are arbitrary).  Returns SI_ERR_BOUNDS when M
 * exceeds the numerical rank of A (s_M <= ~5 eps s_1, psvd's rtol) -- the reference's BoundsError at U[:,1:M]. */
int32_t si_construct_finish(si_ctx* ctx, int32_t M, double* W_swa_out /* N */,
                            double* P_out /* N x M col-major */, double* s_out /* M */,
                            int64_t* K_out);
/* Device addresses of the finished construction's results: W_swa (ld elements, rows [N, ld) zero) and P (ld x M
 * column-major, ld = N rounded up to 64).  Valid until the next si_construct_begin / si_construct_finish / si_destroy.
 * For device-to-device hand-over: an RCCL broadcast of (W_swa, P) to the other ranks' si_infer_setup_dev (independent
 * chains, cfg3), or checks that must not stage 26 GB of P through the host (cfg5).                                  */
int32_t si_construct_result_ptr(si_ctx* ctx, double** W_swa_dev_out, double** P_dev_out, int64_t* ld_out, int32_t* M_out);
/* Copy the results of the FINISHED construction the ctx holds to the host: its own (same values si_construct_finish
 * returned), or one received from another rank (si_bcast_subspace / si_construct_allgather).  Any output may be NULL;
 * N_out / M_out report the sizes (call once with NULL arrays to size them).                                         */
int32_t si_construct_get_result(si_ctx* ctx, double* W_swa_out /* N */, double* P_out /* N x M */, double* s_out /* M */,
                                int64_t* N_out, int32_t* M_out);
/* read back deviation columns [k0, k0+nk) (N x nk col-major) -- parity tests of :51-52 */
int32_t si_construct_get_A(si_ctx* ctx, int64_t k0, int64_t nk, double* A_out);

/* ---- method = :diffusion: replaces src/subspace_construction.jl:202-206 (diffusion_subspace) ------------------------
 * diff_M = fit(DiffMap, A', maxoutdim = M); P = transform(diff_M); return W_swa, P'   (ManifoldLearning 0.6.2).
 * The definition below is  [upstream, from memory, unverifiable offline]  (diffmap.py restates it in NumPy); every point where
 * memory may be wrong is an argument.  With X = A' (K x N):
 *   rescale != 0: per snapshot k, Xr[k, i] = (X[k, i] - min_k) * (1 / (max_k - min_k)), NaN -> 0 (StatsBase UnitRangeTransform)
 *   Kmat_ij = exp(kernel_sign * ||Xr_i - Xr_j||^2 / eps)   kernel_sign -1: upstream's docstring; +1: what 0.6.2's source is
 *                                                          remembered to compute.  eps = 1 is upstream's default
 *   p = rowsums(Kmat); Kmat_ij /= (p_i p_j)^alpha (alpha = 1: upstream's t = 1); q = sqrt(rowsums); Kn_ij = Kmat_ij / (q_i q_j)
 *   U = eigenvectors of Kn by |lambda| descending (lambda_1 = 1, u_1 = q / ||q||);  P = U[:, 2:M+1] ./ U[:, 1]
 * Column signs of P: the entry of largest magnitude of each column is positive (lowest index on a tie).
 * Only the M + 1 leading vectors are computed: u_1 analytically, the rest by block subspace iteration on the device-resident
 * N x N matrix (block min(N - 1, 2M + 16)), stopped when every leading residual ||Kn u - theta u|| <= tol (tol <= 0: 1e-12) or
 * after max_iters (<= 0: 500) iterations.  Not converged is SI_ERR_INVALID with the residual and the count in the message: the
 * spectrum is not separated well enough -- a stated limitation against the reference's full SVD.
 * State rules: si_construct_finish's (pushes must have happened; outputs may be NULL).  Afterwards the ctx holds a finished
 * construction: si_infer_setup(NULL, NULL), si_construct_result_ptr, si_construct_get_result (s = |lambda_2 .. lambda_{M+1}|)
 * and si_bcast_subspace behave as after a PCA finish.  The deviation matrix and the PCA route's state are untouched: a
 * si_construct_finish before and after gives the same bits.
 * lambda_out: the M + 1 eigenvalues, |.| descending, lambda_out[0] = 1.
 * SI_ERR_INVALID: M < 1; eps or alpha not finite; eps <= 0; kernel_sign not +1 / -1; N > 65536 (the N x N fp64 matrix is 34 GB
 * there); a non-finite kernel entry (overflow with kernel_sign = +1).  SI_ERR_BOUNDS: M + 1 > N - 1.  SI_ERR_NOMEM as elsewhere.
 * A ROW-SHARDED construction is not supported: the kernel matrix couples every pair of weights.                       */
int32_t si_construct_finish_diffmap(si_ctx* ctx, int32_t M, double eps, double alpha, int32_t kernel_sign, int32_t rescale,
                                    double tol, int32_t max_iters, double* W_swa_out /* N */, double* P_out /* N x M */,
                                    double* lambda_out /* M + 1 */, int64_t* K_out);
/* iterations and largest leading residual of the last si_construct_finish_diffmap (a refused call: zeros) */
int32_t si_diffmap_info(si_ctx* ctx, int32_t* iters_out, double* residual_out);
/* audit read-back of the last call that got as far as the iteration (converged or not): Kn (N x N col-major) and u_1 (N);
 * either may be NULL */
int32_t si_diffmap_get_kernel(si_ctx* ctx, double* Kn_out, double* u1_out);

/* ---- density + sampling: replaces src/space_inference.jl:88-95,111-116,125 ------------------- */
/* :88 split_data (full X, Y), :90-95 density closure.  W_swa / P may both be NULL: the result of the
 * ctx's finished construction is used in place (no host round trip).  X is in_dim x B, Y is out_dim x B,
 * column-major fp64.
 * compute_dtype: SI_F64 = the reference's arithmetic (src/subspace_construction.jl:31,33 and README.md:56-57 make W_swa, P,
 *   the data and therefore the whole density Float64 -- SURVEY section 0, Q6).
 * SI_F32 = the measured fp32 option of SURVEY section 0 Q6 / 8(b),(d): X is rounded to
 *   fp32 once, W_swa + P*z is formed in fp64 and rounded to fp32 once per evaluation, every Dense layer multiplies and
 *   accumulates in fp32 (v_mfma_f32_32x32x2_f32) with fp32 activations; a narrow last layer (out <= 4), its bias /
 *   activation and the sum of squared errors are fp64.  It applies to si_logdensity, si_forward, the RWMH samplers
 *   (si_sample_rwmh*, si_rwmh_*) and -- since round 5 -- si_logdensity_grad (the fp32 forward with kept activations and the
 *   fp32 reverse sweep of the training step; the pull-back P' g and the optional prior term in fp64: grad rtol 2e-5 of its
 *   scale against the fp64 oracle, tests/test_gpu_f32.py; Dense chains only: on a Conv chain set up with SI_F32 the gradient is
 *   refused with SI_ERR_INVALID); si_predict keeps computing in fp64, and the output map
 *   (si_sample_rwmh_weights, si_reconstruct) delivers the fp64 W_swa + P*z.  Stated tolerance (tests/test_gpu_f32.py,
 *   against the fp64 oracle): model outputs 2e-5 of their scale, lp rtol 1e-5 (north_star: 1e-4); at BASELINE cfg2 the
 *   measured lp difference is rtol 2e-8 or better and none of 1000 accept decisions changes.
 *   Conv / MaxPool / flatten chains (round 5): the same option -- the convolution kernels on fp32 operands
 *   (v_mfma_f32_16x16x4_f32), fp32 activations and pooling, the Dense layers behind `flatten` on the fp32 GEMM kernels, the
 *   squared errors in fp64; outputs within 5e-5 of their scale and lp rtol 1e-5 on the CNN cases of the tests (BASELINE cfg4's
 *   CNN, 4096 images: lp rtol 9e-8, no accept decision of 200 differs, 7.3 -> 4.3 ms per transition).                            */
int32_t si_infer_setup(si_ctx* ctx, const si_layer* layers, int32_t L, int64_t N, int32_t M,
                       const double* W_swa, const double* P, const double* X, const double* Y,
                       int32_t in_dim, int32_t out_dim, int64_t B, double sigma_m,
                       int32_t compute_dtype);
/* si_infer_setup with every array already on the DEVICE (fp64, column-major; P_dev has leading dimension ldP >= N).
 * X_dev / Y_dev are copied device-to-device.  W_swa_dev / P_dev: both NULL = the ctx's finished construction;
 * borrow = 0 copies them; borrow = 1 uses them IN PLACE -- the caller keeps them alive and unchanged until the next
 * set-up or si_destroy, bases 16-byte aligned, ldP even and >= N + (N mod 2), W_swa_dev readable for N + (N mod 2)
 * elements (the streaming kernels read rows in 16-byte pairs).  No host staging: at cfg5 P is 26 GB per rank.      */
int32_t si_infer_setup_dev(si_ctx* ctx, const si_layer* layers, int32_t L, int64_t N, int32_t M,
                           const double* W_swa_dev, const double* P_dev, int64_t ldP, int32_t borrow,
                           const double* X_dev, const double* Y_dev, int32_t in_dim, int32_t out_dim, int64_t B,
                           double sigma_m, int32_t compute_dtype);
/* NON-DEFAULT option: add the prior term the reference writes AFTER its `return` (dead code,
 * src/space_inference.jl:95):  + logpdf(MvNormal(zeros(N), sigma_p), new_W).  sigma_p = 0 switches it off again (the
 * reference's behaviour and the default after every si_infer_setup).  Applies to si_logdensity, its gradient and the
 * RWMH samplers.                                                                                                   */
int32_t si_infer_set_prior(si_ctx* ctx, double sigma_p);
/* NON-DEFAULT option: the likelihood of a classifier in place of the Gaussian on its outputs.  With yhat = f_W(X) (out x B, the
 * model's outputs read as logits whatever the last activation is) and Y (out x B):
 *   SI_LIK_GAUSSIAN     lp = logpdf(MvNormal(vec(yhat), sigma_m), vec(Y))                      (the reference; every set-up starts here)
 *   SI_LIK_CATEGORICAL  lp = sum_b sum_i Y_ib (yhat_ib - lse_b), lse_b the log-sum-exp of column b about its maximum
 *   SI_LIK_BERNOULLI    lp = -sum((1 - Y) yhat + softplus(-yhat)), softplus(-x) = max(-x, 0) + log1p(exp(-|x|))
 * i.e. minus the numerators of SI_COST_LOGITCE / SI_COST_LOGITBCE (costs.py of the Python package is the definition); soft
 * labels are kept as written.  sigma_m is accepted and unused, as for a NeuralODE; the prior term of si_infer_set_prior is added
 * as for the Gaussian.  [upstream, from memory, unverifiable offline]: the reference has no such likelihood -- it is the density
 * that its users' classification cost implies.  Called after a set-up, like si_infer_set_prior.  Applies to si_logdensity, its
 * gradients, every sampler and si_fit_advi; si_forward / si_predict keep returning the model's outputs.  While kind != 0 the routes
 * that form the squared error inside a kernel of their own (the device-resident RWMH loops, the one-launch narrow-chain density,
 * the fused stacked gradient) are not taken: the per-layer launches and the per-point gradient run, and si_chain_kernel_info /
 * si_grad_kernel_info say so.  SI_ERR_STATE before a set-up and while a step-wise RWMH session is open; SI_ERR_INVALID for an
 * unknown kind and for a NeuralODE set-up; a refusal changes nothing.  si_rwmh_begin with d_total > 0 (the data-sharded
 * session) returns SI_ERR_INVALID while kind != 0.                                                                  */
#define SI_LIK_GAUSSIAN 0
#define SI_LIK_CATEGORICAL 1
#define SI_LIK_BERNOULLI 2
int32_t si_infer_set_likelihood(si_ctx* ctx, int32_t kind);
int32_t si_infer_likelihood_info(si_ctx* ctx, int32_t* kind_out);
/* The autoencoder route (src/space_inference.jl:238-318, auto_inference): the density at W_swa + decoder(z) instead of
 * W_swa + P z.  The decoder is a Dense-only chain M -> h_1 -> ... -> h_{D-1} -> N given as a layer table whose w_off / b_off
 * index the flat parameter vector wdec_host (Nd elements of wdec_dtype, Flux.destructure order: [vec(W_l); b_l] per layer).  Call
 * after si_infer_setup / si_infer_setup_dev, like si_infer_set_prior; the next set-up drops it.  From then on every entry point
 * that uses the density -- si_logdensity, si_forward, si_predict, si_reconstruct (the output map W_swa + decoder(z)),
 * si_sample_rwmh, si_sample_rwmh_weights, the si_rwmh_* session, si_logdensity_grad, si_logdensity_grad_batch, si_sample_mala /
 * _hmc / _nuts, si_fit_advi -- uses it, and the stored P is ignored.  dec_layers = NULL with D = 0 clears the decoder: the P route
 * returns bit for bit.  Definition: subspaceinference.jl_amd/autoencoder.py (a_0 = z; u = W a + b with the sum over the input
 * index ascending from 0.0 and the bias added last; a = act(u); every sum fp64).  The parameters stay on the device in the
 * element type they came in (widening on load is exact; a Float32 decoder halves the bytes of the last layer's stream).
 * Routes that form W_swa + P z or P' g inside a kernel of their own are NOT taken while a decoder is set: the device-resident
 * and persistent RWMH loops, the run-time specialised loop and the fused gradient of si_logdensity_grad_batch; the
 * launch-per-step loop and the per-point gradient path run instead, and si_chain_kernel_info's loop flag, si_grad_kernel_info
 * and the fused flag of si_mala / hmc / nuts / advi_kernel_info report 0.
 * SI_ERR_INVALID: a layer that is not SI_LAYER_DENSE; D outside 1 .. 8; the first `in` != M or the last `out` != N of the
 * set-up; widths that do not chain; a hidden width or M above 1024; an offset range outside [0, Nd); an activation id out of
 * range; a set-up with compute_dtype = SI_F32 (the fp32 weight vector is not fed on this route).  SI_ERR_STATE: before a
 * set-up, or while a step-wise RWMH session is open.
 * si_construct_*, si_bcast_subspace and the communicator entry points neither know nor carry a decoder: every rank sets its own. */
int32_t si_infer_set_decoder(si_ctx* ctx, const si_layer* dec_layers, int32_t D, int64_t Nd, const void* wdec_host,
                             int32_t wdec_dtype /* SI_F32 | SI_F64 */);
/* D (0: no decoder set), the last layer's input width and the parameters' element type (outputs may be NULL) */
int32_t si_infer_decoder_info(si_ctx* ctx, int32_t* D_out, int32_t* H_out, int32_t* storage_dtype_out);
/* Y_out[:, c] = decoder(Z[:, c]) alone (N x C, column-major), without W_swa; needs a decoder */
int32_t si_decode(si_ctx* ctx, const double* Z /* M x C */, int64_t C, double* Y_out /* N x C */);
/* gz_out = J_decoder(z)' gy at one point: the decoder's reverse kernels alone, launch for launch those si_logdensity_grad runs
 * around the model's sweep (the audit read-back of tests/test_gpu_decoder_reverse.py).  SI_ERR_STATE: before a set-up, with no
 * decoder set, or while a step-wise RWMH session is open (the buffers are shared). */
int32_t si_decode_vjp(si_ctx* ctx, const double* z /* M */, const double* gy /* N */, double* gz_out /* M */);

/* ---- NeuralODE models (reference src/space_inference.jl:96-101, model_re at src/libs.jl:36-54; docs/src/node_example.md) ----------
 * The model is du/dt = dudt(u; w): a Dense chain d -> ... -> d (optionally behind the elementwise cube u -> (u*u)*u, the tutorial's
 * `x -> x.^3`), integrated with Tsit5 from t0 for every column of U0 and saved at ts (`saveat` without `tstops`).  The density is
 *   lp(z) = - sum_p || sol_p(W) - Y[:, p] ||^2 - ||W||^2,   W = W_swa + P z   (or W_swa + decoder(z)),
 * sigma_m and sigma_p unused as in the reference.  The definition is subspaceinference.jl_amd/node.py; all arithmetic is fp64.
 * A trajectory that reaches max_steps (status 1) or a non-finite state / error / vanishing step (status 2) contributes +Inf:
 * lp = -Inf, and an RWMH proposal there is rejected. */
typedef struct {
  double t0, reltol, abstol;
  double dt;          /* adaptive: > 0 gives the first step (0: the Hairer-Wanner starting-step rule); fixed-step: the step  */
  int32_t adaptive;   /* 1: PI-controlled steps; 0: every step is dt (the last one shortened to end at ts[S-1])              */
  int32_t max_steps;  /* accepted + rejected steps per trajectory, 1 .. 1 000 000 (0: 100 000)                               */
  int32_t pre_power;  /* 1, or 3 for the cube in front of the first Dense layer                                              */
} si_node_opts;
/* An inference set-up for a NeuralODE, in place of si_infer_setup: in_dim = d, out_dim = d*S, B = f.  W_swa / P NULL: the
 * context's finished construction.  Y row i*S + s of column p is state i of trajectory p at ts[s] (Julia's
 * reshape(out_data[:, p], :, d)').  Supported (anything else: SI_ERR_INVALID naming the limit): Dense layers only, 1 <= L <= 8,
 * 1 <= d <= 8, widths <= 256, N <= 8192, 1 <= S <= 4096, ts strictly ascending with ts[0] >= t0, pre_power 1 or 3, tolerances
 * finite and > 0 (adaptive) or dt > 0 (fixed-step), f <= 2^20 (the per-chain sum of the f squared errors is sequential, in the
 * reference's order: the tutorial's f is 100).  `opts` points to an si_node_opts (an untyped pointer in the prototype, so
 * that bindings pass a reference to their own mirror of the struct).
 * While it is active si_logdensity, si_forward (the saved states, d*S x f), si_predict (new initial states d x Bn), si_reconstruct,
 * si_sample_rwmh, si_sample_rwmh_weights, the si_rwmh_* session and si_infer_set_decoder work as for a Chain;
 * si_infer_set_prior and the sharded sampler return SI_ERR_INVALID ("not available for NeuralODE models"), and so do
 * si_logdensity_grad*, si_sample_mala / _hmc / _nuts and si_fit_advi until si_node_set_grad(ctx, 1).  The next si_infer_setup*
 * leaves the mode and drops that switch. */
int32_t si_infer_setup_node(si_ctx* ctx, const si_layer* layers, int32_t L, int64_t N, int32_t M, const double* W_swa,
                            const double* P, const double* U0 /* d x f */, const double* Y /* d*S x f */, int32_t d, int32_t S,
                            int64_t f, const double* ts /* S */, const void* opts /* const si_node_opts* */);
/* The trajectories at Z[:, c] (M x C): the saved states (d*S x f x C, Y's layout; NaN where a failed trajectory saved nothing),
 * the per-trajectory squared errors (+Inf for a failed one), accepted / rejected step counts and status, f x C each.  Every
 * output may be NULL.  The audit read-back and the user's trajectory tool. */
int32_t si_node_solve(si_ctx* ctx, const double* Z, int32_t C, double* U_out, double* sse_out, int32_t* naccept_out,
                      int32_t* nreject_out, int32_t* status_out);
/* c (7), a row by row (21), b~ (7) and the interpolant's constants (4 + 6 * 3) as the kernel holds them: 57 doubles */
int32_t si_node_tableau(double* out);
/* whether a NeuralODE set-up is active, d, S, f and the lanes G that share one trajectory (outputs may be NULL) */
int32_t si_node_info(si_ctx* ctx, int32_t* active_out, int32_t* d_out, int32_t* S_out, int64_t* f_out, int32_t* G_out);
/* The gradient through the solver, off after every si_infer_setup_node.  on = 1 lets si_logdensity_grad, si_logdensity_grad_batch,
 * si_sample_mala / _hmc / _nuts and si_fit_advi through on this set-up; what they differentiate is the DISCRETE ADJOINT of the
 * integration si_node_solve performs with its accepted step sequence frozen (node.py: logdensity_grad): hs_n and every
 * interpolation theta are constants, rejected steps, the starting step and the controller do not enter.  (Not what ForwardDiff
 * gives through OrdinaryDiffEq, where the partials enter the error norm: the two agree to the order of the tolerances.)  A failed
 * trajectory gives lp = -Inf and NaN in every component.  SI_ERR_INVALID naming the reason when a layer is wider than 64, or when
 * the step record of one chain (f * max_steps * (d + 2) doubles) with its gradient slices (f * N) exceeds the 2 GiB workspace
 * budget -- lower max_steps.  on = 0 turns it off and frees the workspace. */
int32_t si_node_set_grad(si_ctx* ctx, int32_t on);
/* whether the switch is on, and the chains one pass of launches carries under the budget (outputs may be NULL) */
int32_t si_node_grad_info(si_ctx* ctx, int32_t* on_out, int32_t* chains_per_pass_out);
/* The audit read-back of that gradient at Z[:, c]: lp (C), d lp / dW with the prior term (N x C) and its pull-back to z (M x C).
 * Every output may be NULL. */
int32_t si_node_grad(si_ctx* ctx, const double* Z /* M x C */, int32_t C, double* lp_out, double* gw_out, double* gz_out);
/* :90-95  lp[c] = logpdf(MvNormal(vec(f_{W_swa+P z_c}(X)), sigma_m), vec(Y)),  Z is M x C          */
int32_t si_logdensity(si_ctx* ctx, const double* Z, int32_t C, double* lp_out /* C */);
/* lp and its gradient with respect to z: grad_out[m] = d lp / d z_m = (P' * d lp / d w)[m].
 * Replaces `l_pi_grad(theta) = (density(theta), getbackend(backend).gradient(density, theta))`
 * (src/space_inference.jl:107): one reverse sweep through the chain instead of M-wide forward duals.         */
int32_t si_logdensity_grad(si_ctx* ctx, const double* z /* M */, double* lp_out, double* grad_out /* M */);
/* The same for C points at once: lp_out[c], grad_out[:, c] = what si_logdensity_grad returns for Z[:, c] (prior term as
 * si_infer_set_prior set it); same state rules.  fp64 Dense chains with the identity / relu / tanh / sigmoid activations whose
 * per-layer images fit a workgroup's LDS (docs/src/nn_example.md:112-118 and its class) run ONE fused forward + reverse launch
 * and ONE reduction launch per group of points, with every sum in a fixed order: a point's result does not depend on C, on its
 * column or on the run.  Every other chain walks the columns through si_logdensity_grad's own path (same bits).            */
int32_t si_logdensity_grad_batch(si_ctx* ctx, const double* Z /* M x C */, int32_t C, double* lp_out /* C */,
                                 double* grad_out /* M x C, column-major */);
/* 1 when the last si_logdensity_grad_batch ran the fused narrow-chain kernel, 0 when it walked the per-point path */
int32_t si_grad_kernel_info(si_ctx* ctx, int32_t* fused_out);
/* :117-120  MALA(x -> MvNormal((sigma_z^2 / 2) .* x, sigma_z)) with the chain state on the device.  Shapes, column-major layout,
 * `itr` (samples INCLUDING the initial state), accept_rate = accepts / (itr - 1) and the chain ids are si_sample_rwmh's; the state
 * rules and the prior term are si_logdensity_grad_batch's.  G_out (may be NULL) receives d lp / d z at every returned state.
 * Chain c draws from Philox chain chain_id0 + c: purpose 0 at step t gives the M normals n_t, purpose 1 at step t gives e_t.  With
 * h = sigma_z^2 / 2:
 *     t = 0:   z = sigma_z n_0;  (lp, g) = value and gradient at z
 *     t >= 1:  zp = z + h g + sigma_z n_t;  (lpp, gp) at zp
 *              fwd = zp - z - h g;  bwd = z - zp - h gp;  logq = -(bwd.bwd - fwd.fwd) / (2 sigma_z^2)
 *              accept iff -e_t < lpp - lp + logq (a NaN rejects);  accept: (z, lp, g) = (zp, lpp, gp);  sample t = (z, lp, g)
 * Chains of si_logdensity_grad_batch's fused class: every transition is four launches per pass queued on the stream (the K4
 * launch, the fused forward + reverse kernel, its reduction, the accept kernel, which also forms the next proposal); the state stays
 * on the device and the host synchronises ONCE, at the end.  More chains than the gradient workspace carries are walked in passes
 * inside each transition.  Every sum has a fixed order: a chain's bits do not depend on nchains, on its column or on the run.
 * EVERY OTHER CHAIN (Conv / MaxPool / flatten, SI_F32, the four later activations, wide layers) runs the same two MALA kernels, but
 * the value and gradient of every proposal come column by column from si_logdensity_grad's path through the host: that route is
 * slow and synchronises once per chain and transition.  It has the same definition.                                             */
int32_t si_sample_mala(si_ctx* ctx, int64_t itr, double sigma_z, uint64_t seed, int32_t chain_id0, int32_t nchains,
                       double* Z_out /* M x itr x C */, double* lp_out /* itr x C */, double* accept_rate_out /* C */,
                       double* G_out /* M x itr x C or NULL */);
/* the last si_sample_mala call: fused_out = 1 when it took the device-resident route, passes_out = gradient passes per transition
 * (fused: ceil(nchains / points per pass); other route: one per chain)                                                          */
int32_t si_mala_kernel_info(si_ctx* ctx, int32_t* fused_out, int32_t* passes_out);
/* :139-160  HMC: StaticTrajectory(Leapfrog(eps), 1) under StanHMCAdaptor(MassMatrixAdaptor(DiagEuclideanMetric), StepSizeAdaptor(delta))
 * after find_good_stepsize (AdvancedHMC 0.2.27) [upstream, unverifiable offline], with position, momentum, step size, metric and
 * adaptor state on the device.  State rules and prior term: si_logdensity_grad_batch's.  Chain c draws from Philox chain
 * chain_id0 + c: purpose 0 at step 0 = the initial point's normals (si_sample_mala's z_0); purpose 1 at step t, block 0 = the
 * uniform u_t = u53(x1, x0); purpose 5 at step t = the momentum normals n_t; purpose 6 at step 0 = the search's momentum rho.
 *     z_0 = sigma_z n_0;  (lp_0, g_0) at z_0;  Minv = 1
 *     search   h0 = lp_0 - rho.rho / 2;  dH(e) = lpp - rp.rp / 2 - h0 after one leapfrog step of size e from (z_0, rho)
 *              eps = 0.1;  direction = dH(eps) > log 0.5 ? +1 : -1
 *              at most 100 times: eps' = 2 eps or eps / 2;  d = dH(eps) (at the OLD eps);  stop when d has left the starting side of
 *              log 0.5, else eps = eps'.  Then (lo, hi) = (eps, eps') sorted and at most 100 times: mid = (lo + hi) / 2,
 *              a = exp(dH(mid));  a > 0.75: lo = mid;  a < 0.25: hi = mid;  else lo = mid and stop.  eps_0 = lo.
 *     t = 1 .. itr, with the adaptor's current (eps, Minv):
 *              r = n_t / sqrt(Minv);  K0 = sum((Minv r) r) / 2;  rh = r + (eps / 2) g;  zp = z + eps (Minv rh);  (lpp, gp) at zp
 *              rp = rh + (eps / 2) gp;  K1 = sum((Minv rp) rp) / 2;  dH = (lpp - K1) - (lp - K0)
 *              a = 0 if lpp - K1 is not finite, 1 if dH >= 0, else exp(dH);  accept iff u_t < a:  (z, lp, g) = (zp, lpp, gp)
 *              column t of Z / lp / G = the state;  alpha[t] = a;  eps[t] and Minv[:, t] = those USED by transition t
 *              t <= n_adapts: dual averaging (gamma 0.05, t0 10, kappa 0.75, mu = log 10 eps) of log eps towards delta; inside a
 *              window (si_host_hmc_windows) the Welford update with the KEPT z; at a window's close
 *              Minv = n / (n + 5) var + 1e-3 5 / (n + 5), the window emptied, the dual averaging restarted at the current eps;
 *              after step n_adapts eps = exp(the averaged log eps)
 * Column 0 of the outputs is the initial state with alpha = 0, eps = eps_0 and Minv = 1.  Every sum over m has si_sample_mala's
 * order: a chain's bits depend on M alone, not on nchains, its column, the pass split or the run.
 * SI_ERR_INVALID unless itr > 0, 0 <= n_adapts <= itr, nchains > 0, chain_id0 >= 0, sigma_z > 0 and 0 < delta < 1 (a NaN is refused).
 * Routes as si_sample_mala's: chains of the fused class queue the gradient's launches and ONE accept launch (which also forms the
 * next proposal) per transition and synchronise once, at the end; every other chain takes the slow per-point route through the host.
 * THE SEARCH IS A SYNCHRONISING PREAMBLE on both routes: after each of its rounds (at most 203) the host reads back one 4-byte count
 * of the chains still searching.                                                                                                 */
int32_t si_sample_hmc(si_ctx* ctx, int64_t itr, int64_t n_adapts, double sigma_z, double delta, uint64_t seed, int32_t chain_id0,
                      int32_t nchains, double* Z_out /* M x (itr+1) x C */, double* lp_out /* (itr+1) x C */,
                      double* alpha_out /* (itr+1) x C */, double* eps_out /* (itr+1) x C */,
                      double* G_out /* like Z_out, or NULL */, double* Minv_out /* like Z_out, or NULL */);
/* the last si_sample_hmc call: fused_out = 1 when it took the device-resident route, passes_out = gradient passes per transition
 * (as si_mala_kernel_info), search_rounds_out = rounds of the step-size search, the one at z_0 included                           */
int32_t si_hmc_kernel_info(si_ctx* ctx, int32_t* fused_out, int32_t* passes_out, int32_t* search_rounds_out);
/* :139-160  NUTS: NUTS{MultinomialTS, GeneralisedNoUTurn}(Leapfrog(eps)) under the same StanHMCAdaptor after the same
 * find_good_stepsize (AdvancedHMC 0.2.27) [upstream, unverifiable offline], with the trajectory tree, step size, metric and adaptor
 * state on the device.  THE DEFINITION is samplers.nuts_iter (the leaf-by-leaf restatement of samplers.nuts) on the Philox streams:
 * purposes 0, 5, 6 and column 0, the search and the adaptor exactly as si_sample_hmc; purpose 7 at step t, block j = the doubling at
 * depth j: direction +1 iff u53(x1, x0) < 0.5, progressive pick with u53(x3, x2); purpose 8 at step t, block 16 leaf + level = the
 * pick of the merge at `level` (1 ..) after leaf `leaf` (the running leaf count of the transition, 1 ..), u53(x1, x0).
 *     t = 1 .. itr:  r0 = n_t / sqrt(Minv);  h0 = lp - sum((Minv r0) r0) / 2;  the tree = the state, logw = 0, rho = r0
 *              doubling j = 0 .. max_depth - 1 in direction v: 2^j leapfrog steps of size v eps from the tree's end on that side; a
 *              leaf has dh = (lp1 - K1, or -inf if that is not finite) - h0, weight exp(dh), alpha = min(1, exp(dh)), and is divergent
 *              iff -dh > max_dh; after leaf k of the doubling the top two sub-trees merge once per trailing zero bit of k:
 *              logw = logaddexp, proposal = the later one's iff log u < logw_later - logw, rho and alpha and n add, and the merged
 *              sub-tree stops iff rho . (Minv r) <= 0 at either of its ends.  A divergent leaf or a stopped sub-tree ends the
 *              transition (its leaves still count into alpha); else the candidate becomes the doubling's proposal iff
 *              log u < logw_doubling - logw_tree, the tree takes the doubling, and the transition ends on the whole tree's U-turn
 *              or after doubling max_depth - 1.  state = candidate;  alpha[t] = sum of the leaves' alpha / max(1, leaves counted)
 *              the adaptor's update with (z, alpha[t]), as si_sample_hmc
 * Outputs as si_sample_hmc (column 0 = the initial state), and per transition depth_out = doublings started, nleaf_out = leapfrog
 * steps, sel_out = the leaf (1-based within the transition) that became the state, 0 = the previous state was kept (column 0: 0).
 * leaf_out (the audit's trace): for chain c the call's leaves in build order, each as (z[M], r[M], lp, g[M]); logging stops
 * silently at leaf_cap, the counts go on; slots no leaf reaches are NaN (all bits set).  A chain's bits depend on M alone, as si_sample_hmc's.
 * SI_ERR_INVALID for what si_sample_hmc refuses, and unless 1 <= max_depth <= 10, max_dh > 0 (a NaN is refused) and leaf_cap >= 1
 * when leaf_out is given.  EVERY ROUND SYNCHRONISES on both routes: one evaluation at the chains' pending points, one kernel, one
 * 4-byte read-back of the chains still building.  Chains advance in lock-step within a transition (a finished chain waits); a
 * transition takes at most 2^max_depth - 1 rounds (SI_ERR_STATE beyond).                                                           */
int32_t si_sample_nuts(si_ctx* ctx, int64_t itr, int64_t n_adapts, double sigma_z, double delta, int32_t max_depth, double max_dh,
                       uint64_t seed, int32_t chain_id0, int32_t nchains, double* Z_out /* M x (itr+1) x C */,
                       double* lp_out /* (itr+1) x C */, double* alpha_out /* (itr+1) x C */, double* eps_out /* (itr+1) x C */,
                       int32_t* depth_out /* (itr+1) x C or NULL */, int32_t* nleaf_out /* likewise */, int32_t* sel_out /* likewise */,
                       double* G_out /* like Z_out, or NULL */, double* Minv_out /* like Z_out, or NULL */,
                       double* leaf_out /* (3M+1) x leaf_cap x C or NULL */, int64_t leaf_cap);
/* the last si_sample_nuts call: route, passes and search rounds as si_hmc_kernel_info; rounds_out = rounds of all transitions,
 * leaves_out = sum of nleaf over chains and transitions (rounds x nchains - leaves = the lock-step waste)                        */
int32_t si_nuts_kernel_info(si_ctx* ctx, int32_t* fused_out, int32_t* passes_out, int32_t* search_rounds_out, int64_t* rounds_out,
                            int64_t* leaves_out);
/* NOT IN THE REFERENCE: elliptical slice sampling (Murray, Adams, MacKay 2010), the sampler Izmailov et al. ("Subspace Inference for
 * Bayesian Deep Learning") run in the subspace, with the chain state on the device.  THE DEFINITION is samplers.ess_iter on the
 * Philox streams.  The target is p(z) ~ exp(density(z)) N(z; 0, sigma_z^2 I), where density is what si_logdensity returns for the
 * current set-up (likelihood, si_infer_set_prior term, decoder and NeuralODE as set).  sigma_z IS HERE THE PRIOR'S STANDARD
 * DEVIATION ON z, NOT A STEP SIZE.  lp[t] = density(z_t): the prior on z is never evaluated and is not added.  The sampler has no
 * proposal scale, never rejects and needs values only, no gradients: it runs at full speed -- si_logdensity's stacked path,
 * fw.slots chains per pass of launches -- on every density the library evaluates, a NeuralODE without si_node_set_grad included.
 * Chain c draws from Philox chain chain_id0 + c: purpose 0 at step 0 = the initial point's normals n_0 (si_sample_mala's z_0);
 * purpose 1 at step t = e_t, si_sample_rwmh's Exp(1) draw; purpose 9 at step t = the M normals n_t; purpose 10 at step t, block j =
 * v_j = u53(x1, x0).
 *     t = 0:   z = sigma_z n_0;  lp = density(z);  nev = 1, theta = 0
 *     t >= 1:  nu = sigma_z n_t;  logy = lp - e_t
 *              theta = 2 pi v_0;  lo = theta - 2 pi;  hi = theta;  k = 0
 *              repeat:  zp = z cos theta + nu sin theta;  lpp = density(zp);  k += 1
 *                       lpp > logy (a NaN compares false)  -> (z, lp) = (zp, lpp);  nev[t] = k;  theta[t] = theta;  stop
 *                       k == max_evals                     -> state kept;  nev[t] = -max_evals;  theta[t] = 0;  stop
 *                       theta < 0 ? lo = theta : hi = theta;   theta = lo + (hi - lo) v_k
 *              column t = (z, lp)
 * `itr` counts the initial state, as in si_sample_rwmh and si_sample_mala; shapes, layout and chain ids are theirs.  Every angle is
 * plain IEEE arithmetic on exact uniforms, formed without contraction.  Only a discontinuous or all-NaN density reaches max_evals.
 * nev_out and theta_out (the audit's trace) may be NULL.  A chain's bits depend on M alone, not on nchains, its column or the run.
 * SI_ERR_INVALID unless itr > 0, nchains > 0, chain_id0 >= 0, sigma_z > 0 and 1 <= max_evals <= 2^24 (a NaN is refused);
 * SI_ERR_STATE while a step-wise session is open.  EVERY ROUND SYNCHRONISES: one evaluation at the chains' pending points, a memset,
 * one kernel, one 4-byte read-back of the chains still shrinking.  Chains advance in lock-step within a transition (a chain that
 * has kept a point waits; its slot is evaluated and ignored); a transition takes at most max_evals rounds.                        */
int32_t si_sample_ess(si_ctx* ctx, int64_t itr, double sigma_z, int32_t max_evals, uint64_t seed, int32_t chain_id0, int32_t nchains,
                      double* Z_out /* M x itr x C */, double* lp_out /* itr x C */, int32_t* nev_out /* itr x C or NULL */,
                      double* theta_out /* itr x C or NULL */);
/* the last si_sample_ess call: passes_out = ceil(nchains / chains per pass of launches) per evaluation; rounds_out and evals_out =
 * the rounds of all transitions and the sum of |nev| over chains and transitions, column 0 left out (rounds x nchains - evals =
 * the lock-step waste).  All zero after a refused call.                                                                         */
int32_t si_ess_kernel_info(si_ctx* ctx, int32_t* passes_out, int64_t* rounds_out, int64_t* evals_out);
/* :126-138  ADVI with its state on the device.  Restates
 *     AdvancedVI.vi(density, ADVI(S, T), theta -> TuringDiagMvNormal(theta[1:M], exp.(theta[M+1:2M])), rand(MvNormal(zeros(2M), sigma_z)))
 * followed by rand(q, D) (AdvancedVI 0.1.3), with that version's default optimiser TruncatedADAGrad(eta = 0.1, tau = 1.0,
 * n_iter = 100) [upstream, from memory, unverifiable offline] and its ELBO = mean of the density at S draws of q + the entropy of
 * q, differentiated through z = mu + exp(omega) .* eta [upstream, from memory, unverifiable offline].  THE DEFINITION:
 * run r draws from Philox chain chain_id0 + r.  Purposes 0 and 1 are RWMH's and MALA's; here purpose 2 is the initial point,
 * 3 the step draws, 4 the final draws; in all of them block j gives components 2j and 2j + 1.  nblk = ceil(M / 2).
 *     theta = [mu; omega] in R^2M
 *     init      theta_0 = sigma_z n,  n = the 2M normals of (purpose 2, step 0, blocks 0 .. M-1)
 *     step t = 0 .. T-1, with sigma = exp(omega) taken from theta_t:
 *        eta_k = the M normals of (purpose 3, step t, block k nblk + j),  k = 0 .. S-1
 *        z_k   = mu + sigma .* eta_k;  (lp_k, g_k) = value and gradient at z_k  (prior term as si_infer_set_prior set it)
 *        H     = M (log 2 pi + 1) / 2 + sum_m omega_m
 *        elbo_t = (((lp_0 / S + H) + lp_1 / S) + ...) + lp_{S-1} / S
 *        dmu_m    = -(sum_k g_k[m]) / S                           (k ascending, from 0.0)
 *        domega_m = -(sum_k (g_k[m] eta_k[m]) sigma_m) / S - 1    (k ascending, from 0.0)
 *        ring     slot t mod W of component p is set to d_p^2
 *        s_p      = sum over slots 0 .. W-1 in slot order (from 0.0); unwritten slots are 0
 *        theta_{t+1,p} = theta_{t,p} - d_p (eta / (tau + sqrt(s_p)))
 *     draws     z_i = mu_T + exp(omega_T) .* n_i,  n_i = the M normals of (purpose 4, step i),  i = 0 .. D-1
 * There is no guard against a non-finite lp: theta goes NaN as the reference's would, and elbo_out shows it.  Every sum has the
 * order written above; sum_m omega_m has si_sample_mala's order (thread i of 256 adds its components 2j, 2j + 1 for j = i,
 * i + 256, ..., then the wave sums, then (r0 + r1) + (r2 + r3)); log 2 pi is the literal 1.8378770664093453.  A run's bits therefore
 * depend on nothing but (seed, chain, M, S, T, W, eta, tau, sigma_z) and the density -- not on nruns, its column, the pass split
 * or the run.
 * State rules: si_logdensity_grad_batch's.  SI_ERR_INVALID: T < 1, S < 1, S nblk >= 2^24, W outside 1 .. 1024, R < 1,
 * chain_id0 < 0, sigma_z <= 0, tau <= 0, eta <= 0, D < 0, theta_out NULL, Z_out NULL with D > 0.
 * Chains of si_logdensity_grad_batch's fused class: per step the R S points go through the fused value + gradient launches in
 * passes of the workspace's capacity, then ONE update launch, which also forms the next step's points; nothing is copied and the
 * host synchronises ONCE, at the end.  EVERY OTHER CHAIN (Conv / MaxPool / flatten, SI_F32, the four later activations, wide
 * layers) runs the same two kernels, but the points go to the host and their values and gradients come back column by column
 * through si_logdensity_grad's path: slow, one round trip per point and step.  It has the same definition.                      */
int32_t si_fit_advi(si_ctx* ctx, int64_t max_iters /* T */, int32_t samples_per_step /* S */, double sigma_z, double eta, double tau,
                    int32_t window /* W */, uint64_t seed, int32_t chain_id0, int32_t nruns /* R */, int64_t ndraws /* D */,
                    double* theta_out /* 2M x R */, double* Z_out /* M x D x R, NULL iff D == 0 */,
                    double* elbo_out /* T x R or NULL */, double* theta_trace_out /* 2M x (T+1) x R or NULL */,
                    double* points_out /* M x S x T x R or NULL */);
/* the last si_fit_advi call: fused_out = 1 when it took the device-resident route, passes_out = gradient passes per step
 * (fused: ceil(R S / points per pass); other route: one per point)                                                               */
int32_t si_advi_kernel_info(si_ctx* ctx, int32_t* fused_out, int32_t* passes_out);
/* same, additionally returning the model output (out_dim x B) of the LAST z -- forward-pass parity  */
int32_t si_forward(si_ctx* ctx, const double* z /* M */, double* Yhat_out /* out_dim x B */);
/* posterior predictive on NEW inputs: Yhat_out[:, :, c] = f_{W_swa + P*Z[:, c]}(Xnew), out_dim x Bn x C column-major.
 * What the reference's users compute on the host from every returned weight sample (docs/src/nn_example.md:207-217,
 * `re(chn[i])(x)`), without materialising the N-long weight vectors.                                  */
int32_t si_predict(si_ctx* ctx, const double* Z /* M x C */, int32_t C, const double* Xnew /* in_dim x Bn */,
                   int64_t Bn, double* Yhat_out);
/* :111-116  DensityModel + RWMH(MvNormal(zeros(M), sigma_z)) + sample(model, spl, itr): `itr` samples
 * per chain INCLUDING the initial draw z0 ~ proposal; accept iff -randexp() < lp' - lp.  Chains
 * chain_id0 .. chain_id0+nchains-1 use the library's Philox4x32-10 streams (seed, chain, step).
 * Z_out is M x itr x nchains, lp_out is itr x nchains (column-major), accept_rate_out nchains.        */
int32_t si_sample_rwmh(si_ctx* ctx, int64_t itr, double sigma_z, uint64_t seed, int32_t chain_id0,
                       int32_t nchains, double* Z_out, double* lp_out, double* accept_rate_out);
/* si_sample_rwmh plus the reference's output map (:125 `map(z -> W_swa + P*z.params, chm)`), delivered WHILE the chain
 * runs: W_out is N x itr x nchains (column-major; sample t of chain c at W_out + N*(t + itr*c)), may be pageable and
 * untouched.  K4 has already formed W_swa + P z' for every proposal; the library keeps the chains' current weights in a
 * small device ring (select on accept, no second K4 pass over P), a second stream DMAs sample t into pinned staging
 * during transition t+1 and host threads (SI_HOST_COPY_THREADS) move it into W_out a few transitions later -- at cfg2
 * 8.4 MB per sample against 3.2 ms of compute.  Bit-identical to si_reconstruct on the returned Z.                   */
int32_t si_sample_rwmh_weights(si_ctx* ctx, int64_t itr, double sigma_z, uint64_t seed, int32_t chain_id0,
                               int32_t nchains, double* Z_out, double* lp_out, double* accept_rate_out, double* W_out);
/* The same chain, one transition at a time, with the proposal's sum of squared errors handed to the caller between
 * evaluation and acceptance: a DATA-SHARDED density (every rank holds a column block of X, Y and the same W_swa, P)
 * all-reduces the per-rank partial SSE there (one 8*nchains-byte RCCL all-reduce per step).  d_total = out_dim * B over
 * ALL ranks (0 = this ctx's own B).  All ranks use the same seed / chain ids, hence take identical decisions.        */
int32_t si_rwmh_begin(si_ctx* ctx, int64_t itr, double sigma_z, uint64_t seed, int32_t chain_id0, int32_t nchains,
                      int64_t d_total);
int32_t si_rwmh_step_eval(si_ctx* ctx, double* sse_local_out /* nchains; NULL = leave them on the device */);
int32_t si_rwmh_step_accept(si_ctx* ctx, const double* sse_total /* nchains; NULL = the device buffer holds them */);
/* device address of the nchains partial sums between step_eval(NULL) and step_accept(NULL): the caller all-reduces it
 * in place over RCCL on the stream given to si_set_stream -- no host round trip, no synchronisation per transition.  */
int32_t si_rwmh_sse_ptr(si_ctx* ctx, double** sse_dev_out, int32_t* nchains_out);
int32_t si_rwmh_end(si_ctx* ctx, double* Z_out, double* lp_out, double* accept_rate_out);
/* drop an open session.  While a session is open, si_logdensity / _grad / si_forward / si_predict / si_sample_rwmh
 * return SI_ERR_STATE (they share the session's proposal and SSE buffers); si_rwmh_begin restarts it.              */
int32_t si_rwmh_abort(si_ctx* ctx);
/* K6 as a DEVICE-RESIDENT loop and K5 as ONE launch for narrow Dense chains -- the sizes the reference itself
 * documents.  Automatic (on = 1, the default):
 *   - weights, data and activations of a chain fit one workgroup's LDS and 2*N*B <= 3 MFLOP (README.md:52-79): si_sample_rwmh
 *     runs all `itr` transitions of all chains in ONE launch, one workgroup per chain;
 *   - fp64 Dense chains with hidden widths <= 256 (docs/src/nn_example.md:112-118, 2-200-50-50-50-1 on 1000 observations): the
 *     density runs EVERY layer in one launch, a workgroup per batch tile with the activations in LDS; si_sample_rwmh runs all
 *     transitions in one PERSISTENT launch when ceil(B / tile) * nchains workgroups are resident together (one per CU), with
 *     two bounded grid barriers per transition -- a barrier that times out (the GPU is shared and the workgroups were not
 *     all resident) ends the call with SI_ERR_HIP, never a hang; more chains than that stack in the grid of the one-launch
 *     density, one pass of launches per transition.
 * Every form gives the SAME BITS as the launch-per-step loop with one launch per layer (on = 0: what the parity tests
 * compare against).  on = 2: the one-launch density, but no device-resident loop.
 * RUN-TIME SPECIALISATION (round 5): for chains with a narrow head whose weight fragments fit a wave's registers (the
 * nn_example model does) the two narrow-chain kernels are compiled once per distinct chain and process by hiprtc from kernel text
 * embedded in the library, with the layer table as compile-time constants (csrc/chain_spec.inc: same arithmetic, same bits;
 * ~1.5 s the first time a chain shape is used; the loop then takes ONE grid barrier per transition).  When hiprtc is not usable
 * the generic kernels run; si_chain_kernel_info says which did.  on = 3 / 4: as 1 / 2 with the generic kernels only.       */
int32_t si_set_chain_loop(si_ctx* ctx, int32_t on);
/* did the last density evaluation / the last si_sample_rwmh* call run the kernels specialised at run time (1) or the generic
 * ones (0)?  si_chain_spec_message: why not (hiprtc's log, or the class limit), "" when they did.                           */
int32_t si_chain_kernel_info(si_ctx* ctx, int32_t* density_specialised, int32_t* loop_specialised);
const char* si_chain_spec_message(si_ctx* ctx);
/* :91 / :125  W_out[:, c] = W_swa + P * Z[:, c]   (N x C col-major).  Pipelined: K4 -> pinned staging (second stream) ->
 * host threads (SI_HOST_COPY_THREADS, default min(8, cpus / 2)) copy into W_out, which may be pageable and untouched.  */
int32_t si_reconstruct(si_ctx* ctx, const double* Z /* M x C */, int64_t C, double* W_out);

/* ---- on-device training step for Dense chains with the mse cost ----------------------------------
 * Replaces the caller-side body of the reference's loop, src/subspace_construction.jl:39-43
 *     gs = gradient(ps) do training_loss = cost(model, d...) end;  Flux.update!(opt, ps, gs)
 * for cost = mse(m(x), y) and opt in {Descent (0), Momentum (1), ADAM (2)} with Flux 0.11.2 semantics (Float32 weights
 * and optimiser state, Float64 arithmetic).  p1 = rho / beta1, p2 = beta2.  The whole (X, Y) is uploaded once; a step
 * takes the observation indices of its batch (the DataLoader's permutation stays with the caller).                  */
int32_t si_train_setup(si_ctx* ctx, const si_layer* layers, int32_t L, int64_t N, const float* w0 /* N */,
                       const double* X, const double* Y, int32_t in_dim, int32_t out_dim, int64_t B_total,
                       int64_t batch_max, int32_t opt_kind, double eta, double p1, double p2);
/* The same with the data in the caller's element type and the arithmetic of the step chosen by it -- WHICH PRECISION A STEP
 * COMPUTES IN.  In the reference the step is `gradient(ps) do cost(model, x, y) end` on Flux arrays (:39-43): with a Float32
 * model (Flux's default) and Float64 data (`rand(10, 100)`, every example of the reference) Julia promotes and the pass is
 * Float64; with Float32 data (ordinary Flux practice) the whole pass -- sgemm forward and reverse, the loss -- is Float32.
 *   data_dtype     SI_F32 / SI_F64: element type of X and Y as the caller holds them
 *   compute_dtype  SI_DTYPE_OF_DATA (the reference's own arithmetic for that data), or SI_F32 / SI_F64 to override
 *                  (Float64 data + SI_F32 rounds X once; Float32 data + SI_F64 widens it: what si_train_setup's callers
 *                  had to do before round 5, wider than the reference and twice the matrix time)
 * SI_F32 (Dense chains; Conv chains: SI_ERR_INVALID, they train in SI_F64): fp32 operands and activations on
 * v_mfma_f32_32x32x2_f32 forward and reverse; the loss, the narrow head's partial sums and every sum over the batch (dW, db)
 * in fp64, rounded once into the Float32 gradient; the optimiser as Flux runs it (Float64 scalars on Float32 arrays, rounded on
 * the store).  Not bit-equal to a BLAS sgemm pass (the sums are blocked differently): measured against the oracle's Float32
 * path (tests/test_gpu_train_f32.py) the weights after 12 ADAM steps agree to 2e-6 of their scale, the loss to 1e-6.
 * si_train_grad_ptr / _get / _set keep exchanging N doubles (holding the Float32 values) in either mode.                  */
enum { SI_DTYPE_OF_DATA = -1 };
int32_t si_train_setup_ex(si_ctx* ctx, const si_layer* layers, int32_t L, int64_t N, const float* w0 /* N */, const void* X,
                          const void* Y, int32_t data_dtype, int32_t in_dim, int32_t out_dim, int64_t B_total, int64_t batch_max,
                          int32_t opt_kind, double eta, double p1, double p2, int32_t compute_dtype);
int32_t si_train_compute_dtype(si_ctx* ctx, int32_t* out /* SI_F32 / SI_F64: what the steps of this set-up compute in */);
/* With loss_out = NULL the call QUEUES the step and returns: idx (caller-owned, may be reused at once) is copied into a pinned
 * staging buffer and shipped asynchronously, a batch that is 0 .. nb-1 in order is used in place; nothing waits for the
 * previous step, so the caller's work between two steps overlaps the GPU's.  Errors of queued work surface at the next
 * synchronising call (a step with loss_out, si_train_get_weights, si_construct_finish, si_synchronize).              */
int32_t si_train_step(si_ctx* ctx, const int64_t* idx /* nb observation indices, 0-based */, int64_t nb,
                      double* loss_out /* mse of the batch before the update; may be NULL (no host sync) */);
/* :45-52 with W taken in place from the device-resident Float32 weights (no extract_params, no PCIe) */
int32_t si_train_push(si_ctx* ctx, double n);
int32_t si_train_get_weights(si_ctx* ctx, float* w_out /* N */);
/* the optimiser state after the device steps, so that the caller's `opt` can be left as Flux.update! leaves it (its
 * IdDict state persists across calls in the reference): m_out = Momentum velocity / ADAM first moment, v_out = ADAM
 * second moment (both Float32, flat layout of the weights; either may be NULL), beta_pows_out[2] = ADAM's running
 * beta1^t, beta2^t.                                                                                                 */
int32_t si_train_get_opt_state(si_ctx* ctx, float* m_out /* N */, float* v_out /* N */, double* beta_pows_out /* 2 */);
/* Data-parallel form of si_train_step (one gradient all-reduce per step).  Every rank holds the same
 * weights / optimiser state and its own nb of the nb_total observations of the batch:
 *   si_train_grad   forward + reverse sweep; leaves  d mse(whole batch)/dw  restricted to this rank's observations
 *                   (i.e. scaled by 1/(out_dim*nb_total)) in a device buffer and returns the local SSE;
 *   the caller sums that buffer over the ranks IN PLACE: RCCL all-reduce on the device pointer of si_train_grad_ptr
 *                   (N doubles; valid until the next si_train_setup), or si_train_grad_get / _set through the host;
 *   si_train_apply  Flux.update!(opt, ps, gs) (:43) from the summed gradient.
 * With nb_total == nb and no exchange, grad + apply is exactly si_train_step.                                       */
int32_t si_train_grad(si_ctx* ctx, const int64_t* idx, int64_t nb, int64_t nb_total, double* sse_local_out /* may be NULL */);
int32_t si_train_grad_ptr(si_ctx* ctx, double** grad_dev_out, int64_t* n_out);
int32_t si_train_grad_get(si_ctx* ctx, double* g_out /* N */);
int32_t si_train_grad_set(si_ctx* ctx, const double* g_in /* N */);
int32_t si_train_apply(si_ctx* ctx);
/* ---- the cost of the training step ------------------------------------------------------------------------------------------
 * The reference's loop takes any `cost`; the device step knows five of Flux 0.11.2's, each with its default agg = mean
 * [upstream Flux 0.11.2 src/losses/functions.jl and NNlib's logsoftmax / logsigmoid, restated from memory, unverifiable
 * offline; costs.py of the Python package is the definition the kernels are held to].  yhat = the chain's output (out x nb),
 * Y the targets, r = yhat - Y, d = out * nb:
 *   SI_COST_MSE       sum r^2 / d                                                             (the default; untouched)
 *   SI_COST_MAE       sum |r| / d;                         d/dyhat = sign(r) / d, sign(0) = 0
 *   SI_COST_HUBER     sum h(r) / d, h = r^2 / 2 for |r| < delta (strict), delta (|r| - delta / 2) otherwise; param = delta
 *   SI_COST_LOGITCE   logitcrossentropy(yhat, Y; dims = 1) = (1 / nb) sum_b -sum_i Y_ib (yhat_ib - lse_b), lse_b the
 *                     log-sum-exp of column b taken about its maximum; d/dyhat = (S_b softmax(yhat)_ib - Y_ib) / nb with
 *                     S_b = sum_i Y_ib kept (Zygote differentiates the formula as written)
 *   SI_COST_LOGITBCE  sum((1 - Y) yhat + softplus(-yhat)) / d, softplus(-x) = max(-x, 0) + log1p(exp(-|x|));
 *                     d/dyhat = (sigmoid(yhat) - Y) / d, the sigmoid evaluated without overflow for either sign
 * `param` is Huber's delta (finite, > 0) and ignored by the others.  The last layer's activation applies as for mse.  The
 * arithmetic of the cost is fp64 on every route; the SI_F32 route rounds Delta once into its Float32 reverse sweep.
 * si_train_set_cost is called after si_train_setup / _ex, like si_infer_set_prior after its set-up; every set-up starts
 * with SI_COST_MSE again.  SI_ERR_STATE without a training state; SI_ERR_INVALID (naming the reason) for an unknown id, a
 * delta that is not finite and positive, a NeuralODE set-up ("not available for NeuralODE training") and a call while a
 * gradient is pending (between si_train_grad and si_train_apply).
 * What the other calls return then: loss_out of si_train_step / si_train_step_dp and the total of si_train_allreduce_grad
 * divided by the cost's denominator (d, or nb for SI_COST_LOGITCE) are the cost; sse_local_out of si_train_grad is the LOCAL
 * NUMERATOR -- sum r^2 (mse), sum |r| (mae), sum h(r) (Huber), -sum_b sum_i Y_ib (yhat_ib - lse_b) (logitce),
 * sum((1 - Y) yhat + softplus(-yhat)) (logitbce) -- over this rank's observations; the gradient is scaled by 1 / (out *
 * nb_total), or 1 / nb_total for SI_COST_LOGITCE.  The sums are formed in a fixed order: the same inputs give the same bits. */
enum { SI_COST_MSE = 0, SI_COST_MAE, SI_COST_HUBER, SI_COST_LOGITCE, SI_COST_LOGITBCE };
int32_t si_train_set_cost(si_ctx* ctx, int32_t cost, double param);
int32_t si_train_cost_info(si_ctx* ctx, int32_t* cost_out, double* param_out);
/* ---- the training step of a NeuralODE (docs/src/node_example.md:272-285) -------------------------------------------------------
 * In place of si_train_setup for a NeuralODE right-hand side (si_infer_setup_node's layers, data layout, `ts` and si_node_opts):
 * a step minimises, over the batch's trajectories,
 *     loss = sum_{p in batch} ||sol_p(W) - Y_p||^2 + ||W||^2 / penalty_div            (penalty_div = 0: no penalty)
 * -- for a batch of one column the tutorial's L1(m, x, y) = sum(abs2, m(vec(x)) .- reshape(y[:,1], :,2)') + sum(sqnorm, ps)/100;
 * several columns sum over them (an extension).  The gradient is the DISCRETE ADJOINT of si_node_set_grad (accepted steps frozen;
 * node.py: train_value_and_grad is the definition) plus (W * 2) / penalty_div -- not Zygote's through DiffEqFlux's NeuralODE, a
 * continuous adjoint by default [upstream, from memory, unverifiable offline]: the two agree to the order of the tolerances, not
 * to rounding.  ||W||^2 is summed over the flat vector, not array by array as `sum(sqnorm, params)`: only the printed loss
 * depends on that order.  Weights and optimiser state are Float32, the arithmetic Float64, as for Chains.
 * After it si_train_step, si_train_grad + si_train_apply (nb_total == nb; sse_local_out receives the loss), si_train_grad_get
 * (also after a si_train_step: the step's gradient stays in the buffer) / _set / _ptr, si_train_push, si_train_get_weights, si_train_get_opt_state and si_train_compute_dtype (SI_F64) work with the
 * meanings above; loss_out is the loss of the batch before the update.  si_train_step_dp and si_train_allreduce_grad return
 * SI_ERR_INVALID ("not available for NeuralODE training").
 * Refused (SI_ERR_INVALID naming the limit): what si_infer_setup_node refuses, a layer wider than 64, and a step record plus
 * gradient slices -- batch_max * (max_steps * (d + 2) + N) doubles -- over the 2 GiB workspace budget ("lower max_steps or the
 * batch size").
 * A FAILED TRAJECTORY (status 1: max_steps reached, 2: a non-finite state) must not reach the weights: that step leaves w, m, v
 * as they were and records its number (1-based, counted from the set-up), the trajectory's position in its batch and the status
 * in a sticky device word; every later step of the set-up is a no-op too.  The next synchronising call (a step with loss_out,
 * si_train_grad, si_train_get_weights, si_train_get_opt_state, si_construct_finish*, si_synchronize) returns SI_ERR_INVALID
 * naming step, trajectory and status -- once; si_train_node_info keeps reporting it (failed_step_out -1: none).  si_train_push is
 * unchanged: it may push the unchanged weights after a failure, the synchronising call that follows raises.  Once the failure has been returned, further steps return SI_ERR_INVALID ("set up again")
 * and the host's beta powers are those of the last step that was taken.
 * Profiling classes of a step: SI_K_SSE the batch gather, ||W||^2 and the zeroing of the slices; SI_K_DENSE the forward with
 * record; SI_K_BACKWARD the reverse kernel; SI_K_RECON the tail kernel (gradient, loss, update, the Float64 copy of w).      */
int32_t si_train_setup_node(si_ctx* ctx, const si_layer* layers, int32_t L, int64_t N, const float* w0 /* N */,
                            const double* U0 /* d x f */, const double* Y /* d*S x f */, int32_t d, int32_t S, int64_t f,
                            const double* ts /* S */, const void* opts /* const si_node_opts* */, int64_t batch_max,
                            int32_t opt_kind, double eta, double p1, double p2, double penalty_div /* 0: no penalty */);
int32_t si_train_node_info(si_ctx* ctx, int32_t* active_out, int32_t* G_out, int64_t* failed_step_out /* -1: none */,
                           int64_t* failed_traj_out, int32_t* failed_status_out);

/* ---- R1: multi-GPU behind the C ABI ------------------------------------------------------------
 * One process per GPU, one si_ctx per process, one RCCL communicator per ctx (RCCL over xGMI; bound with dlopen at the
 * first si_comm_* call -- a host that already carries librccl.so.1, e.g. PyTorch, shares its copy).  The reference is
 * single-process; what these collectives parallelise:  src/subspace_construction.jl:45-52,63 (row-sharded SWA /
 * deviation / Gram / projection), src/space_inference.jl:94 (log-likelihood over column blocks of the data),
 * src/subspace_construction.jl:39-43 (data-parallel training step), and independent chains (no per-step exchange).
 * Every collective is issued on the ctx's stream, in place on buffers the library owns: no host staging and no
 * synchronisation of its own.  All ranks must make the same calls in the same order (RCCL semantics).
 * Failure behaviour: the entry points that prepare something LOCALLY before their collective (si_bcast_subspace,
 * si_construct_allgather, si_sample_rwmh_sharded, si_train_step_dp) first agree on the ranks' local status with one
 * 8-byte all-reduce (max): when any rank failed its preparation, NO rank issues the data collective -- the failing rank
 * returns its own error, the others SI_ERR_COMM.  The thin in-place collectives (si_construct_allreduce_gram,
 * si_rwmh_allreduce_sse, si_train_allreduce_grad, si_comm_*_host) check only local state that is the same on every rank
 * of an SPMD caller (a communicator exists, si_construct_gram / si_rwmh_step_eval / si_train_grad ran); a rank that
 * returns SI_ERR_STATE from one of them while the others are inside it leaves those blocked -- keep the call sequences
 * identical, as with RCCL itself.
 *
 * Start-up: rank 0 calls si_comm_unique_id and ships the 128 bytes to the other ranks by whatever the host has
 * (Julia: Distributed.remotecall / a file; Python: a file or any process group); every rank then calls
 * si_comm_init_rank.                                                                                               */
#define SI_COMM_ID_BYTES 128
enum { SI_COMM_SUM = 0, SI_COMM_MAX = 1 };
int32_t si_comm_unique_id(uint8_t* id_out /* SI_COMM_ID_BYTES */);   /* needs no ctx; errors: si_last_error(NULL) */
int32_t si_comm_init_rank(si_ctx* ctx, int32_t world, int32_t rank, const uint8_t* id /* SI_COMM_ID_BYTES */);
int32_t si_comm_destroy(si_ctx* ctx);                                 /* also done by si_destroy */
/* world = 0 when the ctx has no communicator; rccl_version = ncclGetVersion (0 when RCCL could not be loaded) */
int32_t si_comm_info(si_ctx* ctx, int32_t* world_out, int32_t* rank_out, int32_t* rccl_version_out);
/* small HOST values over the communicator (timings, losses, rank counts): n <= 4096, op = SI_COMM_SUM / SI_COMM_MAX;
 * synchronous.  si_comm_barrier returns when every rank's stream has reached it.                                    */
int32_t si_comm_allreduce_host(si_ctx* ctx, double* inout, int64_t n, int32_t op);
int32_t si_comm_allgather_host(si_ctx* ctx, const double* send /* n */, int64_t n, double* recv /* n x world */);
int32_t si_comm_barrier(si_ctx* ctx);
/* The row partition every sharded entry point assumes: rank's rows [r0, r1) of n_total, boundaries on multiples of 32
 * elements (256 B) so that each shard keeps the kernels' 16-byte alignment.  Pure arithmetic (no ctx, no GPU).      */
int32_t si_row_shard(int64_t n_total, int32_t rank, int32_t world, int64_t* r0_out, int64_t* r1_out);
/* Row-sharded construction: each rank pushes ITS rows of every snapshot (si_construct_begin with N = r1 - r0), then
 *     si_construct_gram;  si_construct_allreduce_gram;                          -- G = sum of the local A'A, K x K fp64
 *     si_construct_needs_refine -> if set: si_construct_refine; si_construct_allreduce_gram   (ill-conditioned A)
 *     si_construct_finish            -- replicated K x K eigensolve, this rank's rows of P
 *     si_construct_allgather(n_total) (optional) -- the FULL (W_swa, P) on every rank, device to device; the ctx then
 *                                       holds a finished construction of n_total rows (si_infer_setup(NULL, NULL)).   */
int32_t si_construct_allreduce_gram(si_ctx* ctx);
int32_t si_construct_allgather(si_ctx* ctx, int64_t n_total);
/* Independent chains (BASELINE cfg3): (W_swa, P, s) of the construction finished on `root` -> every rank's ctx, device
 * to device, once (168 MB at cfg2); receivers then hold a finished construction.  No exchange per transition: rank r
 * runs chains with its own chain ids (si_sample_rwmh), results are gathered with si_comm_allgather_host.            */
int32_t si_bcast_subspace(si_ctx* ctx, int32_t root, int64_t N, int32_t M);
/* Data-sharded density (BASELINE cfg5): each rank's si_infer_setup holds a column block of (X, Y) and the full
 * W_swa / P; all ranks use the same seed / chain ids.  Between si_rwmh_step_eval(NULL) and si_rwmh_step_accept(NULL):
 * all-reduce of the nchains partial sums of squared errors (8 * nchains bytes).  si_sample_rwmh_sharded is the whole
 * loop in one call (eval -> all-reduce -> accept per transition on one stream, no host round trip); d_total =
 * out_dim * observations over ALL ranks.                                                                            */
int32_t si_rwmh_allreduce_sse(si_ctx* ctx);
int32_t si_sample_rwmh_sharded(si_ctx* ctx, int64_t itr, double sigma_z, uint64_t seed, int32_t chain_id0, int32_t nchains,
                               int64_t d_total, double* Z_out, double* lp_out, double* accept_rate_out);
/* Data-parallel training step: after si_train_grad on this rank's share of the batch, sum the N-double gradient and
 * the local SSE over the ranks (one grouped launch); sse_total_out may be NULL (then no host synchronisation).
 * si_train_step_dp = si_train_grad + si_train_allreduce_grad + si_train_apply; loss_out = mse of the WHOLE batch.   */
int32_t si_train_allreduce_grad(si_ctx* ctx, double* sse_total_out);
int32_t si_train_step_dp(si_ctx* ctx, const int64_t* idx, int64_t nb, int64_t nb_total, double* loss_out);

/* ---- the autoencoder of auto_encoder_subspace trained on the device (reference src/subspace_construction.jl:125-140) ----------
 * Chain(encoder, decoder) = N -> e_1 -> ... -> H -> N, Dense only, trained to reproduce the columns of the N x K deviation
 * matrix: loss = sum r^2 / (N nb) over a batch of nb columns, r = sae(x) - x; with `penalty` the loss gains sum w^2 and the
 * gradient 2 w.  subspaceinference.jl_amd/autoencoder.py: train_step is the definition (all arithmetic fp64; parameters and
 * optimiser state in w_dtype, rounded once on the store).  `layers` are the L = E + D layers with their offsets in the packed
 * flux.params order ([vec(W_l); b_l] per layer); w0 holds n_params elements of w_dtype.  X = NULL reads the OPEN construction's
 * deviation matrix in place (fp64 or fp32 storage; N must be the construction's, K is its column count); otherwise X is the
 * N x K fp64 host matrix, copied once.  The two big layers run as N-parallel streaming kernels with the optimiser update fused
 * (their gradients are never written); the three N-long sums have one blocked order that depends on N alone.
 * The state is its own object on the context: independent of si_train_* and of an inference set-up; si_construct_begin,
 * si_ae_train_free and si_destroy free it.
 * Refused with SI_ERR_INVALID, naming the limit: a layer that is not SI_LAYER_DENSE; the first `in` or the last `out` != N; E + D
 * outside 2 .. 16 (the library sees the sum only: that E and D lie in 1 .. 8 EACH is NOT enforced here -- E = 1, D = 15 is
 * accepted -- but by the caller that knows the split, as api.py does); a hidden width > 256; batch_max outside 1 .. 8; widths that do not chain, an
 * unknown activation, offsets that are not the packed order, n_params that differs from their sum; w_dtype or opt_kind unknown;
 * X = NULL on a construction with max_cols > 0 or another N.  SI_ERR_STATE: X = NULL without an open construction that holds
 * columns.  A step refuses nb > batch_max, nb < 1 and an index outside 0 .. K-1.
 * si_ae_train_step: one step on the nb columns idx (the host DataLoader's shuffle, passed step by step); loss_out receives the
 * loss of the batch BEFORE the update, or NULL: the step is queued and nothing synchronises, as si_train_step.
 * si_ae_train_loss: the loss over all K columns, forward only, batch_max columns at a time (the reference's callback).
 * si_ae_train_get_params / _get_opt_state: flat, in w_dtype (m_out, v_out may be NULL; beta_pows_out[2] as si_train_get_opt_state).
 * si_ae_train_info: whether a set-up is active, its N, K, n_params, and whether the last layer's update runs inside the pass over
 * W_D (1: it does).  Profiling classes of a step: SI_K_DENSE the first layer's forward and the head; SI_K_DENSE_MAIN the pass over
 * W_D; SI_K_BACKWARD the head's reverse and the updates of the small arrays and of W_1; SI_K_SSE the passes of si_ae_train_loss. */
int32_t si_ae_train_setup(si_ctx* ctx, const si_layer* layers, int32_t L /* E + D */, int64_t n_params, const void* w0,
                          int32_t w_dtype /* SI_F32 | SI_F64 */, const double* X /* N x K fp64 host, or NULL */, int64_t N, int64_t K,
                          int32_t batch_max, int32_t opt_kind, double eta, double p1, double p2, int32_t penalty);
int32_t si_ae_train_step(si_ctx* ctx, const int64_t* idx /* nb column indices, 0-based */, int64_t nb, double* loss_out /* may be NULL */);
int32_t si_ae_train_loss(si_ctx* ctx, double* loss_out);
int32_t si_ae_train_get_params(si_ctx* ctx, void* w_out /* n_params of w_dtype */);
int32_t si_ae_train_get_opt_state(si_ctx* ctx, void* m_out, void* v_out, double* beta_pows_out /* 2 */);
int32_t si_ae_train_info(si_ctx* ctx, int32_t* active_out, int64_t* N_out, int64_t* K_out, int64_t* n_params_out, int32_t* fused_out);
int32_t si_ae_train_free(si_ctx* ctx);

/* ---- host utility (no GPU needed): the K x K symmetric eigensolver used inside si_construct_finish.
 * a: n x n symmetric column-major, overwritten by the eigenvectors (columns); w: eigenvalues ascending. */
int si_host_sym_eig(int n, double* a, double* w);
/* The route si_construct_finish takes first: only the m largest eigenpairs (Householder reduction with the reflectors
 * kept in factored form, eigenvalues by vector-free QL, eigenvectors by inverse iteration, result verified against g).
 * g: n x n symmetric column-major, left intact; w_top: m eigenvalues DESCENDING; V: n x m eigenvectors.
 * Returns 0 = verified result, 1 = declined / failed verification (si_construct_finish then uses si_host_sym_eig). */
int si_host_sym_eig_top(int n, const double* g, int m, double* w_top, double* V);
/* The second-stage solver of the ill-conditioned route: cyclic two-sided Jacobi with the scaled stopping criterion
 * |a_pq| <= eps*sqrt(a_pp*a_qq) for a symmetric positive semi-definite matrix (eigenvalues accurate relative to
 * themselves for graded matrices).  a: n x n column-major, destroyed; w: eigenvalues DESCENDING; v: eigenvectors.   */
int si_host_jacobi_eig_psd(int n, double* a, double* w, double* v);
/* the window schedule of si_sample_hmc's metric adaptation for n_adapts steps (host only): *window_start .. *window_end are the
 * steps inside a window, splits[0 .. count) the steps that close one (at most `cap` are written).  Init buffer 75, terminal buffer
 * 50, windows doubling from 25, the last stretched to window_end; 15 % / 75 % / 10 % for 20 <= n_adapts < 150; below 20 no step is
 * inside a window.  Returns count.                                                                                              */
int32_t si_host_hmc_windows(int64_t n_adapts, int64_t* window_start, int64_t* window_end, int64_t* splits, int32_t cap);
/* The host copy pool (si_construct_push, si_reconstruct, si_sample_rwmh_weights) sizes itself from the CPUs the process may
 * really use: the affinity mask capped by the cgroup CPU quota (si_host_cpu_budget; a container that shows 256 CPUs and
 * grants 16 gets 16).  Threads per process = SI_HOST_COPY_THREADS if set, else min(8, budget / (2 * nproc)) with nproc = the
 * world of the ctx's communicator (si_comm_init_rank shrinks the pool: 8 ranks on a 16-CPU quota copy with one thread each).
 * si_host_parse_cpu_max: "<quota> <period>" of a cgroup-v2 cpu.max file -> CPUs granted (0 = unlimited / unparsable).    */
int si_host_cpu_budget(void);
double si_host_parse_cpu_max(const char* text);
int si_host_copy_plan(int budget, int nproc, const char* env /* value of SI_HOST_COPY_THREADS or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* SUBSPACE_HIP_H */
