// Internal declarations shared by the translation units of the C ABI and the kernel launchers: the plans of a Chain, the
// training state and the context (every buffer in them held by an owner type of dev_buf.h, grouped by who releases it),
// and the launchers of kernels_*.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "../../include/subspace_hip.h"
#include "dev_buf.h"

namespace si {

// leading dimensions of device matrices are padded to a multiple of this many elements (512 B) so that every
// column starts 512-B aligned, 16-B vector accesses are legal whatever N is (N is odd at cfg2), and the 64-row slabs
// of the Gram kernel never run past a column (the padding rows of A are kept at zero).
constexpr int64_t LD_ALIGN = 64;
inline int64_t pad_ld(int64_t n) { return (n + LD_ALIGN - 1) / LD_ALIGN * LD_ALIGN; }

// one 16-feature tile of a layer as a wave runs it (64 bytes: one scalar load); chain_fused_program builds the lists
enum { SI_CG_SYNC = 1, SI_CG_GLOBAL = 2, SI_CG_MARKER = 4 };
struct CgTileD {
  int64_t woff, boff;      // elements into the weight vector: the layer's W and bias
  int32_t out, row0;       // rows of W (its pitch); first feature of the tile
  int32_t in, pad2;        // columns of W
  int32_t flags;           // SI_CG_SYNC: the wave's last tile of a layer; _GLOBAL: outputs go to yhat; _MARKER: no tile, barrier only
  int32_t img_in, ldi;     // input image (0 X tile, 1 / 2 the two activation images) and its pitch
  int32_t img_out, ldo;    // output image and its pitch
  int32_t act, pad0, pad1;  // act: SI_ACT_* | layer index << 8
};
struct EventPair {
  hipEvent_t a, b;
  int cls;
};

// geometry of one convolution-shaped gather (kernels_conv.hip): the tensor T holds Cp channels (channel-fastest) on a
// Wi x Hi grid per image; GEMM position (wo, ho) and tap (a, c) address ((wo, ho)*snum - pad + (a, c)*dil) / sden
struct ConvGeom {
  int Cp, Wi, Hi, Wo, Ho, KW, KH;
  int snum_w, snum_h, sden_w, sden_h, pad_w, pad_h, dil_w, dil_h;
  int Kvalid;          // Cp*KW*KH: taps at or past it read as zero (k is padded to whole 16-deep tiles)
  int64_t img_stride;  // Cp*Wi*Hi
};

// one layer of a Chain as the device executes it (capi_net.hip builds it from the caller's si_layer table)
struct LayerPlan {
  int kind = 0, act = 0;
  int64_t w_off = 0, b_off = 0;
  int in_feat = 0, out_feat = 0;         // the reference's feature counts (si_layer in / out)
  int64_t in_elems = 0, out_elems = 0;   // per observation in the layout the device uses (channel pitch inside conv stacks)
  int C = 0, Cp = 0, Co = 0, Cop = 0;    // input / output channels and their even pitches
  int Wi = 0, Hi = 0, Wo = 0, Ho = 0, KW = 0, KH = 0, sw = 1, sh = 1;
  int Kp = 0, KpT = 0;                   // padded tap counts of the forward / data-gradient GEMMs
  size_t wp_off = 0, bp_off = 0;         // packed weights / bias inside the pack workspace (doubles)
  ConvGeom g{}, gT{};
};
struct NetPlan {
  std::vector<LayerPlan> L;
  bool has_conv = false;        // any non-Dense layer: the generic path of capi_net.hip runs the chain
  bool input_spatial = false;   // the chain starts on (W, H, C) data: X is re-laid channel-fastest once
  int in_W = 0, in_H = 0, in_C = 0, in_Cp = 0;
  int64_t in_elems = 0;         // per observation, device layout
  int64_t max_elems = 1;        // largest per-observation activation (device layout) over input and all layers
  size_t wpack_elems = 1;       // forward packs of all conv layers
  size_t wt_elems = 1;          // largest transposed pack (data gradient), one layer at a time
  int max_rows = 1;             // largest row count handed to the row-sum kernels
};
// What a layer table means, for the inference set-up and the training set-up alike: built by chain_model_build (capi.hip) and by
// nothing else; every pass over a chain takes it instead of its fields.
struct ChainModel {
  std::vector<si_layer> layers;
  NetPlan plan;                 // validation + geometry; has_conv: the generic path of capi_net.hip runs the chain
  int64_t N = 0;                // length of the flat weight vector
  int32_t in_dim = 0, out_dim = 0;   // (NeuralODE: in_dim = d, out_dim = the d*S rows of the observed trajectories)
  bool f32 = false;             // compute_dtype = SI_F32: fp32 X / weights / activations; the head's partials, the SSE and the batch sums stay fp64
  bool fuse_tail = false;       // narrow last layer of a Dense chain: folded into the epilogue of the layer in front of it
  int fuse_slots = 0, fuse_slots32 = 0;   // feature slots of the fused head on the fp64 / the fp32 kernel (fuse_slots32: only with f32)
  int main_layer = 0;           // the layer with the most flops (its launch also counts as SI_K_DENSE_MAIN)
  int64_t max_stored = 1;       // widest output the forward pass stores, per observation (not the fused layer's, not the head's)
  const si_layer* lay() const { return layers.data(); }   int L() const { return (int)layers.size(); }
  int part_slots() const { return std::max(fuse_slots, fuse_slots32); }   // what one buffer of head partials for either kernel holds
};
struct NetScratch {             // reverse-sweep workspaces (sized by net_scratch_sizes)
  DevBuf<double> bwpart, rspart, wt, dbtmp;
  // gradient mode, a view of SweepWs::pidx: pidx[l] = byte index tensor of conv layer l whose MaxPool ran fused with it (net_grad_fused), else empty
  const DevBuf<uint8_t>* pidx = nullptr;
};
// workspace of one fp32 sweep at up to Bmax observations (see dense_value_and_grad_f32 below)
struct SweepF32Ws {
  std::vector<DevBuf<float>> hs32;
  DevBuf<float> delta32[2];
  DevBuf<float> gw32, wt32, zero32, part32;
  DevBuf<double> rspart64, tailpart64, yhat64;
};
// The training step's gradient routes; the first three: those of every value-and-gradient pass through a Chain (chain_value_and_grad)
enum class TrainRoute { DenseF64, DenseF32, Conv, Node };
// What such a pass keeps between calls for up to Bmax observations, on the route its chain takes (the rest stays empty); sized
// and allocated by sweep_ws_alloc (capi.hip) and nowhere else.
struct SweepWs {
  TrainRoute route = TrainRoute::DenseF64;
  bool ready = false;                  // allocated in full
  std::vector<DevBuf<double>> hs;      // DenseF64, Conv: post-activation output of every layer, out_elems x Bmax (empty where pidx[l] stands in)
  DevBuf<double> delta[2];             // DenseF64, Conv: widest layer (Conv: largest activation) x Bmax
  DevBuf<double> bwpart, rspart;       // DenseF64: split-K partials of dW (or the narrow head's), row-sum partials
  SweepF32Ws f32;                      // DenseF32
  NetScratch net;                      // Conv
  std::vector<DevBuf<uint8_t>> pidx;   // Conv, per layer: window-index bytes of a Conv layer fused with its MaxPool (net_grad_fused)
};

// ---- training of the autoencoder on the device (si_ae_train_*; capi_ae_train.hip, kernels_ae_train.hip; autoencoder.py:
// train_step is the definition).  Chain(encoder, decoder) = N -> e_1 -> ... -> H -> N, Dense only, parameters and ADAM moments in
// the caller's element type in the packed flux.params order; the data are the N x K deviation columns, read IN PLACE from the open
// construction's d_A (borrowed: si_construct_begin drops this state) or from an uploaded copy.
constexpr int SI_AE_MAX_LAYERS = 16, SI_AE_MAX_WIDTH = 256, SI_AE_MAX_BATCH = 8;
struct AeLayers {
  int32_t n = 0;
  int32_t in[SI_AE_MAX_LAYERS] = {0}, out[SI_AE_MAX_LAYERS] = {0}, act[SI_AE_MAX_LAYERS] = {0};
  int32_t a_off[SI_AE_MAX_LAYERS] = {0};   // layer l < n-1: where its output (out x batch_max, column pitch out) sits in acts / deltas
  int64_t w_off[SI_AE_MAX_LAYERS] = {0}, b_off[SI_AE_MAX_LAYERS] = {0};
};
struct AeArgs {                  // every kernel of the step takes this by value
  AeLayers lay;
  int64_t col[SI_AE_MAX_BATCH] = {0};   // the batch's columns of A
  int32_t nb = 0;
  void *w = nullptr, *m = nullptr, *v = nullptr;
  const void* A = nullptr;       // TA elements, column pitch ldA
  int64_t ldA = 0, N = 0, nblk = 0;     // nblk: row blocks of AE_ROWS rows
  int32_t G = 0;                 // workgroups of the two row kernels: min(nblk, AE_GRID)
  double *part1 = nullptr, *part2 = nullptr;   // G x (e_1 nb + 1), G x (H nb + 2) workgroup sums
  double *acts = nullptr, *deltas = nullptr;   // a_l and the unscaled cotangents dt_l of layers 0 .. n-2
  double* loss = nullptr;        // [0] the loss, [1] sum r^2 carried from chunk to chunk by si_ae_train_loss
  int32_t kind = 0, penalty = 0;
  double eta = 0.0, p1 = 0.0, p2 = 0.0, bp1 = 0.0, bp2 = 0.0, s = 0.0;   // s = 2.0 / (N nb)
};
struct AeTrainState {
  AeArgs args;                   // the constants; per step: col, nb, bp1, bp2, s
  int64_t K = 0, n_params = 0;
  int32_t dtype = SI_F64, a_dtype = SI_F64, batch_max = 0;
  bool borrowed = false;         // A is the construction's d_A
  DevBuf<char> w, m, v;          // n_params elements of dtype each
  DevBuf<double> X;              // the uploaded copy (pad_ld(N) x K) when X was given
  DevBuf<double> part1, part2, acts, deltas, loss;
};
int ae_rows();                   // AE_ROWS, AE_GRID of kernels_ae_train.hip
int ae_grid_cap();
// one step's launches on st (dtype / a_dtype: element types of the parameters and of A).  forward: first layer, head.  last:
// the pass over W_D -- with update, the pull-back partials and the fused update of W_D, b_D; without, sum r^2 only.  reverse:
// head reverse, the loss word, the update of the small arrays and of W_1.  loss_chunk: si_ae_train_loss's accumulation.
void launch_ae_forward(hipStream_t st, const AeArgs& a, int32_t dtype, int32_t a_dtype);
void launch_ae_last(hipStream_t st, const AeArgs& a, int32_t dtype, int32_t a_dtype, bool update);
void launch_ae_reverse(hipStream_t st, const AeArgs& a, int32_t dtype, int32_t a_dtype, int num_cu);
void launch_ae_loss_chunk(hipStream_t st, const AeArgs& a, int32_t dtype, bool last, double denom);

struct TrainState;   // on-device training (below, after NodeTrain)

// ---- the context.  Its members are split by WHO RELEASES THEM: assigning a fresh ConstructState / InferState is
// free_construct / free_infer, everything in CtxCore lives until si_destroy deletes the context: nothing in it describes a set-up or
// a step-wise session -- of inference it holds the caller's settings (si_set_chain_loop) and why the specialised kernels last stayed out.
struct CtxCore {
  int device = -1;
  TrainState* train = nullptr;
  std::unique_ptr<AeTrainState> ae;   // si_ae_train_*: its own object, independent of `train` and of an inference set-up
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::string err;
  char devname[256] = {0};
  int num_cu = 256;
  // R1: RCCL communicator of this ctx (comm.hip; an ncclComm_t, kept opaque here), one rank per ctx.  Its two scratch buffers
  // are comm.hip's own (plain hipMalloc / hipFree, released by comm_release)
  void* comm = nullptr;
  int comm_world = 0, comm_rank = 0;
  double* d_commtmp = nullptr;  // device scratch of the host-value collectives
  double* d_gathertmp = nullptr;  // device scratch of si_comm_allgather_host, kept between calls
  size_t gathertmp_cap = 0;

  hipStream_t stream2 = nullptr;   // side stream (pipelined pushes, si_reconstruct's output pipeline, the streamed output map), created on first use
  // pinned host staging for the small construct-time transfers (G down, V up): pageable copies cost tens of us each
  PinBuf<double> h_pin;
  PinBuf<char> h_outpin;         // pinned staging of the samples / lp of a device-resident loop on their way to the caller's arrays
  PinBuf<double> h_stage[2];     // pinned staging of si_reconstruct's output pipeline (kept between calls)
  DevBuf<double> d_stage[2], d_zstage[2];   // its device-side double buffer
  // streamed output map (si_sample_rwmh_weights): device ring of the chains' CURRENT weights, pinned twin, events
  DevBuf<double> d_wring;
  DevBuf<int32_t> d_accflag;
  PinBuf<double> h_wring[4];
  Event ev_wcomp[4], ev_wcopy[4];
  int64_t wring_N = 0;
  int32_t wring_C = 0;
  // profiling
  bool profiling = false;
  uint32_t prof_mask = 0xffffffffu;  // classes that get event pairs while profiling is on
  std::vector<EventPair> pending;
  std::vector<hipEvent_t> event_pool;
  si_stats stats{};

  // construction: what outlives a construction
  int32_t max_cols = 0;
  DevBuf<float> d_wstage;     // staging of si_construct_set_mean
  // pipelined host pushes (si_construct_push): two pinned host buffers -> two device buffers, events mark the H2D of each
  PinBuf<char> h_wpin[2];
  DevBuf<char> d_wpush[2];
  Event ev_wpin[2];           // H2D of buffer b done (copy stream)
  Event ev_wk1[2];            // K1 on buffer b done (compute stream)
  bool wpin_busy[2] = {false, false};
  uint64_t wpin_next = 0;
  DevBuf<double> d_nvals;     // per-push n values of a batched push
  std::vector<double> svals;
  std::vector<double> vfull;      // K x K eigenvectors of A'A, columns DESCENDING by eigenvalue (host)

  // inference: the caller's settings, kept across set-ups
  bool chain_loop_enabled = true;   // si_set_chain_loop: 0 forces the launch-per-step loop (the parity tests compare the two)
  int chain_mode = 1;               // si_set_chain_loop: 0 per-layer launches, 1 automatic, 2 the fused forward without the persistent loops
  bool chain_spec = true;           // si_set_chain_loop 3 / 4: generic kernels only
  std::string spec_message;         // why the specialised kernels did not run, when they did not (hiprtc log, class limits)

  CtxCore() = default;
  CtxCore(const CtxCore&) = delete;
  CtxCore& operator=(const CtxCore&) = delete;
  ~CtxCore();   // (capi_train.hip, where TrainState is complete: releases `train`)
};

// What si_construct_finish_diffmap keeps (capi_diffmap.hip, kernels_diffmap.hip): its own buffers, none shared with the PCA route.
// Part of the construction state: dropped by free_construct and by every si_construct_begin.
struct DiffmapState {
  int64_t N = 0;               // rows of the last finished call (0: none; si_diffmap_get_kernel reads Kn and u_1 of it)
  int32_t iters = 0;           // si_diffmap_info
  double residual = 0.0;
  DevBuf<double> Xr, s, mm;    // rescaled X (Kp x Npad), squared column norms (Npad), per-snapshot min / max (2 K)
  DevBuf<double> Kn;           // ldn x N, padding rows zero: Kmat, normalised in place
  DevBuf<double> part, p, q, u1;   // row-sum partials (blocks x ldn); p, q, u_1 (ldn each)
  DevBuf<int> flag;            // a non-finite kernel entry was seen
  DevBuf<double> Z[2];         // the stacked block [V W] (ldn x 2b) and where the next block / the Ritz vectors go
  DevBuf<double> R, Vt, coef;  // residual vectors (ldn x M), V' for the product (pad_ld(b) x N), coefficient uploads
  DevBuf<double> G, Gpart, res;   // the stacked Gram matrix (2b x 2b), K2's partial slabs, residual norms (M)
};

// ---- construction state (reference src/subspace_construction.jl:31-33,45-52,61-65): what free_construct drops
struct ConstructState {
  bool c_active = false, c_finished = false, gram_valid = false;
  int64_t N = 0, ldA = 0, Kcap = 0, K = 0;  // K = columns held
  int64_t npush = 0;
  DevBuf<double> d_swa;       // N (padded) fp64
  DevBuf<char> d_A;           // BYTES of the ldA x Kcap column-major matrix of a_dtype elements (doubles, or floats with SI_F32); with max_cols>0 a ring of max_cols columns
  int32_t a_dtype = SI_F64;   // storage of the deviation matrix (si_construct_set_storage)
  int32_t a_zero_dtype = -1;  // element type for which the padding rows of d_A are known to be zero (-1: unknown)
  int64_t a_zero_cols = 0;    // ... in the first a_zero_cols columns
  bool a_pending = false;     // si_construct_begin ran, the matrix is allocated / checked by the first push or si_construct_set_storage
  DevBuf<double> d_G;         // K x K
  DevBuf<double> d_Gpart;     // partial slabs
  DevBuf<double> d_V;         // K x Mpad (row k contiguous)
  DevBuf<double> d_P;         // ldA x M
  int32_t M_built = 0;
  // ill-conditioned route (second-stage Gram): B = A * V_full, d_G then holds G2 = B'B
  int refine_stage = 0;           // 0: d_G = A'A;  1: d_B valid and d_G = B'B (possibly all-reduced by the caller)
  DevBuf<double> d_At;            // K > N route: A' (pad_ld(K) x N), kept between finishes of one shape
  DevBuf<double> d_B;             // ldA x K
  DiffmapState dm;                // method = :diffusion
};

// per-chain scalars of si_sample_hmc (kernels_hmc.hip): the adaptor's dual averaging and Welford count, the kinetic energy of the
// proposal's momentum, and the state machine of the step-size search
struct HmcChain {
  double eps, mu, hbar, log_eps_bar, k0;
  int64_t da_t, wn;
  double s_eps, s_next, s_lo, s_hi, s_h0, s_trial;   // search: current / candidate step size, the bracket, H at z_0, the trial's step
  int32_t s_phase, s_dir, s_iter, s_done;
};

// per-chain scalars of si_sample_nuts (kernels_nuts.hip): the trajectory tree of the transition under way and the scalars of the
// stack of sub-tree summaries of the doubling under way (their vectors live in NutsRun::stack)
static constexpr int NUTS_MAX_DEPTH = 10;
struct NutsChain {
  double h0, logw, lpc, alpha_sum;   // H at the transition's start, the tree's log weight, the candidate's lp, the sum of the leaves' alpha
  double s_lp[NUTS_MAX_DEPTH], s_logw[NUTS_MAX_DEPTH], s_alpha[NUTS_MAX_DEPTH];   // per stack entry: lp of its proposal, log weight, sum of alpha
  int32_t s_n[NUTS_MAX_DEPTH], s_sel[NUTS_MAX_DEPTH];                             // its leaves, the leaf that is its proposal
  int64_t nlog;                      // leaves of this call so far (the leaf log's next slot)
  int32_t n_alpha, depth, ndoub, dir, k, sp, nleaf, selc, open;   // leaves counted into alpha_sum; doublings completed / started;
                                     // direction; leaves of the doubling; stack entries; leaves; the candidate's leaf; still building
};

// What every sampler over stacked points keeps per chain (si_sample_mala, si_sample_hmc, si_sample_nuts): the state, the proposal or
// pending point, and the value and gradient at both.  Nothing in it outlives a call: the first kernels of every call write all of it.
struct ChainState {
  int cap = 0;                    // chains it holds (grown on demand: reserve_chain_state, capi_common.h)
  DevBuf<double> z, g, zp, gp;    // M x C each
  DevBuf<double> lp, lpp;         // C each
};

// What a call of a gradient-driven entry point took, for its si_*_kernel_info: the stacked evaluator's route and passes; the rounds
// of the step-size search (HMC, NUTS); the rounds and leaves of all transitions (NUTS).  All zero before a first call and after a
// refused one.
struct CallInfo {
  int32_t fused = 0, passes = 0, search_rounds = 0;
  int64_t rounds = 0, leaves = 0;
};

// The autoencoder route (si_infer_set_decoder; reference src/space_inference.jl:247,278: W_swa + decoder(z)): a Dense-only
// decoder M -> h_1 -> ... -> h_{D-1} -> N with its parameters on the device in the element type they came in.  The layers
// 1 .. D-1 (the "head") read `params` at the caller's offsets; the last layer's W (N x H) is kept a second time with its
// columns pad_ld(N) apart and zero padding rows, so that the streaming kernels read aligned row pairs whatever N is.
constexpr int SI_DEC_MAX_LAYERS = 8;
struct DecoderHead {             // the head's layer table as the two one-workgroup-per-point kernels take it (by value)
  int32_t n = 0;                 // D - 1
  int32_t in[SI_DEC_MAX_LAYERS] = {0}, out[SI_DEC_MAX_LAYERS] = {0}, act[SI_DEC_MAX_LAYERS] = {0}, hid_off[SI_DEC_MAX_LAYERS] = {0};
  int64_t w_off[SI_DEC_MAX_LAYERS] = {0}, b_off[SI_DEC_MAX_LAYERS] = {0};
};
struct DecoderState {
  bool on = false;
  int32_t D = 0, H = 0, dtype = SI_F64, last_act = 0;   // H: the last layer's `in` (M when D = 1)
  int32_t SH = 0;                // sum of the hidden widths: rows of `hid`
  DecoderHead head;
  DevBuf<char> params;           // the flat parameter vector (Nd elements of `dtype`)
  DevBuf<char> lastW, lastb;     // pad_ld(N) x H and pad_ld(N) elements of `dtype`
  DevBuf<double> hid;            // SH x hid_cap: every head layer's output per point (the reverse sweep's act')
  int64_t hid_cap = 0;
  DevBuf<double> y;              // pad_ld(N): decoder(z) at the gradient's point
  DevBuf<double> part, ga;       // the last layer's reverse: block partials (blocks x H), d lp / d a_{D-1} (H)
};

// The NeuralODE route (si_infer_setup_node; reference src/space_inference.jl:96-101): the set-up's layers are the right-hand
// side d -> ... -> d, setup.X holds the initial states (d x f), setup.Y the observed trajectories (d*S x f).  The kernel's arguments
// (kernels_node.hip), by value:
constexpr int SI_NODE_MAX_LAYERS = 8, SI_NODE_MAX_D = 8, SI_NODE_MAX_WIDTH = 256, SI_NODE_MAX_S = 4096, SI_NODE_MAX_STEPS = 1000000;
constexpr int64_t SI_NODE_MAX_N = 8192;
struct NodeLayers {
  int32_t n = 0;
  int32_t in[SI_NODE_MAX_LAYERS] = {0}, out[SI_NODE_MAX_LAYERS] = {0}, act[SI_NODE_MAX_LAYERS] = {0};
  int32_t w_off[SI_NODE_MAX_LAYERS] = {0}, b_off[SI_NODE_MAX_LAYERS] = {0};
};
struct NodeArgs {
  NodeLayers lay;
  const double* w = nullptr;       // chain slot c: w + c * ldw
  int64_t ldw = 0;
  const double* U0 = nullptr;      // d x f
  const double* Y = nullptr;       // d*S x f, or null (no squared errors: sse_p = 0 for a finished trajectory)
  const double* ts = nullptr;      // S
  double* sse_p = nullptr;         // f x nchains
  double* U_out = nullptr;         // d*S x f x nchains in Y's layout, or null
  int32_t *nacc = nullptr, *nrej = nullptr, *status = nullptr;   // f x nchains each, or null
  int64_t f = 0;
  int32_t d = 0, S = 0, N = 0, G = 1, lgG = 0, maxw = 1;
  double t0 = 0.0, reltol = 0.0, abstol = 0.0, dt = 0.0;
  int32_t adaptive = 1, max_steps = 0, pre_power = 1;
  // the gradient through the solver (si_node_set_grad): the forward with record writes (t_n, hs_n, u_n) of accepted step n of
  // trajectory tr at rec + (tr * max_steps + n) * (d + 2); the reverse kernel reads them, with nacc / status, and adds into the
  // trajectory's own slice gsl + tr * N
  double* rec = nullptr;
  double* gsl = nullptr;
};
struct NodeState {
  bool on = false;
  NodeArgs args;                   // everything but the per-call pointers (w, U0, Y, the outputs, f)
  int32_t d = 0, S = 0;
  DevBuf<double> ts;               // S
  DevBuf<double> ssep;             // f x slots: the per-trajectory sums of one pass of launches
  DevBuf<double> uout;             // d*S x f x slots: the saved states, only on request (si_forward)
  // si_node_set_grad(1): the value-and-gradient route's workspace for g_cap chains per pass of launches (capi_node.hip)
  bool grad = false;
  int g_fit = 0, g_cap = 0;        // chains per pass the budget allows / the workspace holds
  DevBuf<double> g_z, g_w, g_ssep, g_sse, g_wsq, g_wsqpart, g_rec, g_slices, g_gw, g_lp, g_gz;
  DevBuf<int32_t> g_cnt;           // nacc, nrej, status: f x g_cap each
};
hipError_t launch_node_solve(hipStream_t st, const NodeArgs& a, int nchains);   // (a.rec set: the forward with record)
void launch_node_sum(hipStream_t st, const double* sse_p, int64_t f, double* sse, int nchains);
hipError_t launch_node_grad(hipStream_t st, const NodeArgs& a, int nchains);    // the reverse kernel: a.rec, a.nacc, a.status -> a.gsl
// gw[:, c] = the chain's f slices added in ascending p from 0.0; lp[c] from the chain's sums as the host forms it
void launch_node_grad_sum(hipStream_t st, const double* gsl, int64_t f, int64_t N, double* gw, int64_t ldg, const double* sse,
                          const double* wsq, double* lp, int nchains);
// the validation si_infer_setup_node and si_train_setup_node share: the layers, the save times and the options -> the constant
// part of the kernel's arguments; nullptr, or the limit that refuses the set-up
const char* node_plan(const si_layer* layers, int32_t L, int64_t N, int32_t d, int32_t S, const double* ts, const si_node_opts* opts,
                      NodeArgs& a);

// si_train_setup_node (capi_train.hip; node.py: train_value_and_grad is the definition): the training step's own solver workspace
// for batch_max trajectories of ONE weight vector -- the inference state's (NodeState) is not shared, the launchers are
struct NodeTrain {
  NodeArgs args;                   // the constants (node_plan); per step: w = TrainOpt::w64, U0 / Y = the batch's columns, f = nb
  DevBuf<double> ts;               // S
  DevBuf<double> ssep;             // batch_max
  DevBuf<double> rec;              // batch_max x max_steps x (d + 2): the step record
  DevBuf<double> slices;           // batch_max x N: the per-trajectory gradient slices
  DevBuf<int32_t> cnt;             // nacc, nrej, status: batch_max each
  DevBuf<double> wsq, wsqpart;     // ||W||^2 and its block partials
  int wsq_blocks = 0;
  DevBuf<int64_t> fail;            // the sticky failure record: [0] the 1-based step that failed first (0: none), [1] trajectory, [2] status
  double penalty_div = 0.0;        // 0: no penalty
  int64_t steps = 0;               // steps queued so far (a step's number is steps + 1)
  int64_t checked = 0;             // the failure record has been read back after this many steps ...
  bool reported = false;           // ... and a failure found in it has been returned to the caller (once)
};
// node_train_tail_kernel (kernels_node_train.hip): the batch's slices -> gw (with the penalty), the loss word, and with `apply`
// the optimiser update and the refreshed Float64 copy of the weights; a failed trajectory or a set failure record stores nothing
// but the record
struct NodeTailArgs {
  const double* slices; const double* ssep; const double* wsq; const int32_t* status;
  int64_t nb, N, step;
  double penalty_div;
  float *w32, *m32, *v32;
  double *w64, *gw, *loss;
  int64_t* fail;
  int kind;
  double eta, p1, p2, bp1, bp2;
};
void launch_node_train_tail(hipStream_t st, const NodeTailArgs& a, bool apply);

// ---- on-device training (capi_train.hip).  One step -- batch, gradient, update -- with four gradient routes, chosen at set-up
// A cost other than mse at the seam of the three training routes (kernels_cost.hip; si_train_set_cost): it produces the loss's
// numerator (into the route's loss word, behind the forward pass's SSE) and Delta_L in place of launch_delta_out*
struct CostTail {
  int kind;           // SI_COST_MAE .. SI_COST_LOGITBCE
  double param;       // Huber's delta
  double inv_denom;   // 1 / (out * nb_total), SI_COST_LOGITCE: 1 / nb_total
  double* part;       // workgroup partials of the numerator (SI_COST_MAX_BLOCKS doubles)
};
// batch indices travel through two pinned buffers (copy in, async H2D, event): a step never synchronises the stream, so the
// caller's work between two steps (its next batch, the K1 push) overlaps the GPU's
struct TrainBatch {
  DevBuf<int64_t> idx;
  PinBuf<int64_t> pin[2];
  Event ev[2];
  bool busy[2] = {false, false};
  int slot = 0;
};
// Flux 0.11.2's Float32 parameters and optimiser state (optimiser_update.h), the Float64 copy the sweeps read, the gradient
struct TrainOpt {
  DevBuf<float> w32, m32, v32;
  DevBuf<double> w64, gw;
  int kind = 0;             // 0 Descent, 1 Momentum, 2 ADAM
  double eta = 0.0, p1 = 0.0, p2 = 0.0, bp1 = 0.0, bp2 = 0.0;
  bool grad_ready = false;  // gw holds a gradient that has not been applied yet
};
struct TrainState {
  TrainRoute route = TrainRoute::DenseF64;
  ChainModel model;                  // (Node: layers, N, in_dim = d, out_dim = d*S alone; X = U0 (d x f), Y = the trajectories (d*S x f))
  int64_t Btot = 0, Bmax = 0;
  DevBuf<double> X, Y, Xb, Yb;       // the data and the gathered batch (DenseF32: X is X32)
  // compute_dtype = SI_F32 (Dense chains; reference src/subspace_construction.jl:39-43 with a Float32 model AND Float32 data):
  DevBuf<float> X32, Xb32;           // fp32 data, activations, deltas, gradient; fp64 for the loss, the head's partials, the batch sums
  DevBuf<double> ssepart, sse;       // the loss word and its block partials
  int sse_blocks = 0;
  int cost = 0;                      // SI_COST_* (si_train_set_cost; every set-up starts with mse)
  double cost_param = 0.0;
  DevBuf<double> costpart;           // workgroup partials of a cost other than mse
  TrainBatch batch;
  TrainOpt opt;
  DevBuf<double> part;               // [model.part_slots()][out_last][Bmax] partial head products
  DevBuf<double> Xc, wpack;          // Conv route (net_value_and_grad, capi_net.hip): X re-laid channel-fastest, the packed weights
  SweepWs sweep;                     // the Chain routes' reverse-sweep workspace for Bmax observations; what a route does not use stays empty
  NodeTrain node;
};
double train_denominator(const TrainState* t, int64_t nb);   // (capi_train.hip) what the cost's numerator of nb observations is divided by

// ---- inference state (reference src/space_inference.jl:88-95,111-116,125): what free_infer drops, grouped by the entry points
// that allocate and use each part; a group that grows on demand carries its own capacity counter.  Every fact about the set-up -- its
// chain, its shapes and the sizes derived from them, the tile program's ranges, the step-wise session -- lives in here: zero or empty after
// free_infer.  InferSetup: the set-up's data, the chain (ChainModel) and the shapes, written by infer_setup_common (sigma_p: si_infer_set_prior), read by everything
struct InferSetup {
  bool ready = false;
  ChainModel model;
  int32_t M = 0;                  // columns of P
  int64_t ldP = 0, B = 0;         // pitch of P; observations
  double sigma_m = 1.0;
  int64_t act_elems = 0;          // pad_ld(model.max_stored * B): slot stride of fw.act
  int sse_blocks = 0, wsq_blocks = 0;   // block partials of the SSE over out_dim * B and of ||w||^2 over N
  const double *swa = nullptr, *P = nullptr;   // device (P: ldP x M); borrowed (the construction's, the caller's) or the owned copies
  DevBuf<double> swa_own, P_own, X, Y;         // W_swa / P when set from host; the data
  double sigma_p = 0.0;           // > 0: the prior term the reference leaves dead is added (si_infer_set_prior; non-default)
  int lik = 0;                    // si_infer_set_likelihood: 0 gaussian, 1 categorical, 2 bernoulli (every set-up starts Gaussian)
  DevBuf<float> X32;              // (model.f32) X rounded once
  DevBuf<double> Xc;              // X re-laid channel-fastest (input_spatial)
  bool fused_ok = false;          // narrow Dense chain: the chain set up is of the fused class
};
// Forward workspace of eval_density for `slots` chain slots: alloc_forward (1 at set-up; grown by ensure_chains for multi-chain calls)
struct InferForward {
  int slots = 0;
  DevBuf<double> w, act[2];       // reconstructed weights, slots x pad_ld(N); ping-pong activations, slots x act_elems (maxwidth x B padded)
  DevBuf<double> ssepart, wsqpart;   // block partials of the SSE (slots x sse_blocks) and of ||w||^2 for the prior (slots x wsq_blocks)
  DevBuf<double> part, yhat;      // slots x [fuse slots][out_last][B] partial last-layer products; slots x out_dim x B, filled on request
  DevBuf<float> w32, act32[2];    // (f32) slots x pad_ld(N), slots x act_elems
  DevBuf<double> wpack;           // packed conv weights of the current evaluation (set-up; one chain at a time)
  DevBuf<float> wpack32;          // the same in fp32 (compute_dtype = SI_F32 on a Conv chain)
};
// Gradient workspace of si_logdensity_grad: ensure_grad allocates it whole on the first call (ws.ready), drop_grad drops it whole
struct InferGrad {
  SweepWs ws;                     // the reverse sweep's, for the set-up's B observations
  DevBuf<double> gw, ptgpart, gz; // gradient w.r.t. the weights, partials of P' g, gradient w.r.t. z (gw, gz: si_decode_vjp's too; ptgpart: capi_node.hip's)
  DevBuf<double> likpart;         // a categorical / Bernoulli likelihood: the CostTail's workgroup partials (SI_COST_MAX_BLOCKS doubles)
};
// si_logdensity_grad_batch and StackedVgrad, fused route (kernels_chain_grad.hip): vgrad_ensure allocates it for `cap` points per pass
struct InferStacked {
  int cls = -1;                   // -1: not looked at yet; 0: the chain is not of the fused class; 1 / 2: it is, with batch tiles of 16 * cls
  int cap = 0, last_fused = 0;    // (last_fused: si_grad_kernel_info)
  DevBuf<double> z, w, part, ssepart, gw, lp, gz;
};
// The step-wise sampler session (si_rwmh_begin .. si_rwmh_end): its sample arrays and scalars; open while Z is allocated
struct StepSession {
  DevBuf<double> Z, lp;           // M x itr x C, itr x C
  int64_t itr = 0, next = 0;
  double sigma_z = 0.0, d = 0.0;
  uint64_t seed = 0;
  int32_t chain0 = 0, C = 0;
  bool evaluated = false;
  bool open() const { return Z != nullptr; }
};
// Per-chain state of the density entry points and the RWMH samplers for `cap` chains (ensure_chains), the session, the kept sample arrays
struct InferChains {
  int32_t cap = 0;
  DevBuf<double> zcur, zprop, lpcur, sse;   // M x C twice, C twice
  DevBuf<double> wsq;             // ||W_swa + P z_c||^2 per chain, only with the prior on
  DevBuf<int64_t> nacc;           // C
  DevBuf<uint64_t> steps;         // C: transition counter of every chain (device-resident)
  StepSession session;
  DevBuf<double> outZ, outlp;     // sample / lp arrays of si_sample_*, kept (an allocation per call was 0.4 ms of 20 transitions)
};
// The narrow chain's one-launch kernels (capi_sample.hip; cgprog: infer_setup_common): the grid loop's buffers and those of the same
// kernels specialised to the chain's shapes at run time (chain_spec_rtc.cpp), for spec_chains chains
struct InferLoops {
  DevBuf<unsigned> gridsync;      // grid loop: one 128-byte counter line per chain + the status line (size() = 32 words per line)
  DevBuf<CgTileD> cgprog;         // the chain's tile program (chain_fused_program)
  int cg_start[5] = {0}, cg_count[5] = {0}, cg_chunks[5] = {0};   // ... and its five tile lists' ranges
  DevBuf<double> specw, specy;    // per chain: 4 weight vectors in fragment order ([parity][accepted, rejected]), 2 output vectors ([parity])
  DevBuf<int> specperm;           // natural weight index -> fragment order
  const void* specperm_for = nullptr;   // (the SpecKernels the permutation was generated by)
  int spec_chains = 0, spec_fo = 0, last_density_spec = 0, last_loop_spec = 0;   // last_*: si_chain_kernel_info, did the last call run them
};
// si_sample_mala (capi_mala.hip), on top of the chain state: the accept counts and the device-side gradient samples
struct InferMala {
  int cap = 0;
  DevBuf<int64_t> nacc;           // C
  DevBuf<double> outG;            // M x itr x C, kept between calls like outZ (si_sample_hmc and si_sample_nuts use it too)
  CallInfo info;                  // si_mala_kernel_info: what the last call took (likewise in the three groups below)
};
// si_sample_hmc (capi_hmc.hip, kernels_hmc.hip), on top of the chain state: the half-kicked momentum of the proposal, the metric
// with its Welford window, the per-chain scalars (HmcChain) and the device-side alpha / eps / Minv samples
struct InferHmc {
  int cap = 0;
  DevBuf<double> rh, minv, wmean, wm2;        // M x C each
  DevBuf<HmcChain> chain;                     // C
  DevBuf<int32_t> open;                       // 1: chains still searching / building (synced_round)
  DevBuf<double> outalpha, outeps, outMinv;   // (itr+1) x C twice, M x (itr+1) x C; kept between calls like outZ
  CallInfo info;
};
// si_sample_nuts (capi_nuts.hip, kernels_nuts.hip), on top of si_sample_hmc's state: both ends of the tree (z, r, g), the sum of its
// momenta, the candidate (z, g), the stack of sub-tree summaries, the per-chain scalars, the device-side samples and the leaf log
struct InferNuts {
  int cap = 0;
  DevBuf<double> zm, rm, gm, zq, rq, gq, rho, zc, gc, stack;   // M x C each; stack: 4 M x NUTS_MAX_DEPTH x C
  DevBuf<NutsChain> tree;                               // C
  DevBuf<int32_t> outdepth, outnleaf, outsel;           // (itr+1) x C each, kept between calls like outZ
  DevBuf<double> outleaf;                               // (3M+1) x leaf_cap x C, only when asked for
  CallInfo info;
};
// si_fit_advi (capi_advi.hip, kernels_advi.hip): theta = [mu; omega] of R runs, the optimiser's ring of squared gradients, the draws eta,
// their points, values and gradients, the traces (grown on demand, kept; every call ends synchronised, so none is in use when replaced)
struct InferAdvi {
  DevBuf<double> theta, ring;     // 2M x R, W x 2M x R (component fastest, then slot)
  DevBuf<double> eta, z, g, lp;   // M x S x R three times, S x R
  DevBuf<double> trace, pts;      // 2M x (T+1) x R, M x S x T x R: only when asked for, kept between calls
  CallInfo info;
};
// si_sample_ess (capi_ess.hip, kernels_ess.hip), on top of the RWMH samplers' state (InferChains: z, lp, the pending point and the
// density's sums): the ellipse's second point, the slice and the bracket, the per-chain counters, the open word of value_round and
// the device-side nev / theta samples.  Not in the reference.
struct EssState {
  int cap = 0;
  DevBuf<double> nu;                       // M x C
  DevBuf<double> logy, theta, lo, hi;      // C each
  DevBuf<int32_t> k, closed;               // C each
  DevBuf<int32_t> open;                    // 1: chains still shrinking (value_round)
  DevBuf<int32_t> outnev;                  // itr x C, kept between calls like outZ
  DevBuf<double> outtheta;                 // itr x C
  int32_t passes = 0;                      // si_ess_kernel_info: what the last call took (zero after a refused one)
  int64_t rounds = 0, evals = 0;
};
struct InferState {
  InferSetup setup;
  NodeState node;                 // on: the set-up is a NeuralODE's; the density integrates instead of evaluating a Chain
  DecoderState dec;               // set: every density entry point forms W_swa + decoder(z); the stored P is ignored
  InferForward fw;
  InferGrad grad;
  InferStacked vg;
  InferChains chains;
  InferLoops loop;
  ChainState chain_state;         // si_sample_mala / _hmc / _nuts (its own buffers: the per-point gradient path uses chains.zprop between two kernels)
  InferMala mala;
  InferHmc hmc;
  InferNuts nuts;
  InferAdvi advi;
  EssState ess;
};

struct Ctx : CtxCore, ConstructState, InferState {};

void free_train(Ctx* c);
void comm_release(Ctx* c);  // comm.hip: destroy the communicator (si_destroy / si_comm_destroy)
// capi.hip: make `c` hold a FINISHED construction of N rows and M columns without a deviation matrix (what a rank that
// receives (W_swa, P) from another rank ends up with).  adopt allocates zeroed W_swa / P; install takes ownership of the
// two device buffers (ld = pad_ld(N), padding rows zero).  Both drop whatever construction / bound inference was there.
int32_t construct_adopt(Ctx* c, int64_t N, int32_t M);
void construct_install(Ctx* c, int64_t N, int32_t M, double* w_swa, double* P);

// error helpers -------------------------------------------------------------------------------
int32_t fail(Ctx* c, int32_t code, const std::string& msg);
#define SI_HIP(c, expr)                                                                    \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return si::fail((c), SI_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

// Dynamic-LDS opt-in of a kernel (hipFuncAttributeMaxDynamicSharedMemorySize) is a per-DEVICE property of the loaded code
// object: a process may hold contexts on several GPUs, so the "already set" note is kept per device.
struct LdsOptIn {
  size_t done[64] = {0};
  void ensure(const void* kern, size_t lds) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (dev >= 0 && done[dev] >= lds) return;
    (void)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (dev >= 0) done[dev] = lds;
  }
};

// profiling scope: records an event pair around kernel launches of one class
struct ProfScope {
  Ctx* c;
  int cls;
  hipEvent_t a = nullptr, b = nullptr;
  ProfScope(Ctx* c, int cls, double flops, double bytes);
  ~ProfScope();
};

// ---- kernel launchers (kernels_*.hip) -------------------------------------------------------
// K1: s <- (n*s + w)/(n+1); acol <- w - s   (three rounded ops, no FMA; reference :46-47,51)
// (a_dtype: element type of the deviation matrix -- SI_F64, the reference's, or the opt-in SI_F32 storage; ldA in ELEMENTS)
void launch_swa_dev_push(hipStream_t st, const void* w, int32_t w_dtype, double* s, void* acol,
                         int64_t N, double n, int num_cu, int32_t a_dtype = SI_F64);
void launch_swa_dev_push_batch(hipStream_t st, const void* w, int32_t w_dtype, int64_t ld, double* s, void* A,
                               int64_t ldA, int64_t N, int count, const double* nvals_dev, int64_t slot0, int64_t kcap,
                               int num_cu, int32_t a_dtype = SI_F64);
// K2: G = A'A over columns [0,K) of A (ldA), rows [0,N); result K x K col-major symmetric in G
// returns bytes of partial workspace required (if Gpart == nullptr nothing is launched)
size_t launch_gram(hipStream_t st, const void* A, int64_t ldA, int64_t N, int64_t K, double* Gpart,
                   double* G, int num_cu, Ctx* prof, int32_t a_dtype = SI_F64);
// K3: P[:, m] = sum_k A[:, k] * V[k*Mpad + m], m < M;  Mpad = project_mpad(M) (V rows zero-padded)
int project_mpad(int M);
void launch_project(hipStream_t st, const void* A, int64_t ldA, int64_t N, int64_t K, const double* V,
                    int32_t M, int32_t Mpad, double* P, int64_t ldP, int num_cu, int32_t a_dtype = SI_F64);
// the same product on the matrix cores (kernels_bwd.hip gemm_f64_kernel); launch_project uses it for M > 32
void launch_project_mfma(hipStream_t st, const double* A, int64_t ldA, int64_t N, int64_t K, const double* V, int32_t M,
                         int32_t Mpad, double* P, int64_t ldP);
// K3 for wide subspaces as a slab stream (kernels_project.hip; K <= 128, else returns false)
bool launch_project_stream(hipStream_t st, const double* A, int64_t ldA, int64_t N, int64_t K, const double* V, int32_t M,
                           int32_t Mpad, double* P, int64_t ldP, int num_cu);
bool launch_project_stream_f32(hipStream_t st, const float* A, int64_t ldA, int64_t N, int64_t K, const double* V, int32_t M,
                               int32_t Mpad, double* P, int64_t ldP, int num_cu);   // the same for an fp32-stored A
// K4: w[c*ldw + r] = swa[r] + sum_m P[r + m*ldP] * Z[m + c*M]
void launch_reconstruct(hipStream_t st, const double* swa, const double* P, int64_t ldP, int64_t N,
                        int32_t M, const double* Z, int32_t C, double* w, int64_t ldw, int num_cu,
                        float* w32 = nullptr /* SI_F32: the same sums rounded once to fp32 */, int64_t ldw32 = 0);
// The decoder's kernels (kernels_decoder.hip); `dtype` is the parameters' element type (SI_F32 / SI_F64), every sum fp64.
// head forward: a_l = act(W_l a_{l-1} + b_l), l = 1 .. D-1, one workgroup per point; hid[:, p] keeps every a_l
void launch_decoder_head_fwd(hipStream_t st, const DecoderHead& hd, const void* params, int32_t dtype, const double* Z, int32_t M,
                             double* hid, int32_t SH, int32_t npoints);
// last layer forward, K4's access pattern: y = act(W_D a + b_D), w = swa + y for point c at w + c * ldw (w may be null) and y
// at y + c * ldy (y may be null); a of point c at A + c * lda
void launch_decoder_last_fwd(hipStream_t st, const double* swa, const void* Wd, int64_t ldD, const void* bd, int32_t dtype, int64_t N,
                             int32_t H, int32_t act, const double* A, int64_t lda, int32_t C, double* w, int64_t ldw, double* y,
                             int64_t ldy, int num_cu);
// last layer reverse: ga[h] = sum_r W_D[r, h] * g[r] * act'(y[r]) (launch_ptg's scheme; part: decoder_rev_blocks() x H)
int decoder_rev_blocks();
void launch_decoder_last_rev(hipStream_t st, const void* Wd, int64_t ldD, int32_t dtype, int64_t N, int32_t H, int32_t act,
                             const double* g, const double* y, double* part, double* ga);
// head reverse: ga -> gz through the transposed head layers, act' from hid; one workgroup per point
void launch_decoder_head_rev(hipStream_t st, const DecoderHead& hd, const void* params, int32_t dtype, const double* ga, int32_t H,
                             const double* hid, int32_t SH, double* gz, int32_t M, int32_t npoints);
// Chain batching of the forward pass: `n` chain slots run in ONE launch (grid.y = slot).  Strides, in elements, from
// one slot to the next: `w` of the reconstructed weight vectors (W, bias, Wlast all live in it), `hin` / `hout` of
// the layer's input / output activations (hin = 0 for the first layer: X is shared), `part` of the fused-tail partials.
struct ChainBatch {
  int n = 1;
  int64_t w = 0, hin = 0, hout = 0, part = 0;
  int64_t part_ld = 0;  // column pitch of the fused-tail partials, 0 = B: nothing sets it (kept: the kernels' SGPR counts move without it)
};
// K5: Hout[i + out*b] = act(sum_k W[i + out*k] * Hin[k + in*b] + bias[i])
void launch_dense_f64(hipStream_t st, const double* W, const double* bias, const double* Hin,
                      double* Hout, int32_t out, int32_t in, int64_t B, int32_t act, const ChainBatch& cb = ChainBatch());
// K5 fused tail: the layer in front of a narrow (out_last <= SI_FUSE_MAX_OUT) last layer does not store its output;
// it writes per-slot partial products with the last layer's weights, summed by launch_tail_sse (block partials of
// (y - yhat)^2 to `blockpart`, to be finished by sse_final via launch_sse_final)
constexpr int SI_FUSE_MAX_OUT = 4;
int dense_fused_slots(int32_t out);
void launch_dense_f64_fused(hipStream_t st, const double* W, const double* bias, const double* Hin, int32_t out,
                            int32_t in, int64_t B, int32_t act, const double* Wlast, int32_t out_last, double* part,
                            const ChainBatch& cb = ChainBatch(), double* Hkeep = nullptr /* also store the layer's output */);
// K5 for a wide layer with a short reduction (kernels_gemm_panel.hip: in <= 128, persistent workgroups that keep their X operands in
// registers, stream W through an LDS ring and let every store drain under the MFMAs of the next tiles); same bits as the big-tile
// kernel.  launch_dense_f64 routes single-chain layers to it by shape (dense_panel_applies).
bool dense_panel_applies(const double* W, int32_t out, int32_t in, int64_t B, int32_t act);
bool launch_dense_f64_panel(hipStream_t st, const double* W, const double* bias, const double* Hin, double* Hout, int32_t out,
                            int32_t in, int64_t B, int32_t act, int grid = 0);
// K5 for small layers (kernels_gemm_small.hip): one wave per (feature slot, 16 observations) tile, operands straight from global
// memory; same bits as the big-tile kernel.  launch_dense_f64 / _fused route to it by shape (dense_small_applies).
bool dense_small_applies(int32_t out, int32_t in, int64_t B, int nchains, int32_t bm);
void launch_dense_small_f64(hipStream_t st, const double* W, const double* bias, const double* Hin, double* Hout, int32_t out,
                            int32_t in, int64_t B, int32_t act, int32_t slot_feats, const ChainBatch& cb);
void launch_dense_small_f64_fused(hipStream_t st, const double* W, const double* bias, const double* Hin, int32_t out, int32_t in,
                                  int64_t B, int32_t act, int32_t slot_feats, int32_t nslots, const double* Wlast, int32_t out_last,
                                  double* part, const ChainBatch& cb, double* Hkeep);
// K5 in fp32 (kernels_gemm_f32.hip; compute_dtype = SI_F32): same operation and chain batching, fp32 operands / outputs on
// v_mfma_f32_32x32x2_f32; the fused head writes fp64 partials that launch_tail_sse sums as in the fp64 path
void launch_dense_f32(hipStream_t st, const float* W, const float* bias, const float* Hin, float* Hout, int32_t out, int32_t in,
                      int64_t B, int32_t act, const ChainBatch& cb = ChainBatch());
int dense_f32_fused_slots(int32_t out, int32_t in, bool aligned);
bool launch_dense_f32_dx(hipStream_t st, const float* Wt, const float* zero_bias, const float* Delta, float* Dout, int32_t out,
                         int32_t in, int64_t B, const float* Hprev, int32_t act_prev);
void launch_dense_f32_fused(hipStream_t st, const float* W, const float* bias, const float* Hin, int32_t out, int32_t in, int64_t B,
                            int32_t act, const float* Wlast, int32_t out_last, double* part, const ChainBatch& cb = ChainBatch(),
                            float* Hkeep = nullptr);
void launch_narrow_f32(hipStream_t st, const double* src, float* dst, int64_t n);
void launch_sse_f32(hipStream_t st, const float* yhat, const double* y, int64_t d, double* part, int nblocks, double* sse_out,
                    int nch = 1, int64_t yhat_stride = 0, double* yhat64 = nullptr, int64_t yhat64_stride = 0, bool with_final = true);
void launch_tail_sse(hipStream_t st, const double* part, int slots, int out_last, int64_t B, const double* bias_last,
                     int act_last, const double* Y, double* yhat, double* blockpart, int nblocks,
                     const ChainBatch& cb = ChainBatch());
// sse_out[ch] = sum of blockpart[ch*nblocks .. +nblocks) for ch < nch
void launch_sse_final(hipStream_t st, const double* blockpart, int nblocks, double* sse_out, int nch = 1);
// K5: sse = sum (y - yhat)^2 over d elements; deterministic two-stage
int sse_num_blocks(int64_t d, int num_cu);
// (nch chain slots: yhat advances by yhat_stride per slot, y is shared, part holds nch*nblocks partials)
// (with_final = false: the block partials stay in `part`; the fused sampler loop sums them inside its accept kernel)
void launch_sse(hipStream_t st, const double* yhat, const double* y, int64_t d, double* part,
                int nblocks, double* sse_out, int nch = 1, int64_t yhat_stride = 0, bool with_final = true);
// backward pass (kernels_bwd.hip): gradient of the log-density w.r.t. the flat weights and its pull-back P' g
void launch_backward_data(hipStream_t st, const double* W, const double* Delta, const double* Hprev, double* DeltaPrev,
                          int32_t out, int32_t in, int64_t B, int32_t act_prev);
// ---- Dense chains, host side (capi.hip): the one forward pass, the reverse sweep, and the two together -------------------------
// Forward pass of a Dense chain on `st`, T = double / float: the plain layers, then either the fused layer (the narrow head in
// its epilogue) + launch_tail_sse + launch_sse_final, or launch_sse / launch_sse_f32 on the last layer's output.  Returns the last
// plain layer's output (X when there is none): without a fused head these are the model outputs in T.
template <typename T>
struct DenseForward {
  const ChainModel* m;    // layers, fuse_tail, main_layer
  const T* w;             // flat weights in the compute type
  const double* w64;      // the same in fp64 (the head's bias is added in fp64; == w for T = double)
  const T* X;             // input of layer 0, in_0 x B, shared by the chain slots
  const double* Y;
  int64_t B;
  // where layer l writes: kept[l] (one buffer per layer, one chain; the fused layer stores its output there as well), or with
  // kept == nullptr pingpong[l & 1], chain slots cb.hout apart
  const DevBuf<T>* kept;
  T* pingpong[2];
  ChainBatch cb;          // slot count and strides (hin is the pass's own: 0 into layer 0, hout behind it)
  int slots;              // feature slots of the fused head
  double* part;           // its partial products, cb.part per chain slot
  double* yhat;           // fp64 model outputs or nullptr: written by launch_tail_sse / launch_sse_f32, chain slots out * B apart
  double* ssepart;
  int sse_blocks;
  double* sse;            // cb.n sums of squared errors
  bool defer_sse_final;   // the block partials stay in ssepart (the caller's next kernel sums them)
  bool count_main;        // m->main_layer's launch is also counted as SI_K_DENSE_MAIN (the head counts with its fused layer)
  bool traffic;           // profile: bytes of the SI_K_DENSE scopes and the SI_K_SSE scope (false: flops of SI_K_DENSE only)
};
template <typename T>
const T* dense_forward(Ctx* ctx, hipStream_t st, const DenseForward<T>& a);
// Reverse sweep through a Dense chain.  On entry delta[0] holds Delta_L (launch_delta_out) and gw is zeroed, both on `st`; on
// return every dW / db of the chain is in gw.
struct DenseSweep {
  const ChainModel* m;
  const double* w;          // flat fp64 weights
  const double* X;          // input of layer 0, in_0 x B
  const DevBuf<double>* hs;  // kept outputs of every layer
  double* delta[2];
  double* gw;
  double* rspart;
  double* bwpart;
  int64_t B;
};
int32_t dense_reverse_sweep(Ctx* ctx, hipStream_t st, const DenseSweep& s);
// Value and gradient in fp64, shared by si_logdensity_grad and the training step: dense_forward with every output kept in sw.hs,
// gw zeroed, Delta_L = scale * (y - yhat) * act_L'(yhat), dense_reverse_sweep; on return gw holds d (scale/2 * -SSE) / dw and
// *sse the sum of squared errors.
struct DenseValueGrad {
  DenseSweep sw;
  const double* Y;
  double* part;         // head partials [m->fuse_slots][out_last][B]
  double *ssepart, *sse;
  int sse_blocks;
  double scale;         // of Delta_L: -2 / d for the mse loss, 1 / sigma^2 for the log-density
  bool traffic;         // as DenseForward::traffic
  const CostTail* cost = nullptr;   // training with another cost: its tail in place of launch_delta_out (scale unused)
};
int32_t dense_value_and_grad_f64(Ctx* ctx, hipStream_t st, const DenseValueGrad& s);
// The same in fp32 (capi_train.hip; kernels_gemm_f32.hip + kernels_bwd_f32.hip): dense_forward<float> with every output kept, the
// SSE (fp64), Delta_L, the fp32 reverse sweep; on return gw32 holds the gradient rounded to fp32 and *sse the sum of squared
// errors.  Shared by the training step and si_logdensity_grad with compute_dtype = SI_F32.
struct DenseSweepF32 {
  const ChainModel* m;
  const float* w32;     // flat fp32 weights
  const double* w64;    // the same in fp64 (the head's bias is added in fp64)
  const float* X32;     // input of layer 0, in_0 x B
  const double* Y;
  SweepF32Ws* ws;
  double* part;         // head partials [m->fuse_slots32][out_last][B]
  double *ssepart, *sse;
  int sse_blocks;
  int64_t B;
  double scale;         // of Delta_L: -2 / d for the mse loss, 1 / sigma^2 for the log-density
  const CostTail* cost = nullptr;   // as DenseValueGrad::cost
};
int32_t dense_value_and_grad_f32(Ctx* ctx, hipStream_t st, const DenseSweepF32& s);
void launch_widen_f32_to_f64(hipStream_t st, const float* src, int64_t n, double* dst, int num_cu);
// dW[out x in] = Delta * Hprev' into dW, through `part` (backward_weight_part_elems doubles): split-K GEMM + fixed-order reduction;
// db != nullptr: db[out] = rowsum(Delta) as well (inside the GEMM where the LDS-DMA kernel runs, else by launch_rowsum)
size_t backward_weight_part_elems(int32_t out, int32_t in, int64_t B, int num_cu);
void launch_backward_weight(hipStream_t st, const double* Delta, const double* Hprev, double* part, int32_t out,
                            int32_t in, int64_t B, int num_cu, double* dW, double* db = nullptr);
void launch_split_reduce(hipStream_t st, const double* part, int nsplit, int64_t elems, double* dst);
void launch_delta_out(hipStream_t st, const double* Y, const double* Yhat, int64_t d, double scale, int act, double* delta);
// the tail of a cost other than mse (kernels_cost.hip): *loss = the cost's numerator over the out x B outputs, summed in a fixed
// order through c.part; delta = dL/dyhat .* act'(yhat).  yhat in fp64 (Yhat64) or fp32 (Yhat32), Delta in TD
constexpr int SI_COST_MAX_BLOCKS = 256;   // doubles in CostTail::part
template <class TD>
void launch_cost_tail(hipStream_t st, const CostTail& c, const double* Y, const double* Yhat64, const float* Yhat32, int32_t out, int64_t B,
                      int act, TD* delta, double* loss);
// the summed negative log-likelihood of a classifier's outputs (kernels_lik.hip; si_infer_set_likelihood), forward only: kind 1
// categorical, 2 Bernoulli on the fp64 outputs of nc chain slots (slot j at Yhat + j * yhat_stride) against Y (out x B), in ONE
// launch; `nparts` partials per slot into part (launch_sse's layout, unused ones zero), then launch_sse_final unless !with_final
void launch_lik(hipStream_t st, int kind, const double* Y, const double* Yhat, int64_t yhat_stride, int32_t out, int64_t B, double* part,
                int nparts, double* nll_out, int nc, bool with_final);
void launch_rowsum(hipStream_t st, const double* D, int32_t out, int64_t B, double* part, double* db);
// reverse sweep through a narrow last layer (out_last <= SI_FUSE_MAX_OUT) in one pass over its input H (F x B):
// DeltaPrev = (W' Delta) .* act_prev'(H), dW = Delta H', dbprev = rowsum(DeltaPrev); part: tail_bwd_part_elems doubles
size_t tail_bwd_part_elems(int32_t out_last, int32_t F);
void launch_tail_bwd(hipStream_t st, const double* W, const double* Delta, const double* H, int32_t out_last, int32_t F,
                     int64_t B, int32_t act_prev, double* DeltaPrev, double* part, double* dW, double* dbprev);
int rowsum_chunks();
// the reverse sweep in fp32 (kernels_bwd_f32.hip): compute_dtype = SI_F32 of the on-device training step
size_t backward_weight_f32_part_elems(int32_t out, int32_t in, int64_t B, int num_cu);
void launch_backward_weight_f32(hipStream_t st, const float* Delta, const float* Hprev, float* part, int32_t out, int32_t in, int64_t B,
                                int num_cu, float* dW);
void launch_transpose_f32(hipStream_t st, const float* W, int32_t out, int32_t in, float* Wt);
size_t rowsum_f32_part_elems(int max_rows);
void launch_mul_dact_rowsum_f32(hipStream_t st, const float* G, const float* H, int rows, int64_t B, int act, float* D, double* part,
                                float* db);   // D = G .* act'(H) (H == nullptr: G itself; D == nullptr: nothing stored), db = rowsum(D)
void launch_delta_out_f32(hipStream_t st, const double* Y, const double* Yhat64, const float* Yhat32, int64_t d, double scale, int act,
                          float* delta);
size_t tail_bwd_f32_part_elems(int32_t out_last, int32_t F);
void launch_tail_bwd_f32(hipStream_t st, const float* W, const float* Delta, const float* H, int32_t out_last, int32_t F, int64_t B,
                         int32_t act_prev, float* DeltaPrev, double* part, float* dW, float* dbprev);
void launch_ptg(hipStream_t st, const double* P, int64_t ldP, int64_t N, int M, const double* g, double* part, double* gz);
int ptg_blocks();
// ---- Conv / MaxPool / flatten (kernels_conv.hip; host side capi_net.hip) ---------------------------------------------
void launch_conv_pack(hipStream_t st, const double* w, const double* b, double* Wp, double* bp, int KW, int KH, int CIN, int COUT,
                      int CINp, int COUTp, int Kp);
void launch_conv_pack_t(hipStream_t st, const double* w, double* Wt, int KW, int KH, int CIN, int COUT, int CINp, int COUTp, int KpT);
void launch_conv_forward(hipStream_t st, const double* Wp, const double* bp, const double* In, double* Out, const ConvGeom& g,
                         int COUTp, int Kp, int64_t npos, int act);
void launch_conv_forward_pool2(hipStream_t st, const double* Wp, const double* bp, const double* In, double* Out, const ConvGeom& g,
                         int COUTp, int Kp, int64_t npos, int act);
void launch_conv_forward_pool2_idx(hipStream_t st, const double* Wp, const double* bp, const double* In, double* Out, uint8_t* Idx,
                                   const ConvGeom& g, int COUTp, int Kp, int64_t npos, int act);
void launch_pool2_bwd_idx(hipStream_t st, const double* G, const double* Hp, const uint8_t* Idx, double* D, int Cp, int W2, int H2,
                          int64_t B, int act, double* part, int nout, double* db);
void launch_conv_backward_data(hipStream_t st, const double* Wt, const double* Delta, double* dX, const ConvGeom& gT, int CINp,
                               int KpT, int64_t npos_in);
int conv_dw_max_splits(int COUTp, int Kp, int64_t npos, int num_cu);   // bound over every position count up to npos (scratch sizing)
int conv_dw_splits(int COUTp, int Kp, int64_t npos, int num_cu, int64_t* ksplit_out);
void launch_conv_backward_weight(hipStream_t st, const double* Delta, const double* In, double* part, const ConvGeom& g, int COUTp,
                                 int Kp, int64_t npos, int nsplit, int64_t ksplit);
void launch_conv_unpack_dw(hipStream_t st, const double* part, int nsplit, double* gw, int KW, int KH, int CIN, int COUT, int CINp,
                           int COUTp, int Kp);
void launch_whcn_to_cwhn(hipStream_t st, const double* X, double* Xc, int W, int H, int C, int Cp, int64_t B);
void launch_cwhn_to_whcn(hipStream_t st, const double* Xc, double* X, int W, int H, int C, int Cp, int64_t B);
void launch_maxpool(hipStream_t st, const double* In, double* Out, int Cp, int Wi, int Hi, int Wo, int Ho, int PW, int PH, int sw,
                    int sh, int64_t B);
void launch_maxpool_bwd(hipStream_t st, const double* In, const double* Out, const double* Gout, double* Gin, int Cp, int Wi, int Hi,
                        int Wo, int Ho, int PW, int PH, int sw, int sh, int64_t B);
void launch_mul_dact(hipStream_t st, const double* G, const double* H, int64_t n, int act, double* D);
size_t dact_rowsum_ws_elems(int max_rows);
void launch_act_inplace(hipStream_t st, double* H, int64_t n, int act);
// the same forward kernels on fp32 operands (kernels_conv.hip compiled a second time with -DSI_CONV_F32: v_mfma_f32_16x16x4_f32,
// the same stagers, LDS images and index maps) -- compute_dtype = SI_F32 on Conv chains
void launch_conv_pack(hipStream_t st, const float* w, const float* b, float* Wp, float* bp, int KW, int KH, int CIN, int COUT, int CINp,
                      int COUTp, int Kp);
void launch_conv_forward(hipStream_t st, const float* Wp, const float* bp, const float* In, float* Out, const ConvGeom& g, int COUTp,
                         int Kp, int64_t npos, int act);
void launch_conv_forward_pool2(hipStream_t st, const float* Wp, const float* bp, const float* In, float* Out, const ConvGeom& g,
                               int COUTp, int Kp, int64_t npos, int act);
void launch_whcn_to_cwhn(hipStream_t st, const float* X, float* Xc, int W, int H, int C, int Cp, int64_t B);
void launch_cwhn_to_whcn(hipStream_t st, const float* Xc, float* X, int W, int H, int C, int Cp, int64_t B);
void launch_maxpool(hipStream_t st, const float* In, float* Out, int Cp, int Wi, int Hi, int Wo, int Ho, int PW, int PH, int sw, int sh,
                    int64_t B);
void launch_act_inplace(hipStream_t st, float* H, int64_t n, int act);
void launch_dense_narrow(hipStream_t st, const float* W, const float* bias, const float* Hin, float* Hout, int out, int in, int64_t B,
                         int act);
bool dense_narrow_applies(int out, int in, int64_t B, int num_cu);
void launch_dense_narrow(hipStream_t st, const double* W, const double* bias, const double* Hin, double* Hout, int out, int in, int64_t B,
                         int act);
void launch_maxpool_bwd_dact_rowsum(hipStream_t st, const double* In, const double* Out, const double* Gout, double* D, int Cp, int Wi,
                                    int Hi, int Wo, int Ho, int PW, int PH, int sw, int sh, int64_t B, int act, double* part, int nout,
                                    double* db);
void launch_mul_dact_rowsum(hipStream_t st, const double* G, const double* H, int rows, int64_t ncols, int act, double* D, double* part,
                            int nout, double* db);
// capi_net.hip: validation + geometry of a layer table (Dense chains included), and the generic forward / reverse sweep
int32_t net_plan(Ctx* c, const char* who, const si_layer* layers, int L, int64_t N, int in_dim, int out_dim, NetPlan& out);
// xin: input in device layout (net_input re-lays a (features x B) matrix when the chain starts on images); outs[l] = where
// layer l writes (out_elems * B doubles each); wpack: plan.wpack_elems doubles
void net_input(Ctx* c, const NetPlan& p, const double* X, double* Xc, int64_t B);
// `outs[l]` receives layer l's output.  pingpong = true (density path: nothing but the last output is needed): `outs` holds TWO
// buffers used alternately per EXECUTED layer, a Conv directly followed by MaxPool((2, 2)) on even sizes runs as one fused
// kernel, and *final_out is the buffer that holds the last layer's output.
// pidx != nullptr (gradient mode, outs[l] per layer, T = double only): a Conv layer with net_grad_fused(p, l) runs fused with its
// MaxPool, writes outs[l + 1] and pidx[l] and leaves outs[l] untouched (it may be nullptr).
// T = float (compute_dtype = SI_F32): the pingpong pass on fp32 weights, input and activations.
template <typename T>
int32_t net_forward(Ctx* c, const NetPlan& p, const T* w, const T* xin, int64_t B, const DevBuf<T>* outs, T* wpack, bool pingpong = false,
                    T** final_out = nullptr, const DevBuf<uint8_t>* pidx = nullptr);
// Conv layer l directly followed by MaxPool((2, 2), stride 2) on even sizes, activation carried by the GEMM epilogue: in
// gradient mode the pair runs as one kernel that keeps a byte index instead of the un-pooled activation
bool net_grad_fused(const NetPlan& p, size_t l);
size_t net_pidx_bytes(const NetPlan& p, size_t l, int64_t B);
void net_scratch_sizes(const NetPlan& p, int64_t B, int num_cu, size_t* bwpart, size_t* rspart, size_t* wt, size_t* dbtmp);
// g0 holds d / d(output of the last layer) (out_feat x B) on entry; g0 / g1: max_elems * B doubles each; hs[l]: kept outputs
int32_t net_backward(Ctx* c, const NetPlan& p, const double* w, const double* xin, int64_t B, const DevBuf<double>* hs, double* g0,
                     double* g1, double* gw, const NetScratch& s);
// Value and gradient of such a chain on c->stream, shared by si_logdensity_grad and the training step: net_forward in gradient mode
// (outputs kept in hs, pool indices in scratch->pidx), the SSE, gw zeroed, Delta = scale * (y - yhat), net_backward.
struct NetValueGrad {
  const NetPlan* plan;
  const double *w, *xin, *Y;
  int64_t B;
  const DevBuf<double>* hs;
  double* wpack;
  double* ssepart;
  int sse_blocks;
  double* sse;
  double* delta[2];     // max_elems * B doubles each
  double* gw;
  const NetScratch* scratch;
  int64_t N;
  double scale;         // -2 / d for the mse loss, 1 / sigma^2 for the log-density
  double bwd_flops;     // what the caller reports for its SI_K_BACKWARD scope
  const CostTail* cost = nullptr;   // as DenseValueGrad::cost
};
int32_t net_value_and_grad(Ctx* c, const NetValueGrad& s);
// K6, device-resident loop (kernels_chain.hip): all `itr` transitions of `nchains` small Dense chains in ONE launch, one
// workgroup per chain, weights / data / activations in LDS; bit-identical to the launch-per-step loop of si_sample_rwmh
constexpr int SI_CHAIN_MAX_LAYERS = 8;
struct ChainLoopArgs {
  si_layer lay[SI_CHAIN_MAX_LAYERS];
  const double *swa, *P, *X, *Y;
  double *Z_out, *lp_out;
  int64_t* nacc_out;
  int64_t ldP, itr;
  uint64_t seed;
  double sigma_z, c0, sigma2;
  int N, M, B, L, chain_id0;
  int slot_feats, fuse_slots, nblocks;   // head slots of layer L-2 (BM / WM of dense_f64_kernel's choice), SSE virtual blocks
  int p_in_lds;
  int o_X, o_Y, o_act0, o_act1, o_part, o_blk, o_z, o_red, o_P, o_swa, o_map;
  int wp[SI_CHAIN_MAX_LAYERS], bp[SI_CHAIN_MAX_LAYERS];   // padded W / bias image of every layer (chain_loop_plan)
  long long* dbg_stamps;   // tools/chain_bench.hip (-DSI_CHAIN_STAMPS) only; nullptr in the library   // LDS offsets (doubles), set by chain_loop_plan
};
size_t chain_loop_plan(ChainLoopArgs& a, size_t lds_limit);   // LDS bytes, 0 = the model does not fit / does not apply
void launch_chain_loop(hipStream_t st, const ChainLoopArgs& a, int nchains, size_t lds);
// K5 fused over all layers + K6 as a persistent grid loop for narrow Dense chains (kernels_chain_grid.hip)
struct ChainFusedPlan {
  si_layer lay[SI_CHAIN_MAX_LAYERS];
  int L, B;
  int fuse_tail, slot_feats, fuse_slots;   // narrow head on the image of layer L-2 (slots of dense_f64_kernel<FUSE>)
  int ld[SI_CHAIN_MAX_LAYERS + 1];         // pitch of the input image of layer l; ld[l + 1] = of its output image
  int o_x, o_buf[2], o_part;               // LDS offsets (doubles)
  int lds_doubles;
  const CgTileD* prog;                     // device: the tile lists (0: a wave owns the batch tile; 1 .. 4: wave 0 .. 3 of a workgroup that shares it)
  int prog_start[5], prog_count[5], prog_chunks[5];
};
void chain_fused_program(const si_layer* layers, int L, bool fuse_tail, std::vector<CgTileD>& prog, int start[5], int count[5],
                         int chunks[5]);
size_t chain_fused_plan(ChainFusedPlan& p, const si_layer* layers, int L, int64_t B, int NB, bool fuse_tail, int slot_feats,
                        int fuse_slots);   // LDS bytes for batch tiles of 16 NB observations; 0 = not a chain of this class
// yhat[chain][o + out_last * b] for `nchains` weight vectors w + chain * w_stride (grid.y), every layer in one launch
// (wave_tiles: one WAVE per batch tile, four regions of `lds` bytes per workgroup, no workgroup barrier; else one workgroup per tile)
void launch_chain_fused(hipStream_t st, const ChainFusedPlan& p, int NB, bool wave_tiles, size_t lds, const double* w, int64_t w_stride,
                        const double* X, double* yhat, int64_t y_stride, int nchains);
struct ChainGridArgs {
  ChainFusedPlan p;
  const double *swa, *P, *X, *Y;
  double *wbuf, *ybuf;        // per chain: W_swa + P z' (w_stride apart) and the model outputs (y_stride apart); handed between workgroups
  int64_t w_stride, y_stride;
  unsigned* cnt;              // 32 words (one 128-byte line) per chain, zeroed before the launch
  unsigned* status;           // raised by a workgroup whose barrier wait timed out
  double *Z_out, *lp_out;
  int64_t* nacc_out;
  int64_t ldP, itr;
  uint64_t seed;
  double sigma_z, c0, sigma2;
  int N, M, G, chain_id0, nblocks;
  int y_in_lds, o_y, o_blk, o_z, o_red, o_flag;   // LDS offsets behind the images (chain_grid_plan)
};
size_t chain_grid_plan(ChainGridArgs& a, size_t lds_fused);
hipError_t launch_chain_grid(hipStream_t st, const ChainGridArgs& a, int NB, int nchains, size_t lds);
// value + gradient of a narrow Dense chain for many points in one launch + one reduction (kernels_chain_grad.hip)
struct ChainVgradPlan {
  si_layer lay[SI_CHAIN_MAX_LAYERS];
  int L, B;
  int ld[SI_CHAIN_MAX_LAYERS + 1];      // pitch of image l (the input of layer l; image L: the model outputs); Delta_l has ld[l + 1]
  int o_img[SI_CHAIN_MAX_LAYERS + 1];   // LDS offsets (doubles): every image is kept for the reverse sweep
  int o_delta[2], o_red;
  int lds_doubles;
};
size_t chain_vgrad_plan(ChainVgradPlan& p, const si_layer* layers, int L, int64_t B, int NB);   // LDS bytes; 0 = not of this class
// part: per (point, workgroup) a partial of grad_w, part_stride apart; ssepart: per (point, workgroup); npoints <= 65535
void launch_chain_vgrad(hipStream_t st, const ChainVgradPlan& p, int NB, size_t lds, const double* w, int64_t w_stride, const double* X,
                        const double* Y, double inv_s2, double* part, int64_t part_stride, double* ssepart, int npoints);
// per point: grad_w = the G partials in order (- w / sigma_p^2 with the prior on) into gw, gz = P' grad_w, lp
void launch_chain_vgrad_reduce(hipStream_t st, const double* part, int G, int64_t N, int64_t part_stride, const double* ssepart,
                               const double* w, int64_t w_stride, const double* P, int64_t ldP, int M, double sigma_p, double c0p,
                               double c0, double sigma2, double* gw, double* lp_out, double* gz_out, int npoints);
int dense_fused_slot_feats(int32_t out);   // features per head slot of the fused fp64 layer (kernels_gemm.hip: BM / WM)
// K6
// What the kernels of every sampler over stacked points share: C chains, one workgroup each.
struct ChainRun {
  double *z, *lp, *g, *zp;                             // state and proposal / pending point: M x C (lp: C)
  const double *lpp, *gp;                              // value and gradient at zp
  double *Z_out, *lp_out, *G_out;                      // the samples, `itr` (MALA) or itr + 1 (HMC, NUTS) columns per chain; G_out may be NULL
  int32_t M, chain_id0;
  int64_t itr;
  uint64_t seed;
  double sigma_z;
};
// kernels_mala.hip: zp = z + h g + sigma_z n_step for C chains (first: sigma_z n_0); transition `step` of C chains given the
// proposals' lpp / gp, sample `step` written to Z_out / lp_out / G_out, the next proposal formed
struct MalaRun : ChainRun {
  int64_t* nacc;                                       // C
  double h;                                            // sigma_z^2 / 2, formed on the host, once
};
void launch_mala_propose(hipStream_t st, const MalaRun& a, int32_t C, uint64_t step, bool first);
void launch_mala_accept(hipStream_t st, const MalaRun& a, int32_t C, uint64_t step, bool propose_next);
// kernels_hmc.hip (the transition, the adaptor update and the step-size search are defined in its header comment).  HmcRun: what
// its kernels and kernels_nuts.hip's share.
struct HmcRun : ChainRun {
  double *rh, *minv, *wmean, *wm2;                     // M x C
  HmcChain* chain;                                     // C
  double *alpha_out, *eps_out, *Minv_out;              // (itr+1) x C twice, M x (itr+1) x C or NULL
  double delta;
};
void launch_hmc_init(hipStream_t st, const HmcRun& a, int32_t C);   // zp = sigma_z n_0, the search's state machine at its start
// one round of the step-size search given (lpp, gp) at the last trial point; open: the chains still searching are counted into it
void launch_hmc_search(hipStream_t st, const HmcRun& a, int32_t C, int32_t* open);
void launch_hmc_propose(hipStream_t st, const HmcRun& a, int32_t C, uint64_t step);
// transition `step` given (lpp, gp) at zp, column `step` of the outputs, the adaptor update the flags name, the proposal of step + 1
void launch_hmc_accept(hipStream_t st, const HmcRun& a, int32_t C, uint64_t step, bool adapting, bool in_window, bool window_close,
                       bool last_adapt, bool propose_next);
// kernels_nuts.hip (the transition is defined in its header comment): what its three kernels share on top of HmcRun
struct NutsRun {
  double *zm, *rm, *gm, *zq, *rq, *gq, *rho, *zc, *gc;   // M x C each: the tree's minus / plus end, its momentum sum, the candidate
  double* stack;                                         // 4 M x NUTS_MAX_DEPTH x C: per entry r of its first leaf, rho, z and g of its proposal
  NutsChain* tree;                                       // C
  int32_t *depth_out, *nleaf_out, *sel_out;              // (itr+1) x C each
  double* leaf_out;                                      // (3M+1) x leaf_cap x C or NULL
  int64_t leaf_cap;
  int32_t max_depth;
  double max_dh;
};
// transition `step` begins: momentum, H, the tree reset, the first direction, the first pending point in HmcRun::zp; first: the call's first
void launch_nuts_begin(hipStream_t st, const HmcRun& a, const NutsRun& n, int32_t C, uint64_t step, bool first);
// one round given (lpp, gp) at the pending points: the leaf, its merges, the end of a doubling, the next pending point; the chains
// still building are counted into open
void launch_nuts_leaf(hipStream_t st, const HmcRun& a, const NutsRun& n, int32_t C, uint64_t step, int32_t* open);
// transition `step` ends: the candidate becomes the state, column `step` of the outputs, the adaptor update the flags name
void launch_nuts_end(hipStream_t st, const HmcRun& a, const NutsRun& n, int32_t C, uint64_t step, bool adapting, bool in_window,
                     bool window_close, bool last_adapt);
// the window schedule of the Stan adaptor for n_adapts steps (host only): first and last step inside a window, the steps that close one
int32_t hmc_windows(int64_t n_adapts, int64_t* window_start, int64_t* window_end, int64_t* splits, int32_t cap);
// kernels_advi.hip (the step is defined in its header comment): R runs, one workgroup each.  AdviRun: what both kernels share.
struct AdviRun {
  double *theta, *ring, *eta, *z;       // 2M x R, W x 2M x R, M x S x R, M x S x R
  double *trace_out, *pts_out;          // 2M x (T+1) x R, M x S x T x R, or NULL
  int32_t M, S, W, chain_id0;
  int64_t T;
  uint64_t seed;
};
// first: theta_0, the cleared ring and the points of step 0;  final: the D draws from theta as it stands
void launch_advi_draw(hipStream_t st, const AdviRun& a, int32_t R, double sigma_z, bool first, bool final, double* Z_out, int64_t D);
// step t given (lp, g) at its points: elbo_t, d, the ring, s, theta_{t+1}, the traces and (form_next) the points of step t + 1
void launch_advi_update(hipStream_t st, const AdviRun& a, int32_t R, const double* lp, const double* g, double eta_opt, double tau,
                        int64_t t, double* elbo_out, bool form_next);
// kernels_ess.hip (the transition is defined in its header comment): C chains, one workgroup each.  The state (z, lp) and the
// pending point zp are the RWMH samplers' buffers (chains.zcur, chains.lpcur, chains.zprop: what eval_density_all evaluates), the
// density's sums at zp are chains.sse / chains.wsq (wsq NULL: no prior term); the constants are rwmh_accept_kernel's
struct EssRun {
  double *z, *lp, *zp, *nu;                            // M x C (lp: C)
  const double *sse, *wsq;                             // C each
  double *logy, *theta, *lo, *hi;                      // C each: the slice's level, the pending angle, the bracket
  int32_t *k, *closed;                                 // C each: evaluations of the transition so far; the transition is decided
  double *Z_out, *lp_out, *theta_out;                  // M x itr x C, itr x C twice
  int32_t* nev_out;                                    // itr x C
  int32_t M, chain_id0, max_evals;
  int64_t itr;
  uint64_t seed;
  double sigma_z, c0, s2, c0p, sp2;
};
void launch_ess_init(hipStream_t st, const EssRun& a, int32_t C);                    // zp = sigma_z n_0
void launch_ess_begin(hipStream_t st, const EssRun& a, int32_t C, uint64_t step);    // nu, logy, the first angle and point of transition `step`
// one round given the sums at zp: keep / cap / shrink for every open chain; the chains that go on are counted into open
void launch_ess_round(hipStream_t st, const EssRun& a, int32_t C, uint64_t step, int32_t* open);
void launch_rwmh_init(hipStream_t st, double* zcur, double* lpcur, int64_t* nacc, uint64_t* steps, int32_t M, int32_t C);
void launch_rwmh_propose(hipStream_t st, const double* zcur, double* zprop, int32_t M, int32_t C,
                         double sigma_z, uint64_t seed, int32_t chain_id0, const uint64_t* steps);
// last stage of the SSE reduction + accept + the next transition's proposal in one launch (kernels_stream.hip rwmh_tail_kernel)
void launch_rwmh_tail(hipStream_t st, const double* ssepart, int nparts, double* sse, double* zcur, double* zprop, double* lpcur,
                      int64_t* nacc, int32_t M, int32_t C, double c0, double sigma2, double sigma_z, uint64_t seed, int32_t chain_id0,
                      uint64_t* steps, double* Z_out, double* lp_out, int64_t itr, int32_t* accflag, bool propose_next);
void launch_rwmh_accept(hipStream_t st, double* zcur, const double* zprop, double* lpcur,
                        const double* sse, int64_t* nacc, int32_t M, int32_t C, double c0,
                        double sigma2, uint64_t seed, int32_t chain_id0, uint64_t* steps,
                        double* Z_out, double* lp_out, int64_t itr, const double* wsq = nullptr, double c0p = 0.0,
                        double sigma_p2 = 1.0, int32_t* accflag = nullptr /* per chain: 1 = this step's proposal was kept */);
// current weights of every chain after a transition: dst[c] = flag[c] ? wprop[c] : prev[c]   (prev == nullptr: all kept)
void launch_weights_select(hipStream_t st, const int32_t* flag, const double* wprop, int64_t ldw, const double* prev, double* dst,
                           int64_t ldd, int64_t N, int32_t C, int num_cu);
void launch_prior_grad(hipStream_t st, double* g, const double* w, int64_t n, double inv_s2, int num_cu);
void launch_widen_f32(hipStream_t st, const float* src, double* dst, int64_t n, int num_cu);
void launch_transpose(hipStream_t st, const void* A, int32_t a_dtype, int64_t lda, int64_t N, int64_t K, double* At, int64_t ldt);
// kernels_diffmap.hip (the diffusion map of si_construct_finish_diffmap; the steps are defined in its header comment)
int dm_blocks(int64_t N);   // 64-row blocks of the pairwise matrix = rows of the row-sum partials
// mm (2 K, only with rescale), Xr (Kp x dm_blocks(N) * 64, zeroed by the caller) and s from the deviation matrix A
void launch_dm_rescale(hipStream_t st, const void* A, int32_t a_dtype, int64_t ldA, int64_t N, int K, int Kp, int rescale, double* mm,
                       double* Xr, double* s);
// Kmat (ldn x N, exactly symmetric) with part[b][i] = its row sums over column block b; *flag raised on a non-finite entry
void launch_dm_pairwise(hipStream_t st, const double* Xr, int Kp, const double* s, int64_t N, int kernel_sign, double eps, double* Kmat,
                        int64_t ldn, double* part, int* flag);
void launch_dm_sum_parts(hipStream_t st, const double* part, int64_t ldn, int64_t N, bool root, double* out);
// Kmat_ij /= (v_i v_j)^alpha with the new row-sum partials (with_sums), or Kmat_ij /= v_i v_j
void launch_dm_scale_rows(hipStream_t st, double* Kmat, int64_t ldn, int64_t N, const double* v, double alpha, bool with_sums, double* part);
void launch_dm_unit(hipStream_t st, const double* q, int64_t N, double* u1);
void launch_dm_deflate(hipStream_t st, double* V, int64_t ldv, int64_t N, int ncol, const double* u1);
void launch_dm_colnorm(hipStream_t st, const double* R, int64_t ldr, int64_t N, int ncol, double* out);
void launch_dm_finish(hipStream_t st, const double* U, int64_t ldu, int64_t N, int M, const double* u1, double* P, int64_t ldp);
// capi.hip: d_P for M columns (an inference bound to a P that is replaced is dropped)
int32_t construct_alloc_P(Ctx* c, int32_t M);

// host copy pool (host_copy.cpp): parallel memcpy between pageable caller arrays and pinned staging
void host_copy(void* dst, const void* src, size_t bytes);
int host_copy_threads();
void host_copy_set_share(int nproc);   // `nproc` processes of the library share this host (one per GPU): shrink the pool's share
int host_cpu_budget();                 // affinity mask capped by the cgroup CPU quota
double parse_cpu_max(const char* text);
int host_copy_plan(int budget, int nproc, const char* env);

// host symmetric eigensolver (eig.cpp): a is n x n symmetric col-major, overwritten by eigenvectors
// (columns), w gets eigenvalues ascending.  Returns 0 on success.
int sym_eig(int n, double* a, double* w);
// M largest eigenpairs without the full eigenvector matrix (eig.cpp); g is left intact; w_top descending, V n x m.
// Verified (residual, orthogonality); returns non-zero when the caller should use sym_eig instead.
int sym_eig_top(int n, const double* g, int m, double* w_top, double* V);
// scaled-criterion two-sided Jacobi for a PSD matrix (eig_dispatch.cpp): a destroyed; w DESCENDING; v eigenvectors
int jacobi_eig_psd(int n, double* a, double* w, double* v);

}  // namespace si

struct si_ctx : public si::Ctx {};
