"""Host-side mirror of the reference's exported API for the hot path (src/SubspaceInference.jl:27-34):

    subspace_construction(model, cost, data, opt; T=10, c=1, M=3, print_freq=1)        -> (W_swa, P)      (Chain + flux.mse, or NeuralODE + flux.node_sse)
    diffusion_subspace(model, cost, data, opt; T=10, c=1, M=3, print_freq=1)           -> (W_swa, P)
    subspace_inference(model, cost, data, opt; σ_z, σ_m, σ_p, itr, T, c, M, ...)        -> (chn, lp, W_swa)
    sub_inference(in_model, data, W_swa, P; σ_z, σ_m, σ_p, itr, M, alg, backend)        -> (chn, lp)
    inference(...)  README-only alias of sub_inference (README.md:153-154); alg=:mh == :rwmh
    auto_encoder_subspace(model, cost, data, opt, encoder, decoder; T=10, c=1, M=3, print_freq=1)   -> (W_swa, decoder)
    auto_inference(m, data, decoder, W_swa; σ_z, σ_m, σ_p, itr, M, alg=:hmc, backend)               -> (chn, lp)
    autoencoder_inference(model, cost, data, opt, encoder, decoder; σ_z, ..., alg=:hmc, backend)    -> (chn, lp)

Same names, argument meaning, defaults and error behaviour (`throw(String)` -> SubspaceError) as the
reference.  Everything numerical goes through the C ABI (include/subspace_hip.h) to the HIP kernels; the
only host arithmetic here is the caller-side training step (flux.py, see its header).  Extra keyword
arguments (device, ctx, seed, max_cols, ...) are additions and default to the reference's behaviour.
Python identifiers may be Greek, so `σ_z=` works as in Julia; `sigma_z=` is accepted too.
"""
import numpy as np

from . import _capi, dist, flux, samplers
from ._capi import Context, SubspaceError

_RWMH_ALGS = ("rwmh", "mh")


def _get_ctx(ctx, device):
    return (ctx, False) if ctx is not None else (Context(device), True)


def _alg_name(alg):
    return str(alg).lstrip(":")


def subspace_construction(model, cost, data, opt, T=10, c=1, M=3, print_freq=1, *, device=0, ctx=None,
                          max_cols=0, verbose=True, keep_on_device=False, device_training="auto", init="zeros",
                          data_parallel=False, a_storage="f64", compute_dtype="auto"):
    """src/subspace_construction.jl:26-67.

    Per batch the host does `gradient` + `update!` (:39-43, caller side) and hands the flattened weights
    (`extract_params`, src/libs.jl:19-22, Float32) plus `n = i/c` to the device, which applies the SWA update,
    forms the deviation column and appends it (:45-52, kernel K1).  After the loop the device forms A'A
    (K2), the host solves the K x K eigenproblem (H1) and the device projects P = A*V_M (K3) == :61-65.

    device_training ("auto" | True | False): when the cost is `flux.mse` (or another cost flux.device_cost knows: flux.mae,
    flux.huber_loss, flux.logitcrossentropy, flux.logitbinarycrossentropy) and the optimiser is a fresh Descent /
    Momentum / ADAM, the training step itself (:39-43) also runs on the GPU (si_train_step: forward, reverse sweep,
    optimiser) and the weights are pushed in place (si_train_push) -- no weight vector crosses PCIe.  The model's
    arrays receive the trained weights at the end, like Flux's in-place `update!`.

    A `flux.NeuralODE` model (docs/src/node_example.md:272-285) trains with the cost `flux.node_sse` (the tutorial's L1: the sum of
    squared errors of the batch's trajectories plus ||W||^2 / 100) and `sensealg="discrete_adjoint"`: `data` holds the initial states
    (d x f) and the observed trajectories (d*S x f); the device step is si_train_setup_node (the forward with record, the reverse
    kernel and node_train_tail_kernel; node.train_value_and_grad is the definition), the host step (device_training=False, Float64
    parameters or a used optimiser) is that definition through flux.gradient / flux.update.  The gradient is the frozen-step discrete
    adjoint, not Zygote's through DiffEqFlux: the two agree to the order of the tolerances.  compute_dtype is "auto" or "f64" and
    data_parallel is not offered; a trajectory that fails (max_steps, a non-finite state) leaves the weights as they were and the
    call raises naming step, trajectory and status.  Any other cost on a NeuralODE raises, as before.

    init ("zeros" | "pretrained"): "zeros" is what the reference's CODE does (W_swa = zeros, :31 -- quirk Q1, the default);
    "pretrained" starts the running mean at the model's weights, as the reference's docs describe (nn_example.md:44).

    compute_dtype ("auto" | "f32" | "f64") of the DEVICE training step: "auto" is the reference's own arithmetic for the data
    handed in -- a Float32 model on Float32 (X, Y) is a Float32 Zygote pass (:39-43), Float64 data (every example of the
    reference: `rand(10, 100)`) promote the pass to Float64; "f32" / "f64" override (Float64 data are then rounded once /
    Float32 data widened).  The host step (device_training=False) follows NumPy's promotion, which is Julia's.

    a_storage ("f64" | "f32"): "f64" keeps the deviation matrix in Float64 like the reference (:33,51-52); "f32" (opt-in,
    SURVEY section 0 Q6) stores every column rounded once to Float32 -- half the memory and half the bytes of the Gram /
    projection kernels, P within 1e-5 of the Float64 result (tests/test_gpu_a32.py).

    data_parallel=True (opt-in; needs a ctx with an RCCL communicator -- one process per GPU, dist.comm_init -- or a torch
    process group) makes the device training step data-parallel: EVERY rank must make this call with the same model, data
    and DataLoader seed; each takes its share of every batch and the gradient is all-reduced once per step inside the
    library (si_train_step_dp), so all ranks return the same (W_swa, P).  The default keeps the step local whatever the
    ctx carries: the documented cfg3 flow (construct on rank 0, then si_bcast_subspace) must not find rank 0 alone inside a
    gradient all-reduce.
    """
    return _swa_construction(model, cost, data, opt, T, c, print_freq,
                             lambda cx: cx.construct_finish(M, want_swa=True, want_p=not keep_on_device)[:2],
                             device=device, ctx=ctx, max_cols=max_cols, verbose=verbose, keep_on_device=keep_on_device,
                             device_training=device_training, init=init, data_parallel=data_parallel, a_storage=a_storage,
                             compute_dtype=compute_dtype)


def diffusion_subspace(model, cost, data, opt, T=10, c=1, M=3, print_freq=1, *, eps=1.0, alpha=1.0, kernel_sign=-1, rescale=True,
                       tol=0.0, max_iters=0, device=0, ctx=None, verbose=True, keep_on_device=False, device_training="auto",
                       init="zeros", a_storage="f64", compute_dtype="auto"):
    """src/subspace_construction.jl:167-207: the SWA loop of `subspace_construction` (:181-200, the same lines), then
    `fit(DiffMap, A', maxoutdim = M); P = transform(diff_M)` (:202-206) instead of the SVD -> (W_swa, P), P being N x M.

    The diffusion map runs on the device (si_construct_finish_diffmap).  Its definition is `diffmap.diffmap_dense`, a restatement of
    ManifoldLearning 0.6.2  [upstream, from memory, unverifiable offline]: `eps` (kernel width, upstream's default 1), `alpha`
    (upstream's t = 1), `kernel_sign` (-1: the Gaussian kernel of upstream's docstring; +1: what its source is remembered to
    compute) and `rescale` (the per-snapshot unit-range transform) are the points a maintainer with Julia may have to change.
    `tol` / `max_iters` steer the block subspace iteration (0: 1e-12 / 500); a spectrum it cannot separate raises.
    The other keywords are `subspace_construction`'s (a ring of `max_cols` columns and a row-sharded / data-parallel
    construction are not offered on this route).  A NeuralODE with `flux.node_sse` trains as in `subspace_construction`."""
    return _swa_construction(model, cost, data, opt, T, c, print_freq,
                             lambda cx: cx.construct_finish_diffmap(M, eps, alpha, kernel_sign, rescale, tol, max_iters, want_swa=True,
                                                                    want_p=not keep_on_device)[:2],
                             device=device, ctx=ctx, max_cols=0, verbose=verbose, keep_on_device=keep_on_device,
                             device_training=device_training, init=init, data_parallel=False, a_storage=a_storage,
                             compute_dtype=compute_dtype)


def _refuse_node_training(model, cost):
    """A NeuralODE trains with `flux.node_sse` (a flux.NodeSSE) and `sensealg="discrete_adjoint"` alone; raised before any context
    is created."""
    if isinstance(model, flux.NeuralODE):
        if not isinstance(cost, flux.NodeSSE):
            raise SubspaceError("training a NeuralODE through the solver is out of scope: pass W_swa, P to sub_inference, or push "
                                "weight snapshots through the construction API (Context.construct_begin / construct_push / construct_finish)")
        if model.sensealg != "discrete_adjoint":
            raise SubspaceError("training a NeuralODE with flux.node_sse needs the gradient through the solver: construct the model "
                                "with sensealg=\"discrete_adjoint\"")
    elif isinstance(cost, flux.NodeSSE):
        raise SubspaceError("flux.node_sse is the cost of a flux.NeuralODE model (a Chain trains with flux.mse)")


def _swa_construction(model, cost, data, opt, T, c, print_freq, finish, *, device, ctx, max_cols, verbose, keep_on_device,
                      device_training, init, data_parallel, a_storage, compute_dtype):
    """What `subspace_construction` and `diffusion_subspace` share (reference :28-59 and :169-200, the same lines twice): training
    with the SWA update and the deviation columns on the device; `finish(ctx)` -> (W_swa, P) is what differs."""
    _refuse_node_training(model, cost)
    is_node = isinstance(model, flux.NeuralODE)
    ps = flux.params(model)
    n_par = int(sum(p.size for p in ps))
    nb = len(data)
    n_push = sum(1 for i in range(1, T + 1) if i % c == 0) * nb
    if n_push == 0:
        # reference: reshape of an empty A, then psvd / U[:,1:M] fails
        raise SubspaceError("BoundsError: no snapshot was collected (mod(i,c) never 0 for i in 1:T)")
    # the device step exists for a Chain with one of flux's costs (flux.device_cost: mse, mae, huber_loss, logitcrossentropy,
    # logitbinarycrossentropy) and for a NeuralODE with flux.node_sse (si_train_setup + si_train_set_cost / si_train_setup_node)
    dev_cost = isinstance(cost, flux.NodeSSE) if is_node else flux.device_cost(cost) is not None
    dev_opt = flux.device_optimiser(opt) if dev_cost and hasattr(data, "index_batches") else None
    # si_train_* keeps Float32 weights and optimiser state (Flux's default): a Float64 model stays on the host step,
    # otherwise "auto" and device_training=False would return different (W_swa, P) for the same inputs
    all_f32 = all(p.dtype == np.float32 for p in ps)
    if device_training is True and (dev_opt is None or not all_f32):
        raise SubspaceError("device_training needs cost = flux.mse, a fresh Descent / Momentum / ADAM optimiser and "
                            "Float32 parameters (the device step keeps Float32 weights and optimiser state)")
    use_dev = dev_opt is not None and all_f32 and device_training in ("auto", True)
    if is_node:
        if compute_dtype not in ("auto", "f64"):
            raise SubspaceError("a NeuralODE trains in Float64: compute_dtype must be \"auto\" or \"f64\"")
        if data_parallel:
            raise SubspaceError("data_parallel=True is not available for NeuralODE training")
    ctx, own = _get_ctx(ctx, device)
    try:
        ctx.construct_begin(n_par, n_push, max_cols)
        if a_storage not in ("f64", "f32"):
            raise SubspaceError("a_storage must be \"f64\" (the reference) or \"f32\"")
        if a_storage == "f32":
            ctx.construct_set_storage(_capi.SI_F32)
        if _alg_name(init) == "pretrained":
            ctx.construct_set_mean(flux.extract_params(ps))
        elif _alg_name(init) != "zeros":
            raise SubspaceError("init must be :zeros (the reference's behaviour) or :pretrained")
        training_loss = 0.0
        if data_parallel not in (True, False):
            raise SubspaceError("data_parallel must be True or False")
        if data_parallel and not use_dev:
            raise SubspaceError("data_parallel=True needs the device training step (cost = flux.mse, Float32 model, a fresh optimiser)")
        use_dp = use_dev and data_parallel is True
        dp_rank, dp_world = dist.world(ctx) if use_dp else (0, 1)
        if use_dev:
            xm, ym, in_size = flux.data_matrices(data)
            bmax = min(data.batchsize, data.nobs)
            if compute_dtype not in ("auto", "f32", "f64"):
                raise SubspaceError("compute_dtype must be \"auto\" (the data's element type, as in the reference), \"f32\" or \"f64\"")
            if is_node:
                table, _ = flux.layer_table(model.chain)
                ctx.train_setup_node(table, n_par, flux.extract_params(ps), xm, ym, model.saveat, bmax, *dev_opt, cost.penalty_div,
                                     **model.options())
            else:
                table, _ = flux.layer_table(model, in_size)
                ctx.train_setup(table, n_par, flux.extract_params(ps), xm, ym, bmax, *dev_opt,
                                compute_dtype={"auto": None, "f32": _capi.SI_F32, "f64": _capi.SI_F64}[compute_dtype])
                if not isinstance(cost, flux.MSE):   # (every set-up starts with mse)
                    ctx.train_set_cost(*flux.device_cost(cost))
        for i in range(1, T + 1):
            if use_dev:
                last = (i % print_freq == 0) or (i == T)
                batches = list(data.index_batches())
                for j, ids in enumerate(batches):
                    if use_dp and (dp_world > 1 or dist._has_comm(ctx)):
                        # data-parallel step: this rank's share of the batch, one gradient all-reduce (dist.py)
                        c0, c1 = dist.col_shard(len(ids), dp_rank, dp_world)
                        loss = dist.train_step_data_parallel(ctx, np.asarray(ids)[c0:c1], len(ids), flux.device_cost(cost)[0])
                    else:
                        loss = ctx.train_step(ids, want_loss=last and j == len(batches) - 1)
                    if loss is not None:
                        training_loss = loss
                    if i % c == 0:
                        ctx.train_push(i / c)
            else:
                for d in data:
                    training_loss, gs = flux.gradient(cost, model, *d)
                    flux.update(opt, ps, gs)
                    if i % c == 0:
                        ctx.construct_push(flux.extract_params(ps), i / c)
            if (i % print_freq == 0) or (i == T):
                if verbose:
                    print("Traing loss: ", training_loss, " Epoch: ", i)  # [sic] reference :57
        if use_dev:
            flux.load_flat(model, ctx.train_get_weights())
            flux.store_device_state(opt, model, *ctx.train_get_opt_state())  # opt continues where the device left it
        return finish(ctx)
    finally:
        if own and not keep_on_device:
            ctx.close()


def sub_inference(in_model, data, W_swa, P, σ_z=1.0, σ_m=1.0, σ_p=1.0, itr=100, M=3, alg="rwmh",
                  backend="forwarddiff", *, sigma_z=None, sigma_m=None, sigma_p=None, device=0, ctx=None,
                  seed=0, chain_id=0, return_z=False, nchains=1, include_prior=False, compute_dtype="f64",
                  device_loop=False, device_sampler=False, device_nuts=False, likelihood="gaussian"):
    """src/space_inference.jl:82-164 for a Chain model and alg = :rwmh.

    A `flux.NeuralODE` model (reference :96-101; docs/src/node_example.md) is accepted for alg = :rwmh / :mh: `data` holds the initial
    states (d x f) and the observed trajectories (d*S x f), the density -sum_p ||sol_p - Y_p||^2 - ||W||^2 integrates every trajectory
    with Tsit5 on the device (si_infer_setup_node; node.py is the definition), and `nchains`, `return_z` and the output map work as
    for a Chain.  The gradient samplers (:mala / :hmc / :nuts / :advi, host loop or device) need the model's
    `sensealg="discrete_adjoint"` (si_node_set_grad: the discrete adjoint of the integration with its accepted steps frozen, DESIGN
    section 19); without it they raise: the gradient through the solver is not built.

    `density(z)` (:90-95: W_swa + P*z -> model_re -> forward over the FULL data -> Gaussian log-likelihood,
    prior term dead) and the RWMH loop (:111-116) run on the device; the output map (:125) materialises
    `W_swa + P*z` for every sample like the reference unless `return_z=True` (then chn is the M x itr matrix
    of subspace samples).  σ_p is accepted and unused, exactly as in the reference (quirk Q4), unless
    `include_prior=True` (non-default) asks for the term the reference's source writes after its `return`.

    `nchains > 1` (RWMH and :mala; not in the reference, which runs one chain per call) runs the independent chains
    chain_id .. chain_id+nchains-1 stacked in every launch of the forward pass (:mala: of the stacked value + gradient,
    si_logdensity_grad_batch, with the host logic of `samplers.mala_chains`): chn becomes a list over chains
    (or the M x itr x nchains array with return_z) and lp is itr x nchains.

    `compute_dtype="f32"` (non-default; SURVEY section 0 Q6: "forward fp64 with fp32 as a measured option") evaluates the
    density of a Dense chain on the fp32 matrix instruction: X rounded once, W_swa + P*z formed in fp64 and rounded once per
    transition, fp32 activations, head + sum of squared errors in fp64 (lp within 1e-5 of the fp64 value, tests/test_gpu_f32.py).
    The gradient samplers (:mala / :hmc / :nuts) keep the fp64 reverse sweep either way.

    `device_loop=True` (alg = :mala and :advi; non-default) runs the chains with their state on the device (si_sample_mala): the
    transition of `samplers.mala` on the library's Philox streams (seed, chain_id + c) instead of NumPy's PCG64, one host
    synchronisation per call instead of one round trip per transition.  The default keeps the host loop and its results.
    alg = :advi exists as the device loop only (si_fit_advi: the reference's ADVI(10, itr) fit and its `rand(q, itr)` on the Philox
    streams, one run per call): without the keyword it raises, as it always has; lp is zeros(itr), as in the reference (:136).

    `device_sampler=True` (alg = :hmc; non-default) runs the reference's one-step HMC with position, momentum, step size, metric
    and adaptor state on the device (si_sample_hmc): the transition, adaptor and step-size search of `samplers.hmc` on the Philox
    streams (seed, chain_id + c), n_adapts = round(itr / 2); the initial state is dropped, so itr samples and lp come back like
    the host path's.  It allows nchains > 1, with :mala's shapes.  The default :hmc stays `samplers.hmc` on PCG64, bit for bit.

    `device_nuts=True` (alg = :nuts; non-default) runs NUTS with its trajectory tree, step size, metric and adaptor state on the
    device (si_sample_nuts; `Context.sample_nuts` / `Context.nuts_kernel_info`): the transition of `samplers.nuts_iter` on the
    Philox streams (seed, chain_id + c), n_adapts = round(itr / 2), max_depth = 10, max_dh = 1000; the initial state is dropped.
    It allows nchains > 1, with :hmc's shapes.  The default :nuts stays `samplers.nuts` on PCG64, bit for bit.

    alg = "ess" (not in the reference; Murray, Adams, MacKay 2010, the sampler of Izmailov et al.'s subspace inference) is elliptical
    slice sampling of exp(density(z)) N(z; 0, σ_z² I) with the chain state on the device (si_sample_ess; `samplers.ess_iter` is the
    definition, on the Philox streams (seed, chain_id + c)).  σ_z is here the PRIOR's standard deviation on z, not a step size: the
    sampler has no proposal scale and never rejects.  lp is the density at every sample; the prior on z is not added.  It needs
    values only, so it always runs on the device and accepts nchains > 1 (with :mala's shapes), return_z, every likelihood,
    include_prior, compute_dtype="f32" (Conv included) and a NeuralODE with or without `sensealg`.  itr counts the initial state.

    `likelihood` (non-default; not in the reference): "gaussian" is the reference's density.  "categorical" and "bernoulli" sample a
    classifier under the likelihood its cost defines (si_infer_set_likelihood; costs.py is the definition): lp = -costs.numerator(
    LOGITCE | LOGITBCE, model outputs, Y), the outputs read as logits, soft labels kept as written, σ_m unused, the prior term of
    `include_prior` added as for the Gaussian.  Every algorithm works; the device-resident RWMH loops and the fused stacked
    gradient are not taken, the launch-per-step loop and the per-point gradient run.  A NeuralODE is refused.
    """
    return _inference(in_model, data, W_swa, P, None, σ_z, σ_m, σ_p, itr, M, alg, sigma_z=sigma_z, sigma_m=sigma_m, sigma_p=sigma_p,
                      device=device, ctx=ctx, seed=seed, chain_id=chain_id, return_z=return_z, nchains=nchains,
                      include_prior=include_prior, compute_dtype=compute_dtype, device_loop=device_loop,
                      device_sampler=device_sampler, device_nuts=device_nuts, likelihood=likelihood)


def _inference(in_model, data, W_swa, P, decoder, σ_z, σ_m, σ_p, itr, M, alg, *, sigma_z, sigma_m, sigma_p, device, ctx, seed, chain_id,
               return_z, nchains, include_prior, compute_dtype, device_loop, device_sampler, device_nuts, likelihood="gaussian"):
    """What `sub_inference` and `auto_inference` share (reference :82-164 and :238-318, the same sampler calls twice): `decoder` is
    None (the density at W_swa + P*z) or the decoder's (layer table, flat parameters), set on the context right after the
    inference set-up (the density, its gradient and the output map at W_swa + decoder(z))."""
    σ_z = σ_z if sigma_z is None else sigma_z
    σ_m = σ_m if sigma_m is None else sigma_m
    σ_p = σ_p if sigma_p is None else sigma_p
    a = _alg_name(alg)
    if a == "advi" and (not device_loop or nchains != 1):
        # (this build has no host ADVI loop for a default to fall back to: the fit exists as the device loop only, one run per call)
        raise SubspaceError("alg = :advi is available with device_loop=True and nchains = 1 only (si_fit_advi; DESIGN section 13)")
    if a not in _RWMH_ALGS and a not in ("mala", "hmc", "nuts", "advi", "ess"):
        raise SubspaceError("%s is not available" % a)  # reference :162
    is_node = isinstance(in_model, flux.NeuralODE)   # reference :96-101: the density integrates the model instead of evaluating it
    if not is_node and not isinstance(in_model, flux.Chain):
        raise SubspaceError("Error: density function is not avaliable for this model")  # [sic] reference :103
    x, y, in_size = flux.data_matrices(data)  # split_data, src/libs.jl:75-77 (full data, not the batches)
    if likelihood not in _capi.LIKELIHOODS:
        raise SubspaceError("likelihood must be \"gaussian\" (the reference's density), \"categorical\" or \"bernoulli\"")
    if likelihood != "gaussian" and is_node:
        raise SubspaceError("likelihood = \"%s\" is not available for NeuralODE models: their density is the sum of squared errors "
                            "of the trajectories" % likelihood)
    if is_node:
        if a not in _RWMH_ALGS and a != "ess" and in_model.sensealg is None:
            raise SubspaceError("alg = :%s needs the gradient of the density, and the gradient through the ODE solver is not built "
                                "for this model: a NeuralODE model is sampled with alg = :rwmh / :mh, or constructed with "
                                "sensealg=\"discrete_adjoint\"" % a)
        if include_prior or compute_dtype != "f64":
            raise SubspaceError("a NeuralODE's density carries -||W||^2 itself and is evaluated in Float64: include_prior and "
                                "compute_dtype = \"f32\" are not available")
        table, n_par = flux.layer_table(in_model.chain)
    else:
        table, n_par = flux.layer_table(in_model, in_size)
    if compute_dtype not in ("f64", "f32"):
        raise SubspaceError("compute_dtype must be \"f64\" (the reference's arithmetic) or \"f32\"")
    cdt = _capi.SI_F32 if compute_dtype == "f32" else _capi.SI_F64
    if likelihood != "gaussian":   # the labels are read element by element against the model's outputs
        out = int(table[-1][1]) if len(table[-1]) == 5 else None   # (a Chain that ends in a Dense layer; else the set-up checks)
        if np.ndim(y) != 2 or np.shape(y)[1] != np.shape(x)[1] or (out is not None and np.shape(y)[0] != out):
            raise SubspaceError("DimensionMismatch: likelihood = \"%s\" needs Y of the shape of the model's outputs (out x B), got %s"
                                % (likelihood, np.shape(y)))
    ctx, own = _get_ctx(ctx, device)
    def setup(w_swa, p):
        if is_node:   # σ_m and σ_p are accepted and unused, as in the reference (:96-101)
            ctx.infer_setup_node(table, n_par, M, w_swa, p, x, y, in_model.saveat, **in_model.options())
            if in_model.sensealg == "discrete_adjoint" and a not in _RWMH_ALGS and a != "ess":
                ctx.node_set_grad(True)
        else:
            ctx.infer_setup(table, n_par, M, w_swa, p, x, y, σ_m, compute_dtype=cdt)
    try:
        if W_swa is None:
            setup(None, None)
        else:
            W_swa = np.asarray(W_swa, dtype=np.float64)
            P = np.asarray(P, dtype=np.float64)
            if P.shape[1] != M:
                # reference: MvNormal(zeros(M), σ_z) proposal against an N x size(P,2) matrix -> DimensionMismatch in P*z
                raise SubspaceError("DimensionMismatch: P has %d columns but M = %d" % (P.shape[1], M))
            setup(W_swa, P)
        if decoder is not None:
            ctx.set_decoder(*decoder)
        # include_prior=True adds the term the reference leaves dead after its `return` (quirk Q4); default: as the reference
        if not is_node:
            ctx.set_prior(σ_p if include_prior else 0.0)
        if likelihood != "gaussian":   # (every set-up starts Gaussian)
            ctx.infer_set_likelihood(_capi.LIKELIHOODS[likelihood])
        if device_sampler and a != "hmc":
            raise SubspaceError("device_sampler=True is available for alg = :hmc only" + (
                " (alg = :%s runs on the device with device_loop=True)" % a if a in ("mala", "advi") else ""))
        if device_nuts and a != "nuts":
            raise SubspaceError("device_nuts=True is available for alg = :nuts only")
        if device_loop and a not in ("mala", "advi"):
            raise SubspaceError("device_loop=True is available for alg = :mala and :advi only")
        if nchains != 1 and a not in _RWMH_ALGS and a not in ("mala", "ess") and not (a == "hmc" and device_sampler) and not (
                a == "nuts" and device_nuts):
            raise SubspaceError("nchains > 1 is available for alg = :rwmh / :mh / :mala / :ess (and :hmc with device_sampler=True, "
                                ":nuts with device_nuts=True) only")
        if a in _RWMH_ALGS:
            if return_z:
                z, lp, _ = ctx.sample_rwmh(itr, σ_z, seed, chain_id, nchains)
                return (z, lp) if nchains > 1 else (z[:, :, 0], lp[:, 0])
            # :125 map(z -> W_swa + P*z.params, chm): the weight samples stream out of the device WHILE the chain runs
            # (si_sample_rwmh_weights: K4's own output, selected on accept; DMA + host copy hidden under the next transitions)
            _, lp, _, w = ctx.sample_rwmh_weights(itr, σ_z, seed, chain_id, nchains)
            if nchains > 1:
                return [[w[:, t, c] for t in range(itr)] for c in range(nchains)], lp
            return [w[:, t, 0] for t in range(itr)], lp[:, 0]
        else:
            # :mala (:117-120) / :hmc, :nuts (:139-160): the sampler logic is host control flow, every density + gradient
            # evaluation is the device reverse sweep (si_logdensity_grad) instead of M-wide ForwardDiff duals (:107)
            if a == "advi":
                # :126-138: vi(density, ADVI(10, itr), q, theta_0), then rand(q, itr); the reference returns zeros(itr) for lp
                _, z, _ = ctx.fit_advi(itr, σ_z, seed, chain_id0=chain_id)
                z, lp = z[:, :, 0], np.zeros(itr)
            elif a == "ess" or (a == "mala" and device_loop) or (a == "hmc" and device_sampler) or (a == "nuts" and device_nuts):
                if a == "ess":
                    # not in the reference: elliptical slice sampling under z ~ N(0, σ_z² I), always on the device (si_sample_ess)
                    z, lp = ctx.sample_ess(itr, σ_z, seed, chain_id, nchains)
                elif a == "nuts":
                    z, lp = (np.asfortranarray(v[..., 1:, :]) for v in ctx.sample_nuts(itr, σ_z, seed, chain_id, nchains, tree=False)[:2])
                elif a == "hmc":
                    # :139-160 with the state on the device; column 0 (the initial state) is not a sample of the reference's
                    z, lp = (np.asfortranarray(v[..., 1:, :]) for v in ctx.sample_hmc(itr, σ_z, seed, chain_id, nchains)[:2])
                else:
                    z, lp, _ = ctx.sample_mala(itr, σ_z, seed, chain_id, nchains)
                if nchains > 1:
                    if return_z:
                        return z, lp
                    return [[w[:, t] for t in range(itr)] for w in (ctx.reconstruct(z[:, :, c]) for c in range(nchains))], lp
                z, lp = z[:, :, 0], lp[:, 0]
            elif a == "mala" and nchains > 1:
                # the chains chain_id .. chain_id + nchains - 1 in lock-step: one stacked gradient call per transition
                # (si_logdensity_grad_batch); chain c is the single-chain run with chain_id + c
                rngs = [np.random.default_rng([int(seed), int(chain_id) + c]) for c in range(nchains)]
                z, lp, _ = samplers.mala_chains(ctx.logdensity_grad_batch, M, itr, σ_z, rngs)
                if return_z:
                    return z, lp
                return [[w[:, t] for t in range(itr)] for w in (ctx.reconstruct(z[:, :, c]) for c in range(nchains))], lp
            else:
                rng = np.random.default_rng([int(seed), int(chain_id)])
                fn = {"mala": samplers.mala, "hmc": samplers.hmc, "nuts": samplers.nuts}[a]
                z, lp, _ = fn(ctx.logdensity_grad, M, itr, σ_z, rng)
        if return_z:
            return z, lp
        w = ctx.reconstruct(z)  # :125  map(z -> W_swa + P*z.params, chm)
        return [w[:, t] for t in range(w.shape[1])], lp
    finally:
        if own:
            ctx.close()


def inference(*args, **kwargs):
    """README.md:153-154 name for `sub_inference`."""
    return sub_inference(*args, **kwargs)


def subspace_inference(model, cost, data, opt, σ_z=1.0, σ_m=1.0, σ_p=1.0, itr=1000, T=25, c=1, M=20,
                       print_freq=1, alg="rwmh", backend="forwarddiff", method="subspace", *, sigma_z=None,
                       sigma_m=None, sigma_p=None, device=0, ctx=None, seed=0, verbose=True, return_z=False,
                       compute_dtype="f64", device_loop=False, device_sampler=False, device_nuts=False, likelihood="gaussian"):
    """src/space_inference.jl:33-54: construction, then sampling; returns (chn, lp, W_swa).
    W_swa and P stay on the device between the two stages (no host round trip).  With a `flux.NeuralODE(...,
    sensealg="discrete_adjoint")` and `flux.node_sse` this is the NeuralODE tutorial's call (docs/src/node_example.md:285)."""
    _refuse_node_training(model, cost)
    m = _alg_name(method)
    if m not in ("subspace", "diffusion"):
        raise SubspaceError("Error: No method found")  # reference :42
    construct = subspace_construction if m == "subspace" else diffusion_subspace  # reference :37-40
    a = _alg_name(alg)
    if a in ("turing_mh", "turing_nuts"):
        raise SubspaceError("Turing samplers are outside the accelerated path (SURVEY section 2)")
    ctx, own = _get_ctx(ctx, device)
    try:
        w_swa, _ = construct(model, cost, data, opt, T=T, c=c, M=M, print_freq=print_freq, ctx=ctx, verbose=verbose,
                             keep_on_device=True)
        chn, lp = sub_inference(model, data, None, None, σ_z=σ_z, σ_m=σ_m, σ_p=σ_p, itr=itr, M=M, alg=alg,
                                backend=backend, sigma_z=sigma_z, sigma_m=sigma_m, ctx=ctx, seed=seed,
                                return_z=return_z, compute_dtype=compute_dtype, device_loop=device_loop,
                                device_sampler=device_sampler, device_nuts=device_nuts, likelihood=likelihood)
        return chn, lp, w_swa
    finally:
        if own:
            ctx.close()


def _decoder_spec(decoder):
    """(layer table, flat parameters in Flux.destructure order and the decoder's own element type) of a Dense-only decoder chain"""
    if not isinstance(decoder, flux.Chain) or not decoder.layers or not all(isinstance(l, flux.Dense) for l in decoder.layers):
        raise SubspaceError("Error: the decoder must be a Chain of Dense layers")
    table, _ = flux.layer_table(decoder)
    return table, flux.extract_params(flux.params(decoder))


def auto_encoder_subspace(model, cost, data, opt, encoder, decoder, T=10, c=1, M=3, print_freq=1, *, include_penalty=False,
                          seed=0, device=0, ctx=None, verbose=True, device_training="auto", init="zeros", a_storage="f64",
                          compute_dtype="auto", device_autoencoder=False):
    """src/subspace_construction.jl:93-143: the SWA loop of `subspace_construction` (:104-123, the same lines), then
    `Chain(encoder, decoder)` trained to reproduce the deviation columns -> (W_swa, decoder); the decoder's arrays are trained in
    place and the same object comes back, as in the reference.

    The loop runs on the device like the other two constructions; the deviation matrix A (N x K) and the mean are then read
    back (the mean through a one-column `construct_finish`, whose projection is discarded) and the autoencoder is trained on the
    host (the default; `device_autoencoder` below) with `flux.gradient` / `flux.update`: cost `mse(sae(X), X)`, a fresh `ADAM()`, `DataLoader(A, batchsize = 5, shuffle =
    true)`, ONE pass (:127-140).  [upstream, unverifiable offline]: that `Flux.train!` makes a single pass over its data and
    that `ADAM()` is ADAM(0.001, (0.9, 0.999)) are restated from Flux 0.11.2 from memory.  `M` is accepted and unused, as in the reference (the decoder's first layer carries it).

    device_autoencoder: False (default) is that host loop.  True trains the autoencoder on the device (si_ae_train_*;
    autoencoder.py: train_step is the definition): A is read in place, never read back; the shuffle stays the host DataLoader's
    permutation, passed step by step; the encoder's and decoder's arrays are written back at the end; a set-up the library refuses
    raises SubspaceError with its message.  "auto": the device when it accepts the set-up, else the host loop.  The device's
    gradient carries the unscaled cotangent and takes its three N-long sums in a blocked order, so the two routes agree to
    rounding, not to the bit.

    include_penalty: the reference writes `+ sum(sqnorm, autops)` on a line of its own AFTER the loss (:130-131), so Julia parses
    it as a separate statement and the penalty is dead -- like the prior term (quirk Q4).  False (default):
    as the reference's code behaves; True adds the term it meant.  `seed` seeds the shuffle of the autoencoder's loader.
    A NeuralODE with `flux.node_sse` trains as in `subspace_construction`."""
    _refuse_node_training(model, cost)
    if not isinstance(encoder, flux.Chain) or not all(isinstance(l, flux.Dense) for l in encoder.layers):
        raise SubspaceError("Error: the encoder must be a Chain of Dense layers")
    dec_table, _ = _decoder_spec(decoder)
    n_par = int(sum(p.size for p in flux.params(model)))
    if encoder.layers[0].W.shape[1] != n_par or int(dec_table[-1][1]) != n_par:
        raise SubspaceError("DimensionMismatch: the encoder takes %d inputs and the decoder returns %d values, but the model has %d "
                            "parameters" % (encoder.layers[0].W.shape[1], int(dec_table[-1][1]), n_par))
    if encoder.layers[-1].W.shape[0] != int(dec_table[0][0]):
        raise SubspaceError("DimensionMismatch: the encoder returns %d values but the decoder takes %d"
                            % (encoder.layers[-1].W.shape[0], int(dec_table[0][0])))

    if device_autoencoder not in (False, True, "auto"):
        raise SubspaceError("device_autoencoder must be False, True or \"auto\"")
    sae = flux.Chain(*encoder.layers, *decoder.layers)          # :127 Chain(encoder, decoder): the same arrays
    autops = flux.params(sae)

    def train_on_device(cx, k):
        """the loop of :134-140 through si_ae_train_*; False when "auto" met a refusal"""
        table, _ = flux.layer_table(sae)
        w0 = flux.extract_params(autops)
        aopt = flux.ADAM()
        try:
            if not 1 <= len(encoder.layers) <= 8 or not 1 <= len(decoder.layers) <= 8:
                raise SubspaceError("si_ae_train_setup: E or D outside 1 .. 8")
            cx.ae_train_setup(table, w0, None, n_par, 5, 2, aopt.eta, aopt.beta[0], aopt.beta[1], penalty=include_penalty)
        except SubspaceError:
            if device_autoencoder == "auto":
                return False
            raise
        try:
            loader = flux.DataLoader(np.zeros((1, k)), batchsize=5, shuffle=True, rng=np.random.default_rng(seed))   # :139
            for ids in loader.index_batches():                     # :140 Flux.train!: one pass
                cx.ae_train_step(ids, want_loss=False)
                if verbose:                                        # :137 cb() = @show autoloss(re_weight)
                    print("autoloss(re_weight) = ", cx.ae_train_loss())
            flux.load_flat(sae, cx.ae_train_get_params())
        finally:
            cx.ae_train_free()
        return True

    def finish(cx):
        nb = len(data)
        k = sum(1 for i in range(1, T + 1) if i % c == 0) * nb
        if device_autoencoder is not False and train_on_device(cx, k):
            return cx.construct_finish(1, want_swa=True, want_p=False)[0], None
        a = cx.construct_get_A(0, k)
        return cx.construct_finish(1, want_swa=True, want_p=False)[0], a

    w_swa, re_weight = _swa_construction(model, cost, data, opt, T, c, print_freq, finish, device=device, ctx=ctx, max_cols=0,
                                         verbose=verbose, keep_on_device=False, device_training=device_training, init=init,
                                         data_parallel=False, a_storage=a_storage, compute_dtype=compute_dtype)
    if re_weight is None:                                      # trained on the device
        return w_swa, decoder
    aopt = flux.ADAM()                                         # :134
    wdata = flux.DataLoader(re_weight, batchsize=5, shuffle=True, rng=np.random.default_rng(seed))   # :139
    for (xb,) in wdata:                                        # :140 Flux.train!: one pass
        loss, gs = flux.gradient(flux.mse, sae, xb, xb)
        if include_penalty:
            gs = [g + 2.0 * p.astype(np.float64) for g, p in zip(gs, autops)]
        flux.update(aopt, autops, gs)
        if verbose:                                            # :137 cb() = @show autoloss(re_weight)
            full = flux.mse(sae, re_weight, re_weight)
            if include_penalty:
                full += float(sum(np.sum(p.astype(np.float64) ** 2) for p in autops))
            print("autoloss(re_weight) = ", full)
    return w_swa, decoder


def auto_inference(m, data, decoder, W_swa, σ_z=1.0, σ_m=1.0, σ_p=1.0, itr=100, M=3, alg="hmc", backend="forwarddiff", *,
                   sigma_z=None, sigma_m=None, sigma_p=None, device=0, ctx=None, seed=0, chain_id=0, return_z=False, nchains=1,
                   include_prior=False, compute_dtype="f64", device_loop=False, device_sampler=False, device_nuts=False,
                   likelihood="gaussian"):
    """src/space_inference.jl:238-318 for a Chain model: `sub_inference` with the density at `W_swa + decoder(z)` (:247) and the
    output map `W_swa + decoder(z)` (:278,291,314) -> (chn, lp).  The default algorithm is :hmc, as in the reference.

    `decoder` is a Chain of Dense layers M -> ... -> N (Float32 or Float64 parameters: they stay on the device in their own
    element type, all sums are Float64).  The decoder's forward and the pull-back of the gradient through it run on the device
    (si_infer_set_decoder; autoencoder.py is the definition); every algorithm and keyword of `sub_inference` is accepted, with
    the same meaning, except compute_dtype="f32", which the decoder route refuses.  While a decoder is set the device-resident
    RWMH loops and the fused stacked gradient are not taken (they form W_swa + P*z themselves): the launch-per-step loop and the
    per-point gradient path run instead.  The inference set-up is given a zero N x M matrix for P -- 8 N M idle bytes on the
    device, the price of sharing the set-up with `sub_inference`."""
    if not isinstance(m, (flux.Chain, flux.NeuralODE)):
        raise SubspaceError("Error: density function is not avaliable for this model")  # [sic] as sub_inference (:103)
    spec = _decoder_spec(decoder)
    n_par = int(sum(p.size for p in flux.params(m)))
    if int(spec[0][0][0]) != M:
        raise SubspaceError("DimensionMismatch: the decoder takes %d inputs but M = %d" % (int(spec[0][0][0]), M))
    if int(spec[0][-1][1]) != n_par:
        raise SubspaceError("DimensionMismatch: the decoder returns %d values but the model has %d parameters"
                            % (int(spec[0][-1][1]), n_par))
    W_swa = np.asarray(W_swa, dtype=np.float64)
    if W_swa.shape != (n_par,):
        raise SubspaceError("DimensionMismatch: W_swa has shape %s but the model has %d parameters" % (W_swa.shape, n_par))
    return _inference(m, data, W_swa, np.zeros((n_par, M), order="F"), spec, σ_z, σ_m, σ_p, itr, M, alg, sigma_z=sigma_z,
                      sigma_m=sigma_m, sigma_p=sigma_p, device=device, ctx=ctx, seed=seed, chain_id=chain_id, return_z=return_z,
                      nchains=nchains, include_prior=include_prior, compute_dtype=compute_dtype, device_loop=device_loop,
                      device_sampler=device_sampler, device_nuts=device_nuts, likelihood=likelihood)


def autoencoder_inference(model, cost, data, opt, encoder, decoder, σ_z=1.0, σ_m=1.0, σ_p=1.0, itr=1000, T=25, c=1, M=20,
                          print_freq=1, alg="hmc", backend="forwarddiff", *, sigma_z=None, sigma_m=None, sigma_p=None, device=0,
                          ctx=None, seed=0, verbose=True, return_z=False, include_penalty=False, include_prior=False,
                          device_loop=False, device_sampler=False, device_nuts=False, device_autoencoder=False, likelihood="gaussian"):
    """src/space_inference.jl:198-210: `auto_encoder_subspace`, then `auto_inference`, on one context -> (chn, lp).  A NeuralODE
    with `flux.node_sse` trains as in `subspace_construction`.  device_autoencoder: as in `auto_encoder_subspace`."""
    _refuse_node_training(model, cost)
    ctx, own = _get_ctx(ctx, device)
    try:
        w_swa, decoder = auto_encoder_subspace(model, cost, data, opt, encoder, decoder, T=T, c=c, M=M, print_freq=print_freq,
                                               include_penalty=include_penalty, seed=seed, ctx=ctx, verbose=verbose,
                                               device_autoencoder=device_autoencoder)
        return auto_inference(model, data, decoder, w_swa, σ_z=σ_z, σ_m=σ_m, σ_p=σ_p, itr=itr, M=M, alg=alg, backend=backend,
                              sigma_z=sigma_z, sigma_m=sigma_m, sigma_p=sigma_p, ctx=ctx, seed=seed, return_z=return_z,
                              include_prior=include_prior, device_loop=device_loop, device_sampler=device_sampler,
                              device_nuts=device_nuts, likelihood=likelihood)
    finally:
        if own:
            ctx.close()
