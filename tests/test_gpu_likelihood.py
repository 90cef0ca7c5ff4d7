"""The categorical and Bernoulli likelihoods of the density on the device (si_infer_set_likelihood; csrc/kernels_lik.hip, the seam
in eval_density and the CostTail seed of logdensity_grad_point) against their definition, tests/likelihood_cases.py: forward through
the oracle, then minus costs.numerator; the gradient costs.dvalue pulled back through the oracle's reverse pass.

Tolerances are the project's own: fp64 lp rtol 1e-10 (rwmh_audit.LP_RTOL_F64), SI_F32 lp rtol 1e-5 (LP_RTOL_F32), fp64 gradient
rtol 1e-8 with atol 1e-10 max(1, |g|_inf) (tests/test_gpu_train_costs.py), SI_F32 gradient 2e-5 of its scale (tests/test_gpu_f32.py).

lp of the gradient call against si_logdensity: within the lp tolerance, NOT to the bit.  The Gaussian path has the bit property on
the Dense routes because both calls end in the same SSE kernels; here the value goes through lik_*_kernel and sse_final_kernel's
tree over sse_blocks partials, the gradient through the training step's cost tail (cost_*_kernel, cost_final_kernel's ascending
sum over its own block count): the per-column terms are the same bits, their order of summation is not.
"""
import numpy as np
import pytest

from subspaceinference_jl_amd import flux
from tests import decoder_cases as dc
from tests import likelihood_cases as lc
from tests import node_cases as nc
from tests import rwmh_audit as ra

pytestmark = pytest.mark.gpu

LP64, LP32 = ra.LP_RTOL_F64, ra.LP_RTOL_F32
G_RTOL, G_ATOL, G32 = 1e-8, 1e-10, 2e-5


@pytest.fixture
def ctx(gpu_ctx):
    """the session's context, handed back with the defaults every other module expects"""
    yield gpu_ctx
    gpu_ctx.set_chain_loop(1)
    try:
        gpu_ctx.rwmh_abort()
        gpu_ctx.infer_set_likelihood(lc.GAUSSIAN)
        gpu_ctx.set_decoder(None, None)
        gpu_ctx.set_prior(0.0)
    except Exception:   # (no set-up, or a NeuralODE's: nothing to put back)
        pass


def _setup(si, ctx, pb, f32=False, kind=None):
    ctx.infer_setup(pb.table, pb.n, pb.m, pb.w, pb.p, pb.x, pb.y, 0.8, compute_dtype=si._capi.SI_F32 if f32 else si._capi.SI_F64)
    assert ctx.infer_likelihood_info() == lc.GAUSSIAN          # every set-up starts Gaussian
    if pb.decoder is not None:
        ctx.set_decoder(*pb.decoder)
    ctx.set_prior(pb.prior)
    ctx.infer_set_likelihood(pb.kind if kind is None else kind)
    assert ctx.infer_likelihood_info() == (pb.kind if kind is None else kind)


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))))


def _grad_close(g, ref):
    return bool(np.allclose(g, ref, rtol=G_RTOL, atol=G_ATOL * max(1.0, float(np.max(np.abs(ref))))))


def _check_value(ctx, pb, rtol, tag):
    """si_logdensity at NPOINTS stacked points against the definition; the same points one by one give the same bits"""
    z = lc.points(pb, lc.NPOINTS)
    ref = np.array([pb.density(z[:, c]) for c in range(lc.NPOINTS)])
    lp = ctx.logdensity(z)
    print("%s: lp rel %.2e" % (tag, _rel(lp, ref)))
    assert np.all(np.isfinite(lp)) and _rel(lp, ref) <= rtol, (tag, lp, ref)
    one = np.array([ctx.logdensity(z[:, c:c + 1])[0] for c in range(lc.NPOINTS)])
    assert np.array_equal(one, lp), (tag, one, lp)
    assert not ctx.chain_kernel_info()[0]                       # the one-launch narrow-chain density steps aside
    return z, lp, ref


def _check_grad(ctx, pb, z, lp_value, lp_rtol, tag, f32=False):
    """si_logdensity_grad / _grad_batch against the definition's analytic gradient"""
    ref = [pb.density_grad(z[:, c]) for c in range(z.shape[1])]
    lp1, g1 = ctx.logdensity_grad(z[:, 0])
    lpb, gb = ctx.logdensity_grad_batch(z)
    assert ctx.grad_kernel_info() == 0                          # the fused stacked value-and-gradient steps aside
    assert lpb[0] == lp1 and np.array_equal(gb[:, 0], g1)       # the batch walks si_logdensity_grad's own path
    gref = np.stack([r[1] for r in ref], axis=1)
    scale = np.max(np.abs(gref), axis=0)
    bound = G32 * scale[None, :] if f32 else G_RTOL * np.abs(gref) + G_ATOL * np.maximum(1.0, scale)[None, :]
    print("%s: gradient lp rel %.2e, worst |g - g_ref| / bound %.2e" % (tag, _rel(lpb, [r[0] for r in ref]), np.max(np.abs(gb - gref) / bound)))
    for c in range(z.shape[1]):
        assert abs(lpb[c] - ref[c][0]) <= lp_rtol * abs(ref[c][0]), (tag, c, lpb[c], ref[c][0])
        assert abs(lpb[c] - lp_value[c]) <= lp_rtol * abs(lp_value[c]), (tag, c)     # (within the lp tolerance: the module's docstring)
        if f32:
            gerr = np.max(np.abs(gb[:, c] - ref[c][1])) / np.max(np.abs(ref[c][1]))
            assert gerr <= G32, (tag, c, gerr)
        else:
            assert _grad_close(gb[:, c], ref[c][1]), (tag, c, gb[:, c], ref[c][1])


VALUE_PARAMS = [(k, o, False) for k, o in lc.VALUE_CASES] + [(lc.CATEGORICAL, 3, True), (lc.CATEGORICAL, 10, True),
                                                              (lc.CATEGORICAL, 65, True), (lc.BERNOULLI, 3, True)]


# ---- value and gradient, Dense fp64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,out,soft", VALUE_PARAMS, ids=lambda v: str(v))
def test_value_and_gradient_against_the_definition(si, ctx, kind, out, soft):
    """Dense 4 -> 6 -> out at B in {1, 7, 37}: both output locations and slot strides (out <= 4: fw.yhat; above: the activation
    buffer), every seg of the column reduction, ragged column groups; soft labels whose columns do not sum to 1"""
    for b in lc.BATCHES:
        pb = lc.dense_problem(out, b, kind, soft=soft)
        if soft and kind == lc.CATEGORICAL:
            assert not np.allclose(np.sum(pb.y, axis=0), 1.0)
        _setup(si, ctx, pb)
        tag = "kind %d out %d B %d%s" % (kind, out, b, " soft" if soft else "")
        z, lp, _ = _check_value(ctx, pb, LP64, tag)
        for mode in (0, 2):                                     # the launch-per-layer density whatever the mode: the same bits
            ctx.set_chain_loop(mode)
            assert np.array_equal(ctx.logdensity(z), lp), (tag, mode)
        ctx.set_chain_loop(1)
        _check_grad(ctx, pb, z, lp, LP64, tag)
        # si_forward keeps returning the model outputs
        yhat = ctx.forward(z[:, 1])
        assert yhat.shape == (out, b) and abs(-lc.nll_from_outputs(kind, yhat, pb.y) - lp[1]) <= LP64 * abs(lp[1])


@pytest.mark.parametrize("out", lc.F32_DIMS)
def test_value_and_gradient_with_f32_compute(si, ctx, out):
    for b in (7, 37):
        pb = lc.dense_problem(out, b, lc.CATEGORICAL)
        _setup(si, ctx, pb, f32=True)
        z, lp, _ = _check_value(ctx, pb, LP32, "f32 out %d B %d" % (out, b))
        _check_grad(ctx, pb, z, lp, LP32, "f32 out %d B %d" % (out, b), f32=True)
    pb = lc.dense_problem(out, 7, lc.BERNOULLI)
    _setup(si, ctx, pb, f32=True)
    _check_value(ctx, pb, LP32, "f32 bernoulli out %d" % out)


@pytest.mark.parametrize("out", lc.F32_DIMS)
def test_bernoulli_gradient_with_f32_compute(si, ctx, out):
    for b in (7, 37):
        pb = lc.dense_problem(out, b, lc.BERNOULLI)
        _setup(si, ctx, pb, f32=True)
        z, lp, _ = _check_value(ctx, pb, LP32, "f32 bernoulli out %d B %d" % (out, b))
        _check_grad(ctx, pb, z, lp, LP32, "f32 bernoulli out %d B %d" % (out, b), f32=True)


def test_value_and_gradient_of_the_conv_chain(si, ctx):
    pb = lc.conv_problem(7)
    _setup(si, ctx, pb)
    z, lp, _ = _check_value(ctx, pb, LP64, "conv fp64")
    _check_grad(ctx, pb, z, lp, LP64, "conv fp64")
    _setup(si, ctx, pb, f32=True)
    _check_value(ctx, pb, LP32, "conv f32")
    with pytest.raises(si.SubspaceError, match="Dense chains only"):     # the existing refusal of SI_F32 gradients on Conv chains stays
        ctx.logdensity_grad(z[:, 0])
    assert np.all(np.isfinite(ctx.logdensity(z)))


def test_value_and_gradient_of_the_conv_chain_with_the_bernoulli_likelihood(si, ctx):
    pb = lc.conv_problem(7, kind=lc.BERNOULLI)
    assert set(np.unique(pb.y)) == {0.0, 1.0} and not np.all(np.sum(pb.y, axis=0) == 1.0)
    _setup(si, ctx, pb)
    z, lp, _ = _check_value(ctx, pb, LP64, "conv bernoulli fp64")
    _check_grad(ctx, pb, z, lp, LP64, "conv bernoulli fp64")
    _setup(si, ctx, pb, f32=True)
    _check_value(ctx, pb, LP32, "conv bernoulli f32")


# ---- loop branches by launch geometry (tests/likelihood_cases.py holds the arithmetic, tests/test_likelihood_cpu.py checks it) ---------
def _num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("kind", (lc.CATEGORICAL, lc.BERNOULLI))
def test_the_capped_grid_of_the_likelihood_kernels(si, ctx, kind):
    """Dense 4 -> 6 -> 10 at out B > 256 * 4 num_cu: the likelihood kernels' grid is sse_blocks = 4 num_cu workgroups, no longer one
    thread per element.  On 256 CUs B = 26300: lik_elem_kernel's grid-stride loop takes a second, ragged lap (856 of 263000
    elements), lik_logitce_kernel walks 6575 column groups on 4096 waves; the gradient's cost tail walks them on its own 1024.
    Every nll summand is non-negative, so the device's fixed-order sum and NumPy's pairwise sum of the definition agree far inside
    the lp tolerance at this size."""
    b = lc.capped_batch(_num_cu())
    assert lc.CAPPED_OUT * b > 256 * 4 * _num_cu()
    pb = lc.dense_problem(lc.CAPPED_OUT, b, kind)
    _setup(si, ctx, pb)
    tag = "capped grid kind %d B %d" % (kind, b)
    z, lp, _ = _check_value(ctx, pb, LP64, tag)
    _check_grad(ctx, pb, z, lp, LP64, tag)


@pytest.mark.parametrize("out,b,f32", [(o, b, False) for o, b in lc.COST_LAP_SHAPES] + [lc.COST_LAP_SHAPES[0] + (True,)], ids=lambda v: str(v))
def test_the_second_lap_of_the_cost_tail_through_the_likelihood_gradient(si, ctx, out, b, f32):
    """cost_logitce_kernel runs on at most 256 workgroups = 1024 waves: (33, 1100) gives seg 64 and 1100 column groups, (10, 4103)
    seg 16 and 1026 groups whose last holds three columns -- a ragged second lap of `grp += nwaves` in both, as <double, double> and
    with SI_F32 as <float, float>"""
    groups = lc.logitce_geometry(out, b)[1]
    assert 4 * lc.COST_MAX_BLOCKS < groups < 8 * lc.COST_MAX_BLOCKS
    pb = lc.dense_problem(out, b, lc.CATEGORICAL)
    _setup(si, ctx, pb, f32=f32)
    tag = "cost lap out %d B %d%s" % (out, b, " f32" if f32 else "")
    z, lp, _ = _check_value(ctx, pb, LP32 if f32 else LP64, tag)
    _check_grad(ctx, pb, z, lp, LP32 if f32 else LP64, tag, f32=f32)


@pytest.mark.parametrize("kind,out,head", lc.HEAD_CASES, ids=lambda v: str(v))
def test_value_and_gradient_with_a_head_activation(si, ctx, kind, out, head):
    """the last layer's activation enters the gradient through dact_full(yhat, act) in the cost tail: sigmoid on the fused narrow tail,
    tanh and softplus on the generic one, relu and tanh under the Bernoulli likelihood"""
    pb = lc.head_problem(kind, out, head)
    assert pb.table[-1][2] == head != lc.I
    _setup(si, ctx, pb)
    tag = "head kind %d out %d act %d" % (kind, out, head)
    z, lp, _ = _check_value(ctx, pb, LP64, tag)
    _check_grad(ctx, pb, z, lp, LP64, tag)


@pytest.mark.parametrize("out", (3, 10))
def test_value_and_gradient_with_a_decoder_and_with_the_prior(si, ctx, out):
    base = lc.dense_problem(out, 37, lc.CATEGORICAL)
    dec = dc.random_decoder((base.m, 4, base.n), (lc.T, lc.I), seed=40 + out, dtype=np.float64)
    for tag, pb in (("decoder", base.with_(decoder=dec)), ("prior", base.with_(prior=0.7)), ("decoder + prior", base.with_(decoder=dec, prior=0.7))):
        _setup(si, ctx, pb)
        z, lp, _ = _check_value(ctx, pb, LP64, "%s out %d" % (tag, out))
        _check_grad(ctx, pb, z, lp, LP64, "%s out %d" % (tag, out))
    pb = lc.dense_problem(3, 7, lc.BERNOULLI).with_(prior=0.7)
    _setup(si, ctx, pb)
    z, lp, _ = _check_value(ctx, pb, LP64, "bernoulli prior")
    _check_grad(ctx, pb, z, lp, LP64, "bernoulli prior")


# ---- exact cases ----------------------------------------------------------------------------------------------------------------------
def test_zero_weights_give_the_uniform_likelihood(si, ctx):
    z = np.asfortranarray(np.random.default_rng(0).standard_normal((3, 2)))
    for kind, outs in ((lc.CATEGORICAL, lc.CATEGORICAL_OUTS), (lc.BERNOULLI, lc.BERNOULLI_OUTS)):
        for out in outs:
            for b in lc.BATCHES:
                pb = lc.dense_problem(out, b, kind)
                zero = pb.with_(w=np.zeros(pb.n), p=np.zeros((pb.n, pb.m), order="F"))
                _setup(si, ctx, zero)
                want = -b * np.log(out) if kind == lc.CATEGORICAL else -out * b * np.log(2.0)
                lp = ctx.logdensity(z)
                assert np.allclose(lp, want, rtol=1e-14, atol=0.0), (kind, out, b, lp, want)


@pytest.mark.parametrize("kind,out", [(lc.CATEGORICAL, 3), (lc.CATEGORICAL, 10), (lc.CATEGORICAL, 65), (lc.BERNOULLI, 1), (lc.BERNOULLI, 10)],
                         ids=lambda v: str(v))
def test_a_last_layer_bias_of_800_stays_finite(si, ctx, kind, out):
    pb0 = lc.dense_problem(out, 7, kind)
    for sign in (1.0, -1.0):
        w = pb0.w.copy()
        w[pb0.table[-1][4]] = sign * 800.0                    # the first output's bias
        pb = pb0.with_(w=w)
        _setup(si, ctx, pb)
        z, lp, ref = _check_value(ctx, pb, LP64, "bias %+g kind %d out %d" % (sign * 800.0, kind, out))
        assert np.all(np.isfinite(lp)) and np.all(np.isfinite(ref))
        lpg, g = ctx.logdensity_grad(z[:, 0])
        assert np.isfinite(lpg) and np.all(np.isfinite(g)) and _grad_close(g, pb.density_grad(z[:, 0])[1])


# ---- RWMH ----------------------------------------------------------------------------------------------------------------------------
def _cached(density):
    memo = {}

    def f(z):
        k = np.ascontiguousarray(z, dtype=np.float64).tobytes()
        if k not in memo:
            memo[k] = density(z)
        return memo[k]
    return f


@pytest.mark.parametrize("nchains", (1, 3))
@pytest.mark.parametrize("case", lc.RWMH_CASES, ids=lambda c: c.name)
def test_every_transition_of_the_rwmh_samplers(si, ctx, case, nchains):
    """si_sample_rwmh and si_sample_rwmh_weights at set_chain_loop 0, 1 and 2, audited transition by transition with the definition as
    the density; the caps certified by tests/test_likelihood_cpu.py held as conditions; the three modes and both entry points give
    the same bits; no device-resident loop runs"""
    pb = lc.rwmh_problem(case)
    _setup(si, ctx, pb, f32=case.f32)
    density = _cached(pb.density)
    args = dict(seed=case.seed, chain_id0=case.chain_id0, nchains=nchains)
    out = {}
    for mode in case.modes:
        ctx.set_chain_loop(mode)
        out[mode, "sample"] = ctx.sample_rwmh(case.itr, case.sigma_z, **args)
        assert ctx.chain_kernel_info()[:2] == (False, False), (case.name, mode)
        out[mode, "weights"] = ctx.sample_rwmh_weights(case.itr, case.sigma_z, **args)
        assert ctx.chain_kernel_info()[:2] == (False, False), (case.name, mode)
    ctx.set_chain_loop(1)
    for (mode, how), res in out.items():
        z, lp, acc = res[:3]
        w = res[3] if how == "weights" else None
        rep = ra.audit(z, lp, acc, density, case.sigma_z, case.seed, case.chain_id0, case.lp_rtol, W=w,
                       reconstruct=(lambda v: ctx.reconstruct(v)[:, 0]) if w is not None else None)
        print("%s C %d mode %d %s: %s" % (case.name, nchains, mode, how, rep.line()))
        assert rep.steps == (case.itr - 1) * nchains
        ra.check_caps(rep, case.f32)
    first = out[case.modes[0], "sample"]
    for key, res in out.items():
        for a, b, what in zip(first, res[:3], ("Z", "lp", "acc")):
            assert np.array_equal(a, b), "%s: %s of %s differs from mode %d" % (case.name, what, key, case.modes[0])


@pytest.mark.parametrize("name", ("dense3", "dense10"))
def test_the_stepwise_session_gives_the_bits_of_sample_rwmh(si, ctx, name):
    case = lc.RWMH_BY_NAME[name]
    pb = lc.rwmh_problem(case)
    _setup(si, ctx, pb)
    ref = ctx.sample_rwmh(case.itr, case.sigma_z, seed=case.seed, chain_id0=case.chain_id0, nchains=case.nchains)
    with pytest.raises(si.SubspaceError) as e:                   # the data-sharded session is refused ...
        ctx.rwmh_begin(case.itr, case.sigma_z, case.seed, case.chain_id0, case.nchains, d_total=4 * pb.y.size)
    assert e.value.code == si._capi.SI_ERR_INVALID
    ctx.rwmh_begin(case.itr, case.sigma_z, case.seed, case.chain_id0, case.nchains)   # ... and leaves the context usable
    for _ in range(case.itr):
        ctx.rwmh_step_accept(ctx.rwmh_step_eval())
    z, lp, acc = ctx.rwmh_end()
    assert np.array_equal(z, ref[0]) and np.array_equal(lp, ref[1]) and np.array_equal(acc, ref[2])
    ctx.infer_set_likelihood(lc.GAUSSIAN)                         # with the Gaussian the sharded session opens as before
    ctx.rwmh_begin(3, case.sigma_z, case.seed, case.chain_id0, 1, d_total=4 * pb.y.size)
    ctx.rwmh_abort()


# ---- gradient samplers: the 3-class Dense chain ---------------------------------------------------------------------------------------
def _accepted(z, c):
    return [0] + [t for t in range(1, z.shape[1]) if not np.array_equal(z[:, t, c], z[:, t - 1, c])]


def test_mala_and_hmc_return_the_public_gradients_bits(si, ctx):
    pb = lc.dense_problem(3, 37, lc.CATEGORICAL)
    _setup(si, ctx, pb)
    z, lp, acc, g = ctx.sample_mala(30, 0.1, seed=5, chain_id0=1, nchains=2, grad=True)
    assert ctx.mala_kernel_info()[0] == 0
    zh, lph, _, _, gh = ctx.sample_hmc(20, 0.1, seed=6, chain_id0=1, nchains=2, grad=True)
    assert ctx.hmc_kernel_info()[0] == 0
    for tag, zz, ll, gg in (("mala", z, lp, g), ("hmc", zh, lph, gh)):
        assert np.all(np.isfinite(ll)) and np.all(np.isfinite(gg))
        moved = 0
        for c in range(2):
            keep = _accepted(zz, c)
            moved += len(keep) - 1
            lpb, gb = ctx.logdensity_grad_batch(np.asfortranarray(zz[:, keep, c]))
            assert ctx.grad_kernel_info() == 0
            assert np.array_equal(ll[keep, c], lpb) and np.array_equal(gg[:, keep, c], gb), (tag, c)
            ref = pb.density_grad(zz[:, keep[-1], c])
            assert abs(lpb[-1] - ref[0]) <= LP64 * abs(ref[0]) and _grad_close(gb[:, -1], ref[1]), (tag, c)
        assert moved >= 2, (tag, moved)                            # the chains moved: the property was checked at accepted states


def test_nuts_and_advi(si, ctx):
    pb = lc.dense_problem(3, 37, lc.CATEGORICAL)
    _setup(si, ctx, pb)
    z, lp = ctx.sample_nuts(12, 0.1, seed=7, chain_id0=1, nchains=2, tree=False)[:2]
    assert ctx.nuts_kernel_info()[0] == 0
    for c in range(2):
        ref = np.array([pb.density(z[:, t, c]) for t in range(z.shape[1])])
        assert np.all(np.isfinite(lp[:, c])) and _rel(lp[:, c], ref) <= LP64, c
        assert _rel(ctx.logdensity(np.asfortranarray(z[:, :, c])), lp[:, c]) <= LP64
    assert len({tuple(z[:, t, 0]) for t in range(z.shape[1])}) > 2   # the chain moved
    a = ctx.fit_advi(10, 0.3, 8, chain_id0=1)
    b = ctx.fit_advi(10, 0.3, 8, chain_id0=1)
    assert ctx.advi_kernel_info()[0] == 0
    for u, v in zip(a, b):
        assert np.all(np.isfinite(u)) and np.array_equal(u, v)


# ---- the default is untouched -----------------------------------------------------------------------------------------------------------
def test_a_detour_leaves_the_gaussian_bits(si, ctx):
    """docs/src/nn_example.md's chain (the specialised grid loop's class): a categorical detour, then si_infer_set_likelihood(0),
    gives the lp, gradient and 40-step RWMH trace of a fresh set-up, and the loop and the fused gradient are taken again"""
    pb = ra._problem(ra.MODEL_B, 31, 0.8, 0.0)
    z = np.asfortranarray(np.random.default_rng(1).standard_normal((31, 3)))

    def setup():
        ctx.infer_setup(pb.table, pb.n, 31, pb.w, pb.p, pb.x, pb.y, 0.8)

    def calls():
        lp = ctx.logdensity(z)
        dens_spec = ctx.chain_kernel_info()[0]
        g = ctx.logdensity_grad_batch(z)
        fused = ctx.grad_kernel_info()
        tr = ctx.sample_rwmh(40, 0.05, seed=11, chain_id0=2, nchains=2)
        return (lp, g[0], g[1]) + tuple(tr), (dens_spec, fused, ctx.chain_kernel_info()[1])

    setup()
    fresh, info = calls()
    assert info[1:] == (1, True), info                          # the fused stacked gradient and the specialised grid loop
    setup()
    ctx.infer_set_likelihood(lc.CATEGORICAL)
    assert ctx.infer_likelihood_info() == lc.CATEGORICAL
    detour, dinfo = calls()
    assert dinfo == (False, 0, False), dinfo
    assert not np.array_equal(detour[0], fresh[0])
    ctx.infer_set_likelihood(lc.GAUSSIAN)
    back, binfo = calls()
    assert binfo == info
    for a, b in zip(fresh, back):
        assert np.array_equal(a, b)
    ctx.infer_set_likelihood(lc.BERNOULLI)
    setup()                                                       # a new set-up starts Gaussian
    assert ctx.infer_likelihood_info() == lc.GAUSSIAN
    assert np.array_equal(ctx.logdensity(z), fresh[0])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(si, ctx):
    inv, state = si._capi.SI_ERR_INVALID, si._capi.SI_ERR_STATE
    pb = lc.dense_problem(3, 7, lc.CATEGORICAL)
    z = lc.points(pb, 2)

    def refused(code, kind=lc.CATEGORICAL, c=None):
        with pytest.raises(si.SubspaceError, match="si_infer_set_likelihood") as e:
            (ctx if c is None else c).infer_set_likelihood(kind)
        assert e.value.code == code, (e.value.code, str(e.value))

    _setup(si, ctx, pb)
    lp = ctx.logdensity(z)
    for kind in (3, -1, 99):                                      # an unknown kind: nothing changes
        refused(inv, kind)
        assert ctx.infer_likelihood_info() == lc.CATEGORICAL and np.array_equal(ctx.logdensity(z), lp)
    ctx.rwmh_begin(4, 0.1, 1, 0, 1)                               # an open step-wise session
    refused(state, lc.BERNOULLI)
    refused(state, lc.GAUSSIAN)
    ctx.rwmh_abort()
    assert ctx.infer_likelihood_info() == lc.CATEGORICAL and np.array_equal(ctx.logdensity(z), lp)
    with si.Context(0) as fresh:                                  # before a set-up
        refused(state, c=fresh)
        assert fresh.infer_likelihood_info() == lc.GAUSSIAN
        _setup(si, fresh, pb)
        assert np.array_equal(fresh.logdensity(z), lp)
    case = nc.EXACT_CASES[0]                                      # a NeuralODE set-up
    npb = nc.problem(case)
    ctx.infer_setup_node([list(r) for r in npb.table], npb.n, case.m, npb.w_swa, npb.p, npb.u0, npb.y, npb.ts, **case.setup_kwargs())
    before = ctx.logdensity(npb.z)
    refused(inv)
    assert ctx.infer_likelihood_info() == lc.GAUSSIAN and np.array_equal(ctx.logdensity(npb.z), before)


# ---- the API ----------------------------------------------------------------------------------------------------------------------------
def test_sub_inference_and_auto_inference(si, ctx):
    rng = np.random.default_rng(3)
    model = flux.Chain(flux.Dense(4, 6, "tanh", rng=rng), flux.Dense(6, 3, rng=rng))
    b, m, itr = 21, 3, 25
    x = rng.standard_normal((4, b))
    y = lc.labels(lc.CATEGORICAL, 3, b, rng)
    data = flux.DataLoader(x, y, batchsize=b)
    table, n = flux.layer_table(model)
    w_swa, p = 0.3 * rng.standard_normal(n), np.asfortranarray(0.3 * rng.standard_normal((n, m)))
    pb = lc.Problem([list(r) for r in table], n, w_swa, p, np.asfortranarray(x), y, lc.CATEGORICAL)
    z, lp = si.sub_inference(model, data, w_swa, p, σ_z=0.3, itr=itr, M=m, alg="rwmh", ctx=ctx, seed=4, return_z=True,
                             likelihood="categorical")
    assert ctx.infer_likelihood_info() == lc.CATEGORICAL and z.shape == (m, itr)
    assert _rel(lp, [pb.density(z[:, t]) for t in range(itr)]) <= LP64
    assert len({tuple(z[:, t]) for t in range(itr)}) > 1
    chn, lpw = si.sub_inference(model, data, w_swa, p, σ_z=0.3, itr=itr, M=m, alg="rwmh", ctx=ctx, seed=4, likelihood="categorical")
    assert np.array_equal(lpw, lp) and np.allclose(chn[-1], w_swa + p @ z[:, -1], rtol=1e-13)
    zg, lpg = si.sub_inference(model, data, w_swa, p, σ_z=0.3, itr=itr, M=m, alg="rwmh", ctx=ctx, seed=4, return_z=True)
    assert ctx.infer_likelihood_info() == lc.GAUSSIAN and not np.array_equal(lpg, lp)      # the default changes nothing
    # Bernoulli through the same call
    yb = lc.labels(lc.BERNOULLI, 3, b, rng)
    zb, lpb = si.sub_inference(model, flux.DataLoader(x, yb, batchsize=b), w_swa, p, σ_z=0.3, itr=itr, M=m, ctx=ctx, seed=4, return_z=True,
                               likelihood="bernoulli")
    assert _rel(lpb, [pb.with_(y=yb, kind=lc.BERNOULLI).density(zb[:, t]) for t in range(itr)]) <= LP64
    # auto_inference: the density at W_swa + decoder(z)
    decoder = flux.Chain(flux.Dense(m, 4, "tanh", rng=rng), flux.Dense(4, n, rng=rng))
    dtable, _ = flux.layer_table(decoder)
    dpb = pb.with_(decoder=([list(r) for r in dtable], flux.extract_params(flux.params(decoder))))
    za, lpa = si.auto_inference(model, data, decoder, w_swa, σ_z=0.3, itr=itr, M=m, alg="rwmh", ctx=ctx, seed=4, return_z=True,
                                likelihood="categorical")
    assert _rel(lpa, [dpb.density(za[:, t]) for t in range(itr)]) <= LP64
