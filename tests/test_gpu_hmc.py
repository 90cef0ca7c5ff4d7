"""si_sample_hmc: the reference's one-step HMC with position, momentum, step size, metric and adaptor state on the device
(csrc/capi_hmc.hip, kernels_hmc.hip).

Every case of tests/hmc_audit.py's list (certified on the oracle alone by tests/test_hmc_audit_cpu.py) runs on the device and its
trace is audited transition by transition and adaptor update by adaptor update: rejects are bit copies, accepts are within the
stated bound of z + eps (Minv (r + eps / 2 g)) formed from the trace's own state, lp and G are within the project's tolerances of the
fp64 oracle, every decision is u_t < alpha[t] exactly, alpha is the oracle's within the first-order effect of those tolerances, eps
and Minv follow the replayed adaptor within their derived bounds and are frozen after n_adapts, eps[0] is the replayed search's
bit for bit.  The conditions hold on the device as on the oracle.

Then what the audit cannot see: the route taken, lp and G equal to the public gradient's bits at every kept state, column 0 equal
to si_sample_mala's, independence of a chain's bits from nchains / column / run / pass, the optional outputs, the state rules, and the
opt-in keyword of sub_inference."""
import numpy as np
import pytest

from oracle import subspace_oracle as so
from tests import hmc_audit as ha
from tests.test_gpu_chain_grid import NN_EXAMPLE

pytestmark = pytest.mark.gpu


def _setup(si, ctx, case):
    pb = ha.problem(case)
    ctx.infer_setup(pb.table, pb.n, case.m, pb.w, pb.p, pb.x, pb.y, case.sigma_m,
                    compute_dtype=si._capi.SI_F32 if case.f32 else si._capi.SI_F64)
    if case.prior > 0.0:
        ctx.set_prior(case.prior)   # (si_infer_setup switches the prior off: set it afterwards)
    return pb


def _run(ctx, case, grad=True, metric=True, **kw):
    args = dict(seed=case.seed, chain_id0=case.chain_id0, nchains=case.nchains, n_adapts=None if case.n_adapts < 0 else case.n_adapts,
                delta=case.delta)
    args.update(kw)
    return ctx.sample_hmc(case.itr, case.sigma_z, grad=grad, metric=metric, **args)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("case", ha.CASES, ids=lambda c: c.name)
def test_every_transition_of_si_sample_hmc(si, gpu_ctx, case):
    try:
        _setup(si, gpu_ctx, case)
        z, lp, alpha, eps, g, minv = _run(gpu_ctx, case)
        fused, passes, rounds = gpu_ctx.hmc_kernel_info()
        cols = case.itr + 1
        assert z.shape == g.shape == minv.shape == (case.m, cols, case.nchains)
        assert lp.shape == alpha.shape == eps.shape == (cols, case.nchains)
        assert fused == int(case.fused), (case.name, fused, passes)
        assert passes == (1 if case.fused else case.nchains)
        rep = ha.audit_case(case, z, lp, alpha, eps, g, minv)
        print("%s: fused %d, passes %d, search rounds %d: %s" % (case.name, fused, passes, rounds, rep.line()))
        ha.check_caps(case, rep)
        # one round for z_0, then one per evaluation of the longest search (undecidable searches aside, the replay's own count)
        assert 3 <= rounds <= 203
        if rep.undecidable == 0:
            assert rounds == 1 + max(rep.search_evals), (rounds, rep.search_evals)
        # column 0 is si_sample_mala's column 0 for the same seed and chain
        zm, lpm, _, gm = gpu_ctx.sample_mala(1, case.sigma_z, seed=case.seed, chain_id0=case.chain_id0, nchains=case.nchains, grad=True)
        assert np.array_equal(z[:, 0, :], zm[:, 0, :]) and np.array_equal(lp[0, :], lpm[0, :]) and np.array_equal(g[:, 0, :], gm[:, 0, :])
        if case.fused:
            # lp and G at column 0 and at every accepted column are the public gradient's bits at that state
            for c in range(case.nchains):
                keep = [0] + [t for t in range(1, cols) if not np.array_equal(z[:, t, c], z[:, t - 1, c])]
                lpb, gb = gpu_ctx.logdensity_grad_batch(np.asfortranarray(z[:, keep, c]))
                assert gpu_ctx.grad_kernel_info() == 1
                assert np.array_equal(lp[keep, c], lpb) and np.array_equal(g[:, keep, c], gb), (case.name, c)
    finally:
        gpu_ctx.set_prior(0.0)


def test_a_chains_bits_do_not_depend_on_the_call(si, gpu_ctx):
    case = ha.CASE_BY_NAME["A-M33"]
    _setup(si, gpu_ctx, case)
    assert (case.chain_id0, case.nchains) == (2, 3)
    three = _run(gpu_ctx, case)
    again = _run(gpu_ctx, case)
    assert _same(three, again)                                  # a second identical call
    solo = _run(gpu_ctx, case, chain_id0=3, nchains=1)          # chain 3 alone is column 1 of chains 2 .. 4
    assert gpu_ctx.hmc_kernel_info()[:2] == (1, 1)
    for a, b in zip(three, solo):
        assert np.array_equal(a[..., 1], b[..., 0])
    assert 0.0 < three[2][1:, 1].mean() < 1.0 and not np.all(three[5][:, -1, 1] == 1.0)


def test_two_passes_inside_each_transition(si, gpu_ctx):
    """the 32768-observation shape of tests/test_gpu_mala.py: the gradient workspace's cap holds 8 points, 10 chains take two passes
    per transition and per round of the search"""
    dims, acts, _, m = NN_EXAMPLE
    b, c, itr, sigma_z = 32768, 10, 6, 0.002
    rng = np.random.default_rng(5)
    table, n = so.layer_table(list(dims), list(acts))
    x, y = rng.standard_normal((dims[0], b)), rng.standard_normal((dims[-1], b))
    w, p = 0.3 * rng.standard_normal(n), np.asfortranarray(0.05 * rng.standard_normal((n, m)))
    gpu_ctx.infer_setup(table, n, m, w, p, x, y, 0.8)
    try:
        out = gpu_ctx.sample_hmc(itr, sigma_z, seed=11, chain_id0=2, nchains=c, grad=True, metric=True)
        assert gpu_ctx.hmc_kernel_info()[:2] == (1, 2)
        assert all(np.all(np.isfinite(a)) for a in out)
        for col in (0, 9):   # one chain of each pass equals its solo run
            solo = gpu_ctx.sample_hmc(itr, sigma_z, seed=11, chain_id0=2 + col, nchains=1, grad=True, metric=True)
            assert gpu_ctx.hmc_kernel_info()[:2] == (1, 1)
            for a, s in zip(out, solo):
                assert np.array_equal(a[..., col], s[..., 0]), col
        # column 0 of every chain against the public gradient (both passes wrote their own columns)
        lpb, gb = gpu_ctx.logdensity_grad_batch(np.asfortranarray(out[0][:, 0, :]))
        assert np.array_equal(out[1][0, :], lpb) and np.array_equal(out[4][:, 0, :], gb)
    finally:
        # (hand the 2 GB workspace back: the next set-up releases it)
        t2, n2 = so.layer_table([3, 5], [0])
        r2 = np.random.default_rng(0)
        gpu_ctx.infer_setup(t2, n2, 2, r2.standard_normal(n2), r2.standard_normal((n2, 2)), r2.standard_normal((3, 17)), r2.standard_normal((5, 17)), 1.0)


@pytest.mark.parametrize("name", ["ragged-M5", "softplus"])
def test_the_gradient_and_metric_outputs_are_optional(si, gpu_ctx, name):
    case = ha.CASE_BY_NAME[name]
    _setup(si, gpu_ctx, case)
    full = _run(gpu_ctx, case)
    bare = _run(gpu_ctx, case, grad=False, metric=False)
    assert len(bare) == 4 and _same(full[:4], bare)
    only_g = _run(gpu_ctx, case, metric=False)
    only_m = _run(gpu_ctx, case, grad=False)
    assert len(only_g) == 5 and _same(full[:5], only_g) and len(only_m) == 5 and _same(full[:4] + full[5:], only_m)
    assert gpu_ctx.hmc_kernel_info()[0] == int(case.fused)


def test_state_rules(si, gpu_ctx):
    caps = si._capi
    fresh = si.Context(0)
    try:
        fresh._m = 2
        with pytest.raises(si.SubspaceError) as e:
            fresh.sample_hmc(4, 0.1, seed=1)
        assert e.value.code == caps.SI_ERR_STATE and "si_infer_setup" in str(e.value)
        assert fresh.hmc_kernel_info() == (0, 0, 0)
    finally:
        fresh.close()
    case = ha.CASE_BY_NAME["small-M2-search"]
    _setup(si, gpu_ctx, case)
    zpts = np.asfortranarray(np.random.default_rng(0).standard_normal((case.m, 3)))
    good_grad = gpu_ctx.logdensity_grad_batch(zpts)
    good_rwmh = gpu_ctx.sample_rwmh(8, 0.3, seed=4, nchains=2)
    good_mala = gpu_ctx.sample_mala(8, 1.0, seed=4, nchains=2, grad=True)
    good_hmc = _run(gpu_ctx, case)

    def unchanged():
        assert _same(good_grad, gpu_ctx.logdensity_grad_batch(zpts))
        assert _same(good_rwmh, gpu_ctx.sample_rwmh(8, 0.3, seed=4, nchains=2))
        assert _same(good_mala, gpu_ctx.sample_mala(8, 1.0, seed=4, nchains=2, grad=True))
        assert _same(good_hmc, _run(gpu_ctx, case))

    nan = float("nan")
    for bad in (dict(itr=0), dict(nchains=0), dict(chain_id0=-1), dict(sigma_z=0.0), dict(sigma_z=-0.1), dict(sigma_z=nan),
                dict(n_adapts=-1), dict(n_adapts=5), dict(delta=0.0), dict(delta=1.0), dict(delta=nan)):
        kw = dict(itr=4, sigma_z=0.1, nchains=1, chain_id0=0, n_adapts=2, delta=0.8)
        kw.update(bad)
        with pytest.raises(si.SubspaceError) as e:
            gpu_ctx.sample_hmc(kw.pop("itr"), kw.pop("sigma_z"), seed=1, **kw)
        assert e.value.code == caps.SI_ERR_INVALID, bad
    unchanged()
    gpu_ctx.rwmh_begin(4, 0.1, seed=1)
    try:
        with pytest.raises(si.SubspaceError) as e:
            gpu_ctx.sample_hmc(4, 0.1, seed=1)
        assert e.value.code == caps.SI_ERR_STATE and "step-wise RWMH session" in str(e.value)
    finally:
        gpu_ctx.rwmh_abort()
    unchanged()
    # a Conv chain set up with SI_F32 has no gradient: the call says so and leaves the context usable
    conv = ha.CASE_BY_NAME["conv-f64"]
    pb = ha.problem(conv)
    gpu_ctx.infer_setup(pb.table, pb.n, conv.m, pb.w, pb.p, pb.x, pb.y, conv.sigma_m, compute_dtype=caps.SI_F32)
    with pytest.raises(si.SubspaceError) as e:
        gpu_ctx.sample_hmc(4, 0.5, seed=1)
    assert e.value.code == caps.SI_ERR_INVALID
    assert np.all(np.isfinite(gpu_ctx.sample_rwmh(4, 0.5, seed=1)[1]))
    _setup(si, gpu_ctx, case)
    unchanged()


def test_sub_inference_device_sampler(si, gpu_ctx):
    from subspaceinference_jl_amd import flux, samplers
    rng = np.random.default_rng(0)
    model = flux.Chain(flux.Dense(4, 8, "relu", rng=rng), flux.Dense(8, 1, rng=rng))
    x, y = rng.standard_normal((4, 50)), rng.standard_normal((1, 50))
    data = flux.DataLoader(x, y, batchsize=50)
    _, n = flux.layer_table(model)
    w_swa, p = 0.1 * rng.standard_normal(n), 0.05 * rng.standard_normal((n, 3))
    kw = dict(σ_z=0.3, itr=12, M=3, ctx=gpu_ctx, seed=5, alg=":hmc")
    z, lp = si.sub_inference(model, data, w_swa, p, chain_id=1, return_z=True, device_sampler=True, **kw)
    zd, lpd, alpha, eps = gpu_ctx.sample_hmc(12, 0.3, seed=5, chain_id0=1, nchains=1)   # (sub_inference left its set-up in the ctx)
    assert gpu_ctx.hmc_kernel_info()[:2] == (1, 1)
    assert z.shape == (3, 12) and lp.shape == (12,)
    assert np.array_equal(z, zd[:, 1:, 0]) and np.array_equal(lp, lpd[1:, 0])
    z3, lp3 = si.sub_inference(model, data, w_swa, p, chain_id=1, nchains=3, return_z=True, device_sampler=True, **kw)
    assert z3.shape == (3, 12, 3) and lp3.shape == (12, 3) and np.array_equal(z3[:, :, 0], z) and np.array_equal(lp3[:, 0], lp)
    chn, lpw = si.sub_inference(model, data, w_swa, p, chain_id=1, device_sampler=True, **kw)
    assert len(chn) == 12 and np.array_equal(lpw, lp) and np.allclose(chn[5], w_swa + p @ z[:, 5], rtol=1e-13)
    chn3, _ = si.sub_inference(model, data, w_swa, p, chain_id=1, nchains=3, device_sampler=True, **kw)
    assert len(chn3) == 3 and len(chn3[2]) == 12 and np.allclose(chn3[2][7], w_swa + p @ z3[:, 7, 2], rtol=1e-13)
    for alg in (":mala", ":nuts", ":rwmh"):
        with pytest.raises(si.SubspaceError) as e:
            si.sub_inference(model, data, w_swa, p, itr=5, M=3, ctx=gpu_ctx, alg=alg, device_sampler=True)
        assert ("device_loop" in str(e.value)) == (alg == ":mala")
    with pytest.raises(si.SubspaceError):
        si.sub_inference(model, data, w_swa, p, itr=5, M=3, ctx=gpu_ctx, alg=":hmc", nchains=2)
    # the default is the host loop on PCG64, unchanged: the direct samplers.hmc call with the same generator
    zh, lph = si.sub_inference(model, data, w_swa, p, chain_id=1, return_z=True, **kw)
    zh2, lph2 = si.sub_inference(model, data, w_swa, p, chain_id=1, return_z=True, device_sampler=False, **kw)
    zs, lps, _ = samplers.hmc(gpu_ctx.logdensity_grad, 3, 12, 0.3, np.random.default_rng([5, 1]))
    assert np.array_equal(zh, zs) and np.array_equal(lph, lps) and np.array_equal(zh2, zs) and np.array_equal(lph2, lps)
    assert not np.array_equal(zh, z)
