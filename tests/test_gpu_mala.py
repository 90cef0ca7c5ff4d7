"""si_sample_mala: MALA with the chain state on the device (csrc/capi_mala.hip, kernels_mala.hip).

Every case of tests/mala_audit.py's list (certified on the oracle alone by tests/test_mala_audit_cpu.py) runs on the device and its
trace is audited transition by transition: rejects are bit copies, accepts are within 16 ulp of z + h g + sigma_z n_t formed from the
trace's own state, lp and G are within the project's tolerances of the fp64 oracle, every decidable decision is the oracle's, the
accept count is exact.  The conditions hold on the device as on the oracle: both branches in every chain, no undecidable step in fp64.

Then what the audit cannot see: the route taken (fused for the Dense cases, per point for conv / SI_F32 / softplus), lp and G equal
to the public gradient's bits at every kept state, independence of a chain's bits from nchains / column / run / pass, the optional
gradient output, the state rules, and the opt-in keyword of sub_inference."""
import numpy as np
import pytest

from oracle import subspace_oracle as so
from tests import mala_audit as ma
from tests.test_gpu_chain_grid import NN_EXAMPLE

pytestmark = pytest.mark.gpu


def _setup(si, ctx, case):
    pb = ma.problem(case)
    ctx.infer_setup(pb.table, pb.n, case.m, pb.w, pb.p, pb.x, pb.y, case.sigma_m,
                    compute_dtype=si._capi.SI_F32 if case.f32 else si._capi.SI_F64)
    if case.prior > 0.0:
        ctx.set_prior(case.prior)   # (si_infer_setup switches the prior off: set it afterwards)
    return pb


def _run(ctx, case, grad=True, **kw):
    args = dict(seed=case.seed, chain_id0=case.chain_id0, nchains=case.nchains)
    args.update(kw)
    return ctx.sample_mala(case.itr, case.sigma_z, grad=grad, **args)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("case", ma.CASES, ids=lambda c: c.name)
def test_every_transition_of_si_sample_mala(si, gpu_ctx, case):
    try:
        _setup(si, gpu_ctx, case)
        z, lp, acc, g = _run(gpu_ctx, case)
        fused, passes = gpu_ctx.mala_kernel_info()
        assert z.shape == g.shape == (case.m, case.itr, case.nchains) and lp.shape == (case.itr, case.nchains) and acc.shape == (case.nchains,)
        assert fused == int(case.fused), (case.name, fused, passes)
        assert passes == (1 if case.fused else case.nchains)
        rep = ma.audit_case(case, z, lp, acc, g)
        print("%s: fused %d, passes %d: %s" % (case.name, fused, passes, rep.line()))
        ma.check_caps(case, rep)
        if case.fused:
            # lp and G at step 0 and at every accepted step are the public gradient's bits at that state
            for c in range(case.nchains):
                keep = [0] + [t for t in range(1, case.itr) if not np.array_equal(z[:, t, c], z[:, t - 1, c])]
                lpb, gb = gpu_ctx.logdensity_grad_batch(np.asfortranarray(z[:, keep, c]))
                assert gpu_ctx.grad_kernel_info() == 1
                assert np.array_equal(lp[keep, c], lpb) and np.array_equal(g[:, keep, c], gb), (case.name, c)
    finally:
        gpu_ctx.set_prior(0.0)


def test_a_chains_bits_do_not_depend_on_the_call(si, gpu_ctx):
    case = ma.CASE_BY_NAME["A-M33"]
    _setup(si, gpu_ctx, case)
    assert (case.chain_id0, case.nchains) == (2, 3)
    three = _run(gpu_ctx, case)
    again = _run(gpu_ctx, case)
    assert _same(three, again)                                  # a second identical call
    solo = _run(gpu_ctx, case, chain_id0=3, nchains=1)          # chain 3 alone is column 1 of chains 2 .. 4
    assert gpu_ctx.mala_kernel_info() == (1, 1)
    for a, b in zip(three, solo):
        assert np.array_equal(a[..., 1], b[..., 0])
    assert 0.0 < three[2][1] < 1.0


def test_two_passes_inside_each_transition(si, gpu_ctx):
    """nn_example's chain on 32768 observations: 2048 workgroups of 16 observations per point, so the gradient workspace's cap holds
    8 points and 10 chains take two passes per transition (si_logdensity_grad_batch's formula, reported by si_mala_kernel_info)"""
    dims, acts, _, m = NN_EXAMPLE
    b, c, itr, sigma_z = 32768, 10, 6, 0.002
    rng = np.random.default_rng(5)
    table, n = so.layer_table(list(dims), list(acts))
    x, y = rng.standard_normal((dims[0], b)), rng.standard_normal((dims[-1], b))
    w, p = 0.3 * rng.standard_normal(n), np.asfortranarray(0.05 * rng.standard_normal((n, m)))
    gpu_ctx.infer_setup(table, n, m, w, p, x, y, 0.8)
    try:
        z, lp, acc, g = gpu_ctx.sample_mala(itr, sigma_z, seed=11, chain_id0=2, nchains=c, grad=True)
        assert gpu_ctx.mala_kernel_info() == (1, 2)
        assert np.all(np.isfinite(z)) and np.all(np.isfinite(lp)) and np.all(np.isfinite(g))
        for col in (0, 9):   # one chain of each pass equals its solo run
            solo = gpu_ctx.sample_mala(itr, sigma_z, seed=11, chain_id0=2 + col, nchains=1, grad=True)
            assert gpu_ctx.mala_kernel_info() == (1, 1)
            for a, s in zip((z, lp, acc, g), solo):
                assert np.array_equal(a[..., col], s[..., 0]), col
        # step 0 of every chain against the public gradient (both passes wrote their own columns)
        lpb, gb = gpu_ctx.logdensity_grad_batch(np.asfortranarray(z[:, 0, :]))
        assert np.array_equal(lp[0, :], lpb) and np.array_equal(g[:, 0, :], gb)
    finally:
        # (hand the 2 GB workspace back: the next set-up releases it)
        t2, n2 = so.layer_table([3, 5], [0])
        r2 = np.random.default_rng(0)
        gpu_ctx.infer_setup(t2, n2, 2, r2.standard_normal(n2), r2.standard_normal((n2, 2)), r2.standard_normal((3, 17)), r2.standard_normal((5, 17)), 1.0)


@pytest.mark.parametrize("name", ["ragged-M5", "softplus"])
def test_the_gradient_output_is_optional(si, gpu_ctx, name):
    case = ma.CASE_BY_NAME[name]
    _setup(si, gpu_ctx, case)
    with_g = _run(gpu_ctx, case)
    without = _run(gpu_ctx, case, grad=False)
    assert len(without) == 3 and _same(with_g[:3], without)
    assert gpu_ctx.mala_kernel_info()[0] == int(case.fused)


def test_state_rules(si, gpu_ctx):
    caps = si._capi
    fresh = si.Context(0)
    try:
        fresh._m = 2
        with pytest.raises(si.SubspaceError) as e:
            fresh.sample_mala(4, 0.1, seed=1)
        assert e.value.code == caps.SI_ERR_STATE and "si_infer_setup" in str(e.value)
        assert fresh.mala_kernel_info() == (0, 0)
    finally:
        fresh.close()
    case = ma.CASE_BY_NAME["small-M2"]
    _setup(si, gpu_ctx, case)
    zpts = np.asfortranarray(np.random.default_rng(0).standard_normal((case.m, 3)))
    good_grad = gpu_ctx.logdensity_grad_batch(zpts)
    good_rwmh = gpu_ctx.sample_rwmh(8, 0.3, seed=4, nchains=2)
    good_mala = _run(gpu_ctx, case)

    def unchanged():
        assert _same(good_grad, gpu_ctx.logdensity_grad_batch(zpts))
        assert _same(good_rwmh, gpu_ctx.sample_rwmh(8, 0.3, seed=4, nchains=2))
        assert _same(good_mala, _run(gpu_ctx, case))

    for bad in (dict(itr=0), dict(nchains=0), dict(sigma_z=0.0), dict(sigma_z=-0.1), dict(sigma_z=float("nan"))):
        kw = dict(itr=4, sigma_z=0.1, nchains=1)
        kw.update(bad)
        with pytest.raises(si.SubspaceError) as e:
            gpu_ctx.sample_mala(kw["itr"], kw["sigma_z"], seed=1, nchains=kw["nchains"])
        assert e.value.code == caps.SI_ERR_INVALID, bad
    unchanged()
    gpu_ctx.rwmh_begin(4, 0.1, seed=1)
    try:
        with pytest.raises(si.SubspaceError) as e:
            gpu_ctx.sample_mala(4, 0.1, seed=1)
        assert e.value.code == caps.SI_ERR_STATE and "step-wise RWMH session" in str(e.value)
    finally:
        gpu_ctx.rwmh_abort()
    unchanged()
    # a Conv chain set up with SI_F32 has no gradient: the call says so and leaves the context usable
    conv = ma.CASE_BY_NAME["conv-f64"]
    pb = ma.problem(conv)
    gpu_ctx.infer_setup(pb.table, pb.n, conv.m, pb.w, pb.p, pb.x, pb.y, conv.sigma_m, compute_dtype=caps.SI_F32)
    with pytest.raises(si.SubspaceError) as e:
        gpu_ctx.sample_mala(4, 0.5, seed=1)
    assert e.value.code == caps.SI_ERR_INVALID
    assert np.all(np.isfinite(gpu_ctx.sample_rwmh(4, 0.5, seed=1)[1]))


def test_sub_inference_device_loop(si, gpu_ctx):
    from subspaceinference_jl_amd import flux, samplers
    rng = np.random.default_rng(0)
    model = flux.Chain(flux.Dense(4, 8, "relu", rng=rng), flux.Dense(8, 1, rng=rng))
    x, y = rng.standard_normal((4, 50)), rng.standard_normal((1, 50))
    data = flux.DataLoader(x, y, batchsize=50)
    _, n = flux.layer_table(model)
    w_swa, p = 0.1 * rng.standard_normal(n), 0.05 * rng.standard_normal((n, 3))
    kw = dict(σ_z=0.3, itr=12, M=3, ctx=gpu_ctx, seed=5, alg=":mala")
    z, lp = si.sub_inference(model, data, w_swa, p, chain_id=1, return_z=True, device_loop=True, **kw)
    zd, lpd, _ = gpu_ctx.sample_mala(12, 0.3, seed=5, chain_id0=1, nchains=1)     # (sub_inference left its set-up in the ctx)
    assert gpu_ctx.mala_kernel_info() == (1, 1)
    assert np.array_equal(z, zd[:, :, 0]) and np.array_equal(lp, lpd[:, 0])
    z3, lp3 = si.sub_inference(model, data, w_swa, p, chain_id=1, nchains=3, return_z=True, device_loop=True, **kw)
    assert z3.shape == (3, 12, 3) and np.array_equal(z3[:, :, 0], z) and np.array_equal(lp3[:, 0], lp)
    chn, lpw = si.sub_inference(model, data, w_swa, p, chain_id=1, device_loop=True, **kw)
    assert len(chn) == 12 and np.array_equal(lpw, lp) and np.allclose(chn[5], w_swa + p @ z[:, 5], rtol=1e-13)
    with pytest.raises(si.SubspaceError):
        si.sub_inference(model, data, w_swa, p, itr=5, M=3, ctx=gpu_ctx, alg=":hmc", device_loop=True)
    # the default is the host loop on PCG64, unchanged: the direct samplers.mala call with the same generator
    zh, lph = si.sub_inference(model, data, w_swa, p, chain_id=1, return_z=True, **kw)
    zh2, lph2 = si.sub_inference(model, data, w_swa, p, chain_id=1, return_z=True, device_loop=False, **kw)
    zs, lps, _ = samplers.mala(gpu_ctx.logdensity_grad, 3, 12, 0.3, np.random.default_rng([5, 1]))
    assert np.array_equal(zh, zs) and np.array_equal(lph, lps) and np.array_equal(zh2, zs) and np.array_equal(lph2, lps)
    assert not np.array_equal(zh, z)
