"""si_fit_advi: the reference's ADVI with its state on the device (csrc/capi_advi.hip, kernels_advi.hip).

Every case of tests/advi_audit.py's list (certified on the oracle alone by tests/test_advi_audit_cpu.py) runs on the device and its
trace is audited update by update: theta_0, the points, every update against the fp64 oracle's gradients at the trace's own points,
the ELBO estimates, the final state and the draws.

Then what the audit's tolerances cannot see.  On the fused cases the (lp, g) that logdensity_grad_batch returns at the trace's points
reproduce, with non-contracted NumPy, the mu half of every theta_{t+1} and every elbo_t BIT FOR BIT (advi_audit.mu_replay: dmu, the
ring, s and the update use only +, *, / and sqrt).  Also: the route taken, independence of a run's bits from nruns / column / run /
pass, the optional outputs, the state rules, every refused argument, and the opt-in keyword of sub_inference."""
import numpy as np
import pytest

from oracle import subspace_oracle as so
from tests import advi_audit as aa
from tests.test_advi_audit_cpu import GOOD, REFUSED
from tests.test_gpu_chain_grid import NN_EXAMPLE

pytestmark = pytest.mark.gpu


def _setup(si, ctx, case):
    pb = aa.problem(case)
    ctx.infer_setup(pb.table, pb.n, case.m, pb.w, pb.p, pb.x, pb.y, case.sigma_m,
                    compute_dtype=si._capi.SI_F32 if case.f32 else si._capi.SI_F64)
    if case.prior > 0.0:
        ctx.set_prior(case.prior)   # (si_infer_setup switches the prior off: set it afterwards)
    return pb


def _run(ctx, case, trace=True, **kw):
    args = dict(samples_per_step=case.s, eta=case.eta, tau=case.tau, window=case.w, chain_id0=case.chain_id0, nruns=case.nruns,
                ndraws=case.ndraws, trace=trace)
    args.update(kw)
    return ctx.fit_advi(case.t, case.sigma_z, case.seed, **args)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _replay_bits(ctx, theta_trace, points, elbo, s, w, eta, tau):
    """the mu half of every update and every elbo_t from logdensity_grad_batch's (lp, g) at the trace's own points, bit for bit"""
    m, ns, nt, nr = points.shape
    lp, g = ctx.logdensity_grad_batch(np.asfortranarray(points.reshape(m, -1, order="F")))   # one call: a point's bits do not depend on it
    assert ctx.grad_kernel_info() == 1
    lp, g = lp.reshape(ns, nt, nr, order="F"), g.reshape(m, ns, nt, nr, order="F")
    for r in range(nr):
        aa.mu_replay(theta_trace[:, :, r], lambda t: (lp[:, t, r], g[:, :, t, r]), s, w, eta, tau)
        for t in range(nt):
            want = aa.elbo_of(lp[:, t, r], aa.entropy(theta_trace[m:, t, r]))
            assert elbo[t, r] == want, (r, t, elbo[t, r], want)


@pytest.mark.parametrize("case", aa.CASES, ids=lambda c: c.name)
def test_every_step_of_si_fit_advi(si, gpu_ctx, case):
    try:
        _setup(si, gpu_ctx, case)
        theta, z, elbo, tr, pts = _run(gpu_ctx, case)
        fused, passes = gpu_ctx.advi_kernel_info()
        assert theta.shape == (2 * case.m, case.nruns) and z.shape == (case.m, case.ndraws, case.nruns) and elbo.shape == (case.t, case.nruns)
        assert tr.shape == (2 * case.m, case.t + 1, case.nruns) and pts.shape == (case.m, case.s, case.t, case.nruns)
        assert fused == int(case.fused), (case.name, fused, passes)
        assert passes == (1 if case.fused else case.nruns * case.s)
        rep = aa.audit_case(case, tr, pts, elbo, theta, z)
        print("%s: fused %d, passes %d: %s" % (case.name, fused, passes, rep.line()))
        assert rep.steps == case.t * case.nruns
        if case.fused:
            _replay_bits(gpu_ctx, tr, pts, elbo, case.s, case.w, case.eta, case.tau)
    finally:
        gpu_ctx.set_prior(0.0)


def test_a_runs_bits_do_not_depend_on_the_call(si, gpu_ctx):
    case = aa.CASE_BY_NAME["M3-R3"]
    _setup(si, gpu_ctx, case)
    assert (case.chain_id0, case.nruns) == (2, 3)
    three = _run(gpu_ctx, case)
    again = _run(gpu_ctx, case)
    assert _same(three, again)                                  # a second identical call
    solo = _run(gpu_ctx, case, chain_id0=3, nruns=1)            # run 3 alone is column 1 of runs 2 .. 4
    assert gpu_ctx.advi_kernel_info() == (1, 1)
    for a, b in zip(three, solo):
        assert np.array_equal(a[..., 1], b[..., 0])
    assert not np.array_equal(three[0][:, 0], three[0][:, 1])


def test_two_passes_inside_each_step(si, gpu_ctx):
    """tests/test_gpu_mala.py::test_two_passes_inside_each_transition's shape: nn_example's chain on 32768 observations, 2048
    workgroups of 16 observations per point, so the gradient workspace holds 8 points and the 10 points of a step take two passes"""
    dims, acts, _, m = NN_EXAMPLE
    b, s, t = 32768, 10, 3
    rng = np.random.default_rng(5)
    table, n = so.layer_table(list(dims), list(acts))
    x, y = rng.standard_normal((dims[0], b)), rng.standard_normal((dims[-1], b))
    w, p = 0.3 * rng.standard_normal(n), np.asfortranarray(0.05 * rng.standard_normal((n, m)))
    gpu_ctx.infer_setup(table, n, m, w, p, x, y, 0.8)
    try:
        theta, z, elbo, tr, pts = gpu_ctx.fit_advi(t, 0.002, 11, samples_per_step=s, chain_id0=2, ndraws=2, trace=True)
        assert gpu_ctx.advi_kernel_info() == (1, 2)
        assert all(np.all(np.isfinite(a)) for a in (theta, z, elbo, tr, pts))
        # the same theta bits as with the points evaluated through logdensity_grad_batch (both passes wrote their own columns)
        _replay_bits(gpu_ctx, tr, pts, elbo, s, 100, 0.1, 1.0)
        assert np.array_equal(theta[:, 0], tr[:, t, 0])
    finally:
        # (hand the 2 GB workspace back: the next set-up releases it)
        t2, n2 = so.layer_table([3, 5], [0])
        r2 = np.random.default_rng(0)
        gpu_ctx.infer_setup(t2, n2, 2, r2.standard_normal(n2), r2.standard_normal((n2, 2)), r2.standard_normal((3, 17)), r2.standard_normal((5, 17)), 1.0)


def _raw(si, ctx, m, *, max_iters=5, samples_per_step=10, sigma_z=0.3, eta=0.1, tau=1.0, window=100, seed=11, chain_id0=0, nruns=1,
         ndraws=5, want=("theta", "z")):
    """si_fit_advi itself, with NULL for every output not in `want`: (status, the outputs asked for)"""
    t, s, r, d = max(int(max_iters), 0), max(int(samples_per_step), 0), max(int(nruns), 0), max(int(ndraws), 0)
    shapes = dict(theta=(2 * m, r), z=(m, d, r), elbo=(t, r), trace=(2 * m, t + 1, r), points=(m, min(s, 64), t, r))
    out = {k: (np.full(shapes[k], np.nan, order="F") if k in want else None) for k in shapes}
    rc = ctx.lib.si_fit_advi(ctx.h, int(max_iters), int(samples_per_step), float(sigma_z), float(eta), float(tau), int(window), int(seed),
                             int(chain_id0), int(nruns), int(ndraws), *(si._capi._ptr(out[k]) for k in ("theta", "z", "elbo", "trace", "points")))
    return rc, out


@pytest.mark.parametrize("name", ["M3-S10", "softplus"])
def test_the_optional_outputs_are_optional(si, gpu_ctx, name):
    case = aa.CASE_BY_NAME[name]
    _setup(si, gpu_ctx, case)
    theta, z, elbo, tr, pts = _run(gpu_ctx, case)
    assert _same((theta, z, elbo), _run(gpu_ctx, case, trace=False))
    kw = dict(max_iters=case.t, samples_per_step=case.s, sigma_z=case.sigma_z, window=case.w, seed=case.seed, chain_id0=case.chain_id0,
              nruns=case.nruns, ndraws=case.ndraws)
    rc, out = _raw(si, gpu_ctx, case.m, **kw)                                   # elbo, trace and points NULL
    assert rc == 0 and np.array_equal(out["theta"], theta) and np.array_equal(out["z"], z)
    rc, out = _raw(si, gpu_ctx, case.m, **dict(kw, ndraws=0), want=("theta",))   # D = 0 with Z_out = NULL
    assert rc == 0 and np.array_equal(out["theta"], theta)
    assert gpu_ctx.advi_kernel_info()[0] == int(case.fused)
    rc, out = _raw(si, gpu_ctx, case.m, **kw, want=("theta", "z", "points"))
    assert rc == 0 and np.array_equal(out["points"], pts)
    # D > 0 needs somewhere to put the draws, and theta_out is never optional
    assert _raw(si, gpu_ctx, case.m, **kw, want=("theta",))[0] == si._capi.SI_ERR_INVALID
    assert _raw(si, gpu_ctx, case.m, **kw, want=("z",))[0] == si._capi.SI_ERR_INVALID


def test_state_rules_and_refused_arguments(si, gpu_ctx):
    caps = si._capi
    fresh = si.Context(0)
    try:
        fresh._m = 2
        with pytest.raises(si.SubspaceError) as e:
            fresh.fit_advi(4, 0.1, seed=1)
        assert e.value.code == caps.SI_ERR_STATE and "si_infer_setup" in str(e.value)
        assert fresh.advi_kernel_info() == (0, 0)
    finally:
        fresh.close()
    case = aa.CASE_BY_NAME["M3-S10"]
    _setup(si, gpu_ctx, case)
    good = _run(gpu_ctx, case)
    good_mala = gpu_ctx.sample_mala(6, 0.3, seed=4, nchains=2)
    # the library itself refuses every row of the table (Context.fit_advi mirrors it and would not let the call through)
    assert GOOD["m"] == case.m
    for bad in REFUSED:
        kw = {k: v for k, v in dict(GOOD, **bad).items() if k != "m"}
        rc, _ = _raw(si, gpu_ctx, case.m, **kw)
        assert rc == caps.SI_ERR_INVALID, bad
        assert b"si_fit_advi" in gpu_ctx.lib.si_last_error(gpu_ctx.h)
        assert gpu_ctx.advi_kernel_info() == (0, 0)
        with pytest.raises(si.SubspaceError) as e:
            gpu_ctx.fit_advi(kw.pop("max_iters"), kw.pop("sigma_z"), 1, **kw)
        assert e.value.code == caps.SI_ERR_INVALID, bad
    assert _same(good, _run(gpu_ctx, case))
    gpu_ctx.rwmh_begin(4, 0.1, seed=1)
    try:
        with pytest.raises(si.SubspaceError) as e:
            _run(gpu_ctx, case)
        assert e.value.code == caps.SI_ERR_STATE and "step-wise RWMH session" in str(e.value)
    finally:
        gpu_ctx.rwmh_abort()
    assert _same(good, _run(gpu_ctx, case))
    assert _same(good_mala, gpu_ctx.sample_mala(6, 0.3, seed=4, nchains=2))


def test_sub_inference_device_loop(si, gpu_ctx):
    from subspaceinference_jl_amd import flux
    rng = np.random.default_rng(0)
    model = flux.Chain(flux.Dense(4, 8, "relu", rng=rng), flux.Dense(8, 1, rng=rng))
    x, y = rng.standard_normal((4, 50)), rng.standard_normal((1, 50))
    data = flux.DataLoader(x, y, batchsize=50)
    _, n = flux.layer_table(model)
    w_swa, p = 0.1 * rng.standard_normal(n), 0.05 * rng.standard_normal((n, 3))
    itr = 12
    kw = dict(σ_z=0.3, itr=itr, M=3, ctx=gpu_ctx, seed=5, alg=":advi")
    z, lp = si.sub_inference(model, data, w_swa, p, chain_id=1, return_z=True, device_loop=True, **kw)
    _, zd, _ = gpu_ctx.fit_advi(itr, 0.3, 5, chain_id0=1)         # (sub_inference left its set-up in the ctx; the defaults are the reference's)
    assert gpu_ctx.advi_kernel_info() == (1, 1)
    assert z.shape == (3, itr) and np.array_equal(z, zd[:, :, 0])
    assert lp.shape == (itr,) and not np.any(lp)
    chn, lpw = si.sub_inference(model, data, w_swa, p, chain_id=1, device_loop=True, **kw)
    assert len(chn) == itr and not np.any(lpw) and len(lpw) == itr
    for i in range(itr):
        assert np.allclose(chn[i], w_swa + p @ z[:, i], rtol=1e-13)
    with pytest.raises(si.SubspaceError):
        si.sub_inference(model, data, w_swa, p, chain_id=1, nchains=2, device_loop=True, **kw)
    with pytest.raises(si.SubspaceError, match="device_loop=True"):
        si.sub_inference(model, data, w_swa, p, chain_id=1, **kw)
    with pytest.raises(si.SubspaceError):
        si.sub_inference(model, data, w_swa, p, itr=5, M=3, ctx=gpu_ctx, alg=":nuts", device_loop=True)
