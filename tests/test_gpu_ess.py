"""si_sample_ess: elliptical slice sampling with the chain state on the device (csrc/capi_ess.hip, kernels_ess.hip) -- not in the
reference.

Every case of tests/ess_audit.py's list (certified on the oracle alone by tests/test_ess_audit_cpu.py) runs on the device and its
trace is audited transition by transition: column 0 is sigma_z n_0, stuck steps are bit copies, kept points lie on the ellipse at the
device's own angle within K = 32 units and on the slice, lp is within the project's tolerance of the fp64 oracle, every decidable
comparison of the replayed bracket is the device's and, while all are, theta and nev are the replay's bit for bit.  The conditions
hold on the device as on the oracle: in every fp64 chain a first point kept, two shrinks in a row and both shrink sides, no
undecidable comparison.

Then what the audit cannot see: si_ess_kernel_info's passes, rounds and evals against nev, lp equal to si_logdensity's bits at every
kept state, independence of a chain's bits from nchains / column / run / pass, the optional trace outputs, the refusals, and
alg = "ess" of sub_inference."""
import numpy as np
import pytest

from subspaceinference_jl_amd import flux
from tests import ess_audit as ea
from tests import likelihood_cases as lc
from tests import node_cases as nc
from tests.test_gpu_likelihood import ctx  # noqa: F401  (the fixture that hands the context back with its defaults)

pytestmark = pytest.mark.gpu


def _setup(si, ctx, case):
    f64, f32 = si._capi.SI_F64, si._capi.SI_F32
    if case.kind == "lik":
        pb = lc.sampler_problem(case.model[1])[0]
        ctx.infer_setup(pb.table, pb.n, pb.m, pb.w, pb.p, pb.x, pb.y, 0.8, compute_dtype=f32 if case.f32 else f64)
        ctx.set_prior(pb.prior)
        ctx.infer_set_likelihood(pb.kind)
    elif case.kind == "decoder":
        pb, (dtable, wdec) = ea.decoder_of(case)
        ctx.infer_setup([list(r) for r in pb.table], pb.n, case.m, pb.w_swa, np.zeros((pb.n, case.m), order="F"), pb.x, pb.y, pb.sigma_m)
        ctx.set_decoder(dtable, wdec)
    elif case.kind == "node":
        ncase = getattr(nc, case.model[1])
        pb = nc.problem(ncase)
        ctx.infer_setup_node([list(r) for r in pb.table], pb.n, case.m, pb.w_swa, pb.p, pb.u0, pb.y, pb.ts, **ncase.setup_kwargs())
    else:
        pb = ea.ra._problem(case.model, case.m, case.sigma_m, case.prior)
        ctx.infer_setup(pb.table, pb.n, case.m, pb.w, pb.p, pb.x, pb.y, case.sigma_m, compute_dtype=f32 if case.f32 else f64)
        if case.prior > 0.0:
            ctx.set_prior(case.prior)   # (si_infer_setup switches the prior off: set it afterwards)


def _run(ctx, case, trace=True, **kw):
    args = dict(seed=case.seed, chain_id0=case.chain_id0, nchains=case.nchains, max_evals=case.max_evals)
    args.update(kw)
    return ctx.sample_ess(case.itr, case.sigma_z, trace=trace, **args)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _is_conv(case):
    return case.model[0] == "conv"


@pytest.mark.parametrize("case", ea.CASES, ids=lambda c: c.name)
def test_every_transition_of_si_sample_ess(si, ctx, case):
    _setup(si, ctx, case)
    z, lp, nev, theta = _run(ctx, case)
    passes, rounds, evals = ctx.ess_kernel_info()
    assert z.shape == (case.m, case.itr, case.nchains) and lp.shape == nev.shape == theta.shape == (case.itr, case.nchains)
    assert nev.dtype == np.int32
    rep = ea.audit_case(case, z, lp, nev, theta)
    print("%s: passes %d, rounds %d, evals %d, waste %d: %s" % (case.name, passes, rounds, evals, rounds * case.nchains - evals, rep.line()))
    ea.check_caps(case, rep)
    # a Conv chain fills the chip one chain at a time; every other case of the list fits one pass of launches
    assert passes == (case.nchains if _is_conv(case) else 1)
    assert evals == rep.evals == int(np.abs(nev[1:]).sum())
    assert rounds == rep.rounds == sum(int(np.abs(nev[t]).max()) for t in range(1, case.itr))
    # lp at column 0 and at every kept state is si_logdensity's bits at that state
    for c in range(case.nchains):
        keep = [t for t in range(case.itr) if nev[t, c] > 0]
        assert np.array_equal(lp[keep, c], ctx.logdensity(np.asfortranarray(z[:, keep, c]))), (case.name, c)


def test_a_chains_bits_do_not_depend_on_the_call(si, ctx):
    case = ea.CASE_BY_NAME["A-M33"]
    _setup(si, ctx, case)
    assert (case.chain_id0, case.nchains) == (2, 3)
    three = _run(ctx, case)
    again = _run(ctx, case)
    assert _same(three, again)                                  # a second identical call
    solo = _run(ctx, case, chain_id0=3, nchains=1)              # chain 3 alone is column 1 of chains 2 .. 4
    assert ctx.ess_kernel_info()[0] == 1
    for a, b in zip(three, solo):
        assert np.array_equal(a[..., 1], b[..., 0])
    assert int(np.abs(solo[2][1:]).sum()) == ctx.ess_kernel_info()[1] == ctx.ess_kernel_info()[2]   # one chain: no lock-step waste


def test_two_conv_chains_take_two_passes_and_equal_their_solo_runs(si, ctx):
    case = ea.CASE_BY_NAME["conv-f64"]
    _setup(si, ctx, case)
    assert case.nchains == 2
    both = _run(ctx, case)
    assert ctx.ess_kernel_info()[0] == 2
    for col in range(2):
        solo = _run(ctx, case, chain_id0=case.chain_id0 + col, nchains=1)
        assert ctx.ess_kernel_info()[0] == 1
        for a, s in zip(both, solo):
            assert np.array_equal(a[..., col], s[..., 0]), col


@pytest.mark.parametrize("name", ["ragged-M5", "lik-cat3"])
def test_the_trace_outputs_are_optional(si, ctx, name):
    case = ea.CASE_BY_NAME[name]
    _setup(si, ctx, case)
    with_trace = _run(ctx, case)
    info = ctx.ess_kernel_info()
    without = _run(ctx, case, trace=False)
    assert len(without) == 2 and _same(with_trace[:2], without) and ctx.ess_kernel_info() == info


def test_refusals(si, ctx):
    caps = si._capi
    fresh = si.Context(0)
    try:
        fresh._m = 2
        with pytest.raises(si.SubspaceError) as e:
            fresh.sample_ess(4, 0.1, seed=1)
        assert e.value.code == caps.SI_ERR_STATE and "si_infer_setup" in str(e.value)
        assert fresh.ess_kernel_info() == (0, 0, 0)
    finally:
        fresh.close()
    case = ea.CASE_BY_NAME["small-M2"]
    _setup(si, ctx, case)
    good_rwmh = ctx.sample_rwmh(8, 0.3, seed=4, nchains=2)
    good = _run(ctx, case)
    assert ctx.ess_kernel_info()[1] > 0

    def unchanged():
        assert _same(good_rwmh, ctx.sample_rwmh(8, 0.3, seed=4, nchains=2))
        assert _same(good, _run(ctx, case))

    for bad in (dict(itr=0), dict(nchains=0), dict(chain_id0=-1), dict(sigma_z=0.0), dict(sigma_z=-0.1), dict(sigma_z=float("nan")),
                dict(max_evals=0), dict(max_evals=-3)):
        kw = dict(itr=4, sigma_z=0.1, nchains=1, chain_id0=0, max_evals=128)
        kw.update(bad)
        with pytest.raises(si.SubspaceError) as e:
            ctx.sample_ess(kw["itr"], kw["sigma_z"], seed=1, chain_id0=kw["chain_id0"], nchains=kw["nchains"], max_evals=kw["max_evals"])
        assert e.value.code == caps.SI_ERR_INVALID, bad
        assert ctx.ess_kernel_info() == (0, 0, 0)             # a refused call reports zeros
    unchanged()
    ctx.rwmh_begin(4, 0.1, seed=1)
    try:
        with pytest.raises(si.SubspaceError) as e:
            ctx.sample_ess(4, 0.1, seed=1)
        assert e.value.code == caps.SI_ERR_STATE and "step-wise RWMH session" in str(e.value)
    finally:
        ctx.rwmh_abort()
    unchanged()


def test_sub_inference_alg_ess(si, ctx):
    rng = np.random.default_rng(0)
    # ---- a Dense chain
    model = flux.Chain(flux.Dense(4, 8, "relu", rng=rng), flux.Dense(8, 1, rng=rng))
    x, y = rng.standard_normal((4, 50)), rng.standard_normal((1, 50))
    data = flux.DataLoader(x, y, batchsize=50)
    _, n = flux.layer_table(model)
    w_swa, p = 0.1 * rng.standard_normal(n), 0.3 * rng.standard_normal((n, 3))
    kw = dict(σ_z=2.0, itr=12, M=3, ctx=ctx, seed=5, alg=":ess")
    z, lp = si.sub_inference(model, data, w_swa, p, chain_id=1, return_z=True, **kw)
    zd, lpd = ctx.sample_ess(12, 2.0, seed=5, chain_id0=1, nchains=1)              # (sub_inference left its set-up in the ctx)
    assert z.shape == (3, 12) and lp.shape == (12,) and np.array_equal(z, zd[:, :, 0]) and np.array_equal(lp, lpd[:, 0])
    assert np.array_equal(lp, ctx.logdensity(z)) and len({tuple(z[:, t]) for t in range(12)}) == 12     # it never rejects
    z3, lp3 = si.sub_inference(model, data, w_swa, p, chain_id=1, nchains=3, return_z=True, **kw)
    assert z3.shape == (3, 12, 3) and lp3.shape == (12, 3) and np.array_equal(z3[:, :, 0], z) and np.array_equal(lp3[:, 0], lp)
    chn, lpw = si.sub_inference(model, data, w_swa, p, chain_id=1, **kw)
    assert len(chn) == 12 and np.array_equal(lpw, lp) and np.array_equal(np.stack(chn, axis=1), ctx.reconstruct(z))
    chn3, _ = si.sub_inference(model, data, w_swa, p, chain_id=1, nchains=3, **kw)
    assert len(chn3) == 3 and len(chn3[2]) == 12 and np.array_equal(chn3[2][7], ctx.reconstruct(z3[:, :, 2])[:, 7])
    zf, lpf = si.sub_inference(model, data, w_swa, p, chain_id=1, return_z=True, compute_dtype="f32", include_prior=True, **kw)
    assert zf.shape == (3, 12) and np.all(np.isfinite(lpf)) and not np.array_equal(lpf, lp)
    # ---- a classifier under the categorical likelihood
    cmodel = flux.Chain(flux.Dense(4, 6, "tanh", rng=rng), flux.Dense(6, 3, rng=rng))
    yc = lc.labels(lc.CATEGORICAL, 3, 50, rng)
    ctable, cn = flux.layer_table(cmodel)
    cw, cp = 0.3 * rng.standard_normal(cn), np.asfortranarray(0.3 * rng.standard_normal((cn, 3)))
    zc, lpc = si.sub_inference(cmodel, flux.DataLoader(x, yc, batchsize=50), cw, cp, chain_id=1, return_z=True, likelihood="categorical", **kw)
    assert ctx.infer_likelihood_info() == lc.CATEGORICAL and zc.shape == (3, 12)
    pb = lc.Problem([list(r) for r in ctable], cn, cw, cp, np.asfortranarray(x), yc, lc.CATEGORICAL)
    ref = np.array([pb.density(zc[:, t]) for t in range(12)])
    assert np.max(np.abs(lpc - ref) / np.abs(ref)) <= ea.LP_RTOL_F64
    zcd, lpcd = ctx.sample_ess(12, 2.0, seed=5, chain_id0=1)
    assert np.array_equal(zc, zcd[:, :, 0]) and np.array_equal(lpc, lpcd[:, 0])
    # ---- a NeuralODE constructed without sensealg: the gradient samplers refuse it, this one needs values only
    case = nc.CASE_BY_NAME["ad-tutorial"]
    npb = nc.problem(case)
    nrng = np.random.default_rng(5)
    node = flux.NeuralODE(flux.Chain(flux.cube, flux.Dense(2, 15, "tanh", rng=nrng), flux.Dense(15, 2, rng=nrng)), (0.0, 1.5), npb.ts,
                          reltol=1e-7, abstol=1e-9)
    assert node.sensealg is None
    ndata = flux.DataLoader(npb.u0, npb.y, batchsize=100)
    np_ = np.asfortranarray(0.05 * nrng.standard_normal((npb.n, 3)))
    zn, lpn = si.sub_inference(node, ndata, npb.w_swa, np_, σ_z=0.5, itr=6, M=3, alg="ess", ctx=ctx, seed=4, return_z=True)
    assert zn.shape == (3, 6) and np.all(np.isfinite(lpn)) and np.array_equal(ctx.logdensity(zn), lpn)
    znd, lpnd = ctx.sample_ess(6, 0.5, seed=4)
    assert np.array_equal(zn, znd[:, :, 0]) and np.array_equal(lpn, lpnd[:, 0])
    with pytest.raises(si.SubspaceError, match="gradient through the ODE solver is not built"):
        si.sub_inference(node, ndata, npb.w_swa, np_, itr=4, M=3, alg="mala", ctx=ctx)
