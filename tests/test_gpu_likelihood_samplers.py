"""The gradient samplers under the categorical and Bernoulli likelihoods on the device: si_sample_mala, si_sample_hmc, si_sample_nuts
and si_fit_advi after si_infer_set_likelihood, audited transition by transition (update by update) with the definition of
tests/likelihood_cases.py as value_grad.

Under a likelihood every one of the four steps aside from its device-resident route and evaluates its points through
logdensity_grad_point, seeded by the training step's cost tail with inv_denom = -1.  So each test asserts the route, then hands the
finished trace to the sampler's own audit (tests/mala_audit.py, hmc_audit.py, nuts_audit.py, advi_audit.py) at the case's own
tolerances -- the proposals, the accept / reject decisions, alpha, the step-size search, the adaptor's eps and Minv, the tree, the
ADVI updates and ELBO estimates, all against the likelihood's definition -- under the conditions tests/test_likelihood_cpu.py
certifies on the definition alone: both branches in every chain, no undecidable step or search at fp64.

Then what the audits cannot see: lp and G at every kept state are si_logdensity_grad_batch's bits, HMC's column 0 is MALA's, the mu
half of every ADVI update and every elbo_t are replayed bit for bit from si_logdensity_grad_batch's values, and a chain's bits do not
depend on the chains beside it.  And that the audits can fail here: a device trace audited against a wrong density is rejected."""
import numpy as np
import pytest

from oracle import subspace_oracle as so
from tests import advi_audit as aa
from tests import hmc_audit as ha
from tests import likelihood_cases as lc
from tests import mala_audit as ma
from tests import nuts_audit as na
from tests.rwmh_audit import AuditFailure
from tests.test_gpu_likelihood import _setup, ctx  # noqa: F401  (ctx: the fixture that hands the context back with its defaults)

pytestmark = pytest.mark.gpu


def _begin(si, ctx, sp):
    pb, vg = lc.sampler_problem(sp.name)
    _setup(si, ctx, pb, f32=sp.f32)                             # decoder and prior included
    return pb, vg


def _mala(ctx, case, **kw):
    args = dict(seed=case.seed, chain_id0=case.chain_id0, nchains=case.nchains, grad=True)
    args.update(kw)
    out = ctx.sample_mala(case.itr, case.sigma_z, **args)
    assert ctx.mala_kernel_info()[0] == 0
    return out


def _hmc(ctx, case, **kw):
    args = dict(seed=case.seed, chain_id0=case.chain_id0, nchains=case.nchains, n_adapts=None, delta=case.delta, grad=True, metric=True)
    args.update(kw)
    out = ctx.sample_hmc(case.itr, case.sigma_z, **args)
    assert ctx.hmc_kernel_info()[:2] == (0, args["nchains"])
    return out


def _nuts(ctx, case, **kw):
    args = dict(seed=case.seed, chain_id0=case.chain_id0, nchains=case.nchains, n_adapts=None, delta=case.delta, max_depth=case.max_depth,
                max_dh=case.max_dh, grad=True, metric=True, leaf_cap=case.leaf_cap)
    args.update(kw)
    out = ctx.sample_nuts(case.itr, case.sigma_z, **args)
    assert ctx.nuts_kernel_info()[0] == 0
    return out


def _advi(ctx, case, **kw):
    args = dict(samples_per_step=case.s, eta=case.eta, tau=case.tau, window=case.w, chain_id0=case.chain_id0, nruns=case.nruns,
                ndraws=case.ndraws, trace=True)
    args.update(kw)
    out = ctx.fit_advi(case.t, case.sigma_z, case.seed, **args)
    assert ctx.advi_kernel_info() == (0, args["nruns"] * case.s)
    return out


def _kept_states_hold_the_public_gradients_bits(ctx, z, lp, g, tag):
    """column 0 and every accepted column: lp and G are logdensity_grad_batch's bits at that state, on the per-point path"""
    for c in range(z.shape[2]):
        keep = [0] + [t for t in range(1, z.shape[1]) if not np.array_equal(z[:, t, c], z[:, t - 1, c])]
        lpb, gb = ctx.logdensity_grad_batch(np.asfortranarray(z[:, keep, c]))
        assert ctx.grad_kernel_info() == 0
        assert np.array_equal(lp[keep, c], lpb) and np.array_equal(g[:, keep, c], gb), (tag, c)


# ---- MALA ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sp", lc.SAMPLER_PROBLEMS, ids=lambda s: s.name)
def test_every_transition_of_mala(si, ctx, sp):
    case = lc.mala_case(sp)
    _, vg = _begin(si, ctx, sp)
    z, lp, acc, g = _mala(ctx, case)
    assert z.shape == g.shape == (case.m, case.itr, case.nchains)
    rep = ma.audit_case(case, z, lp, acc, g, value_grad=vg)
    print("mala %s: %s" % (sp.name, rep.line()))
    ma.check_caps(case, rep)
    _kept_states_hold_the_public_gradients_bits(ctx, z, lp, g, sp.name)


# ---- HMC -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sp", lc.SAMPLER_PROBLEMS, ids=lambda s: s.name)
def test_every_transition_of_hmc(si, ctx, sp):
    case = lc.hmc_case(sp)
    _, vg = _begin(si, ctx, sp)
    z, lp, alpha, eps, g, minv = _hmc(ctx, case)
    assert z.shape == g.shape == minv.shape == (case.m, case.itr + 1, case.nchains)
    rep = ha.audit_case(case, z, lp, alpha, eps, g, minv, value_grad=vg)
    print("hmc %s: %s" % (sp.name, rep.line()))
    ha.check_caps(case, rep)
    _kept_states_hold_the_public_gradients_bits(ctx, z, lp, g, sp.name)
    # column 0 is si_sample_mala's column 0 for the same seed and chain
    zm, lpm, _, gm = ctx.sample_mala(1, case.sigma_z, seed=case.seed, chain_id0=case.chain_id0, nchains=case.nchains, grad=True)
    assert ctx.mala_kernel_info()[0] == 0
    assert np.array_equal(z[:, 0, :], zm[:, 0, :]) and np.array_equal(lp[0, :], lpm[0, :]) and np.array_equal(g[:, 0, :], gm[:, 0, :])


# ---- NUTS ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sp", lc.SAMPLER_PROBLEMS, ids=lambda s: s.name)
def test_every_transition_of_nuts(si, ctx, sp):
    case = lc.nuts_case(sp)
    _, vg = _begin(si, ctx, sp)
    tr = na.Trace(*_nuts(ctx, case))
    assert tr.leaf.shape == (3 * case.m + 1, case.leaf_cap, case.nchains)
    leaves = ctx.nuts_kernel_info()[4]
    assert leaves == int(tr.nleaf.sum())
    rep = na.audit_case(case, tr, value_grad=vg)
    depths = np.bincount(np.concatenate([np.asarray(d, dtype=np.int64) for d in rep.chain_depths]), minlength=case.max_depth + 1)
    print("nuts %s: %s; transitions per depth %s, full trees %d" % (
        sp.name, rep.line(), depths.tolist(), int((tr.nleaf[1:] == 2 ** case.max_depth - 1).sum())))
    na.check_caps(case, rep)
    assert rep.leaves == leaves


# ---- ADVI ----------------------------------------------------------------------------------------------------------------------------
def _replay_bits(ctx, theta_trace, points, elbo, case):
    """tests/test_gpu_advi.py's _replay_bits on the per-point route: the mu half of every update and every elbo_t from
    logdensity_grad_batch's (lp, g) at the trace's own points, bit for bit.  The stacked evaluation of a step leaves its points to
    the same logdensity_grad_point, and dmu, the ring, s and the update use only +, *, / and sqrt."""
    m, ns, nt, nr = points.shape
    lp, g = ctx.logdensity_grad_batch(np.asfortranarray(points.reshape(m, -1, order="F")))
    assert ctx.grad_kernel_info() == 0
    lp, g = lp.reshape(ns, nt, nr, order="F"), g.reshape(m, ns, nt, nr, order="F")
    for r in range(nr):
        aa.mu_replay(theta_trace[:, :, r], lambda t: (lp[:, t, r], g[:, :, t, r]), case.s, case.w, case.eta, case.tau)
        for t in range(nt):
            want = aa.elbo_of(lp[:, t, r], aa.entropy(theta_trace[m:, t, r]))
            assert elbo[t, r] == want, (r, t, elbo[t, r], want)


@pytest.mark.parametrize("sp", lc.ADVI_PROBLEMS, ids=lambda s: s.name)
def test_every_step_of_advi(si, ctx, sp):
    case = lc.advi_case(sp)
    _, vg = _begin(si, ctx, sp)
    theta, z, elbo, tr, pts = _advi(ctx, case)
    assert tr.shape == (2 * case.m, case.t + 1, case.nruns) and pts.shape == (case.m, case.s, case.t, case.nruns)
    rep = aa.audit_case(case, tr, pts, elbo, theta, z, value_grad=vg)
    print("advi %s: %s" % (sp.name, rep.line()))
    assert rep.steps == case.t * case.nruns
    if not sp.f32:
        _replay_bits(ctx, tr, pts, elbo, case)


# ---- a chain's bits do not depend on the chains beside it -------------------------------------------------------------------------------
def test_a_chains_bits_do_not_depend_on_the_call(si, ctx):
    sp = lc.SAMPLER_BY_NAME["cat10"]
    _begin(si, ctx, sp)
    assert (lc.SAMPLER_CHAIN_ID0, lc.SAMPLER_CHAINS) == (2, 2)
    for tag, run, case, key in (("mala", _mala, lc.mala_case(sp), "nchains"), ("hmc", _hmc, lc.hmc_case(sp), "nchains"),
                                ("nuts", _nuts, lc.nuts_case(sp), "nchains"), ("advi", _advi, lc.advi_case(sp), "nruns")):
        two = run(ctx, case)
        solo = run(ctx, case, chain_id0=3, **{key: 1})           # chain 3 alone is column 1 of chains 2 .. 3
        assert len(two) == len(solo)
        for a, b in zip(two, solo):
            assert np.array_equal(a[..., 1], b[..., 0], equal_nan=True), tag
        assert not np.array_equal(two[0][..., 0], two[0][..., 1]), tag


# ---- the audits can fail on a device trace ------------------------------------------------------------------------------------------------
def test_a_wrong_density_is_rejected(si, ctx):
    """the device's own traces audited against a deliberately wrong value_grad: the Gaussian density of the same problem (MALA, cat3),
    and the likelihood with the sign of the prior term flipped (HMC and ADVI, cat3-prior)"""
    sp = lc.SAMPLER_BY_NAME["cat3"]
    pb, vg = _begin(si, ctx, sp)
    case = lc.mala_case(sp)
    out = _mala(ctx, case)
    ma.check_caps(case, ma.audit_case(case, *out, value_grad=vg))

    def gaussian(z):
        lp, g, _ = so.logdensity_grad(pb.table, pb.w, pb.p, pb.x, pb.y, 0.8, z)
        return lp, g
    with pytest.raises(AuditFailure, match="lp is"):
        ma.audit_case(case, *out, value_grad=lc.cached(gaussian))

    sp = lc.SAMPLER_BY_NAME["cat3-prior"]
    pb, vg = _begin(si, ctx, sp)
    bare = pb.with_(prior=0.0)

    def flipped(z):
        lp, g = bare.density_grad(z)
        w = pb.weights(z)
        return lp - so.log_prior(w, pb.prior), g + pb.p.T @ w / (pb.prior * pb.prior)
    flipped = lc.cached(flipped)
    z0 = lc.points(pb, 1)[:, 0]
    assert np.allclose(0.5 * (np.asarray(flipped(z0)[1]) + vg(z0)[1]), bare.density_grad(z0)[1], rtol=1e-13)
    case = lc.hmc_case(sp)
    out = _hmc(ctx, case)
    ha.check_caps(case, ha.audit_case(case, *out, value_grad=vg))
    with pytest.raises(AuditFailure):
        ha.audit_case(case, *out, value_grad=flipped)
    case = lc.advi_case(sp)
    theta, z, elbo, tr, pts = _advi(ctx, case)
    assert aa.audit_case(case, tr, pts, elbo, theta, z, value_grad=vg).steps == case.t * case.nruns
    with pytest.raises(AuditFailure):
        aa.audit_case(case, tr, pts, elbo, theta, z, value_grad=flipped)
