"""The gradient through the NeuralODE solver on the device (si_node_set_grad, si_node_grad, the gradient entry points and the
gradient-driven samplers on a node set-up; csrc/kernels_node.hip: the forward with record, node_grad_kernel, node_grad_sum_kernel)
against its definition, node.logdensity_grad, over the lists of tests/node_grad_cases.py: bit equality wherever no transcendental
function is involved, counts / statuses and GRAD_TOL (measured on the CPU) where one is, lp to the bits of si_logdensity on every
route, the pull-back, batch = single point, independence of chain slot / C / pass split / column / run, the decoder bridge, the
failure statuses, the four samplers, sub_inference at the tutorial's shape, and the refusals."""
import numpy as np
import pytest

from subspaceinference_jl_amd import autoencoder, flux, node
from tests import advi_audit as aa
from tests import hmc_audit as ha
from tests import mala_audit as ma
from tests import nuts_audit as nta
from tests import node_cases as nc
from tests import node_grad_cases as gc
from tests import rwmh_audit as ra

pytestmark = pytest.mark.gpu


def _setup(ctx, case, pb=None, grad=True, **over):
    pb = gc.problem(case) if pb is None else pb
    kw = case.setup_kwargs()
    kw.update(over)
    ctx.infer_setup_node([list(r) for r in pb.table], pb.n, case.m, pb.w_swa, pb.p, pb.u0, pb.y, pb.ts, **kw)
    if grad:
        ctx.node_set_grad(True)
    return pb


def _close(a, b):
    """the pull-back's bound, as tests/test_gpu_grad_batch.py holds P' g: rtol 1e-8, atol 1e-9 max|g|"""
    return np.all(np.abs(a - b) <= ma.G_RTOL_F64 * np.abs(b) + ma.G_ATOL_F64 * np.max(np.abs(b)))


def _every_route(ctx, pb, z):
    """lp and gz from si_node_grad, si_logdensity_grad_batch and si_logdensity_grad: the same bits, and lp those of si_logdensity"""
    lp, gw, gz = ctx.node_grad(z)
    lpb, gzb = ctx.logdensity_grad_batch(z)
    assert np.array_equal(lpb, lp) and np.array_equal(gzb, gz, equal_nan=True)
    for c in range(z.shape[1]):
        lp1, gz1 = ctx.logdensity_grad(z[:, c])
        assert lp1 == lp[c] and np.array_equal(gz1, gz[:, c], equal_nan=True)
    assert np.array_equal(ctx.logdensity(z), lp)
    return lp, gw, gz


@pytest.mark.parametrize("case", gc.EXACT_CASES, ids=lambda c: c.name)
def test_fixed_step_without_transcendentals_is_bit_equal(gpu_ctx, case):
    pb = _setup(gpu_ctx, case)
    assert gpu_ctx.node_grad_info()[0] is True
    lp, gw, gz = _every_route(gpu_ctx, pb, pb.z)
    lp_ref, gw_ref = gc.definition(case)
    _, _, na, nr, st = gpu_ctx.node_solve(pb.z, want_u=False)
    for c in range(case.C):
        sol = gc.recorded(case, c)
        assert np.array_equal(na[:, c], sol.naccept) and not nr.any() and not st.any()
    assert np.array_equal(lp, lp_ref)
    assert np.array_equal(gw, gw_ref)
    assert _close(gz, pb.p.T @ gw_ref)
    if case.name == "g-s1-at-t0":
        assert np.array_equal(gw, -2.0 * np.stack([pb.weights(pb.z[:, c]) for c in range(case.C)], axis=1))


@pytest.mark.parametrize("case", gc.TRANS_CASES + gc.ADAPTIVE_CASES, ids=lambda c: c.name)
def test_transcendental_and_adaptive_cases_hold_counts_and_the_measured_bound(gpu_ctx, case):
    pb = _setup(gpu_ctx, case)
    lp, gw, gz = _every_route(gpu_ctx, pb, pb.z)
    lp_ref, gw_ref = gc.definition(case)
    _, _, na, nr, st = gpu_ctx.node_solve(pb.z, want_u=False)
    for c in range(case.C):
        sol = gc.recorded(case, c)
        assert np.array_equal(na[:, c], sol.naccept) and np.array_equal(nr[:, c], sol.nreject) and not st.any()
    print("%s: spread gw %.3e (bound %.3e), lp %.3e (bound %.3e)" % (case.name, nc.spread(gw_ref, gw), gc.GRAD_TOL, nc.spread(lp_ref, lp), nc.VALUE_TOL))
    assert nc.spread(lp_ref, lp) <= nc.VALUE_TOL
    assert nc.spread(gw_ref, gw) <= gc.GRAD_TOL
    assert _close(gz, pb.p.T @ gw)


def test_pass_split_chain_slot_c_and_run_do_not_change_a_bit(gpu_ctx):
    case = gc.PASS_SPLIT        # three chains per pass under the budget: C = 4 takes two passes, C = 7 three
    pb = _setup(gpu_ctx, case)
    assert gpu_ctx.node_grad_info() == (True, 3)
    lp, gw, gz = _every_route(gpu_ctx, pb, pb.z)
    lp_ref, gw_ref = gc.definition(case)
    assert np.array_equal(lp, lp_ref) and np.array_equal(gw, gw_ref)
    z7 = np.asfortranarray(np.concatenate([pb.z[:, ::-1], pb.z[:, 1:]], axis=1))     # other slots, other passes, another C
    lp7, gw7, gz7 = gpu_ctx.node_grad(z7)
    order = [3, 2, 1, 0, 1, 2, 3]
    assert np.array_equal(lp7, lp[order]) and np.array_equal(gw7, gw[:, order]) and np.array_equal(gz7, gz[:, order])
    again = gpu_ctx.node_grad(z7)
    assert all(np.array_equal(a, b) for a, b in zip(again, (lp7, gw7, gz7)))
    lpb, gzb = gpu_ctx.logdensity_grad_batch(z7)
    assert np.array_equal(lpb, lp7) and np.array_equal(gzb, gz7)


def test_a_trajectory_does_not_depend_on_its_column_or_neighbours(gpu_ctx):
    case = gc.CASE_BY_NAME["g-ad-tanh-cube"]
    pb = gc.problem(case)
    z = np.asfortranarray(np.repeat(pb.z[:, :1], 5, axis=1))
    z[:, 2] = 0.3                                               # a different neighbour in the middle
    _setup(gpu_ctx, case, pb)
    lp, gw, gz = gpu_ctx.node_grad(z)
    for c in (1, 3, 4):
        assert lp[c] == lp[0] and np.array_equal(gw[:, c], gw[:, 0]) and np.array_equal(gz[:, c], gz[:, 0])
    assert not np.array_equal(gw[:, 2], gw[:, 0])
    # two trajectories in either order: their slices are added from 0.0, and a + b = b + a
    out = []
    for idx in ([2, 6], [6, 2]):
        gpu_ctx.infer_setup_node([list(r) for r in pb.table], pb.n, case.m, pb.w_swa, pb.p, np.asfortranarray(pb.u0[:, idx]),
                                 np.asfortranarray(pb.y[:, idx]), pb.ts, **case.setup_kwargs())
        gpu_ctx.node_set_grad(True)
        out.append(gpu_ctx.node_grad(z[:, :1]))
    assert all(np.array_equal(a, b) for a, b in zip(*out))


def test_the_decoder_bridge(gpu_ctx):
    case = gc.CASE_BY_NAME["g-w15"]
    pb = _setup(gpu_ctx, case)
    rng = np.random.default_rng(4)
    z = np.asfortranarray(0.5 * rng.standard_normal((case.m, 3)))
    lp0, gw0, gz0 = gpu_ctx.node_grad(z)
    # the identity decoder W_D = P, b = 0 is the P route's weights: the same lp and gw to the bits
    gpu_ctx.set_decoder([(case.m, pb.n, flux.identity, 0, pb.n * case.m)], np.concatenate([pb.p.reshape(-1, order="F"), np.zeros(pb.n)]))
    lp1, gw1, gz1 = _every_route(gpu_ctx, pb, z)
    assert np.array_equal(lp1, lp0) and np.array_equal(gw1, gw0) and _close(gz1, gz0)
    # a two-layer tanh decoder: gw is the definition's at the decoded weights, gz autoencoder.py's reverse of it
    h = 4
    table = [(case.m, h, flux.tanh, 0, case.m * h), (h, pb.n, flux.identity, case.m * h + h, case.m * h + h + h * pb.n)]
    wdec = 0.1 * rng.standard_normal(case.m * h + h + h * pb.n + pb.n)
    gpu_ctx.set_decoder(table, wdec)
    lp2, gw2, gz2 = _every_route(gpu_ctx, pb, z)
    w = gpu_ctx.reconstruct(z)
    for c in range(3):
        lp_ref, gw_ref = node.logdensity_grad(pb.table, w[:, c], pb.u0, pb.y, pb.ts, case.opts())
        assert lp2[c] == lp_ref and np.array_equal(gw2[:, c], gw_ref)
        assert _close(gz2[:, c], autoencoder.decode_vjp(table, wdec, z[:, c], gw_ref))
    gpu_ctx.set_decoder(None, None)
    lp3, gw3, gz3 = gpu_ctx.node_grad(z)
    assert np.array_equal(lp3, lp0) and np.array_equal(gw3, gw0) and np.array_equal(gz3, gz0)


@pytest.mark.parametrize("case,status", [(nc.FAIL_STEPS, 1), (nc.FAIL_BLOWUP, 2)], ids=["max-steps", "blow-up"])
def test_a_failed_trajectory_is_minus_infinity_and_nan(gpu_ctx, case, status):
    pb = _setup(gpu_ctx, case, nc.problem(case))
    assert (gpu_ctx.node_solve(pb.z, want_u=False)[4] == status).all()
    lp, gw, gz = _every_route(gpu_ctx, pb, pb.z)
    assert np.all(np.isneginf(lp)) and np.all(np.isnan(gw)) and np.all(np.isnan(gz))


def test_a_failing_chain_leaves_the_others_of_its_launch_alone(gpu_ctx):
    case = nc.FAIL_PROPOSAL      # du/dt = w u^3 + b, w = -0.5 + 3 z: the solution leaves every bound before t = 1 once z > 0.37
    pb = _setup(gpu_ctx, case, nc.fail_proposal_problem())
    z = np.asfortranarray([[0.0, 0.6, -0.1, 1.5, 0.0]])
    st = gpu_ctx.node_solve(z, want_u=False)[4]
    bad = (st != 0).any(axis=0)
    assert list(bad) == [False, True, False, True, False]
    lp, gw, gz = _every_route(gpu_ctx, pb, z)
    assert np.all(np.isneginf(lp[bad])) and np.all(np.isnan(gw[:, bad])) and np.all(np.isnan(gz[:, bad]))
    for c in np.flatnonzero(~bad):
        lp1, gw1, gz1 = gpu_ctx.node_grad(z[:, c:c + 1])
        assert lp1[0] == lp[c] and np.array_equal(gw1[:, 0], gw[:, c]) and np.array_equal(gz1[:, 0], gz[:, c])
        lp_ref, gw_ref = node.logdensity_grad(pb.table, pb.weights(z[:, c]), pb.u0, pb.y, pb.ts, case.opts())
        assert np.isfinite(lp[c]) and nc.spread(lp_ref, lp[c]) <= nc.VALUE_TOL and nc.spread(gw_ref, gw[:, c]) <= gc.GRAD_TOL


# ---- the samplers ----------------------------------------------------------------------------------------------------------------
def _value_grad(case, pb):
    """the definition as the audits' callable: z -> (lp, P' d lp / dW)"""
    def f(z):
        lp, gw = node.logdensity_grad(pb.table, pb.weights(np.asarray(z, dtype=np.float64).reshape(-1)), pb.u0, pb.y, pb.ts, case.opts())
        return lp, pb.p.T @ gw
    return f


def _states_are_the_batch_entry_points(ctx, z, lp, g):
    """every returned lp / gradient sample equals si_logdensity_grad_batch at the returned state, to the bits; all trajectories there
    integrate"""
    for c in range(z.shape[2]):
        zc = np.asfortranarray(z[:, :, c])
        lpb, gb = ctx.logdensity_grad_batch(zc)
        assert np.array_equal(lp[:, c], lpb) and np.array_equal(g[:, :, c], gb)
        assert not ctx.node_solve(zc, want_u=False)[4].any() and np.all(np.isfinite(lpb)) and np.all(np.isfinite(gb))


@pytest.mark.parametrize("nchains", [1, 3])
def test_mala(gpu_ctx, nchains):
    case = gc.SAMPLER
    pb = _setup(gpu_ctx, case)
    z, lp, acc, g = gpu_ctx.sample_mala(10, 0.05, 7, 2, nchains, grad=True)
    _states_are_the_batch_entry_points(gpu_ctx, z, lp, g)
    print(ma.audit(z, lp, acc, g, _value_grad(case, pb), 0.05, 7, 2).line())
    again = gpu_ctx.sample_mala(10, 0.05, 7, 2, nchains, grad=True)
    assert all(np.array_equal(a, b) for a, b in zip(again, (z, lp, acc, g)))
    if nchains == 3:
        z1, lp1, _, g1 = gpu_ctx.sample_mala(10, 0.05, 7, 2, 1, grad=True)
        assert np.array_equal(z1[:, :, 0], z[:, :, 0]) and np.array_equal(lp1[:, 0], lp[:, 0]) and np.array_equal(g1[:, :, 0], g[:, :, 0])


@pytest.mark.parametrize("nchains", [1, 3])
def test_hmc(gpu_ctx, nchains):
    case = gc.SAMPLER
    pb = _setup(gpu_ctx, case)
    z, lp, alpha, eps, g, minv = gpu_ctx.sample_hmc(8, 0.1, 7, 2, nchains, grad=True, metric=True)
    _states_are_the_batch_entry_points(gpu_ctx, z, lp, g)
    print(ha.audit(z, lp, alpha, eps, g, minv, _value_grad(case, pb), 0.1, 7, 2, ha.n_adapts_of(8)).line())
    if nchains == 3:
        one = gpu_ctx.sample_hmc(8, 0.1, 7, 2, 1, grad=True, metric=True)
        assert all(np.array_equal(a[..., 0], b[..., 0]) for a, b in zip(one, (z, lp, alpha, eps, g, minv)))


def _nuts_audit(ctx, case, pb, nchains):
    """a run at max_depth = 3 with its tree and leaf log, audited leaf by leaf against the definition"""
    out = ctx.sample_nuts(6, 0.1, 7, 2, nchains, max_depth=3, grad=True, metric=True, leaf_cap=6 * 7)
    rep = nta.audit(nta.Trace(*out), _value_grad(case, pb), 0.1, 7, 2, ha.n_adapts_of(6), 0.8, 3, 1000.0, (ma.LP_RTOL_F64, ma.G_RTOL_F64, ma.G_ATOL_F64))
    print("%s, %d chains: %s" % (case.name, nchains, rep.line()))
    return out


@pytest.mark.parametrize("nchains", [1, 3])
def test_nuts(gpu_ctx, nchains):
    case = gc.SAMPLER
    pb = _setup(gpu_ctx, case)
    z, lp, alpha, eps, g = gpu_ctx.sample_nuts(6, 0.1, 7, 2, nchains, tree=False, grad=True)
    _states_are_the_batch_entry_points(gpu_ctx, z, lp, g)
    if nchains == 1:
        _nuts_audit(gpu_ctx, case, pb, 1)
    else:
        # three chains: one of the trees leaves the region where the adaptive case's step decisions are certified,
        # so the leaf-by-leaf audit runs on the fixed-step tanh problem, whose step sequence cannot differ from the definition's
        fixed = gc.SAMPLER_FIXED
        out = _nuts_audit(gpu_ctx, fixed, _setup(gpu_ctx, fixed), 3)
        _states_are_the_batch_entry_points(gpu_ctx, out[0], out[1], out[7])
        _setup(gpu_ctx, case)
    again = gpu_ctx.sample_nuts(6, 0.1, 7, 2, nchains, tree=False, grad=True)
    assert all(np.array_equal(a, b) for a, b in zip(again, (z, lp, alpha, eps, g)))
    if nchains == 3:
        one = gpu_ctx.sample_nuts(6, 0.1, 7, 2, 1, tree=False, grad=True)
        assert all(np.array_equal(a[..., 0], b[..., 0]) for a, b in zip(one, (z, lp, alpha, eps, g)))


@pytest.mark.parametrize("nruns", [1, 3])
def test_advi(gpu_ctx, nruns):
    case = gc.SAMPLER
    pb = _setup(gpu_ctx, case)
    theta, z, elbo, trace, points = gpu_ctx.fit_advi(6, 0.1, 7, samples_per_step=3, chain_id0=2, nruns=nruns, trace=True)
    assert theta.shape == (2 * case.m, nruns) and z.shape == (case.m, 6, nruns) and np.all(np.isfinite(theta)) and np.all(np.isfinite(elbo))
    # every update, ELBO estimate and draw against the definition
    print(aa.audit(trace, points, elbo, theta, z, _value_grad(case, pb), 0.1, 7, 2).line())
    # ... and the mu half of every update and every ELBO estimate from si_logdensity_grad_batch at the trace's own points, to the bits
    m, ns, nt, nr = points.shape
    flat = np.asfortranarray(points.reshape(m, -1, order="F"))
    lpb, gb = gpu_ctx.logdensity_grad_batch(flat)
    assert not gpu_ctx.node_solve(flat, want_u=False)[4].any() and np.all(np.isfinite(lpb)) and np.all(np.isfinite(gb))
    lpb, gb = lpb.reshape(ns, nt, nr, order="F"), gb.reshape(m, ns, nt, nr, order="F")
    for r in range(nr):
        aa.mu_replay(trace[:, :, r], lambda t: (lpb[:, t, r], gb[:, :, t, r]), ns, 100, 0.1, 1.0)
        for t in range(nt):
            assert elbo[t, r] == aa.elbo_of(lpb[:, t, r], aa.entropy(trace[m:, t, r])), (r, t)
    again = gpu_ctx.fit_advi(6, 0.1, 7, samples_per_step=3, chain_id0=2, nruns=nruns)
    assert all(np.array_equal(a, b) for a, b in zip(again, (theta, z, elbo)))
    if nruns == 3:
        one = gpu_ctx.fit_advi(6, 0.1, 7, samples_per_step=3, chain_id0=2, nruns=1)
        assert all(np.array_equal(a[..., 0], b[..., 0]) for a, b in zip(one, (theta, z, elbo)))


def test_a_sampler_over_two_passes_of_launches(gpu_ctx):
    """four MALA chains where the budget carries three per pass: StackedVgrad's pass loop, held to the batch entry point"""
    case = gc.PASS_SPLIT
    _setup(gpu_ctx, case)
    z, lp, acc, g = gpu_ctx.sample_mala(4, 0.02, 7, 2, 4, grad=True)
    assert gpu_ctx.mala_kernel_info() == (0, 2)
    _states_are_the_batch_entry_points(gpu_ctx, z, lp, g)
    z1, lp1, _, g1 = gpu_ctx.sample_mala(4, 0.02, 7, 5, 1, grad=True)       # the chain of the second pass, alone
    assert np.array_equal(z1[:, :, 0], z[:, :, 3]) and np.array_equal(lp1[:, 0], lp[:, 3]) and np.array_equal(g1[:, :, 0], g[:, :, 3])


def test_the_sum_over_f_is_the_single_trajectories_sum(gpu_ctx):
    """independence of f on an adaptive case: the f = 7 gradient against the seven f = 1 gradients added on the host.  gw = (sum_p
    slice_p) - 2 W, so a slice comes back as gw_p + 2 W with two roundings of its own; the bound is those roundings and the sums',
    4 f eps sum_p (|gw_p| + 2 |W|) per element, far below any effect of a trajectory's neighbours on its bits' values"""
    case = gc.CASE_BY_NAME["g-ad-tanh-cube"]
    pb = _setup(gpu_ctx, case)
    z = np.asfortranarray(pb.z[:, :1])
    lp7, gw7, _ = gpu_ctx.node_grad(z)
    w = gpu_ctx.reconstruct(z)[:, 0]
    acc, tot = np.zeros(pb.n), np.zeros(pb.n)
    for p in range(case.f):
        gpu_ctx.infer_setup_node([list(r) for r in pb.table], pb.n, case.m, pb.w_swa, pb.p, np.asfortranarray(pb.u0[:, p:p + 1]),
                                 np.asfortranarray(pb.y[:, p:p + 1]), pb.ts, **case.setup_kwargs())
        gpu_ctx.node_set_grad(True)
        gp = gpu_ctx.node_grad(z)[1][:, 0]
        acc, tot = acc + (gp + 2.0 * w), tot + (np.abs(gp) + 2.0 * np.abs(w))
    bound = 4.0 * case.f * np.finfo(np.float64).eps * tot
    print("f = 7 against seven f = 1: worst |difference| / bound %.3f" % float(np.max(np.abs(acc - (gw7[:, 0] + 2.0 * w)) / bound)))
    assert np.all(np.abs(acc - (gw7[:, 0] + 2.0 * w)) <= bound)


def test_sub_inference_hmc_at_the_tutorial_shape(si, gpu_ctx):
    case = nc.CASE_BY_NAME["ad-tutorial"]
    pb = nc.problem(case)
    rng = np.random.default_rng(5)

    def model(**kw):
        return flux.NeuralODE(flux.Chain(flux.cube, flux.Dense(2, 15, "tanh", rng=np.random.default_rng(5)), flux.Dense(15, 2, rng=np.random.default_rng(6))),
                              (0.0, 1.5), pb.ts, reltol=1e-7, abstol=1e-9, max_steps=2000, **kw)
    data = flux.DataLoader(pb.u0, pb.y, batchsize=100)
    p = np.asfortranarray(0.05 * rng.standard_normal((pb.n, 3)))

    def run(**kw):
        return si.sub_inference(model(sensealg="discrete_adjoint"), data, pb.w_swa, p, σ_z=0.1, itr=6, M=3, alg="hmc", ctx=gpu_ctx, seed=4, **kw)
    z, lp = run(return_z=True)
    assert z.shape == (3, 6) and np.all(np.isfinite(lp)) and gpu_ctx.node_grad_info()[0] is True
    assert np.array_equal(gpu_ctx.logdensity(z), lp)
    z2, lp2 = run(return_z=True)
    assert np.array_equal(z2, z) and np.array_equal(lp2, lp)
    zd, lpd = run(return_z=True, device_sampler=True, nchains=2)
    assert zd.shape == (3, 6, 2) and np.all(np.isfinite(lpd))
    for c in range(2):
        assert np.array_equal(gpu_ctx.logdensity(zd[:, :, c]), lpd[:, c])
    with pytest.raises(si.SubspaceError, match="gradient through the ODE solver is not built"):
        si.sub_inference(model(), data, pb.w_swa, p, itr=4, M=3, alg="hmc", ctx=gpu_ctx)


def test_refusals(si, gpu_ctx):
    inval = si._capi.SI_ERR_INVALID
    # the switch is off after every set-up: the old words
    case = gc.SAMPLER
    pb = _setup(gpu_ctx, case, grad=False)
    z = np.zeros((case.m, 2), order="F")
    assert gpu_ctx.node_grad_info() == (False, 0)
    for call in (lambda: gpu_ctx.logdensity_grad(z[:, 0]), lambda: gpu_ctx.logdensity_grad_batch(z), lambda: gpu_ctx.node_grad(z),
                 lambda: gpu_ctx.sample_mala(4, 0.1, 1), lambda: gpu_ctx.sample_hmc(4, 0.1, 1), lambda: gpu_ctx.sample_nuts(4, 0.1, 1),
                 lambda: gpu_ctx.fit_advi(4, 0.1, 1)):
        with pytest.raises(si.SubspaceError, match="not available for NeuralODE models.*si_node_set_grad") as e:
            call()
        assert e.value.code == inval
    gpu_ctx.node_set_grad(True)
    lp_on = gpu_ctx.node_grad(z)[0]
    gpu_ctx.node_set_grad(False)
    with pytest.raises(si.SubspaceError, match="not available for NeuralODE models"):
        gpu_ctx.logdensity_grad(z[:, 0])
    assert np.array_equal(gpu_ctx.logdensity(z), lp_on)
    # a layer wider than 64
    wide = nc.CASE_BY_NAME["ex-d2-h65-p1"]
    _setup(gpu_ctx, wide, nc.problem(wide), grad=False)
    with pytest.raises(si.SubspaceError, match="wider than 64") as e:
        gpu_ctx.node_set_grad(True)
    assert e.value.code == inval and gpu_ctx.node_grad_info() == (False, 0)
    # a record over the budget: f = 100, d = 8, max_steps = 10^6 is 8 GB for one chain
    gpu_ctx.infer_setup_node([[8, 8, 0, 0, 64]], 72, 2, np.zeros(72), np.zeros((72, 2), order="F"), np.zeros((8, 100), order="F"),
                             np.zeros((16, 100), order="F"), np.array([0.5, 1.0]), adaptive=False, dt=0.5, max_steps=1000000)
    with pytest.raises(si.SubspaceError, match="lower max_steps") as e:
        gpu_ctx.node_set_grad(True)
    assert e.value.code == inval and np.all(np.isfinite(gpu_ctx.logdensity(np.zeros((2, 1)))))
    # a Chain set-up drops the switch; so does the next node set-up
    _setup(gpu_ctx, case)
    assert gpu_ctx.node_grad_info()[0] is True
    cp = ra.problem(ra.CASE_BY_NAME["A-M33"])
    gpu_ctx.infer_setup([list(r) for r in cp.table], cp.n, 33, cp.w, cp.p, cp.x, cp.y, cp.sigma_m)
    assert gpu_ctx.node_grad_info() == (False, 0) and gpu_ctx.node_info()[0] is False
    with pytest.raises(si.SubspaceError, match="si_infer_setup_node first"):
        gpu_ctx.node_set_grad(True)
    lp, g = gpu_ctx.logdensity_grad(np.zeros(33))       # (the Chain's own gradient is untouched)
    assert np.isfinite(lp) and np.all(np.isfinite(g))
    _setup(gpu_ctx, case, grad=False)
    assert gpu_ctx.node_grad_info() == (False, 0)
