"""NeuralODE models on the device (si_infer_setup_node, si_node_solve; csrc/kernels_node.hip) against their definition,
subspaceinference_jl_amd/node.py, over the case lists of tests/node_cases.py: the tableau, bit equality wherever no transcendental
function is involved, step counts / statuses and VALUE_TOL (measured on the CPU) where one is, independence of a trajectory's bits
from f / column / C / chain slot, every density entry point, the RWMH samplers audited transition by transition, the failure
path, the decoder bridge, the refusals, and sub_inference at the tutorial's shape."""
import numpy as np
import pytest

from subspaceinference_jl_amd import flux, node
from tests import node_cases as nc
from tests import rwmh_audit as ra

pytestmark = pytest.mark.gpu


def _setup(ctx, case, pb=None, **over):
    pb = nc.problem(case) if pb is None else pb
    kw = case.setup_kwargs()
    kw.update(over)
    ctx.infer_setup_node([list(r) for r in pb.table], pb.n, case.m, pb.w_swa, pb.p, pb.u0, pb.y, pb.ts, **kw)
    return pb


def _definition(case, pb):
    """the definition at every column of pb.z: U (d*S, f, C), sse (f, C), naccept, nreject, status, lp (C)"""
    sols = [nc.definition_at(case, pb, pb.z[:, c]) for c in range(case.C)]
    lp = np.array([(0.0 - (node.sse_total(s.sse) / 0.5) / 2.0) + (0.0 - (node.sum_squares(pb.weights(pb.z[:, c])) / 0.5) / 2.0)
                   for c, s in enumerate(sols)])
    return (np.stack([s.U for s in sols], axis=2), np.stack([s.sse for s in sols], axis=1), np.stack([s.naccept for s in sols], axis=1),
            np.stack([s.nreject for s in sols], axis=1), np.stack([s.status for s in sols], axis=1), lp)


def test_tableau_is_the_definitions(gpu_ctx):
    assert np.array_equal(gpu_ctx.node_tableau(), node.TABLEAU)


@pytest.mark.parametrize("case", nc.EXACT_CASES, ids=lambda c: c.name)
def test_fixed_step_without_transcendentals_is_bit_equal(gpu_ctx, case):
    pb = _setup(gpu_ctx, case)
    assert gpu_ctx.node_info() == (True, case.d, case.S, case.f, node.group_lanes(pb.table))
    for c in range(case.C):
        assert np.array_equal(gpu_ctx.reconstruct(pb.z[:, c:c + 1])[:, 0], pb.weights(pb.z[:, c]))
    u, sse, na, nr, st = gpu_ctx.node_solve(pb.z)
    u_ref, sse_ref, na_ref, nr_ref, st_ref, lp_ref = _definition(case, pb)
    assert np.array_equal(st, st_ref) and not st.any()
    assert np.array_equal(na, na_ref) and np.array_equal(nr, nr_ref) and not nr.any()
    assert np.array_equal(u, u_ref)
    assert np.array_equal(sse, sse_ref)
    assert np.array_equal(gpu_ctx.logdensity(pb.z), lp_ref)


@pytest.mark.parametrize("case", nc.TRANS_CASES + nc.ADAPTIVE_CASES, ids=lambda c: c.name)
def test_transcendental_and_adaptive_cases_hold_counts_and_the_measured_bound(gpu_ctx, case):
    pb = _setup(gpu_ctx, case)
    u, sse, na, nr, st = gpu_ctx.node_solve(pb.z)
    u_ref, sse_ref, na_ref, nr_ref, st_ref, lp_ref = _definition(case, pb)
    assert np.array_equal(st, st_ref) and not st.any()
    assert np.array_equal(na, na_ref) and np.array_equal(nr, nr_ref)
    lp = gpu_ctx.logdensity(pb.z)
    print("%s: spread U %.3e, sse %.3e, lp %.3e (bound %.3e)" % (case.name, nc.spread(u_ref, u), nc.spread(sse_ref, sse), nc.spread(lp_ref, lp),
                                                                  nc.VALUE_TOL))
    assert nc.spread(u_ref, u) <= nc.VALUE_TOL
    assert nc.spread(sse_ref, sse) <= nc.VALUE_TOL
    assert nc.spread(lp_ref, lp) <= nc.VALUE_TOL


def test_a_trajectory_does_not_depend_on_f_column_c_or_chain_slot(gpu_ctx):
    case = nc.CASE_BY_NAME["ad-tutorial"]
    pb = nc.problem(case)
    z = np.asfortranarray(np.repeat(pb.z[:, :1], 9, axis=1))
    z[:, 4] = 0.3                                        # a different neighbour in the middle
    _setup(gpu_ctx, case, pb)
    u9, sse9, na9, nr9, _ = gpu_ctx.node_solve(z)
    for c in (1, 8):                                     # chain slot and C
        assert np.array_equal(u9[:, :, c], u9[:, :, 0]) and np.array_equal(sse9[:, c], sse9[:, 0]) and np.array_equal(na9[:, c], na9[:, 0])
    assert not np.array_equal(u9[:, :, 4], u9[:, :, 0])
    u1, sse1, na1, nr1, _ = gpu_ctx.node_solve(z[:, :1])
    assert np.array_equal(u1[:, :, 0], u9[:, :, 0]) and np.array_equal(sse1[:, 0], sse9[:, 0])
    # other f, other column: trajectories 10 .. 16 alone, in reverse order
    idx = np.arange(16, 9, -1)
    gpu_ctx.infer_setup_node([list(r) for r in pb.table], pb.n, case.m, pb.w_swa, pb.p, np.asfortranarray(pb.u0[:, idx]),
                             np.asfortranarray(pb.y[:, idx]), pb.ts, **case.setup_kwargs())
    us, sses, nas, nrs, _ = gpu_ctx.node_solve(z[:, :1])
    assert np.array_equal(us[:, :, 0], u9[:, idx, 0]) and np.array_equal(sses[:, 0], sse9[idx, 0])
    assert np.array_equal(nas[:, 0], na9[idx, 0]) and np.array_equal(nrs[:, 0], nr9[idx, 0])


def test_forward_and_predict_are_node_solve(gpu_ctx):
    case = nc.CASE_BY_NAME["ad-d3-wide"]
    pb = _setup(gpu_ctx, case)
    u = gpu_ctx.node_solve(pb.z)[0]
    assert np.array_equal(gpu_ctx.forward(pb.z[:, 2]), u[:, :, 2])
    assert np.array_equal(gpu_ctx.predict(pb.z, pb.u0), u)
    assert np.array_equal(gpu_ctx.predict(pb.z[:, 3:5], np.asfortranarray(pb.u0[:, 1:])), u[:, 1:, 3:5])   # new initial states: another Bn


# ---- RWMH --------------------------------------------------------------------------------------------------------------------------
def _audit(case, pb, z, lp, acc, w=None):
    rep = ra.audit(z, lp, acc, nc.density(case, pb), nc.RWMH["sigma_z"], nc.RWMH["seed"], nc.RWMH["chain_id0"], ra.LP_RTOL_F64, W=w,
                   reconstruct=(lambda zz: pb.weights(np.asarray(zz))) if w is not None else None)
    ra.check_caps(rep)
    return rep


def test_rwmh_is_audited_transition_by_transition(gpu_ctx):
    case, r = nc.RWMH_FIXED, nc.RWMH
    pb = _setup(gpu_ctx, case)
    z3, lp3, acc3 = gpu_ctx.sample_rwmh(r["itr"], r["sigma_z"], r["seed"], r["chain_id0"], 3)
    _audit(case, pb, z3, lp3, acc3)
    for c in range(3):   # the definition's lp at the returned z, bit for bit (no transcendental in the density)
        assert np.array_equal(lp3[:, c], [nc.density(case, pb)(z3[:, t, c]) for t in range(r["itr"])])
    # the step-wise session
    gpu_ctx.rwmh_begin(r["itr"], r["sigma_z"], r["seed"], r["chain_id0"], 3)
    for _ in range(r["itr"]):
        gpu_ctx.rwmh_step_accept(gpu_ctx.rwmh_step_eval())
    zs, lps, accs = gpu_ctx.rwmh_end()
    assert np.array_equal(zs, z3) and np.array_equal(lps, lp3) and np.array_equal(accs, acc3)
    # nine stacked chains: the first three are the three above
    z9, lp9, acc9 = gpu_ctx.sample_rwmh(r["itr"], r["sigma_z"], r["seed"], r["chain_id0"], 9)
    _audit(case, pb, z9, lp9, acc9)
    assert np.array_equal(z9[:, :, :3], z3) and np.array_equal(lp9[:, :3], lp3)
    # the output map, and the same bits twice
    zw, lpw, accw, w = gpu_ctx.sample_rwmh_weights(r["itr"], r["sigma_z"], r["seed"], r["chain_id0"], 3)
    assert np.array_equal(zw, z3) and np.array_equal(lpw, lp3) and np.array_equal(accw, acc3)
    for c in range(3):
        assert np.array_equal(w[:, :, c], gpu_ctx.reconstruct(zw[:, :, c]))
    _audit(case, pb, zw, lpw, accw, w)
    again = gpu_ctx.sample_rwmh(r["itr"], r["sigma_z"], r["seed"], r["chain_id0"], 3)
    assert np.array_equal(again[0], z3) and np.array_equal(again[1], lp3) and np.array_equal(again[2], acc3)


def test_rwmh_adaptive_lp_is_logdensity_at_the_returned_z(gpu_ctx):
    case, r = nc.RWMH_ADAPTIVE, nc.RWMH
    _setup(gpu_ctx, case)
    z, lp, acc = gpu_ctx.sample_rwmh(r["itr"], r["sigma_z"], r["seed"], r["chain_id0"], 2)
    assert 0.0 < acc.min() and acc.max() < 1.0
    for c in range(2):
        assert np.array_equal(lp[:, c], gpu_ctx.logdensity(z[:, :, c]))
    zw, lpw, accw, w = gpu_ctx.sample_rwmh_weights(r["itr"], r["sigma_z"], r["seed"], r["chain_id0"], 2)
    assert np.array_equal(zw, z) and np.array_equal(lpw, lp)
    for c in range(2):
        assert np.array_equal(w[:, :, c], gpu_ctx.reconstruct(z[:, :, c]))


@pytest.mark.parametrize("case,status", [(nc.FAIL_STEPS, 1), (nc.FAIL_BLOWUP, 2)], ids=["max-steps", "blow-up"])
def test_a_failed_trajectory_is_minus_infinity_and_a_rejected_proposal(gpu_ctx, case, status):
    pb = _setup(gpu_ctx, case)
    u, sse, na, nr, st = gpu_ctx.node_solve(pb.z)
    st_ref = _definition(case, pb)[4]
    # (these cases are not on the certified list: statuses, sums and densities are held to the definition, step counts are not)
    assert np.array_equal(st, st_ref) and (st == status).all()
    assert np.all(np.isposinf(sse)) and np.isnan(u).any(axis=0).all() and np.all(na + nr <= case.max_steps)
    assert np.all(np.isneginf(gpu_ctx.logdensity(pb.z)))
    # every point fails: step 0 is kept as always, every later proposal is rejected
    z, lp, acc = gpu_ctx.sample_rwmh(8, 0.3, 5, 0, 2)
    assert np.all(np.isneginf(lp)) and np.all(acc == 0.0) and np.all(z == z[:, :1, :])


@pytest.mark.parametrize("chain_id0", [2, 4])
def test_a_failing_proposal_from_a_finite_state_is_rejected(gpu_ctx, chain_id0):
    """max_steps = 50: the chain starts where every trajectory integrates and meets proposals whose trajectories do not"""
    from oracle import philox
    case, r = nc.FAIL_PROPOSAL, nc.FAIL_PROPOSAL_RWMH
    pb = _setup(gpu_ctx, case, nc.fail_proposal_problem())
    z, lp, acc = gpu_ctx.sample_rwmh(r["itr"], r["sigma_z"], r["seed"], chain_id0, 1)
    assert np.all(np.isfinite(lp)) and 0.0 < acc[0] < 1.0
    ra.audit(z, lp, acc, nc.density(case, pb), r["sigma_z"], r["seed"], chain_id0, ra.LP_RTOL_F64)
    zp = np.asfortranarray(np.stack([z[:, t - 1, 0] + r["sigma_z"] * philox.normals(r["seed"], chain_id0, t, case.m)
                                     for t in range(1, r["itr"])], axis=1))
    _, sse, _, _, st = gpu_ctx.node_solve(zp, want_u=False)
    st_ref = np.stack([nc.definition_at(case, pb, zp[:, j]).status for j in range(zp.shape[1])], axis=1)
    failed = (st != 0).any(axis=0)
    assert np.array_equal(st, st_ref) and failed.sum() >= 3 and np.array_equal(np.isinf(sse), st != 0)
    assert np.all(np.isneginf(gpu_ctx.logdensity(zp)[failed]))
    for j in np.flatnonzero(failed):     # proposal j + 1 failed from the finite state z[:, j]: the chain stays, bit for bit
        assert np.array_equal(z[:, j + 1, 0], z[:, j, 0]) and lp[j + 1, 0] == lp[j, 0]


def test_identity_decoder_is_the_p_route(gpu_ctx):
    case = nc.RWMH_ADAPTIVE
    pb = _setup(gpu_ctx, case)
    z = np.asfortranarray(np.random.default_rng(3).standard_normal((case.m, 3)))

    def calls():
        return gpu_ctx.reconstruct(z), gpu_ctx.logdensity(z), gpu_ctx.node_solve(z)[0], gpu_ctx.sample_rwmh(9, 0.5, 3, 1, 2)
    w0, lp0, u0, s0 = calls()
    gpu_ctx.set_decoder([(case.m, pb.n, flux.identity, 0, pb.n * case.m)], np.concatenate([pb.p.reshape(-1, order="F"), np.zeros(pb.n)]))
    w1, lp1, u1, s1 = calls()
    gpu_ctx.set_decoder(None, None)
    assert np.array_equal(w1, w0) and np.array_equal(lp1, lp0) and np.array_equal(u1, u0)
    assert all(np.array_equal(a, b) for a, b in zip(s1, s0))


def test_refusals(si, gpu_ctx):
    case = nc.RWMH_FIXED
    pb = nc.problem(case)
    table = [list(r) for r in pb.table]

    def refused(needle, table=table, n=pb.n, u0=pb.u0, y=pb.y, ts=pb.ts, **over):
        kw = case.setup_kwargs()
        kw.update(over)
        with pytest.raises(si.SubspaceError) as e:
            gpu_ctx.infer_setup_node(table, n, case.m, np.zeros(n), np.zeros((n, case.m), order="F"), u0, y, ts, **kw)
        assert e.value.code == si._capi.SI_ERR_INVALID and needle in str(e.value), str(e.value)
    refused("1 to 8 Dense layers", table=[[2, 2, 0, 0, 4]] * 9, n=6)
    refused("d must be 1 to 8", table=[[9, 9, 0, 0, 81]], n=90, u0=np.zeros((9, 3)), y=np.zeros((36, 3)))
    refused("widths must be 1 to 256", table=[[2, 257, 0, 0, 514], [257, 2, 0, 771, 1285]], n=1287)
    refused("N must be 1 to 8192", table=[[2, 256, 0, 0, 512]] + [[256, 256, 0, 0, 0]] + [[256, 2, 0, 0, 0]], n=8193)
    refused("do not chain", table=[[2, 3, 0, 0, 6], [4, 2, 0, 9, 17]], n=19)
    refused("must map d to d", table=[[2, 3, 0, 0, 6]], n=9)
    refused("offset range", table=[[2, 3, 0, 0, 6], [3, 2, 0, 9, 16]], n=17)
    refused("unknown activation", table=[[2, 3, 9, 0, 6], [3, 2, 0, 9, 15]])
    refused("strictly ascending", ts=np.array([0.0, 0.5, 0.5, 1.0]))
    refused("not before t0", ts=np.array([-0.1, 0.5, 0.7, 1.0]))
    refused("pre_power", pre_power=2)
    refused("max_steps", max_steps=1000001)
    refused("dt must be finite and positive", dt=0.0)
    refused("reltol and abstol", adaptive=True, reltol=0.0)
    refused("reltol and abstol", adaptive=True, abstol=float("inf"))
    with pytest.raises(si.SubspaceError, match="save times S must be 1 to 4096"):
        gpu_ctx.infer_setup_node([[1, 1, 0, 0, 1]], 2, 1, np.zeros(2), np.zeros((2, 1)), np.zeros((1, 1)), np.zeros((4097, 1)),
                                 np.arange(4097.0), adaptive=False, dt=1.0)
    # what a node set-up does not offer
    _setup(gpu_ctx, case)
    z = np.zeros((case.m, 2), order="F")
    for call in (lambda: gpu_ctx.logdensity_grad(z[:, 0]), lambda: gpu_ctx.logdensity_grad_batch(z), lambda: gpu_ctx.sample_mala(4, 0.1, 1),
                 lambda: gpu_ctx.sample_hmc(4, 0.1, 1), lambda: gpu_ctx.sample_nuts(4, 0.1, 1), lambda: gpu_ctx.fit_advi(4, 0.1, 1),
                 lambda: gpu_ctx.set_prior(0.5), lambda: gpu_ctx.rwmh_begin(4, 0.1, 1, 0, 1, 24)):
        with pytest.raises(si.SubspaceError, match="not available for NeuralODE models") as e:
            call()
        assert e.value.code == si._capi.SI_ERR_INVALID
    assert np.all(np.isfinite(gpu_ctx.logdensity(z)))   # the set-up is still there


def test_a_chain_setup_after_a_node_setup_keeps_its_density(gpu_ctx):
    pb = ra.problem(ra.CASE_BY_NAME["A-M33"])
    z = np.asfortranarray(np.random.default_rng(0).standard_normal((33, 3)) * 0.1)

    def chain():
        gpu_ctx.infer_setup([list(r) for r in pb.table], pb.n, 33, pb.w, pb.p, pb.x, pb.y, pb.sigma_m)
        assert gpu_ctx.node_info()[0] is False
        return gpu_ctx.logdensity(z), gpu_ctx.sample_rwmh(12, 0.05, 11, 2, 2)
    lp0, s0 = chain()
    _setup(gpu_ctx, nc.RWMH_FIXED)
    assert gpu_ctx.node_info()[0] is True
    lp1, s1 = chain()
    assert np.array_equal(lp1, lp0) and all(np.array_equal(a, b) for a, b in zip(s1, s0))
    gpu_ctx.set_prior(0.7)   # (a Chain set-up takes the prior again)
    gpu_ctx.set_prior(0.0)


def test_sub_inference_at_the_tutorial_shape(si, gpu_ctx):
    case = nc.CASE_BY_NAME["ad-tutorial"]
    pb = nc.problem(case)
    rng = np.random.default_rng(5)
    model = flux.NeuralODE(flux.Chain(flux.cube, flux.Dense(2, 15, "tanh", rng=rng), flux.Dense(15, 2, rng=rng)), (0.0, 1.5), pb.ts,
                           reltol=1e-7, abstol=1e-9)
    data = flux.DataLoader(pb.u0, pb.y, batchsize=100)
    p = np.asfortranarray(0.05 * rng.standard_normal((pb.n, 3)))

    def run(**kw):
        return si.sub_inference(model, data, pb.w_swa, p, σ_z=0.3, itr=20, M=3, alg="rwmh", ctx=gpu_ctx, seed=4, **kw)
    z, lp = run(return_z=True)
    z2, lp2 = run(return_z=True)
    assert z.shape == (3, 20) and np.array_equal(z2, z) and np.array_equal(lp2, lp)
    assert np.array_equal(gpu_ctx.logdensity(z), lp) and np.all(np.isfinite(lp))
    chn, lpw = run()
    assert np.array_equal(lpw, lp) and np.array_equal(np.stack(chn, axis=1), gpu_ctx.reconstruct(z))
    zc, lpc = run(return_z=True, nchains=2)
    assert np.array_equal(zc[:, :, 0], z) and np.array_equal(lpc[:, 0], lp)
    for alg in ("mala", "hmc", "nuts"):
        with pytest.raises(si.SubspaceError, match="gradient through the ODE solver is not built"):
            si.sub_inference(model, data, pb.w_swa, p, itr=4, M=3, alg=alg, ctx=gpu_ctx)
