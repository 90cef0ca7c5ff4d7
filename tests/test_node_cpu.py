"""The NeuralODE definition (subspaceinference_jl_amd/node.py) on the CPU alone: the Tsit5 tableau's order conditions and its
interpolant's, convergence of order 5 and accuracy against scipy's DOP853, a linear problem against expm, the termination
statuses, the certification of the adaptive case list that tests/test_gpu_node.py runs on the device (no decision near err = 1,
identical step counts under a few ulp of libm), the measured value tolerance, and the API's argument errors."""
import numpy as np
import pytest
from scipy.integrate import solve_ivp
from scipy.linalg import expm

import subspaceinference_jl_amd as si
from oracle import subspace_oracle as so
from subspaceinference_jl_amd import flux, node
from tests import node_cases as nc
from tests import rwmh_audit as ra

C = np.array(node.C)
A = np.zeros((7, 7))
for _i, _row in enumerate(node.A):
    A[_i, :len(_row)] = _row
B = A[6].copy()
BT = np.array(node.BT)


def _conditions(b, order, th=1.0):
    """the rooted-tree conditions up to `order` for weights b, at theta (continuous form: right-hand sides scaled by theta^r)"""
    ac = A @ C
    out = [b.sum() - th]
    if order >= 2:
        out += [b @ C - th ** 2 / 2]
    if order >= 3:
        out += [b @ C ** 2 - th ** 3 / 3, b @ ac - th ** 3 / 6]
    if order >= 4:
        out += [b @ C ** 3 - th ** 4 / 4, b @ (C * ac) - th ** 4 / 8, b @ (A @ C ** 2) - th ** 4 / 12, b @ (A @ ac) - th ** 4 / 24]
    if order >= 5:
        out += [b @ C ** 4 - 1 / 5, b @ (C ** 2 * ac) - 1 / 10, b @ (C * (A @ C ** 2)) - 1 / 15, b @ (C * (A @ ac)) - 1 / 30, b @ (ac * ac) - 1 / 20,
                b @ (A @ C ** 3) - 1 / 20, b @ (A @ (C * ac)) - 1 / 40, b @ (A @ (A @ C ** 2)) - 1 / 60, b @ (A @ (A @ ac)) - 1 / 120]
    return np.abs(np.array(out))


def test_tableau_meets_the_order_conditions():
    assert np.abs(A.sum(axis=1) - C).max() <= 1e-14
    assert len(_conditions(B, 5)) == 17 and _conditions(B, 5).max() <= 1e-14
    for s in (1.0, -1.0):   # the embedded method b +- b~ is of order 4 and not of order 5
        assert _conditions(B + s * BT, 4).max() <= 1e-14
        assert _conditions(B + s * BT, 5).max() > 1e-6
    assert node.TABLEAU.shape == (57,) and np.array_equal(node.TABLEAU[:7], C) and np.array_equal(node.TABLEAU[28:35], BT)


def test_interpolant_meets_the_continuous_order_four_conditions():
    for th in np.linspace(0.0, 1.0, 41)[1:]:
        b = np.array(node.interp_weights(th))
        assert _conditions(b, 4, th).max() <= 1e-14, th
    assert np.abs(np.array(node.interp_weights(1.0)) - B).max() <= 1e-14


# ---- the tutorial's network: x.^3 -> Dense(2, 15, tanh) -> Dense(15, 2) ------------------------------------------------------------
def _tutorial(f=3, seed=0):
    rng = np.random.default_rng(seed)
    table = [(2, 15, flux.tanh, 0, 30), (15, 2, flux.identity, 45, 75)]
    w = 0.5 * rng.standard_normal(77)
    u0 = rng.standard_normal((2, f))
    return table, w, u0, np.linspace(0.0, 1.5, 30)


def _dop853(table, w, u0, ts, pre_power):
    def f(t, u):
        return node.rhs(table, w, u.reshape(-1, 1), pre_power)[:, 0]
    cols = [solve_ivp(f, (0.0, ts[-1]), u0[:, j], method="DOP853", rtol=1e-13, atol=1e-13, t_eval=ts).y for j in range(u0.shape[1])]
    return np.stack([c.reshape(-1) for c in cols], axis=1)   # row i*S + s


def test_fixed_step_convergence_is_of_order_five():
    table, w, u0, ts = _tutorial()
    ref = _dop853(table, w, u0, ts, 3)
    err = [np.abs(node.solve(table, w, u0, ts, node.Opts(adaptive=0, dt=h, pre_power=3)).U - ref).max() for h in (0.05, 0.025, 0.0125)]
    print("errors", err, "ratios", err[0] / err[1], err[1] / err[2])
    assert 20.0 <= err[0] / err[1] <= 45.0 and 20.0 <= err[1] / err[2] <= 45.0


def test_linear_problem_against_expm():
    m = np.array([[-0.3, 1.1], [-1.1, -0.2]])
    table = [(2, 2, flux.identity, 0, 4)]
    w = np.concatenate([m.reshape(-1, order="F"), np.zeros(2)])
    u0 = np.array([[1.0, -0.5], [0.25, 2.0]])
    ts = np.array([0.3, 1.0, 2.0])
    sol = node.solve(table, w, u0, ts, node.Opts(reltol=1e-10, abstol=1e-12))
    ref = np.stack([np.stack([expm(m * t) @ u0[:, j] for t in ts], axis=1).reshape(-1) for j in range(2)], axis=1)
    assert not sol.status.any() and np.abs(sol.U - ref).max() <= 1e-8


def test_adaptive_definition_against_dop853():
    table, w, u0, ts = _tutorial(f=5, seed=1)
    ref = _dop853(table, w, u0, ts, 3)
    for tol in (1e-5, 1e-7, 1e-9):
        sol = node.solve(table, w, u0, ts, node.Opts(reltol=tol, abstol=tol * 1e-2, pre_power=3))
        ratio = np.abs(sol.U - ref).max() / tol
        print("reltol %g: error / tolerance %.3f, accepted %.1f, rejected %.1f" % (tol, ratio, sol.naccept.mean(), sol.nreject.mean()))
        assert not sol.status.any() and ratio <= 10.0   # (global error within a small multiple of the local tolerance on this problem)


def test_statuses_one_and_two_are_reached():
    for case, status in ((nc.FAIL_STEPS, 1), (nc.FAIL_BLOWUP, 2)):
        pb = nc.problem(case)
        sol = nc.definition_at(case, pb, pb.z[:, 0])
        assert (sol.status == status).all(), (case.name, sol.status)
        assert np.all(np.isposinf(sol.sse)) and np.isnan(sol.U).any(axis=0).all()
        assert np.isneginf(nc.density(case, pb)(pb.z[:, 0]))
    sol = nc.definition_at(nc.FAIL_STEPS, nc.problem(nc.FAIL_STEPS), nc.problem(nc.FAIL_STEPS).z[:, 0])
    assert np.all(sol.naccept + sol.nreject == nc.FAIL_STEPS.max_steps)


@pytest.mark.parametrize("case", nc.ADAPTIVE_CASES + [nc.RWMH_ADAPTIVE], ids=lambda c: c.name)
def test_adaptive_cases_are_certified(case):
    """no decision within MIN_MARGIN of err = 1, and the same step counts with every transcendental result moved by +-4 ulp"""
    pb = nc.problem(case)
    for c in range(case.C):
        base = nc.definition_at(case, pb, pb.z[:, c])
        assert not base.status.any() and base.min_margin >= nc.MIN_MARGIN, (case.name, c, base.min_margin)
        for seed in (1, 2):
            nud = nc.definition_at(case, pb, pb.z[:, c], nudge=node.Nudge(4, seed))
            assert np.array_equal(nud.naccept, base.naccept) and np.array_equal(nud.nreject, base.nreject) and not nud.status.any()
    if case.name == "ad-tutorial":
        assert base.nreject.sum() > 0   # the list reaches the reject branch


def test_value_tolerance_is_the_measured_spread_times_eight():
    worst, where = 0.0, None
    for case in nc.TRANS_CASES + nc.ADAPTIVE_CASES:
        pb = nc.problem(case)
        for c in range(case.C):
            base = nc.definition_at(case, pb, pb.z[:, c])
            for seed in (1, 2):
                nud = nc.definition_at(case, pb, pb.z[:, c], nudge=node.Nudge(2, seed))
                s = max(nc.spread(base.U, nud.U), nc.spread(base.sse, nud.sse), nc.spread(node.sse_total(base.sse), node.sse_total(nud.sse)))
                if s > worst:
                    worst, where = s, case.name
    print("largest spread under +-2 ulp: %.3e (%s); VALUE_TOL = %.3e" % (worst, where, nc.VALUE_TOL))
    # the constant is the measurement (the nudges are seeded: it is deterministic), rounded up in its second digit
    assert worst <= nc.MEASURED_SPREAD <= 1.1 * worst
    assert nc.VALUE_TOL == 8 * nc.MEASURED_SPREAD


def test_exact_cases_cover_the_shape_list():
    cs = nc.EXACT_CASES
    assert {c.d for c in cs} == {1, 2, 3} and {len(c.hidden) + 1 for c in cs} == {1, 2, 3}
    assert {w for c in cs for w in c.hidden} >= {1, 3, 15, 16, 17, 65}
    assert {c.S for c in cs} >= {1, 2, 5, 30} and {c.f for c in cs} >= {1, 3, 64, 65} and {c.C for c in cs} >= {1, 2, 9}
    assert {c.pre_power for c in cs} == {1, 3} and {c.t_first > c.t0 for c in cs} == {True, False}
    assert {a for c in nc.ALL_CASES for a in c.acts} == set(range(8))
    for c in cs:
        assert all(a in (nc.I, nc.R, nc.LR) for a in c.acts) and not c.adaptive
    sol = nc.definition_at(nc.CASE_BY_NAME["ex-saves-in-step"], nc.problem(nc.CASE_BY_NAME["ex-saves-in-step"]), np.zeros(2))
    assert sol.naccept.max() == 4 and not sol.status.any()      # 30 save times in 4 steps


@pytest.mark.parametrize("case", nc.ALL_CASES + [nc.RWMH_FIXED, nc.RWMH_ADAPTIVE], ids=lambda c: c.name)
def test_every_listed_case_finishes_on_the_definition(case):
    pb = nc.problem(case)
    for c in range(case.C):
        sol = nc.definition_at(case, pb, pb.z[:, c])
        assert not sol.status.any() and np.all(np.isfinite(sol.U)) and np.all(np.isfinite(sol.sse))
        assert (sol.nreject == 0).all() or case.adaptive


@pytest.mark.parametrize("chain", [2, 4])
def test_failing_proposal_case_is_what_it_claims(chain):
    """a finite start, at least three proposals that fail from a finite state and are rejected, and the same statuses at +-4 ulp"""
    from oracle import philox
    case, r, pb = nc.FAIL_PROPOSAL, nc.FAIL_PROPOSAL_RWMH, nc.fail_proposal_problem()
    dens = nc.density(case, pb)
    z, lp, nacc = so.rwmh(dens, case.m, r["itr"], r["sigma_z"], r["seed"], chain=chain)
    assert np.all(np.isfinite(lp)) and 0 < nacc < r["itr"] - 1
    ra.audit(z[:, :, None], lp[:, None], np.array([nacc / (r["itr"] - 1)]), dens, r["sigma_z"], r["seed"], chain, ra.LP_RTOL_F64)
    failed = 0
    for t in range(1, r["itr"]):
        zp = z[:, t - 1] + r["sigma_z"] * philox.normals(r["seed"], chain, t, case.m)
        sol = nc.definition_at(case, pb, zp)
        for seed in (1, 2):
            assert np.array_equal(nc.definition_at(case, pb, zp, nudge=node.Nudge(4, seed)).status, sol.status)
        if sol.status.any():
            failed += 1
            assert set(sol.status) <= {0, 1, 2} and np.array_equal(z[:, t], z[:, t - 1]) and lp[t] == lp[t - 1]
    assert failed >= 3


def test_rwmh_case_reaches_both_branches_on_the_definition():
    case, r = nc.RWMH_FIXED, nc.RWMH
    pb = nc.problem(case)
    dens = nc.density(case, pb)
    for c in range(9):
        z, lp, nacc = so.rwmh(dens, case.m, r["itr"], r["sigma_z"], r["seed"], chain=r["chain_id0"] + c)
        rep = ra.audit(z[:, :, None], lp[:, None], np.array([nacc / (r["itr"] - 1)]), dens, r["sigma_z"], r["seed"], r["chain_id0"] + c, ra.LP_RTOL_F64)
        ra.check_caps(rep)


def test_sum_squares_and_the_density_formula():
    rng = np.random.default_rng(0)
    for n in (1, 77, 256, 257, 8192):
        w = rng.standard_normal(n)
        assert abs(node.sum_squares(w) - w @ w) <= 1e-13 * (w @ w)
    case = nc.RWMH_FIXED
    pb = nc.problem(case)
    w = pb.weights(pb.z[:, 0])
    sol = nc.definition_at(case, pb, pb.z[:, 0])
    assert nc.density(case, pb)(pb.z[:, 0]) == -node.sse_total(sol.sse) - node.sum_squares(w)
    assert node.group_lanes(pb.table) == 4 and node.group_lanes([(2, 65, 0, 0, 0), (65, 2, 0, 0, 0)]) == 64


def test_argument_errors():
    table = [(2, 3, flux.relu, 0, 6), (3, 2, flux.identity, 9, 15)]
    ts = np.array([0.5, 1.0])
    ok = node.Opts()
    node.check(table, 17, 2, ts, ok)
    for needle, args in (("1 to 8 Dense layers", ([], 17, 2, ts, ok)), ("d must be 1 to 8", (table, 17, 9, ts, ok)),
                         ("N must be 1 to 8192", (table, 8193, 2, ts, ok)), ("do not chain", (table, 17, 3, ts, ok)),
                         ("must map d to d", (table[:1], 17, 2, ts, ok)), ("offset range", (table, 16, 2, ts, ok)),
                         ("strictly ascending", (table, 17, 2, ts[::-1], ok)), ("not before t0", (table, 17, 2, ts, node.Opts(t0=0.6))),
                         ("pre_power", (table, 17, 2, ts, node.Opts(pre_power=2))), ("max_steps", (table, 17, 2, ts, node.Opts(max_steps=1000001))),
                         ("reltol and abstol", (table, 17, 2, ts, node.Opts(reltol=-1.0))),
                         ("dt must be finite and positive", (table, 17, 2, ts, node.Opts(adaptive=0))),
                         ("S must be 1 to 4096", (table, 17, 2, np.arange(4097.0), ok))):
        with pytest.raises(si.SubspaceError, match=needle):
            node.check(*args)
    node.check(table, 17, 2, ts, node.Opts(max_steps=0))   # 0 is the default of 100 000, as in the C ABI
    u = np.ones((2, 1))
    w17 = 0.1 * np.arange(17.0)
    assert np.array_equal(node.solve(table, w17, u, ts, node.Opts(max_steps=0)).U, node.solve(table, w17, u, ts, node.Opts()).U)
    # the model class and the API
    with pytest.raises(si.SubspaceError, match="Dense layers"):
        flux.NeuralODE(flux.Chain(flux.Dense(2, 2), flux.cube), (0.0, 1.0), ts)
    with pytest.raises(si.SubspaceError, match="must be a Chain"):
        flux.NeuralODE(flux.Dense(2, 2), (0.0, 1.0), ts)
    model = flux.NeuralODE(flux.Chain(flux.cube, flux.Dense(2, 3, "tanh"), flux.Dense(3, 2)), (0.0, 1.0), 0.25, reltol=1e-7, abstol=1e-9)
    assert model.pre_power == 3 and np.array_equal(model.saveat, [0.0, 0.25, 0.5, 0.75, 1.0]) and len(flux.params(model)) == 4
    flux.load_flat(model, np.arange(17.0))
    assert model.dudt.layers[1].W[1, 0] == 1.0 and model(np.ones((2, 3))).shape == (10, 3)
    data = flux.DataLoader(np.ones((2, 3)), np.ones((10, 3)), batchsize=3)
    for alg in ("mala", "hmc", "nuts", "advi"):
        with pytest.raises(si.SubspaceError, match="gradient through the ODE solver is not built"):
            si.sub_inference(model, data, np.zeros(17), np.zeros((17, 3)), alg=alg, device_loop=(alg == "advi"))
    with pytest.raises(si.SubspaceError, match="include_prior"):
        si.sub_inference(model, data, np.zeros(17), np.zeros((17, 3)), include_prior=True)
    for fn in (si.subspace_construction, si.diffusion_subspace, si.subspace_inference):
        with pytest.raises(si.SubspaceError, match="through the solver is out of scope"):
            fn(model, flux.mse, data, flux.Descent(), verbose=False)
    enc, dec = flux.Chain(flux.Dense(17, 3)), flux.Chain(flux.Dense(3, 17))
    with pytest.raises(si.SubspaceError, match="through the solver is out of scope"):
        si.auto_encoder_subspace(model, flux.mse, data, flux.Descent(), enc, dec, verbose=False)
