"""The gradient through the NeuralODE solver on its definition alone (subspaceinference_jl_amd/node.py: solve(record=True), replay,
grad_w, logdensity_grad) over the lists of tests/node_grad_cases.py: the replay is the solve, the gradient is the derivative of the
replayed density (Richardson-extrapolated central differences, each case to its own measured bound), a catalogue of wrong
adjoints that the bound must catch, the measured constants held to fresh measurements, the adaptive cases' certification, and
the API's switch.  No GPU needed."""
import numpy as np
import pytest

import subspaceinference_jl_amd as si
from subspaceinference_jl_amd import flux, node
from tests import node_cases as nc
from tests import node_grad_cases as gc


@pytest.mark.parametrize("case", gc.ALL_CASES + [gc.SAMPLER], ids=lambda c: c.name)
def test_replay_is_the_solve(case):
    pb = gc.problem(case)
    for c in range(case.C):
        sol = gc.recorded(case, c)
        assert not sol.status.any() and sol.naccept.max() <= gc.MAX_STEPS_SEEN
        plain = nc.definition_at(case, pb, pb.z[:, c])
        assert np.array_equal(sol.U, plain.U) and np.array_equal(sol.sse, plain.sse)       # recording changes nothing
        assert [r.t.size for r in sol.record] == list(sol.naccept) and all(r.status == 0 for r in sol.record)
        u, sse = node.replay(pb.table, gc.weights(case, c), pb.u0, pb.ts, case.opts(), sol.record, y=pb.y)
        assert np.array_equal(u, sol.U) and np.array_equal(sse, sol.sse)
        for p, r in enumerate(sol.record):      # step n + 1 starts where step n ended; the last step ends at the last save time
            assert np.array_equal(r.t[1:], (r.t + r.hs)[:-1]) and (r.t.size == 0 or r.t[0] == case.t0)
            assert r.u.shape == (case.d, r.t.size) and (r.t.size == 0 or np.array_equal(r.u[:, 0], pb.u0[:, p]))


def test_the_lists_cover_the_shape_list():
    cs = gc.EXACT_CASES + [gc.PASS_SPLIT]
    assert {w for c in cs for w in c.hidden} >= {1, 3, 5, 15, 64} and (3, 5) in {c.hidden for c in cs}
    assert {c.d for c in cs} >= {1, 8} and {c.f for c in gc.ALL_CASES} >= {1, 3, 5, 7} and {c.pre_power for c in cs} == {1, 3}
    assert all(c.f <= 7 and c.S <= 6 and max(c.hidden) <= node.GRAD_MAX_WIDTH for c in gc.ALL_CASES)
    assert all(all(a in (gc.I, gc.R, gc.LR) for a in c.acts) and not c.adaptive for c in cs)
    for c in gc.ALL_CASES:                      # f is no multiple of the trajectories per workgroup
        assert c.f % (256 // node.group_lanes(gc.problem(c).table)) != 0
    one = gc.CASE_BY_NAME["g-s1-at-t0"]
    assert one.S == 1 and gc.problem(one).ts[0] == one.t0 and gc.recorded(one).naccept.max() == 0
    several = gc.recorded(gc.CASE_BY_NAME["g-saves-in-step"])
    assert several.naccept.max() == 2           # five save times after t0 in two steps, the last one at the second step's end
    ends = gc.recorded(gc.CASE_BY_NAME["g-saves-at-ends"]).record[0]
    assert np.array_equal(ends.t + ends.hs, gc.problem(gc.CASE_BY_NAME["g-saves-at-ends"]).ts[1:])
    short = gc.recorded(gc.CASE_BY_NAME["g-w15"]).record[0]
    assert short.hs[-1] < short.h[-1] and np.array_equal(short.hs[:-1], short.h[:-1])       # a shortened last step
    assert gc.recorded(gc.CASE_BY_NAME["g-ad-tanh-cube"]).min_margin < np.inf
    # d = 8, f = 7, max_steps = 10^6: three chains per pass under the 2 GiB budget, C = 4
    ps = gc.PASS_SPLIT
    per_chain = 8.0 * ps.f * (ps.max_steps * (ps.d + 2) + gc.problem(ps).n)
    assert int(2.0 ** 31 // per_chain) == 3 and ps.C == 4


def test_without_integration_the_gradient_is_minus_two_w():
    case = gc.CASE_BY_NAME["g-s1-at-t0"]
    pb = gc.problem(case)
    lp, gw = gc.definition(case)
    for c in range(case.C):
        assert np.array_equal(gw[:, c], -2.0 * pb.weights(pb.z[:, c]))


@pytest.mark.parametrize("case", gc.ALL_CASES, ids=lambda c: c.name)
def test_gradient_against_extrapolated_central_differences(case):
    err, dis = gc.fd_error(case)
    print("%s: |g.v - fd| %.3e, disagreement of the two finest levels %.3e (held %.3e), bound %.3e"
          % (case.name, err, dis, gc.FD_DISAGREEMENT[case.name], gc.FD_TOL[case.name]))
    # the constant is the measurement (seeded, deterministic), rounded up: within 10 % above a fresh one
    assert dis <= gc.FD_DISAGREEMENT[case.name] <= 1.1 * dis
    assert gc.FD_TOL[case.name] == 8 * gc.FD_DISAGREEMENT[case.name]
    assert err <= gc.FD_TOL[case.name]


def test_every_mutant_is_caught_a_hundredfold():
    """each wrong adjoint exceeds a case's bound by at least MUTANT_FACTOR on at least one listed case"""
    cases = [c for c in gc.ALL_CASES if gc.FD_TOL[c.name] > 0.0]
    report = {}
    for m in node.MUTANTS:
        best = max(((gc.fd_error(c, mutant=m)[0] / gc.FD_TOL[c.name], c.name) for c in cases))
        report[m] = best
        print("%-26s %.3e x the bound on %s" % (m, best[0], best[1]))
    missed = [m for m, (r, _) in report.items() if not r >= gc.MUTANT_FACTOR]
    assert not missed, missed
    assert set(report) == {"interp-k7-dropped", "k1-dropped", "h-for-hs", "theta-of-wrong-step", "cube-derivative-missing", "end-save-twice"}
    with pytest.raises(si.SubspaceError, match="unknown mutant"):
        gc.fd_error(cases[0], mutant="none-such")


def test_grad_tolerance_is_the_measured_spread_times_eight():
    worst, where = 0.0, None
    for case in gc.TRANS_CASES + gc.ADAPTIVE_CASES:
        pb = gc.problem(case)
        for c in range(case.C):
            w = pb.weights(pb.z[:, c])
            base = node.logdensity_grad(pb.table, w, pb.u0, pb.y, pb.ts, case.opts())[1]
            for seed in (1, 2):
                nud = node.logdensity_grad(pb.table, w, pb.u0, pb.y, pb.ts, case.opts(), nudge=node.Nudge(2, seed))[1]
                s = nc.spread(base, nud)
                if s > worst:
                    worst, where = s, case.name
    print("largest spread of gw under +-2 ulp: %.3e (%s); GRAD_TOL = %.3e" % (worst, where, gc.GRAD_TOL))
    assert worst <= gc.MEASURED_GRAD_SPREAD <= 1.1 * worst
    assert gc.GRAD_TOL == 8 * gc.MEASURED_GRAD_SPREAD


@pytest.mark.parametrize("case", gc.ADAPTIVE_CASES + [gc.SAMPLER], ids=lambda c: c.name)
def test_adaptive_cases_are_certified(case):
    """no decision within MIN_MARGIN of err = 1, and the same step counts with every transcendental result moved by +-4 ulp"""
    pb = gc.problem(case)
    for c in range(case.C):
        base = nc.definition_at(case, pb, pb.z[:, c])
        assert not base.status.any() and base.min_margin >= nc.MIN_MARGIN, (case.name, c, base.min_margin)
        for seed in (1, 2):
            nud = nc.definition_at(case, pb, pb.z[:, c], nudge=node.Nudge(4, seed))
            assert np.array_equal(nud.naccept, base.naccept) and np.array_equal(nud.nreject, base.nreject) and not nud.status.any()


def test_a_failed_trajectory_gives_minus_infinity_and_nan():
    for case in (nc.FAIL_STEPS, nc.FAIL_BLOWUP):
        pb = nc.problem(case)
        lp, gw = node.logdensity_grad(pb.table, pb.weights(pb.z[:, 0]), pb.u0, pb.y, pb.ts, case.opts())
        assert np.isneginf(lp) and gw.shape == (pb.n,) and np.all(np.isnan(gw))
        sol = node.solve(pb.table, pb.weights(pb.z[:, 0]), pb.u0, pb.ts, case.opts(), y=pb.y, record=True)
        sl = node.grad_slices(pb.table, pb.weights(pb.z[:, 0]), pb.u0, pb.ts, case.opts(), pb.y, sol.record)
        assert np.all(np.isnan(sl[:, sol.status != 0])) and np.all(np.isposinf(node.replay(pb.table, pb.weights(pb.z[:, 0]), pb.u0, pb.ts,
                                                                                         case.opts(), sol.record, y=pb.y)[1]))


def test_the_api_switch():
    ts = np.linspace(0.0, 1.0, 5)
    chain = flux.Chain(flux.cube, flux.Dense(2, 3, "tanh"), flux.Dense(3, 2))
    with pytest.raises(si.SubspaceError, match="sensealg must be None or"):
        flux.NeuralODE(chain, (0.0, 1.0), ts, sensealg="forwarddiff")
    assert flux.NeuralODE(chain, (0.0, 1.0), ts).sensealg is None
    assert flux.NeuralODE(chain, (0.0, 1.0), ts, sensealg="discrete_adjoint").sensealg == "discrete_adjoint"
    data = flux.DataLoader(np.ones((2, 3)), np.ones((10, 3)), batchsize=3)
    for alg in ("mala", "hmc", "nuts", "advi"):     # without it: the old words, then the option's name
        with pytest.raises(si.SubspaceError, match="gradient through the ODE solver is not built.*sensealg=\"discrete_adjoint\""):
            si.sub_inference(flux.NeuralODE(chain, (0.0, 1.0), ts), data, np.zeros(17), np.zeros((17, 3)), alg=alg, device_loop=(alg == "advi"))
    model = flux.NeuralODE(chain, (0.0, 1.0), ts, sensealg="discrete_adjoint")
    for fn in (si.subspace_construction, si.diffusion_subspace, si.subspace_inference):     # training keeps raising
        with pytest.raises(si.SubspaceError, match="through the solver is out of scope"):
            fn(model, flux.mse, data, flux.Descent(), verbose=False)
