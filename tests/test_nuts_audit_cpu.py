"""samplers.nuts_iter and tests/nuts_audit.py, without a GPU.

  * the restatement: nuts_iter on the sequential callback IS samplers.nuts, bit for bit -- the iterative tree pinned to the recursive one
  * nuts_audit.oracle_trace without a mutant IS nuts_iter on the Philox callback, bit for bit, and its replayed tree statistics agree
  * the oracle's own trace of every case passes the audit within the caps, also with every value and gradient moved to the edge of
    the stated tolerances; the case list reaches every exit of the tree (the coverage certificate)
  * every mutant -- a wrong kernel -- is rejected on at least one case
  * the float64 replay of every decision sits under a quarter of the decision's derived tolerance from a longdouble replay
tests/test_gpu_nuts.py holds the device's traces to the same audit."""
import numpy as np
import pytest

from subspaceinference_jl_amd import samplers
from tests import hmc_audit as ha
from tests import nuts_audit as na
from tests.rwmh_audit import AuditFailure


def _vg(case):
    return ha.value_grad_of(ha.problem(case))


@pytest.mark.parametrize("name,kw", [("small-M2-adapt200", {}), ("ragged-M5", {}), ("A-M33", dict(max_depth=2)),
                                     ("small-M1", dict(max_dh=0.3)), ("A-M65", dict(max_depth=4, max_dh=2.0))])
def test_nuts_iter_is_nuts_bit_for_bit(name, kw):
    case = ha.CASE_BY_NAME[name]
    vg, m, itr = _vg(case), case.m, 40
    want = samplers.nuts(vg, m, itr, case.sigma_z, np.random.default_rng([3, case.m]), **kw)
    stats = []
    got = samplers.nuts_iter(vg, m, itr, case.sigma_z, samplers.sequential_draw(np.random.default_rng([3, case.m]), m), stats=stats, **kw)
    assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]) and want[2] == got[2]
    assert len(stats) == itr and all(1 <= d <= kw.get("max_depth", 10) and 1 <= n < 2 ** d and 0 <= s <= n for d, n, s in stats)
    if "max_depth" in kw:
        assert max(n for _, n, _ in stats) == 2 ** kw["max_depth"] - 1       # the depth limit was reached
    if "max_dh" in kw:
        assert any(n < 2 ** (d - 1) for d, n, _ in stats if d > 1) or any(s == 0 for _, _, s in stats)


@pytest.mark.parametrize("name", ["small-M2", "A-M33", "small-M2-maxdh", "relu-deep-overflow", "small-M2-window"])
def test_the_oracle_is_nuts_iter_on_the_philox_callback(name):
    case = na.CASE_BY_NAME[name]
    tr = na.cached_oracle_trace(case)
    vg = na.value_grad_of(na.problem(case))
    for c in range(case.nchains):
        stats = []
        z, lp, acc = samplers.nuts_iter(vg, case.m, case.itr, case.sigma_z, na.philox_draw(case.seed, case.chain_id0 + c, case.m),
                                        delta=case.delta, max_depth=case.max_depth, max_dh=case.max_dh, n_adapts=case.adapts, stats=stats)
        assert np.array_equal(z, tr.Z[:, 1:, c]) and np.array_equal(lp, tr.lp[1:, c]) and acc == float(np.mean(tr.alpha[1:, c]))
        assert stats == [(int(tr.depth[t, c]), int(tr.nleaf[t, c]), int(tr.sel[t, c])) for t in range(1, case.itr + 1)]


@pytest.mark.parametrize("case", na.CASES, ids=lambda c: c.name)
def test_the_oracles_trace_passes_the_audit(case):
    tr = na.cached_oracle_trace(case)
    rep = na.audit_case(case, tr)
    print(case.name, rep.line())
    na.check_caps(case, rep)
    assert rep.leaves == int(tr.nleaf.sum()) and not np.isnan(tr.leaf[0, :int(tr.nleaf[:, 0].sum()), 0]).any()
    # ... and with every value and gradient at the edge of the stated tolerances
    moved = na.oracle_trace(case, value_grad=na.perturbed(na.value_grad_of(na.problem(case)), case.tols, 5))
    rep2 = na.audit_case(case, moved)
    na.check_caps(case, rep2)


def test_the_cases_reach_every_exit():
    got = {}
    for case in na.CASES:
        for ex in na.coverage(case, na.cached_oracle_trace(case)):
            got.setdefault(ex, []).append(case.name)
    print({k: len(v) for k, v in got.items()})
    assert set(got) == set(na.EXITS), set(na.EXITS) ^ set(got)
    assert "small-M2-depth2" in got["depth limit"] and "relu-deep-overflow" in got["nonfinite"] and "A-M2-steep" in got["divergence"]
    closes = sum(na.audit_case(c, na.cached_oracle_trace(c)).closes for c in na.CASES if c.name == "small-M2-window")
    assert closes == 1
    sizes = na.cached_oracle_trace(na.CASE_BY_NAME["A-M5x8"]).nleaf[1:, :].sum(axis=0)
    assert len(set(sizes.tolist())) >= 4, sizes    # the eight chains' trees differ


MUTANT_CASES = ["small-M2", "ragged-M5", "A-M33", "small-M2-depth2", "small-M2-maxdh", "small-M2-window", "A-M5x8"]


@pytest.mark.parametrize("mutant", na.MUTANTS)
def test_every_mutant_is_rejected(mutant):
    assert len(na.MUTANTS) >= 15
    rejected = []
    for name in MUTANT_CASES:
        case = na.CASE_BY_NAME[name]
        try:
            rep = na.audit_case(case, na.oracle_trace(case, mutant=mutant))
            na.check_caps(case, rep)
        except AuditFailure as e:
            rejected.append((name, str(e)[:120]))
            break
        except AssertionError as e:   # (a mutant may only fail by an audit condition, not by drowning in undecidable transitions)
            continue
    print(mutant, rejected)
    assert rejected, "the audit accepts the mutant %s on every case" % mutant


def test_the_float64_replay_against_longdouble():
    assert np.finfo(np.longdouble).eps < 2.0 ** -60
    worst = {}
    for case in na.CASES:
        tr = na.cached_oracle_trace(case)
        d64 = na.audit_case(case, tr, check_oracle=False).decisions
        dl = na.audit_case(case, tr, ft=np.longdouble, check_oracle=False).decisions
        assert [d[:3] for d in d64] == [d[:3] for d in dl], case.name
        for (c, t, kind, a, tol), (_, _, _, b, _) in zip(d64, dl):
            if np.isfinite(a) and np.isfinite(b):
                worst[kind] = max(worst.get(kind, 0.0), abs(a - b) / tol)
    print({k: "%.3g" % v for k, v in worst.items()})
    assert set(worst) >= {"divergence", "merge pick", "sub-tree U-turn", "progressive pick", "tree U-turn"}
    assert all(v < 0.25 for v in worst.values()), worst
