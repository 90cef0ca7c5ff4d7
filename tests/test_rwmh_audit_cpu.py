"""The per-transition RWMH audit (tests/rwmh_audit.py) on the oracle alone -- no GPU.

  * the audit passes on so.rwmh traces of every case of the list (the sizes at which the device samplers branch on M), and the
    oracle alone meets the caps there: both branches in every chain, no undecidable step (SI_F32 cases: the fp64 oracle with its density perturbed by
    the project's fp32 tolerance of 1e-5, at most 5 % undecidable);
  * every mutation of a trace that a wrong kernel could produce makes it fail, with a message naming chain, step and component;
  * a chain continued from a state perturbed by one ulp still passes: no whole-chain lockstep is needed.
"""
import dataclasses
import re

import numpy as np
import pytest

from oracle import philox
from tests import rwmh_audit as ra

REAL_CASES = [c for c in ra.CASES if c.itr > 1]


@pytest.mark.parametrize("case", REAL_CASES, ids=lambda c: c.name)
def test_oracle_trace_passes_and_meets_the_caps(case):
    pb = ra.problem(case)
    if case.f32:
        # what an fp32 density may return: the fp64 value off by up to 0.9e-5 of itself, a fixed function of z
        z, lp, acc = ra.oracle_trace(case, lambda v: pb.density(v) * (1.0 + 0.9e-5 * np.cos(1e6 * float(np.sum(v)))))
        assert not np.array_equal(lp, ra.cached_oracle_trace(case)[1])
    else:
        z, lp, acc = ra.cached_oracle_trace(case)
    w = None
    if case.how == "weights":
        w = np.stack([np.stack([pb.reconstruct(z[:, t, c]) for t in range(case.itr)], axis=1) for c in range(case.nchains)], axis=2)
    rep = ra.audit_case(case, z, lp, acc, W=w, reconstruct=pb.reconstruct if w is not None else None)
    print(case.name, rep.line())
    ra.check_caps(rep, case.f32)
    assert rep.steps == (case.itr - 1) * case.nchains and rep.worst_z_ratio <= 1.0
    if not case.f32:
        assert rep.worst_z_ratio == 0.0 and rep.worst_lp_rel == 0.0   # the oracle against itself


def test_a_chain_of_one_sample():
    case = ra.CASE_BY_NAME["I-M2-itr1"]
    z, lp, acc = ra.cached_oracle_trace(case)
    rep = ra.audit_case(case, z, lp, acc)
    assert rep.steps == 0 and np.all(acc == 0.0)
    with pytest.raises(ra.AuditFailure, match="chain 1 .*acc"):
        ra.audit_case(case, z, lp, np.array([0.0, 0.5, 0.0]))


# ----------------------------------------------------------------------------------------------- mutations
MUT = ra.CASE_BY_NAME["H-M33-weights"]   # M = 33: 17 Philox blocks, the last one half used


@pytest.fixture(scope="module")
def trace():
    pb = ra.problem(MUT)
    z, lp, acc = ra.cached_oracle_trace(MUT)
    w = np.stack([np.stack([pb.reconstruct(z[:, t, c]) for t in range(MUT.itr)], axis=1) for c in range(MUT.nchains)], axis=2)
    w.setflags(write=False)
    accepted = np.any(z[:, 1:, :] != z[:, :-1, :], axis=0)   # [t - 1, c]
    return pb, z, lp, acc, w, accepted


def _step(accepted, c, want, after=2, also_next=None):
    """first step t >= after of chain c that was accepted / rejected (and whose successor was, when asked)"""
    for t in range(after, accepted.shape[0]):
        if accepted[t - 1, c] == want and (also_next is None or accepted[t, c] == also_next):
            return t
    raise AssertionError("no such step")


def _fails(trace, z, lp, acc, pattern, w=None):
    pb = trace[0]
    with pytest.raises(ra.AuditFailure) as ei:
        ra.audit_case(MUT, z, lp, acc, W=w, reconstruct=pb.reconstruct if w is not None else None)
    msg = str(ei.value)
    assert re.search(pattern, msg), msg
    return msg


def _noise(c, t):
    return MUT.sigma_z * philox.normals(MUT.seed, MUT.chain_id0 + c, t, MUT.m)


def test_the_unmutated_trace_passes(trace):
    pb, z, lp, acc, w, _ = trace
    rep = ra.audit_case(MUT, z, lp, acc, W=w, reconstruct=pb.reconstruct)
    assert rep.accepts > 0 and rep.rejects > 0 and rep.undecidable == 0


def test_mutation_accept_flipped_to_reject(trace):
    pb, z, lp, acc, _, accepted = trace
    c, t = 1, _step(accepted, 1, True)
    z, lp = z.copy(), lp.copy()
    z[:, t, c], lp[t, c] = z[:, t - 1, c], lp[t - 1, c]
    _fails(trace, z, lp, acc, r"chain 1 .*step %d: the trace rejected.*says accept" % t)


def test_mutation_reject_flipped_to_accept(trace):
    pb, z, lp, acc, _, accepted = trace
    c, t = 2, _step(accepted, 2, False)
    z, lp = z.copy(), lp.copy()
    z[:, t, c] = z[:, t - 1, c] + _noise(c, t)
    lp[t, c] = pb.density(z[:, t, c])
    _fails(trace, z, lp, acc, r"chain 2 .*step %d: the trace accepted.*says reject" % t)


def test_mutation_component_shifted_by_64_ulp(trace):
    pb, z, lp, acc, _, accepted = trace
    c, t = 0, _step(accepted, 0, True)
    m = int(np.argmax(np.abs(z[:, t, c]) / (np.abs(z[:, t - 1, c]) + np.abs(_noise(c, t)))))
    z = z.copy()
    z[m, t, c] += 64 * np.spacing(z[m, t, c])
    _fails(trace, z, lp, acc, r"chain 0 .*step %d: component %d " % (t, m))
    # ... while two ulp pass: the trace cut off behind step t, with the acceptance rate of what is left
    z2 = np.array(trace[1][:, :t + 1, c:c + 1], order="F")
    z2[m, t, 0] += 2 * np.spacing(z2[m, t, 0])
    acc2 = np.array([accepted[:t, c].sum() / t])
    cut = dataclasses.replace(MUT, itr=t + 1, nchains=1, chain_id0=MUT.chain_id0 + c)
    rep = ra.audit_case(cut, z2, lp[:t + 1, c:c + 1], acc2)
    assert 0.0 < rep.worst_z_ratio <= 4.0 / ra.Z_ULPS   # (two spacings of z are at most 4 * 2^-53 (|z_prev| + |noise|))


@pytest.mark.parametrize("m", [0, 1], ids=["within-a-block", "across-two-blocks"])
def test_mutation_components_swapped(trace, m):
    pb, z, lp, acc, _, accepted = trace
    c, t = 1, _step(accepted, 1, True)
    z = z.copy()
    nz = _noise(c, t)
    z[m, t, c], z[m + 1, t, c] = z[m, t - 1, c] + nz[m + 1], z[m + 1, t - 1, c] + nz[m]   # each moved by the other's draw
    msg = _fails(trace, z, lp, acc, r"chain 1 .*step %d: component %d " % (t, m))
    assert "the draw of component %d" % (m + 1) in msg and "Philox block %d, own block %d" % ((m + 1) // 2, m // 2) in msg


@pytest.mark.parametrize("what", ["next-step", "next-chain"])
def test_mutation_draw_of_another_step_or_chain(trace, what):
    pb, z, lp, acc, _, accepted = trace
    c, t = 0, _step(accepted, 0, True)
    z, lp = z.copy(), lp.copy()
    z[:, t, c] = z[:, t - 1, c] + (_noise(c, t + 1) if what == "next-step" else _noise(c + 1, t))
    lp[t, c] = pb.density(z[:, t, c])
    msg = _fails(trace, z, lp, acc, r"chain 0 .*step %d: component 0 " % t)
    assert ("the draw of step %d" % (t + 1) if what == "next-step" else "the draw of Philox chain %d" % (MUT.chain_id0 + 1)) in msg
    assert "%d of %d components off" % (MUT.m, MUT.m) in msg


def test_mutation_column_written_one_step_late(trace):
    pb, z, lp, acc, _, accepted = trace
    c = 2
    t = _step(accepted, c, True, also_next=True)
    z = z.copy()
    z[:, t + 1, c] = z[:, t, c]       # the layout shift: column t lands in column t + 1
    _fails(trace, z, lp, acc, r"chain 2 .*step %d: .*bit copy.*lp changed" % (t + 1))


def test_mutation_acceptance_count_off_by_one(trace):
    pb, z, lp, acc, _, _ = trace
    acc = acc.copy()
    acc[1] += 1.0 / (MUT.itr - 1)
    _fails(trace, z, lp, acc, r"chain 1 .*acc is")


def test_mutation_one_ulp_on_a_reject_step(trace):
    pb, z, lp, acc, _, accepted = trace
    c, t = 0, _step(accepted, 0, False)
    z = z.copy()
    z[7, t, c] = np.nextafter(z[7, t, c], np.inf)
    msg = _fails(trace, z, lp, acc, r"chain 0 .*step %d: component \d+ " % t)
    assert "did not move" in msg   # 32 components stayed where they were, one moved by an ulp: neither a reject nor an accept


def test_mutation_accepted_step_keeps_the_previous_lp(trace):
    pb, z, lp, acc, _, accepted = trace
    c, t = 1, _step(accepted, 1, True)
    lp = lp.copy()
    lp[t, c] = lp[t - 1, c]
    _fails(trace, z, lp, acc, r"chain 1 .*step %d: lp is .*density\(Z\[:, t\]\)" % t)


def test_mutation_weights_recomputed_on_a_reject_step(trace):
    pb, z, lp, acc, w, accepted = trace
    c, t = 2, _step(accepted, 2, False)
    w = w.copy()
    col = pb.reconstruct(z[:, t, c])
    col[5] = np.nextafter(col[5], np.inf)
    w[:, t, c] = col
    _fails(trace, z, lp, acc, r"chain 2 .*step %d: a reject step, but weight 5 changed" % t, w=w)
    # and on an accepted step the column must be reconstruct(Z[:, t]) itself
    t = _step(accepted, c, True)
    w = trace[4].copy()
    w[9, t, c] = np.nextafter(w[9, t, c], np.inf)
    _fails(trace, z, lp, acc, r"chain 2 .*step %d: weight 9 is" % t, w=w)


def test_a_perturbed_chain_still_passes_without_lockstep(trace):
    """why the audit exists: one ulp on a mid-chain state (what another libm may give) and the chain continued from there.  Every
    later state differs from the oracle's chain, a decision may flip and the chains part for good -- each transition is still right"""
    pb, z0, lp0, acc0, _, accepted = trace
    c = 0
    t0 = _step(accepted, c, True, after=MUT.itr // 3)
    z, lp = z0.copy(), lp0.copy()
    z[5, t0, c] = np.nextafter(z[5, t0, c], np.inf)
    lp[t0, c] = pb.density(z[:, t0, c])
    nacc = int(accepted[:t0, c].sum())
    for t in range(t0 + 1, MUT.itr):           # so.rwmh's transition, continued from the perturbed state
        zp = z[:, t - 1, c] + _noise(c, t)
        lpp = pb.density(zp)
        if -philox.randexp(MUT.seed, MUT.chain_id0 + c, t) < lpp - lp[t - 1, c]:
            z[:, t, c], lp[t, c] = zp, lpp
            nacc += 1
        else:
            z[:, t, c], lp[t, c] = z[:, t - 1, c], lp[t - 1, c]
    acc = acc0.copy()
    acc[c] = nacc / (MUT.itr - 1)
    assert not np.array_equal(z[:, t0:, c], z0[:, t0:, c])
    rep = ra.audit_case(MUT, z, lp, acc)
    assert rep.undecidable == 0 and 0.0 < rep.worst_z_ratio <= 2.0 / ra.Z_ULPS
