"""The per-transition MALA audit (tests/mala_audit.py) on the oracle alone -- no GPU.

  * the audit passes on the Philox-driven host MALA's trace of every case of the list, and the oracle alone meets the conditions
    there: both branches in every chain, no undecidable step (the SI_F32 case: the fp64 oracle with its value and gradient perturbed
    within the project's fp32 tolerances of 1e-5 and 2e-5 of the gradient's scale, at most 5 % undecidable);
  * every mutant of the catalogue -- the trace a kernel with that mistake would produce -- is rejected on at least one case;
  * single mutations of a good trace fail with a message naming chain and step;
  * the Python wrapper is bound to the exported symbol and the header declares it.
"""
import os
import re

import numpy as np
import pytest

from tests import mala_audit as ma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL_CASES = [c for c in ma.CASES if c.itr > 1]


def _f32_value_grad(case):
    """what an fp32 density and reverse sweep may return: the fp64 value off by up to 0.9e-5 of itself and every gradient component
    by up to 1.8e-5 of the largest, both fixed functions of z"""
    vg = ma.value_grad_of(ma.problem(case))

    def f(z):
        lp, g = vg(z)
        ph = 1e6 * float(np.sum(z))
        return lp * (1.0 + 0.9e-5 * np.cos(ph)), g + 1.8e-5 * np.max(np.abs(g)) * np.sin(ph + np.arange(g.size))
    return f


@pytest.mark.parametrize("case", REAL_CASES, ids=lambda c: c.name)
def test_oracle_trace_passes_and_meets_the_conditions(case):
    if case.f32:
        z, lp, acc, g = ma.oracle_trace(case, _f32_value_grad(case))
        assert not np.array_equal(lp, ma.cached_oracle_trace(case)[1])
    else:
        z, lp, acc, g = ma.cached_oracle_trace(case)
    rep = ma.audit_case(case, z, lp, acc, g)
    print(case.name, rep.line())
    ma.check_caps(case, rep)
    assert rep.worst_z_ratio <= 1.0
    if not case.f32:
        assert rep.worst_z_ratio == 0.0 and rep.worst_lp_rel == 0.0 and rep.worst_g_ratio == 0.0   # the oracle against itself


def test_a_chain_of_one_sample():
    case = ma.CASE_BY_NAME["A-M2-itr1"]
    z, lp, acc, g = ma.cached_oracle_trace(case)
    rep = ma.audit_case(case, z, lp, acc, g)
    ma.check_caps(case, rep)
    assert rep.steps == 0 and np.all(acc == 0.0)
    with pytest.raises(ma.AuditFailure, match="chain 1 .*acc"):
        ma.audit_case(case, z, lp, np.array([0.0, 0.5, 0.0]), g)


def test_the_conv_case_stays_clear_of_tied_pooling_windows(monkeypatch):
    """NNlib's maxpool gradient goes to the first window element with `y ≈ x` (rtol sqrt(eps)).  Where saturated tanh units put
    several elements of a window within sqrt(eps) of each other that rule stops naming the maximum, and the gradient depends on
    it at the level of the audit's tolerance.  The conv case must not go there: at every state of its trace the oracle's gradient
    is the same bits with the rule as with the exact maximum (rtol = 0)."""
    import math

    from oracle import subspace_oracle as so

    class ExactMax:
        def __getattr__(self, k):
            return getattr(math, k)

        def sqrt(self, v):   # (the only sqrt of the oracle's reverse sweep is the rule's rtol)
            return 0.0
    case = ma.CASE_BY_NAME["conv-f64"]
    pb = ma.problem(case)
    z = ma.cached_oracle_trace(case)[0]
    states = [z[:, t, c] for c in range(case.nchains) for t in range(case.itr)]
    with_rule = [so.logdensity_grad(pb.table, pb.w, pb.p, pb.x, pb.y, pb.sigma_m, v)[1] for v in states]
    monkeypatch.setattr(so, "math", ExactMax())
    exact = [so.logdensity_grad(pb.table, pb.w, pb.p, pb.x, pb.y, pb.sigma_m, v)[1] for v in states]
    assert all(np.array_equal(a, b) for a, b in zip(with_rule, exact))


# ----------------------------------------------------------------------------------------------- the mutant catalogue
# the cases a mutant is tried on, cheapest first; the decision mutants (no_logq, fwd_bwd_swapped, e_from_purpose0) need a step
# whose decision the mistake flips, which a case may or may not hold
MUTANT_CASES = ("small-M2", "ragged-M5", "A-M33", "A-M2-high-words", "B-M3")


@pytest.mark.parametrize("mutant", ma.MUTANTS)
def test_every_mutant_is_rejected_on_at_least_one_case(mutant):
    caught = []
    for name in MUTANT_CASES:
        case = ma.CASE_BY_NAME[name]
        z, lp, acc, g = ma.oracle_trace(case, mutant=mutant)
        try:
            ma.audit_case(case, z, lp, acc, g)
        except ma.AuditFailure as e:
            caught.append((name, str(e)))
            break
    print(mutant, caught)
    assert caught, "the audit accepts the traces of mutant %s on every case" % mutant
    assert re.search(r"chain \d+ \(Philox chain \d+\)", caught[0][1])


# ----------------------------------------------------------------------------------------------- single mutations
MUT = ma.CASE_BY_NAME["A-M33"]   # M = 33: 17 Philox blocks, the last one half used


@pytest.fixture(scope="module")
def trace():
    z, lp, acc, g = ma.cached_oracle_trace(MUT)
    accepted = np.any(z[:, 1:, :] != z[:, :-1, :], axis=0)   # [t - 1, c]
    return z, lp, acc, g, accepted


def _step(accepted, c, want, after=2):
    for t in range(after, accepted.shape[0]):
        if accepted[t - 1, c] == want:
            return t
    raise AssertionError("no such step")


def _fails(z, lp, acc, g, pattern):
    with pytest.raises(ma.AuditFailure) as ei:
        ma.audit_case(MUT, z, lp, acc, g)
    assert re.search(pattern, str(ei.value)), str(ei.value)


def test_mutation_accept_flipped_to_reject(trace):
    z, lp, acc, g, accepted = trace
    c, t = 1, _step(accepted, 1, True)
    z, lp, g = z.copy(), lp.copy(), g.copy()
    z[:, t, c], lp[t, c], g[:, t, c] = z[:, t - 1, c], lp[t - 1, c], g[:, t - 1, c]
    _fails(z, lp, acc, g, r"chain 1 .*step %d: the trace rejected.*says accept" % t)


def test_mutation_gradient_changed_on_a_reject_step(trace):
    z, lp, acc, g, accepted = trace
    c, t = 2, _step(accepted, 2, False)
    g = g.copy()
    g[4, t, c] = np.nextafter(g[4, t, c], np.inf)
    _fails(z, lp, acc, g, r"chain 2 .*step %d: .*reject.* gradient component 4 changed" % t)


def test_mutation_component_shifted_by_64_ulp(trace):
    z, lp, acc, g, accepted = trace
    c, t = 0, _step(accepted, 0, True)
    m = int(np.argmax(np.abs(z[:, t, c])))
    z = z.copy()
    z[m, t, c] += 64 * np.spacing(z[m, t, c])
    _fails(z, lp, acc, g, r"chain 0 .*step %d: component %d " % (t, m))


def test_mutation_gradient_off_by_its_tolerance_times_four(trace):
    z, lp, acc, g, accepted = trace
    c, t = 0, _step(accepted, 0, True)
    g = g.copy()
    g[7, t, c] += 4.0 * (ma.G_RTOL_F64 * abs(g[7, t, c]) + ma.G_ATOL_F64 * np.max(np.abs(g[:, t, c])))
    _fails(z, lp, acc, g, r"chain 0 .*step %d: gradient component 7 " % t)


def test_mutation_acceptance_count_off_by_one(trace):
    z, lp, acc, g, _ = trace
    acc = acc.copy()
    acc[1] += 1.0 / (MUT.itr - 1)
    _fails(z, lp, acc, g, r"chain 1 .*acc is")


# ----------------------------------------------------------------------------------------------- the binding
def test_the_wrapper_is_bound_to_the_exported_symbol_and_the_header_declares_it(si):
    from ctypes import POINTER, c_double, c_int32, c_int64, c_uint64, c_void_p
    sig = si._capi.SIGNATURES
    assert sig["si_sample_mala"] == (c_int32, [c_void_p, c_int64, c_double, c_uint64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p])
    assert sig["si_mala_kernel_info"] == (c_int32, [c_void_p, POINTER(c_int32), POINTER(c_int32)])
    lib = si.load()
    for name in ("si_sample_mala", "si_mala_kernel_info"):
        fn = getattr(lib, name)            # AttributeError: the library does not export it
        assert fn.argtypes == sig[name][1] and fn.restype is sig[name][0]
    assert callable(si.Context.sample_mala) and callable(si.Context.mala_kernel_info)
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "subspace_hip.h")).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", header)
    assert ("int32_t si_sample_mala(si_ctx* ctx, int64_t itr, double sigma_z, uint64_t seed, int32_t chain_id0, int32_t nchains, "
            "double* Z_out , double* lp_out , double* accept_rate_out , double* G_out );") in flat
    assert "int32_t si_mala_kernel_info(si_ctx* ctx, int32_t* fused_out, int32_t* passes_out);" in flat
    # a NULL context is refused before anything touches a device
    assert lib.si_sample_mala(None, 1, 0.1, 0, 0, 1, None, None, None, None) == si._capi.SI_ERR_INVALID
    assert lib.si_mala_kernel_info(None, None, None) == si._capi.SI_ERR_INVALID
    # the opt-in keyword of the Python API, off by default
    import inspect
    assert inspect.signature(si.sub_inference).parameters["device_loop"].default is False
