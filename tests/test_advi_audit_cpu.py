"""The per-update ADVI audit (tests/advi_audit.py) on the oracle alone -- no GPU.

  * the audit passes on the Philox-driven host ADVI's trace of every case of the list (the SI_F32 case: the fp64 oracle with its
    value and gradient perturbed within the project's fp32 tolerances);
  * every mutant of the catalogue -- the trace a kernel with that mistake would produce -- is rejected on at least one case
    (ring_slot_next: by the bit-for-bit restatement of the update, see advi_audit's header);
  * on a one-layer identity Dense chain, where the posterior in z is exactly Gaussian and the ELBO of a diagonal normal is closed
    form, the host ADVI climbs: exact ELBO(theta_T) > exact ELBO(theta_0), and it ends within twice the measured gap of the
    mean-field optimum;
  * the signatures, the defaults, the argument-refusal table and the binding.
"""
import inspect
import os
import re

import numpy as np
import pytest

from tests import advi_audit as aa
from tests.test_mala_audit_cpu import _f32_value_grad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", aa.CASES, ids=lambda c: c.name)
def test_oracle_trace_passes(case):
    if case.f32:
        out = aa.oracle_trace(case, _f32_value_grad(case))
        assert not np.array_equal(out[2], aa.cached_oracle_trace(case)[2])
    else:
        out = aa.cached_oracle_trace(case)
    rep = aa.audit_case(case, *out)
    print(case.name, rep.line())
    assert rep.steps == case.t * case.nruns
    assert max(rep.worst_theta0_ratio, rep.worst_point_ratio, rep.worst_update_ratio, rep.worst_draw_ratio) <= 1.0
    if not case.f32:   # the oracle against itself: only the rounding of theta_{t+1} - theta_t is left
        assert rep.worst_theta0_ratio == 0.0 and rep.worst_point_ratio == 0.0 and rep.worst_draw_ratio == 0.0 and rep.worst_elbo_rel == 0.0
        assert rep.worst_update_ratio < 1e-3


def test_the_case_list_covers_what_the_kernels_branch_on():
    c = aa.CASE_BY_NAME
    assert {x.m for x in aa.CASES} >= {1, 3, 33, 300} and {x.s for x in aa.CASES} >= {1, 10}
    assert (c["M33-W4-T11"].w, c["M33-W4-T11"].t) == (4, 11) and (c["M33-W100-T7"].w, c["M33-W100-T7"].t) == (100, 7)
    assert (c["M3-R3"].nruns, c["M3-R3"].chain_id0) == (3, 2) and any(x.prior > 0.0 for x in aa.CASES)
    assert [x.name for x in aa.CASES if not x.fused] == ["conv-f64", "dense-f32", "softplus"]
    for x in aa.CASES:
        if x.fused:
            assert aa.problem(x).x.shape[1] <= 64
        else:
            assert x.t <= 6 and x.s <= 3


# ----------------------------------------------------------------------------------------------- the mutant catalogue
MUTANT_CASES = ("M3-S10", "M33-W4-T11", "M33-W100-T7", "M3-R3")   # cheapest first; the ring mutants need the case that wraps


def test_the_catalogue_names_the_mutants_asked_for():
    assert set(aa.MUTANTS) >= {"no_minus_one", "no_sigma", "eta0_reused", "no_over_s", "ring_slot_next", "s_without_current",
                               "ring_never_wraps", "no_sqrt", "update_sign", "draws_purpose0", "final_from_prev_theta", "omega0_zero"}
    assert aa.BIT_ONLY_MUTANTS == ("ring_slot_next",)


@pytest.mark.parametrize("mutant", [m for m in aa.MUTANTS if m not in aa.BIT_ONLY_MUTANTS])
def test_every_mutant_is_rejected_on_at_least_one_case(mutant):
    caught = []
    for name in MUTANT_CASES:
        case = aa.CASE_BY_NAME[name]
        try:
            aa.audit_case(case, *aa.oracle_trace(case, mutant=mutant))
        except aa.AuditFailure as e:
            caught.append((name, str(e)))
            break
    print(mutant, caught)
    assert caught, "the audit accepts the traces of mutant %s on every case" % mutant
    assert re.search(r"run \d+ \(Philox chain \d+\), step \d+", caught[0][1])


def _oracle_lp_g(case, points, r):
    vg = aa.value_grad_of(aa.problem(case))

    def f(t):
        vals = [vg(points[:, k, t, r]) for k in range(case.s)]
        return np.array([v[0] for v in vals]), np.stack([v[1] for v in vals], axis=1)
    return f


def test_the_slot_mutant_is_a_reordering_that_only_the_bit_replay_rejects():
    """slot (t + 1) mod W holds the same W addends in another order: the audit's tolerances cannot tell, the restated bits can"""
    case = aa.CASE_BY_NAME["M33-W4-T11"]
    good, bad = aa.cached_oracle_trace(case), aa.oracle_trace(case, mutant="ring_slot_next")
    aa.audit_case(case, *bad)                                   # within every tolerance ...
    assert not np.array_equal(good[0], bad[0])                  # ... and yet another trace
    aa.mu_replay(good[0][:, :, 0], _oracle_lp_g(case, good[1], 0), case.s, case.w, case.eta, case.tau)
    with pytest.raises(aa.AuditFailure, match=r"step \d+: mu\["):
        aa.mu_replay(bad[0][:, :, 0], _oracle_lp_g(case, bad[1], 0), case.s, case.w, case.eta, case.tau)
    # and the replay follows the mutant's own trace when told to imitate it: the difference is the slot and nothing else
    aa.mu_replay(bad[0][:, :, 0], _oracle_lp_g(case, bad[1], 0), case.s, case.w, case.eta, case.tau, mutant="ring_slot_next")


@pytest.mark.parametrize("name", ["M3-S10", "M3-R3"])
def test_the_bit_replay_accepts_the_oracle(name):
    case = aa.CASE_BY_NAME[name]
    tr, pts = aa.cached_oracle_trace(case)[:2]
    for r in range(case.nruns):
        aa.mu_replay(tr[:, :, r], _oracle_lp_g(case, pts, r), case.s, case.w, case.eta, case.tau)


# ----------------------------------------------------------------------------------------------- single mutations
MUT = aa.CASE_BY_NAME["M33-W100-T7"]


def _fails(out, pattern):
    with pytest.raises(aa.AuditFailure) as ei:
        aa.audit_case(MUT, *out)
    assert re.search(pattern, str(ei.value)), str(ei.value)


def test_mutation_a_point_shifted_by_64_ulp():
    out = [a.copy() for a in aa.cached_oracle_trace(MUT)]
    out[1][5, 1, 3, 0] += 64 * np.spacing(out[1][5, 1, 3, 0])
    _fails(out, r"run 0 .*step 3: point 1: component 5 ")


def test_mutation_an_update_off_by_a_millionth():
    out = [a.copy() for a in aa.cached_oracle_trace(MUT)]
    out[0][40, 5:, 0] += 1e-6 * abs(out[0][40, 5, 0] - out[0][40, 4, 0])    # omega_7 from step 4's update on, shifted
    out[3][40, 0] = out[0][40, -1, 0]
    _fails(out, r"run 0 .*step 4: the update .* component 40 ")


def test_mutation_elbo_and_final_theta():
    out = [a.copy() for a in aa.cached_oracle_trace(MUT)]
    out[2][2, 0] *= 1.0 + 1e-9
    _fails(out, r"run 0 .*step 2: elbo is")
    out = [a.copy() for a in aa.cached_oracle_trace(MUT)]
    out[3][0, 0] = np.nextafter(out[3][0, 0], np.inf)
    _fails(out, r"run 0 .*step 7: theta component 0 ")


# ----------------------------------------------------------------------------------------------- the exactly Gaussian posterior
GAUSS = aa.Case("gauss-M3", ((4, 2), (aa.I_,), 40), 3, True, 150, s=10, sigma_z=0.3, sigma_m=0.8, seed=11)


def test_the_host_advi_climbs_the_exact_elbo_of_a_gaussian_posterior():
    """one identity Dense layer: the model output is affine in z, so lp(z) = lp(z*) - (z - z*)' L (z - z*) / 2 exactly, and for
    q = N(mu, diag(sigma^2)):  ELBO = lp(z*) - ((mu - z*)' L (mu - z*) + sum_m L_mm sigma_m^2) / 2 + M (log 2 pi + 1) / 2 + sum omega.
    The mean-field optimum is mu = z*, sigma_m^2 = 1 / L_mm."""
    vg = aa.value_grad_of(aa.problem(GAUSS))
    m = GAUSS.m
    g0 = vg(np.zeros(m))[1]
    lam = -np.stack([vg(e)[1] - g0 for e in np.eye(m)], axis=1)
    assert np.allclose(lam, lam.T, rtol=1e-9, atol=1e-9 * np.max(np.abs(lam))) and np.all(np.linalg.eigvalsh(lam) > 0.0)
    zs = np.linalg.solve(lam, g0)
    assert np.allclose(vg(zs)[1], 0.0, atol=1e-8 * np.max(np.abs(g0)))
    lps = vg(zs)[0]
    # (the density is exactly quadratic: the closed form reproduces the oracle away from z*)
    zt = np.array([0.3, -0.2, 0.5])
    assert abs(vg(zt)[0] - (lps - 0.5 * (zt - zs) @ lam @ (zt - zs))) <= 1e-9 * abs(lps)

    def exact_elbo(th):
        mu, om = th[:m], th[m:]
        return lps - 0.5 * ((mu - zs) @ lam @ (mu - zs) + np.sum(np.diag(lam) * np.exp(2.0 * om))) + aa.entropy(om)

    best = exact_elbo(np.concatenate([zs, -0.5 * np.log(np.diag(lam))]))
    trace = aa.oracle_trace(GAUSS)[0][:, :, 0]
    e0, et = exact_elbo(trace[:, 0]), exact_elbo(trace[:, -1])
    print("exact ELBO: theta_0 %r, theta_T %r, mean-field optimum %r; gaps %r -> %r" % (e0, et, best, best - e0, best - et))
    assert best >= et > e0
    # measured on the CPU for this (seed 11, T 150, S 10): the gap to the optimum falls from 11.9686 to 3.4721 nats (the step of
    # TruncatedADAGrad(0.1, 1.0, 100) is at most 0.1 per component and update); asserted with twice the remaining gap
    assert best - et <= 2.0 * GAPT_MEASURED, (best - et, GAPT_MEASURED)


GAPT_MEASURED = 3.4721


# ----------------------------------------------------------------------------------------------- signatures, refusals, the binding
def test_signatures_and_defaults(si):
    assert inspect.signature(si.sub_inference).parameters["device_loop"].default is False
    assert inspect.signature(si.subspace_inference).parameters["device_loop"].default is False
    p = inspect.signature(si.Context.fit_advi).parameters
    assert list(p)[:4] == ["self", "max_iters", "sigma_z", "seed"]
    assert (p["samples_per_step"].default, p["eta"].default, p["tau"].default, p["window"].default) == (10, 0.1, 1.0, 100)   # ADVI(10, itr), TruncatedADAGrad(0.1, 1.0, 100)
    assert (p["chain_id0"].default, p["nruns"].default, p["ndraws"].default, p["trace"].default) == (0, 1, None, False)
    assert callable(si.Context.advi_kernel_info)


GOOD = dict(m=3, max_iters=5, samples_per_step=10, sigma_z=0.3, eta=0.1, tau=1.0, window=100, chain_id0=0, nruns=1, ndraws=5)
REFUSED = [dict(max_iters=0), dict(samples_per_step=0), dict(m=4, samples_per_step=2 ** 23), dict(window=0), dict(window=1025), dict(nruns=0),
           dict(chain_id0=-1), dict(sigma_z=0.0), dict(sigma_z=-1.0), dict(sigma_z=float("nan")), dict(tau=0.0), dict(tau=float("nan")),
           dict(eta=0.0), dict(eta=-0.1), dict(ndraws=-1)]


def test_the_refusal_table_is_mirrored(si):
    caps = si._capi
    assert caps.advi_refusal(**GOOD) is None
    assert caps.advi_refusal(**dict(GOOD, window=1, ndraws=0)) is None and caps.advi_refusal(**dict(GOOD, window=1024)) is None
    assert caps.advi_refusal(**dict(GOOD, m=4, samples_per_step=2 ** 23 - 1)) is None     # S nblk = 2^24 - 2
    seen = set()
    for bad in REFUSED:
        why = caps.advi_refusal(**dict(GOOD, **bad))
        assert why is not None, bad
        seen.add(why)
    assert seen == {what for what, _ in caps.ADVI_REFUSALS}     # every row of the table is reached, one by one
    # the header states the same table
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "subspace_hip.h")).read().replace(" * ", " "))
    assert ("SI_ERR_INVALID: T < 1, S < 1, S nblk >= 2^24, W outside 1 .. 1024, R < 1, chain_id0 < 0, sigma_z <= 0, tau <= 0, "
            "eta <= 0, D < 0") in header
    # Context.fit_advi refuses before it sizes an array or touches the library
    ctx = object.__new__(si.Context)
    ctx.h = None
    for bad in REFUSED:
        kw = dict(GOOD, **bad)
        ctx._m = kw.pop("m")
        with pytest.raises(si.SubspaceError) as e:
            ctx.fit_advi(kw.pop("max_iters"), kw.pop("sigma_z"), 1, **kw)
        assert e.value.code == caps.SI_ERR_INVALID, bad


def test_the_wrapper_is_bound_to_the_exported_symbol_and_the_header_declares_it(si):
    from ctypes import POINTER, c_double, c_int32, c_int64, c_uint64, c_void_p
    sig = si._capi.SIGNATURES
    assert sig["si_fit_advi"] == (c_int32, [c_void_p, c_int64, c_int32, c_double, c_double, c_double, c_int32, c_uint64, c_int32, c_int32,
                                            c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p])
    assert sig["si_advi_kernel_info"] == (c_int32, [c_void_p, POINTER(c_int32), POINTER(c_int32)])
    lib = si.load()
    for name in ("si_fit_advi", "si_advi_kernel_info"):
        fn = getattr(lib, name)            # AttributeError: the library does not export it
        assert fn.argtypes == sig[name][1] and fn.restype is sig[name][0]
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "subspace_hip.h")).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", header)
    assert ("int32_t si_fit_advi(si_ctx* ctx, int64_t max_iters , int32_t samples_per_step , double sigma_z, double eta, double tau, "
            "int32_t window , uint64_t seed, int32_t chain_id0, int32_t nruns , int64_t ndraws , double* theta_out , double* Z_out , "
            "double* elbo_out , double* theta_trace_out , double* points_out );") in flat
    assert "int32_t si_advi_kernel_info(si_ctx* ctx, int32_t* fused_out, int32_t* passes_out);" in flat
    # a NULL context is refused before anything touches a device
    assert lib.si_fit_advi(None, 1, 1, 0.1, 0.1, 1.0, 1, 0, 0, 1, 0, None, None, None, None, None) == si._capi.SI_ERR_INVALID
    assert lib.si_advi_kernel_info(None, None, None) == si._capi.SI_ERR_INVALID
    # sub_inference without the keyword keeps raising, and the message names the keyword (no device is touched before it)
    with pytest.raises(si.SubspaceError, match="device_loop=True"):
        si.sub_inference(None, None, None, None, alg=":advi")
    with pytest.raises(si.SubspaceError, match="nchains = 1"):
        si.sub_inference(None, None, None, None, alg=":advi", device_loop=True, nchains=2)
