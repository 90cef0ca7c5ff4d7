"""The per-transition HMC audit (tests/hmc_audit.py) on the oracle alone -- no GPU.

  * the audit passes on the Philox-driven host HMC's trace of every case of the list, and the oracle alone meets the conditions
    there: both branches in every chain (cases of at most 8 transitions are exempt: too few steps to demand a reject), no undecidable
    step-size search in fp64 (the SI_F32 case: the fp64 oracle perturbed within the project's fp32 tolerances, at most
    rwmh_audit.F32_UNDECIDABLE_CAP of its chains);
  * every mutant of the catalogue -- the trace a kernel with that mistake would produce -- is rejected on at least one case;
  * the two derived adaptor bounds are certified: on every case the float64 replay sits within a quarter of the bound of a
    longdouble replay;
  * the audit's restatements (Adaptor, search) are samplers.StanAdaptor and samplers.find_good_stepsize bit for bit, and
    si_host_hmc_windows is StanAdaptor's schedule for every n_adapts in 0 .. 2000;
  * the host HMC on the Philox stream has samplers.hmc's stationary moments on the Gaussian target of tests/test_capi_cpu.py;
  * the Python wrapper is bound to the exported symbols and the header declares them.
"""
import math
import os
import re

import numpy as np
import pytest

from tests import hmc_audit as ha
from tests import test_mala_audit_cpu as mala_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL_CASES = [c for c in ha.CASES if c.itr > 1]


def _trace(case):
    if case.f32:
        return ha.oracle_trace(case, mala_cpu._f32_value_grad(case))
    return ha.cached_oracle_trace(case)


@pytest.mark.parametrize("case", ha.CASES, ids=lambda c: c.name)
def test_oracle_trace_passes_and_meets_the_conditions(case):
    tr = _trace(case)
    if case.f32:
        assert not np.array_equal(tr[1], ha.cached_oracle_trace(case)[1])
    rep = ha.audit_case(case, *tr)
    print(case.name, rep.line(), "search evaluations", rep.search_evals if len(rep.search_evals) <= 8 else max(rep.search_evals))
    ha.check_caps(case, rep)
    assert tr[0].shape == (case.m, case.itr + 1, case.nchains)
    assert rep.worst_z_ratio <= 1.0 and rep.worst_logeps_ratio <= 0.25 and rep.worst_minv_ratio <= 0.25
    if not case.f32:
        assert rep.worst_z_ratio == 0.0 and rep.worst_lp_rel == 0.0 and rep.worst_g_ratio == 0.0   # the oracle against itself
    assert rep.mean_alpha == [float(tr[2][1:, c].mean()) for c in range(case.nchains)]


def test_the_cases_cover_the_adaptation_schedules():
    by = ha.CASE_BY_NAME
    assert by["A-M2-itr1"].adapts == 0 and by["A-M2-itr5"].adapts == 2 and by["A-M5-itr8"].adapts == 4
    assert by["small-M1"].adapts == 30 and by["small-M2-adapt200"].adapts == 200 and by["small-M2-adapt-all"].adapts == 40
    closes = {n: ha.Adaptor(1, by[n].adapts, 0.1).window_splits for n in ("A-M5-itr8", "small-M1", "small-M2-adapt200", "small-M2-adapt-all")}
    assert closes == {"A-M5-itr8": [], "small-M1": [27], "small-M2-adapt200": [100, 150], "small-M2-adapt-all": [36]}
    rep = ha.audit_case(by["small-M2-adapt200"], *ha.cached_oracle_trace(by["small-M2-adapt200"]))
    assert rep.closes == 2 * by["small-M2-adapt200"].nchains
    assert {c.m for c in ha.CASES} >= {1, 2, 5, 33, 65, 513}


# ----------------------------------------------------------------------------------------------- the mutant catalogue
MUTANT_CASES = ("small-M1", "small-M2-search", "small-M2-adapt-all", "ragged-M5", "A-M2-high-words", "small-M2-adapt200")


@pytest.mark.parametrize("mutant", ha.MUTANTS)
def test_every_mutant_is_rejected_on_at_least_one_case(mutant):
    caught = []
    for name in MUTANT_CASES:
        case = ha.CASE_BY_NAME[name]
        try:
            ha.audit_case(case, *ha.oracle_trace(case, mutant=mutant))
        except ha.AuditFailure as e:
            caught.append((name, str(e)))
            break
    print(mutant, caught)
    assert caught, "the audit accepts the traces of mutant %s on every case" % mutant
    assert re.search(r"chain \d+ \(Philox chain \d+\)", caught[0][1])


def test_single_mutations_fail_with_chain_and_step():
    case = ha.CASE_BY_NAME["ragged-M5"]
    z, lp, al, ep, g, mi = (a.copy() for a in ha.cached_oracle_trace(case))
    accepted = np.any(z[:, 1:, :] != z[:, :-1, :], axis=0)
    t = 1 + int(np.flatnonzero(accepted[:, 1])[2])

    def fails(pattern, **kw):
        args = dict(Z=z, lp=lp, alpha=al, eps=ep, G=g, Minv=mi)
        args.update(kw)
        with pytest.raises(ha.AuditFailure) as ei:
            ha.audit_case(case, args["Z"], args["lp"], args["alpha"], args["eps"], args["G"], args["Minv"])
        assert re.search(pattern, str(ei.value)), str(ei.value)
    z2 = z.copy()
    z2[3, t, 1] += 64 * np.spacing(z2[3, t, 1])
    fails(r"chain 1 .*step %d: component 3 " % t, Z=z2)
    al2 = al.copy()
    al2[t, 1] = 0.0                              # an accepted step whose alpha says reject
    fails(r"chain 1 .*step %d: the trace accepted" % t, alpha=al2)
    ep2 = ep.copy()
    ep2[40:, 0] = ep2[40:, 0] * (1.0 + 1e-9)     # frozen after n_adapts = 30, but not the adapted value
    fails(r"chain 0 .*step 39", eps=ep2)
    mi2 = mi.copy()
    mi2[2, 10:, 0] = 1.0 + 2.0 ** -52
    fails(r"chain 0 .*step 9: no window closed", Minv=mi2)
    e0 = ep.copy()
    e0[0, 1] *= 2.0
    fails(r"chain 1 .*step 0: eps\[0\]", eps=e0)


# ----------------------------------------------------------------------------------------------- the two adaptor bounds, certified
def _replay_ratios(case, tr):
    """the audit's replay in float64 against the same replay in longdouble: worst |difference| / bound for log eps and for Minv"""
    z, _, al, ep, _, mi = tr
    worst_e = worst_m = 0.0
    for c in range(case.nchains):
        ads = [ha.Adaptor(case.m, case.adapts, ep[0, c], case.delta, ft=ft) for ft in (float, np.longdouble)]
        win_first, k_before = None, 0
        for t in range(1, min(case.adapts, case.itr) + 1):
            if ads[0].window_start <= t <= ads[0].window_end and win_first is None:
                win_first = t
            mu = float(ads[0].mu)
            for ad in ads:
                ad.adapt(z[:, t, c], al[t, c])
            last = t == case.adapts and ads[0].t > 0
            vals = [float(ad.log_eps_bar) if last else float(np.log(ad.eps)) for ad in ads]
            k = ads[0].t if not ads[0].closed else k_before + 1
            bound = ha.logeps_bar_bound(k, mu, ads[0].max_abs_log_eps) if last else ha.logeps_bound(k, mu)
            # the float64 recursion itself, against longdouble; and the device's column (here: the oracle's) against the float64 replay
            worst_e = max(worst_e, abs(float(ads[0].log_eps_bar if last else ads[0].log_eps) - float(ads[1].log_eps_bar if last else ads[1].log_eps)) / bound,
                          abs(vals[0] - vals[1]) / bound)
            if ads[0].closed:
                want, mbound = ha.window_minv(z[:, win_first:t + 1, c])
                worst_m = max(worst_m, float(np.max(np.abs(np.asarray(ads[0].minv, dtype=np.longdouble) - want) / mbound)))
                if t + 1 <= case.itr:
                    assert np.array_equal(np.asarray(ads[0].minv, dtype=np.float64), mi[:, t + 1, c])
                    for ad in ads:
                        ad.eps = ad.ft(ep[t + 1, c])
                        ad.restart(ep[t + 1, c])
                win_first = None
            k_before = ads[0].t
    return worst_e, worst_m


def test_the_adaptor_bounds_are_certified_against_longdouble():
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, "this check needs a longdouble wider than float64"
    worst_e = worst_m = 0.0
    for case in REAL_CASES:
        e, m = _replay_ratios(case, _trace(case))
        print("%s: float64 against longdouble replay: log eps %.3g of its bound, Minv %.3g of its bound" % (case.name, e, m))
        worst_e, worst_m = max(worst_e, e), max(worst_m, m)
    print("worst: log eps %.3g, Minv %.3g" % (worst_e, worst_m))
    assert worst_e <= 0.25 and worst_m <= 0.25
    assert worst_m > 0.0     # (at least one case closes a window)


# ----------------------------------------------------------------------------------------------- the restatements
def test_adaptor_and_search_are_the_samplers_statements_bit_for_bit():
    from subspaceinference_jl_amd import samplers
    rng = np.random.default_rng(3)
    for n_adapts, steps in ((0, 5), (2, 5), (19, 30), (30, 60), (200, 260), (40, 40)):
        a, b = samplers.StanAdaptor(3, n_adapts, 0.37), ha.Adaptor(3, n_adapts, 0.37)
        assert (a.window_start, a.window_end, a.window_splits) == (b.window_start, b.window_end, b.window_splits)
        for _ in range(steps):
            z, acc = rng.standard_normal(3) * np.array([0.1, 1.0, 7.0]), float(rng.random() * 1.2)
            changed = a.adapt(z, acc)
            b.adapt(z, acc)
            assert a.eps == b.eps and np.array_equal(a.minv, b.minv) and a.hbar == b.hbar and a.log_eps_bar == b.log_eps_bar
            assert b.closed or not changed

    class Fixed:
        def __init__(self, v):
            self.v = v

        def standard_normal(self, n):
            assert n == self.v.size
            return self.v
    mu = np.array([0.5, -1.0, 2.0])
    tols = (ha.ma.LP_RTOL_F64, ha.ma.G_RTOL_F64, ha.ma.G_ATOL_F64)
    for scale in (1.0, 30.0, 0.02, 1e-4):      # searches that go up, down, and far down
        fn = lambda z: (-0.5 * scale * float((z - mu) @ (z - mu)), -scale * (z - mu))
        for k in range(4):
            z, rho = rng.standard_normal(3), rng.standard_normal(3)
            lp, g = fn(z)
            want = samplers.find_good_stepsize(fn, z, lp, g, Fixed(rho))
            got, _, evals = ha.search(fn, z, lp, g, rho, tols)
            assert got == want and 2 <= evals <= 201, (scale, k, got, want, evals)


def test_window_schedule_of_the_library_is_stan_adaptors(si):
    from subspaceinference_jl_amd import samplers
    for n in range(0, 2001):
        ad = samplers.StanAdaptor(1, n, 0.1)
        assert si._capi.host_hmc_windows(n) == (ad.window_start, ad.window_end, ad.window_splits), n


def test_philox_hmc_has_the_host_samplers_stationary_moments():
    """tests/test_capi_cpu.py::test_gradient_samplers_on_gaussian_target, its target N(mu, I), its tolerances (mean within 0.2,
    variance within 0.3 after 500 of 6000 samples, acceptance statistic in (0.3, 1]) -- for oracle_trace on the Philox stream"""
    mu = np.array([0.5, -1.0, 2.0])
    fn = lambda z: (-0.5 * float((z - mu) @ (z - mu)), -(z - mu))
    case = ha.Case("gauss", None, 3, 1.0, True, nchains=1, itr=6000, seed=1, chain_id0=0)
    z, lp, al, ep, g, mi = ha.oracle_trace(case, fn)
    burn = z[:, 501:, 0]
    assert np.all(np.abs(burn.mean(axis=1) - mu) < 0.2)
    assert np.all(np.abs(burn.var(axis=1) - 1.0) < 0.3)
    assert 0.3 < float(al[1:, 0].mean()) <= 1.0
    assert np.all(ep[3001:, 0] == ep[3001, 0]) and not np.all(mi[:, -1, 0] == 1.0)


# ----------------------------------------------------------------------------------------------- the binding
def test_the_wrapper_is_bound_to_the_exported_symbols_and_the_header_declares_them(si):
    import inspect
    from ctypes import POINTER, c_double, c_int32, c_int64, c_uint64, c_void_p
    sig = si._capi.SIGNATURES
    assert sig["si_sample_hmc"] == (c_int32, [c_void_p, c_int64, c_int64, c_double, c_double, c_uint64, c_int32, c_int32] + [c_void_p] * 6)
    assert sig["si_hmc_kernel_info"] == (c_int32, [c_void_p, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32)])
    assert sig["si_host_hmc_windows"] == (c_int32, [c_int64, POINTER(c_int64), POINTER(c_int64), c_void_p, c_int32])
    lib = si.load()
    for name in ("si_sample_hmc", "si_hmc_kernel_info", "si_host_hmc_windows"):
        fn = getattr(lib, name)            # AttributeError: the library does not export it
        assert fn.argtypes == sig[name][1] and fn.restype is sig[name][0]
    assert callable(si.Context.sample_hmc) and callable(si.Context.hmc_kernel_info) and callable(si._capi.host_hmc_windows)
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "subspace_hip.h")).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", header)
    assert ("int32_t si_sample_hmc(si_ctx* ctx, int64_t itr, int64_t n_adapts, double sigma_z, double delta, uint64_t seed, int32_t chain_id0, "
            "int32_t nchains, double* Z_out , double* lp_out , double* alpha_out , double* eps_out , double* G_out , double* Minv_out );") in flat
    assert "int32_t si_hmc_kernel_info(si_ctx* ctx, int32_t* fused_out, int32_t* passes_out, int32_t* search_rounds_out);" in flat
    assert "int32_t si_host_hmc_windows(int64_t n_adapts, int64_t* window_start, int64_t* window_end, int64_t* splits, int32_t cap);" in flat
    # a NULL context is refused before anything touches a device
    assert lib.si_sample_hmc(None, 1, 0, 0.1, 0.8, 0, 0, 1, None, None, None, None, None, None) == si._capi.SI_ERR_INVALID
    assert lib.si_hmc_kernel_info(None, None, None, None) == si._capi.SI_ERR_INVALID
    # the opt-in keyword of the Python API, off by default and keyword-only; n_adapts = None is the reference's round(itr / 2)
    for fn in (si.sub_inference, si.subspace_inference):
        p = inspect.signature(fn).parameters["device_sampler"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert [ha.n_adapts_of(i) for i in (1, 2, 3, 5, 7, 400)] == [0, 1, 2, 2, 4, 200]
    assert math.isclose(inspect.signature(si.Context.sample_hmc).parameters["delta"].default, 0.8)
