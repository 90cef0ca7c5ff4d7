"""The categorical and Bernoulli likelihoods (si_infer_set_likelihood) without a GPU: the definition of tests/likelihood_cases.py
against finite differences and closed forms, the header and the library's exports, the refusals of the API, and the certificate
of the RWMH cases on the definition alone -- every chain of every case both accepts and rejects and no step is undecidable at
fp64 (SI_F32: at most rwmh_audit.F32_UNDECIDABLE_CAP of the steps) -- which tests/test_gpu_likelihood.py then holds as conditions.
The same certificate for every (sampler, problem) pair of the gradient samplers (MALA, HMC, NUTS, ADVI), with the definition as the
value_grad of tests/mala_audit.py, hmc_audit.py, nuts_audit.py and advi_audit.py, which tests/test_gpu_likelihood_samplers.py holds
on the device; and the launch-geometry arithmetic behind the loop-branch tests of tests/test_gpu_likelihood.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from oracle import subspace_oracle as so
from tests import advi_audit as aa
from tests import hmc_audit as ha
from tests import likelihood_cases as lc
from tests import mala_audit as ma
from tests import nuts_audit as na
from tests import rwmh_audit as ra
from tests.rwmh_audit import AuditFailure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the definition -----------------------------------------------------------------------------------------------------------------
def _fd_problems():
    from tests import decoder_cases as dc
    out = [("cat-3", lc.dense_problem(3, 7, lc.CATEGORICAL)), ("cat-10-soft", lc.dense_problem(10, 7, lc.CATEGORICAL, soft=True)),
           ("ber-1", lc.dense_problem(1, 7, lc.BERNOULLI)), ("ber-3-soft", lc.dense_problem(3, 7, lc.BERNOULLI, soft=True)),
           ("conv", lc.conv_problem(7)), ("cat-3-prior", lc.dense_problem(3, 7, lc.CATEGORICAL).with_(prior=0.7))]
    pb = lc.dense_problem(3, 7, lc.CATEGORICAL)
    out.append(("cat-3-decoder", pb.with_(decoder=dc.random_decoder((pb.m, 4, pb.n), (lc.T, lc.I), seed=5))))
    # a head activation: the seed of the reverse pass is dvalue .* act'(yhat)
    out += [("head-%d-%d-act%d" % case, lc.head_problem(*case)) for case in lc.HEAD_CASES]
    out.append(("conv-bernoulli", lc.conv_problem(7, kind=lc.BERNOULLI)))
    return out


@pytest.mark.parametrize("name,pb", _fd_problems(), ids=lambda v: v if isinstance(v, str) else "")
def test_the_gradient_of_the_definition_is_its_finite_difference(name, pb):
    z = lc.points(pb, 1)[:, 0]
    lp, g = pb.density_grad(z)
    assert lp == pb.density(z)
    h = 1e-6
    for k in range(pb.m):
        e = np.zeros(pb.m)
        e[k] = h
        fd = (pb.density(z + e) - pb.density(z - e)) / (2.0 * h)
        # central differences: h^2 / 6 |f'''| truncation + eps |lp| / h rounding, both below 1e-6 of the scale here
        assert abs(fd - g[k]) <= 1e-6 * max(1.0, np.max(np.abs(g))), (name, k, fd, g[k])


def test_closed_forms_of_the_definition():
    for out, b in ((2, 1), (10, 7), (130, 37)):
        pb = lc.dense_problem(out, b, lc.CATEGORICAL)
        assert np.isclose(lc.value_w(pb.table, np.zeros(pb.n), pb.x, pb.y, lc.CATEGORICAL), -b * np.log(out), rtol=1e-14)
    for out, b in ((1, 1), (3, 7), (10, 37)):
        pb = lc.dense_problem(out, b, lc.BERNOULLI)
        assert np.isclose(lc.value_w(pb.table, np.zeros(pb.n), pb.x, pb.y, lc.BERNOULLI), -out * b * np.log(2.0), rtol=1e-14)
    # the categorical likelihood of one-hot labels is the log of the softmax probability of the labelled class, naively formed
    pb = lc.dense_problem(5, 7, lc.CATEGORICAL)
    yhat = so.forward(pb.table, pb.w, pb.x)
    naive = np.sum(pb.y * np.log(np.exp(yhat) / np.sum(np.exp(yhat), axis=0, keepdims=True)))
    assert np.isclose(lc.value_w(pb.table, pb.w, pb.x, pb.y, lc.CATEGORICAL), naive, rtol=1e-12)
    # soft labels are kept as written: the value is linear in Y, S_b is not normalised away
    soft = lc.dense_problem(5, 7, lc.CATEGORICAL, soft=True)
    assert not np.allclose(np.sum(soft.y, axis=0), 1.0)
    v1 = lc.value_w(soft.table, soft.w, soft.x, soft.y, lc.CATEGORICAL)
    v2 = lc.value_w(soft.table, soft.w, soft.x, 2.0 * soft.y, lc.CATEGORICAL)
    assert np.isclose(v2, 2.0 * v1, rtol=1e-13)
    # a last-layer bias of +-800 stays finite
    for kind, out in ((lc.CATEGORICAL, 3), (lc.BERNOULLI, 3)):
        pb = lc.dense_problem(out, 7, kind)
        for sign in (1.0, -1.0):
            w = pb.w.copy()
            w[pb.table[-1][4]] = sign * 800.0
            assert np.isfinite(lc.value_w(pb.table, w, pb.x, pb.y, kind))


# ---- header, exports, bindings ----------------------------------------------------------------------------------------------------
def test_the_header_declares_and_the_library_exports_both_symbols():
    import subspaceinference_jl_amd as si
    from subspaceinference_jl_amd import _capi
    raw = open(os.path.join(ROOT, "include", "subspace_hip.h")).read()
    for name, val in (("SI_LIK_GAUSSIAN", 0), ("SI_LIK_CATEGORICAL", 1), ("SI_LIK_BERNOULLI", 2)):
        assert re.search(r"^#define\s+%s\s+%d\s*$" % (name, val), raw, flags=re.M), name
        assert getattr(_capi, name) == val
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    assert re.search(r"\bint32_t\s+si_infer_set_likelihood\s*\(\s*si_ctx\s*\*\s*\w*\s*,\s*int32_t\s+\w+\s*\)\s*;", text)
    assert re.search(r"\bint32_t\s+si_infer_likelihood_info\s*\(\s*si_ctx\s*\*\s*\w*\s*,\s*int32_t\s*\*\s*\w+\s*\)\s*;", text)
    assert _capi.SIGNATURES["si_infer_set_likelihood"] == (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32])
    assert _capi.SIGNATURES["si_infer_likelihood_info"] == (ctypes.c_int32, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)])
    lib = si.load()
    kind = ctypes.c_int32(7)
    assert lib.si_infer_set_likelihood(None, 1) == _capi.SI_ERR_INVALID          # (a NULL ctx is refused, not read)
    assert lib.si_infer_likelihood_info(None, ctypes.byref(kind)) == _capi.SI_ERR_INVALID and kind.value == 7
    assert _capi.LIKELIHOODS == {"gaussian": 0, "categorical": 1, "bernoulli": 2}
    for f in ("infer_set_likelihood", "infer_likelihood_info"):
        assert callable(getattr(si.Context, f))


def test_api_keyword_and_refusals():
    import subspaceinference_jl_amd as si
    from subspaceinference_jl_amd import flux
    for f in (si.sub_inference, si.auto_inference, si.subspace_inference, si.autoencoder_inference):
        assert inspect.signature(f).parameters["likelihood"].default == "gaussian", f.__name__
    m = flux.Chain(flux.Dense(3, 2))
    data = flux.DataLoader(np.zeros((3, 4)), np.zeros((2, 4)))
    w, p = np.zeros(8), np.zeros((8, 1))
    # (all three are raised before a device is touched)
    with pytest.raises(si.SubspaceError, match="likelihood must be"):
        si.sub_inference(m, data, w, p, M=1, likelihood="poisson")
    with pytest.raises(si.SubspaceError, match="DimensionMismatch: likelihood"):
        si.sub_inference(m, flux.DataLoader(np.zeros((3, 4)), np.zeros((1, 4))), w, p, M=1, likelihood="categorical")
    with pytest.raises(si.SubspaceError, match="DimensionMismatch: likelihood"):
        si.sub_inference(m, flux.DataLoader(np.zeros((3, 4)), np.zeros((3, 4))), w, p, M=1, likelihood="bernoulli")
    node = flux.NeuralODE(flux.Chain(flux.Dense(2, 2)), (0.0, 1.0), saveat=[0.5, 1.0])
    with pytest.raises(si.SubspaceError, match="not available for NeuralODE"):
        si.sub_inference(node, flux.DataLoader(np.zeros((2, 3)), np.zeros((4, 3))), np.zeros(6), np.zeros((6, 1)), M=1,
                         likelihood="categorical")
    dec = flux.Chain(flux.Dense(1, 8))
    with pytest.raises(si.SubspaceError, match="likelihood must be"):
        si.auto_inference(m, data, dec, w, M=1, likelihood="x")


# ---- the certificate of the RWMH cases ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lc.RWMH_CASES, ids=lambda c: c.name)
def test_rwmh_cases_reach_both_branches_on_the_definition(case):
    pb = lc.rwmh_problem(case)
    dens = pb.density
    if case.f32:
        # what an fp32 density may return: the fp64 value off by up to 0.9e-5 of itself, a fixed function of z (tests/test_rwmh_audit_cpu.py)
        dens = lambda v: pb.density(v) * (1.0 + 0.9e-5 * np.cos(1e6 * float(np.sum(v))))
    z, lp, acc = lc.rwmh_oracle_trace(case, dens)
    rep = ra.audit(z, lp, acc, pb.density, case.sigma_z, case.seed, case.chain_id0, case.lp_rtol)
    print(case.name, rep.line(), rep.chain_accepts, rep.chain_rejects)
    ra.check_caps(rep, case.f32)
    assert rep.steps == (case.itr - 1) * case.nchains and rep.worst_z_ratio <= 1.0
    if not case.f32:
        assert rep.undecidable == 0 and rep.worst_lp_rel == 0.0
        # the margins are far from the tolerance: a device density within lp_rtol of the definition decides every step alike
        assert rep.min_margin_over_tol > 10.0


# ---- the launch geometry the branch tests of tests/test_gpu_likelihood.py and test_gpu_train_costs.py rely on ----------------------------
def test_the_branch_shapes_reach_their_branches():
    raw = open(os.path.join(ROOT, "subspaceinference.jl_amd", "csrc", "si_internal.h")).read()
    assert int(re.search(r"constexpr\s+int\s+SI_COST_MAX_BLOCKS\s*=\s*(\d+)\s*;", raw).group(1)) == lc.COST_MAX_BLOCKS
    waves = 4 * lc.COST_MAX_BLOCKS
    assert lc.logitce_geometry(33, 1100) == (64, 1100) and lc.logitce_geometry(10, 4103) == (16, 1026) and 4103 % 4 == 3
    for out, b in lc.COST_LAP_SHAPES:
        groups = lc.logitce_geometry(out, b)[1]
        assert waves < groups < 2 * waves                     # a second lap that most waves do not take
    # every shape of the suite so far stays on the first lap
    assert max(lc.logitce_geometry(o, max(lc.BATCHES))[1] for o in lc.CATEGORICAL_OUTS) <= waves
    for num_cu in (1, 64, 104, 228, 256, 304):
        b, cap = lc.capped_batch(num_cu), 4 * num_cu
        d = lc.CAPPED_OUT * b
        assert -(-d // 256) > cap and 256 * cap < d < 2 * 256 * cap          # the grid is capped; a ragged second lap
        assert lc.logitce_geometry(lc.CAPPED_OUT, b)[1] > 4 * cap             # ... and more column groups than waves
    assert lc.capped_batch(256) == 26300


# ---- the certificate of the gradient samplers' cases ------------------------------------------------------------------------------------
# On the definition alone, for every (sampler, problem) pair of likelihood_cases: the oracle's trace passes the sampler's audit under
# the sampler's own caps -- both branches in every chain, no undecidable step or search at fp64 -- and so does the trace of the
# definition moved to 0.9 of the stated tolerances (nuts_audit.perturbed), audited against the unmoved definition.  These are the
# conditions tests/test_gpu_likelihood_samplers.py holds on the device's traces.
PERTURB_SEEDS = (5, 6)


def _vgs(sp, case):
    vg = lc.sampler_problem(sp.name)[1]
    return [vg] + [lc.cached(na.perturbed(vg, case.tols, seed)) for seed in PERTURB_SEEDS]


@pytest.mark.parametrize("sp", lc.SAMPLER_PROBLEMS, ids=lambda s: s.name)
def test_mala_cases_on_the_definition(sp):
    case = lc.mala_case(sp)
    vg = lc.sampler_problem(sp.name)[1]
    for k, moved in enumerate(_vgs(sp, case)):
        rep = ma.audit_case(case, *ma.oracle_trace(case, value_grad=moved), value_grad=vg)
        print(sp.name, "moved" if k else "exact", rep.line())
        ma.check_caps(case, rep)
        if not sp.f32:
            assert rep.undecidable == 0 and rep.min_margin_over_tol > 10.0


@pytest.mark.parametrize("sp", lc.SAMPLER_PROBLEMS, ids=lambda s: s.name)
def test_hmc_cases_on_the_definition(sp):
    case = lc.hmc_case(sp)
    assert case.adapts == 20
    vg = lc.sampler_problem(sp.name)[1]
    for k, moved in enumerate(_vgs(sp, case)):
        rep = ha.audit_case(case, *ha.oracle_trace(case, value_grad=moved), value_grad=vg)
        print(sp.name, "moved" if k else "exact", rep.line())
        ha.check_caps(case, rep)


@pytest.mark.parametrize("sp", lc.SAMPLER_PROBLEMS, ids=lambda s: s.name)
def test_nuts_cases_on_the_definition(sp):
    case = lc.nuts_case(sp)
    vg = lc.sampler_problem(sp.name)[1]
    for k, moved in enumerate(_vgs(sp, case)):
        tr = na.oracle_trace(case, value_grad=moved)
        rep = na.audit_case(case, tr, value_grad=vg, check_oracle=(k == 0))
        print(sp.name, "moved" if k else "exact", rep.line(), sorted(na.coverage(case, tr)))
        na.check_caps(case, rep)
        if k > 0:
            # (with the oracle's checks on as well: the moved leaves and the moved search stay inside the stated tolerances)
            na.check_caps(case, na.audit_case(case, tr, value_grad=vg))
        if k == 0:
            # every problem reaches both U-turns, a kept state and chains whose trees differ
            assert na.coverage(case, tr) >= {"sub-tree U-turn", "tree U-turn", "sel = 0", "a chain waits"}, sp.name


@pytest.mark.parametrize("sp", lc.ADVI_PROBLEMS, ids=lambda s: s.name)
def test_advi_cases_on_the_definition(sp):
    case = lc.advi_case(sp)
    assert case.t > case.w                                      # the ring wraps
    vg = lc.sampler_problem(sp.name)[1]
    for k, moved in enumerate(_vgs(sp, case)):
        rep = aa.audit_case(case, *aa.oracle_trace(case, value_grad=moved), value_grad=vg)
        print(sp.name, "moved" if k else "exact", rep.line())
        assert rep.steps == case.t * case.nruns


def test_the_advi_exceptions_are_the_ones_the_elbo_bound_excludes():
    assert [sp.name for sp in lc.SAMPLER_PROBLEMS if not sp.advi] == ["cat65", "ber1", "conv"]
    assert len(lc.SAMPLER_PROBLEMS) == 11 and len(lc.ADVI_PROBLEMS) == 8


# (sampler, mutant): the trace a kernel with that mistake would produce on cat3 is still rejected with the likelihood as value_grad
AUDITS = {"mala": (ma, lc.mala_case), "hmc": (ha, lc.hmc_case), "nuts": (na, lc.nuts_case), "advi": (aa, lc.advi_case)}


@pytest.mark.parametrize("sampler,mutant", [("mala", "lp_stale"), ("hmc", "lp_stale"), ("nuts", "stale_gradient_edge"),
                                            ("advi", "no_minus_one")])
def test_the_audits_keep_their_teeth_on_the_likelihood(sampler, mutant):
    mod, make = AUDITS[sampler]
    assert mutant in mod.MUTANTS
    sp = lc.SAMPLER_BY_NAME["cat3"]
    case, vg = make(sp), lc.sampler_problem(sp.name)[1]
    tr = mod.oracle_trace(case, value_grad=vg, mutant=mutant)
    with pytest.raises(AuditFailure) as e:
        mod.audit_case(case, tr, value_grad=vg) if sampler == "nuts" else mod.audit_case(case, *tr, value_grad=vg)
    print(sampler, mutant, str(e.value)[:160])
