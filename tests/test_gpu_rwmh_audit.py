"""The device samplers, transition by transition (tests/rwmh_audit.py; its case list is certified on the oracle alone by
tests/test_rwmh_audit_cpu.py): every form behind si_sample_rwmh, si_sample_rwmh_weights and the step-wise session, at the M where
the kernels branch, with proposals that move and chains that accept about half of them.

The audit takes the device's own previous state as given, so no decision has to stay in lockstep with another chain: every step
of every trace is a reject (bit copies) or an accept within 16 ulp on z of Z[:, t-1] + sigma_z n_t and within the project's
log-density tolerance of the fp64 oracle's density; decisions, acceptance counts and weight samples are checked as
tests/rwmh_audit.py says.  The caps are conditions: both branches in every chain, no undecidable step in fp64, at most 5 % with
SI_F32.

Which form runs (csrc/capi_sample.hip, sample_rwmh_impl), in the order it is tried in mode 1 (mode 3: the same, generic kernels only):
  one-workgroup loop (kernels_chain.hip)        chain_loop_applies: fp64 Dense chain with a fused head, no prior, M <= 1024,
                                                2 N B <= 3e6 -- MODEL_A (N = 1218, B = 200: 4.9e5) at every M <= 1024, any number of
                                                chains; P in LDS while N M doubles fit beside the images (M = 1, 2), from global above
  grid loop (kernels_chain_grid.hip)            fused_ok, no prior, C <= fw_slots, G C <= num_cu with G = ceil(B / 16 nb): MODEL_A at
                                                M = 1025 (G = 13), MODEL_B (G = 63, 2 chains), MODEL_C (G = 57, 3 chains; wide head:
                                                no fused tail, hence never specialised)
    specialised (chain_spec.inc)                ... and a fused narrow head, out B <= 1024, M <= 256: MODEL_B at M <= 256; its
                                                register-resident P rows at M <= 32 (rs = 256 here): M = 31 -- reported by
                                                chain_kernel_info(), asserted below
  launch per step (kernels_stream.hip)          everything else: the prior case, conv chains, SI_F32; mode 2 (rwmh_tail_kernel:
                                                C <= fw_slots, no prior) and mode 0 (rwmh_propose_kernel / rwmh_accept_kernel)
The one-workgroup and generic grid loops report nothing of their own; for them the derivation above stands in, and
chain_kernel_info() must at least say that no specialised loop ran.
"""
import time

import numpy as np
import pytest

from tests import rwmh_audit as ra

pytestmark = pytest.mark.gpu


def _cached(density):
    """the traces of two modes are bit-identical where the project is right: the second audit then costs no oracle time"""
    memo = {}

    def f(z):
        k = np.ascontiguousarray(z, dtype=np.float64).tobytes()
        if k not in memo:
            memo[k] = density(z)
        return memo[k]
    return f


def _setup(si, ctx, case):
    pb = ra.problem(case)
    ctx.infer_setup(pb.table, pb.n, case.m, pb.w, pb.p, pb.x, pb.y, case.sigma_m,
                    compute_dtype=si._capi.SI_F32 if case.f32 else si._capi.SI_F64)
    if case.prior > 0.0:
        ctx.set_prior(case.prior)   # (si_infer_setup switches the prior off: set it afterwards)
    return pb


def _expect_specialised_loop(case, mode):
    return case.model == ra.MODEL_B and mode == 1 and case.m <= 256


def _audit(case, pb, density, z, lp, acc, tag, w=None, reconstruct=None):
    rep = ra.audit(z, lp, acc, density, case.sigma_z, case.seed, case.chain_id0, case.lp_rtol, W=w, reconstruct=reconstruct)
    print("%s %s: %s" % (case.name, tag, rep.line()))
    assert rep.steps == (case.itr - 1) * case.nchains
    if case.itr > 1:
        ra.check_caps(rep, case.f32)
    return rep


SAMPLE_CASES = [c for c in ra.CASES if c.how == "sample"]


@pytest.mark.parametrize("case", SAMPLE_CASES, ids=lambda c: c.name)
def test_every_transition_of_si_sample_rwmh(si, gpu_ctx, case):
    """cases A, A', B, B', C, D, E, G and I of the list through si_sample_rwmh in every mode the case names; traces of two modes
    of one case must also be the same bits (tests/test_gpu_chain.py, test_gpu_chain_grid.py: now at M = 33 .. 1025 as well)"""
    try:
        pb = _setup(si, gpu_ctx, case)
        density = _cached(pb.density)
        out = {}
        for mode in case.modes:
            gpu_ctx.set_chain_loop(mode)
            t0 = time.perf_counter()
            out[mode] = gpu_ctx.sample_rwmh(case.itr, case.sigma_z, seed=case.seed, chain_id0=case.chain_id0, nchains=case.nchains)
            dt = time.perf_counter() - t0
            d, l, msg = gpu_ctx.chain_kernel_info()
            print("%s mode %d: %.3f s, density_specialised %s, loop_specialised %s" % (case.name, mode, dt, d, l))
            assert l == _expect_specialised_loop(case, mode), (case.name, mode, d, l, msg)
            if mode == 3:
                assert not d, (case.name, msg)   # the generic kernels when asked for
            if l:   # what hiprtc cost: the same call again runs the kernels already built
                t0 = time.perf_counter()
                again = gpu_ctx.sample_rwmh(case.itr, case.sigma_z, seed=case.seed, chain_id0=case.chain_id0, nchains=case.nchains)
                dt2 = time.perf_counter() - t0
                print("%s mode %d: first call %.3f s, second call %.3f s (run-time compilation: %.3f s)" % (case.name, mode, dt, dt2, dt - dt2))
                assert all(np.array_equal(a, b) for a, b in zip(out[mode], again))
        for mode in case.modes:
            _audit(case, pb, density, *out[mode], "mode %d" % mode)
        first = case.modes[0]
        for mode in case.modes[1:]:
            for a, b, what in zip(out[first], out[mode], ("Z", "lp", "acc")):
                assert np.array_equal(a, b), "%s: %s of mode %d differs from mode %d" % (case.name, what, mode, first)
    finally:
        gpu_ctx.set_chain_loop(1)
        gpu_ctx.set_prior(0.0)


def test_the_conv_case_is_the_conv_tests_first_case():
    from tests.test_gpu_conv import CASES
    assert ra.CONV_MODELS["conv0"] == CASES[0]


def test_every_transition_of_the_stepwise_session(si, gpu_ctx):
    """case F: si_rwmh_begin / step_eval / step_accept / end (sw_Z, sw_lp) at M = 65, the caller handing the SSE back unchanged;
    and the same bits as si_sample_rwmh (tests/test_gpu_parity.py holds that at M = 4)"""
    case = ra.CASE_BY_NAME["F-M65-stepwise"]
    try:
        pb = _setup(si, gpu_ctx, case)
        gpu_ctx.set_chain_loop(1)
        gpu_ctx.rwmh_begin(case.itr, case.sigma_z, case.seed, case.chain_id0, case.nchains)
        for _ in range(case.itr):
            gpu_ctx.rwmh_step_accept(gpu_ctx.rwmh_step_eval())
        z, lp, acc = gpu_ctx.rwmh_end()
        _audit(case, pb, _cached(pb.density), z, lp, acc, "step-wise")
        gpu_ctx.set_chain_loop(0)
        ref = gpu_ctx.sample_rwmh(case.itr, case.sigma_z, seed=case.seed, chain_id0=case.chain_id0, nchains=case.nchains)
        assert np.array_equal(z, ref[0]) and np.array_equal(lp, ref[1]) and np.array_equal(acc, ref[2])
    finally:
        gpu_ctx.set_chain_loop(1)
        gpu_ctx.set_prior(0.0)


def test_every_transition_with_the_output_map(si, gpu_ctx):
    """case H: si_sample_rwmh_weights in mode 1 (the one-workgroup loop, then ONE K4 pass over all samples) and mode 0 (K4's own
    output selected on accept, through the ring): W[:, t] is a bit copy on rejects and si_reconstruct(Z[:, t]) on every step
    (the standard of tests/test_gpu_boundary_r3.py)"""
    case = ra.CASE_BY_NAME["H-M33-weights"]
    try:
        pb = _setup(si, gpu_ctx, case)
        density = _cached(pb.density)
        out = {}
        for mode in case.modes:
            gpu_ctx.set_chain_loop(mode)
            out[mode] = gpu_ctx.sample_rwmh_weights(case.itr, case.sigma_z, seed=case.seed, chain_id0=case.chain_id0, nchains=case.nchains)
            assert not gpu_ctx.chain_kernel_info()[1]
        gpu_ctx.set_chain_loop(1)
        for mode in case.modes:
            z, lp, acc, w = out[mode]
            _audit(case, pb, density, z, lp, acc, "weights, mode %d" % mode, w=w, reconstruct=lambda v: gpu_ctx.reconstruct(v)[:, 0])
        for a, b in zip(out[case.modes[0]], out[case.modes[1]]):
            assert np.array_equal(a, b)
    finally:
        gpu_ctx.set_chain_loop(1)
        gpu_ctx.set_prior(0.0)
