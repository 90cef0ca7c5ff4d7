"""Which sampler form a si_sample_rwmh call runs (csrc/capi_sample.hip, sample_rwmh_impl), told by the launches it counts.

The three forms give the same bits (tests/test_gpu_chain.py, test_gpu_chain_grid.py, test_gpu_rwmh_audit.py), so a call that
falls through to a slower form passes every other test.  The SI_K_RWMH class of stats() counts one launch per device-resident
loop, one for rwmh_init, one per propose that is not folded into the tail of the transition before it, and one per tail or
accept; with chain_kernel_info() that tells the forms apart:

  one-workgroup loop / grid loop           1
  per step, fused tail (mode 2)            init + the first propose + itr tails        = itr + 2
  per step, separate kernels               init + itr (propose + accept)               = 2 itr + 1

The first six rows are also audited transition by transition (tests/rwmh_audit.py), so that the count sits on a correct chain;
the oracle's own trace of each case reaches both branches in every chain, which lets the caps be held as conditions.
"""
from dataclasses import dataclass

import numpy as np
import pytest

from tests import rwmh_audit as ra

pytestmark = pytest.mark.gpu

ITR = 12


@dataclass(frozen=True)
class Row:
    case: ra.Case
    mode: int                 # set_chain_loop
    launches: int             # stats()["rwmh"]["launches"] of ONE call
    loop_specialised: int     # chain_kernel_info()[1]
    audited: bool = True


def _case(name, model, m, nchains, **kw):
    return ra.Case(name, model, m, (), nchains=nchains, itr=ITR, **kw)


A = _case("forms-A", ra.MODEL_A, 33, 3)
B = _case("forms-B", ra.MODEL_B, 31, 2)
ROWS = [
    Row(A, 1, 1, 0),                                                                   # one-workgroup loop
    Row(B, 1, 1, 1),                                                                   # grid loop, specialised
    Row(B, 3, 1, 0),                                                                   # grid loop, generic
    Row(A, 2, ITR + 2, 0),                                                             # per step, fused tail
    Row(A, 0, 2 * ITR + 1, 0),                                                         # per step, separate kernels
    Row(_case("forms-A-prior", ra.MODEL_A, 33, 3, prior=0.7), 1, 2 * ITR + 1, 0),      # the prior: no loop, no fused tail
    # Conv chains carry one chain per pass of launches: 2 chains > fw_slots, no fused tail
    Row(_case("forms-conv", ("conv", "conv0"), 5, 2, sigma_z=0.8), 1, 2 * ITR + 1, 0, audited=False),
]


def _setup(si, ctx, case):
    pb = ra.problem(case)
    ctx.infer_setup(pb.table, pb.n, case.m, pb.w, pb.p, pb.x, pb.y, case.sigma_m)
    if case.prior > 0.0:
        ctx.set_prior(case.prior)   # (si_infer_setup switches the prior off: set it afterwards)
    return pb


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "%s-mode%d" % (r.case.name, r.mode))
def test_the_call_runs_the_form_it_ran_before(si, gpu_ctx, row):
    case = row.case
    try:
        _setup(si, gpu_ctx, case)
        gpu_ctx.set_chain_loop(row.mode)
        gpu_ctx.reset_stats()
        z, lp, acc = gpu_ctx.sample_rwmh(case.itr, case.sigma_z, seed=case.seed, chain_id0=case.chain_id0, nchains=case.nchains)
        launches = gpu_ctx.stats()["rwmh"]["launches"]
        _, loop_spec, msg = gpu_ctx.chain_kernel_info()
        print("%s mode %d: %d rwmh launches, loop_specialised %d" % (case.name, row.mode, launches, loop_spec))
        assert launches == row.launches, (case.name, row.mode, launches, row.launches)
        assert loop_spec == row.loop_specialised, (case.name, row.mode, loop_spec, msg)
        if row.audited:
            # the case itself, on the oracle alone: both branches in every chain, no undecidable step
            ra.check_caps(ra.audit_case(case, *ra.cached_oracle_trace(case)))
            rep = ra.audit_case(case, z, lp, acc)
            print("%s mode %d: %s" % (case.name, row.mode, rep.line()))
            assert rep.steps == (case.itr - 1) * case.nchains
            ra.check_caps(rep)
    finally:
        gpu_ctx.set_chain_loop(1)
        gpu_ctx.set_prior(0.0)


def test_the_output_map_of_the_loop_is_one_k4_pass(si, gpu_ctx):
    """si_sample_rwmh_weights on the one-workgroup loop's class: the loop, then ONE K4 pass over all itr * C samples"""
    case = A
    try:
        _setup(si, gpu_ctx, case)
        gpu_ctx.set_chain_loop(1)
        gpu_ctx.reset_stats()
        z, _, _, w = gpu_ctx.sample_rwmh_weights(case.itr, case.sigma_z, seed=case.seed, chain_id0=case.chain_id0, nchains=case.nchains)
        st = gpu_ctx.stats()
        assert st["rwmh"]["launches"] == 1 and st["reconstruct"]["launches"] == 1, (st["rwmh"], st["reconstruct"])
        assert not gpu_ctx.chain_kernel_info()[1]
        assert w.shape == (ra.problem(case).n, case.itr, case.nchains) and np.all(np.isfinite(w))
    finally:
        gpu_ctx.set_chain_loop(1)
