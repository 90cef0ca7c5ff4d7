"""The four device samplers, bit for bit: si_sample_mala, si_sample_hmc, si_sample_nuts and si_fit_advi (csrc/kernels_mala.hip,
kernels_hmc.hip, kernels_nuts.hip, kernels_advi.hip over csrc/sampler_device.h).

The audits of these samplers compare lp and g through tolerances in places, so they cannot by themselves show that a change of the
kernels moved nothing.  Here every output array of the cases in tools/sampler_digests.py -- the smallest shapes that reach each
path: M = 1, odd M, a second lap of the thread-strided loops, several chains, the prior, window closes, divergent and non-finite
leaves, the ring wrap, the route that is not fused -- has the SHA-256 that tools/sampler_digests.py recorded on an MI355X in
tests/golden/device_sampler_digests.json.  A DELIBERATE change of the kernels' arithmetic re-records that file with the tool;
anything else that fails here has changed a chain's bits.

Then the one thing the shared chain state (ChainState, csrc/si_internal.h) adds: MALA, HMC and NUTS in turn on one context, with the
capacity growing across samplers and a smaller number of chains after a larger one, each call equal in every output to the same
call on a fresh context."""
import json
import os

import numpy as np
import pytest

from tests import mala_audit as ma
from tools import sampler_digests as sd

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_sampler_digests.json")))
IDS = ["%s/%s" % (s, n) for s, names in sd.CASES.items() for n in names]


def test_the_golden_file_holds_exactly_the_tools_cases():
    assert sorted(GOLDEN) == sorted(IDS)
    for key in IDS:
        assert sorted(GOLDEN[key]) == sorted(sd.OUTPUTS[key.split("/")[0]]), key


@pytest.mark.parametrize("key", IDS)
def test_every_output_has_the_recorded_bits(si, gpu_ctx, key):
    sampler, name = key.split("/")
    got = sd.digests_of(sampler, sd.run_case(si, gpu_ctx, sampler, name))
    assert got == GOLDEN[key], (key, [k for k in got if got[k] != GOLDEN[key][k]])


def test_one_chain_state_serves_the_three_samplers_in_turn(si):
    case = ma.CASE_BY_NAME["A-M33"]
    pb = ma.problem(case)
    calls = [("mala", 3), ("hmc", 8), ("nuts", 2), ("mala", 8), ("hmc", 3)]

    def run(ctx, sampler, c):
        kw = dict(seed=case.seed, chain_id0=case.chain_id0, nchains=c, grad=True)
        if sampler == "mala":
            return ctx.sample_mala(12, case.sigma_z, **kw)
        if sampler == "hmc":
            return ctx.sample_hmc(12, case.sigma_z, metric=True, **kw)
        return ctx.sample_nuts(6, case.sigma_z, max_depth=4, metric=True, leaf_cap=6 * 15, **kw)

    def setup(ctx):
        ctx.infer_setup(pb.table, pb.n, case.m, pb.w, pb.p, pb.x, pb.y, case.sigma_m)

    with si.Context(0) as shared:
        setup(shared)
        for sampler, c in calls:
            got = run(shared, sampler, c)
            with si.Context(0) as fresh:
                setup(fresh)
                want = run(fresh, sampler, c)
            assert len(got) == len(want)
            for i, (a, b) in enumerate(zip(got, want)):
                assert np.array_equal(a, b, equal_nan=True), (sampler, c, i)
