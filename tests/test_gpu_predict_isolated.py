"""si_predict leaves the chain set up as it found it: one chain per density route (csrc/capi_infer.hip, eval_density), every
result the context gives before a predict call is given again, bit for bit, after it, and a second predict call returns the bits
of the first.  predict evaluates on data of its own width Bn with a workspace of its own; whatever it touched of the set-up's B,
activation stride, SSE block count, compute type or buffers would show in the calls that follow it.

Only the public Python API is used, so the file holds for any library that keeps the interface.  That predict's own numbers are
right is held elsewhere (PREDICT_B = 37 in tests/dense_routes.py, tests/test_gpu_dense_exact.py, tests/test_gpu_conv_exact.py).
"""
import numpy as np
import pytest

from tests import rwmh_audit as ra

pytestmark = pytest.mark.gpu

M, NCOLS, BN, ITR = 5, 3, 37, 12   # Bn = 37: no multiple of 16, and none of the B of the problems below (200, 900, 7)

# one chain per route of the density: (problem of tests/rwmh_audit.py, SI_F32)
CHAINS = {
    "A-f64": (ra.MODEL_A, False),            # fused head, narrow class: the single launch for the density, the per-layer launches for forward / predict
    "C-f64": (ra.MODEL_C, False),            # no fused head: the outputs stay in the activation buffer, chain slots act_elems apart
    "A-f32": (ra.MODEL_A, True),             # the fp32 per-layer launches; predict runs in fp64 all the same
    "conv0-f64": (("conv", "conv0"), False),   # spatial input: X re-laid channel-fastest, for the set-up's B and again for Bn
}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).copy()


def _record(ctx, case, z):
    """the bits of everything the context computes from the set-up's own data"""
    out = {"logdensity": _bits(ctx.logdensity(z)), "forward": _bits(ctx.forward(z[:, 0]))}
    lp, g = ctx.logdensity_grad(z[:, 0])
    out["grad_lp"], out["grad"] = _bits([lp]), _bits(g)
    zs, lps, acc = ctx.sample_rwmh(ITR, case.sigma_z, seed=case.seed, chain_id0=case.chain_id0, nchains=NCOLS)
    out["rwmh_Z"], out["rwmh_lp"], out["rwmh_acc"] = _bits(zs), _bits(lps), _bits(acc)
    return out


@pytest.mark.parametrize("name", list(CHAINS))
def test_predict_leaves_the_set_up_untouched(si, gpu_ctx, name):
    model, f32 = CHAINS[name]
    case = ra.Case(name, model, M, (1,), nchains=NCOLS, itr=ITR, f32=f32)
    pb = ra.problem(case)
    rng = np.random.default_rng(37)
    z = np.asfortranarray(0.5 * rng.standard_normal((M, NCOLS)))
    xnew = np.asfortranarray(rng.standard_normal((pb.x.shape[0], BN)))
    try:
        gpu_ctx.set_chain_loop(1)
        gpu_ctx.infer_setup(pb.table, pb.n, M, pb.w, pb.p, pb.x, pb.y, case.sigma_m,
                            compute_dtype=si._capi.SI_F32 if f32 else si._capi.SI_F64)
        before = _record(gpu_ctx, case, z)
        first = gpu_ctx.predict(z, xnew)
        assert first.shape == (pb.y.shape[0], BN, NCOLS) and np.all(np.isfinite(first))
        after = _record(gpu_ctx, case, z)
        for what in before:
            assert np.array_equal(before[what], after[what]), "%s: %s changed over a predict call" % (name, what)
        assert np.array_equal(_bits(first), _bits(gpu_ctx.predict(z, xnew))), "%s: the second predict call differs from the first" % name
    finally:
        gpu_ctx.set_chain_loop(1)
