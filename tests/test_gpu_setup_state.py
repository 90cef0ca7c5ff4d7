"""What the library knows about the chain set up lives and dies with the set-up: a set-up that was dropped refuses every entry
point, a step-wise session does not survive a new set-up, a set-up on a used context equals the same set-up on a fresh one bit
for bit -- whatever was set up before it -- and the training and the inference set-up describe a chain the same way."""
import numpy as np
import pytest

from tests import rwmh_audit
from oracle import subspace_oracle as so
from subspaceinference_jl_amd import _capi
from subspaceinference_jl_amd._capi import SI_ERR_STATE, SI_F32, SI_F64, SubspaceError

pytestmark = pytest.mark.gpu

R, I = so.ACT_RELU, so.ACT_IDENTITY


def _chain(dims, acts, b, m, seed):
    rng = np.random.default_rng(seed)
    table, n = so.layer_table(list(dims), list(acts))
    return dict(table=table, n=n, m=m, w=0.3 * rng.standard_normal(n), p=np.asfortranarray(0.05 * rng.standard_normal((n, m))),
                x=np.asfortranarray(rng.standard_normal((dims[0], b))), y=np.asfortranarray(rng.standard_normal((dims[-1], b))),
                xnew=np.asfortranarray(rng.standard_normal((dims[0], 10))), z=0.1 * rng.standard_normal(m))


def _setup(ctx, c, dtype=SI_F64):
    ctx.infer_setup(c["table"], c["n"], c["m"], c["w"], c["p"], c["x"], c["y"], 0.8, compute_dtype=dtype)


SMALL = _chain((2, 16, 16, 1), (R, R, I), 64, 3, 1)        # the one-workgroup loop
GRID5 = _chain((2, 20, 20, 5), (R, R, I), 96, 3, 2)        # a head of 5: no fused head, the generic grid loop
SPEC = _chain((2, 40, 40, 1), (R, R, I), 1024, 3, 3)       # the grid loop, specialised at run time
WIDE = _chain(rwmh_audit.MODEL_C[0], rwmh_audit.MODEL_C[1], rwmh_audit.MODEL_C[2], 3, 4)   # sigmoid head of 9: the per-layer route


def _refused(call, *args, **kw):
    with pytest.raises(SubspaceError) as bad:
        call(*args, **kw)
    assert bad.value.code == SI_ERR_STATE, (call.__name__, bad.value.code, str(bad.value))


def _same(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert np.array_equal(np.asarray(u), np.asarray(v))


def test_a_dropped_setup_refuses_everything(si):
    c = SMALL
    with si.Context(0) as fresh:
        _setup(fresh, c)
        want = fresh.sample_rwmh(5, 0.1, seed=1)
    with si.Context(0) as ctx:
        _setup(ctx, c)
        ctx.logdensity(c["z"])
        # no finished construction to take W_swa / P from: the set-up fails after the old one was freed
        _refused(ctx.infer_setup, c["table"], c["n"], c["m"], None, None, c["x"], c["y"], 0.8)
        z = c["z"]
        _refused(ctx.logdensity, z)
        _refused(ctx.logdensity_grad, z)
        _refused(ctx.forward, z)
        _refused(ctx.predict, z, c["xnew"])
        _refused(ctx.reconstruct, z)
        _refused(ctx.sample_rwmh, 5, 0.1, seed=1)
        _refused(ctx.sample_mala, 5, 0.1, seed=1)
        _refused(ctx.rwmh_begin, 4, 0.1, seed=3)
        _refused(ctx.rwmh_step_eval, on_device=True)
        _refused(ctx.set_prior, 2.0)
        _refused(ctx.infer_set_likelihood, 1)
        assert ctx.infer_likelihood_info() == 0
        assert ctx.decoder_info()[0] == 0
        _setup(ctx, c)
        _same(ctx.sample_rwmh(5, 0.1, seed=1), want)


def test_a_session_does_not_survive_a_new_setup(si):
    def session(ctx):
        ctx.rwmh_begin(4, 0.1, seed=3, nchains=2)
        for _ in range(4):
            ctx.rwmh_step_accept(ctx.rwmh_step_eval())
        return ctx.rwmh_end()

    with si.Context(0) as fresh:
        _setup(fresh, GRID5)
        want = session(fresh)
    with si.Context(0) as ctx:
        _setup(ctx, SMALL)
        ctx.rwmh_begin(4, 0.1, seed=3, nchains=2)
        ctx.rwmh_step_accept(ctx.rwmh_step_eval())
        sse = ctx.rwmh_step_eval()          # evaluated, not accepted
        _setup(ctx, GRID5)
        _refused(ctx.rwmh_step_accept, sse)
        _refused(ctx.rwmh_step_eval)
        _refused(ctx.rwmh_end)
        _refused(ctx.rwmh_sse_ptr)
        ctx.sample_rwmh(3, 0.1, seed=4)     # not refused: no session is open
        _same(session(ctx), want)


def _probe(ctx, c):
    out = list(ctx.sample_rwmh(6, 0.1, seed=2, nchains=3))
    info = ctx.chain_kernel_info()[:2]
    lp, g = ctx.logdensity_grad(c["z"])
    return out + [lp, g, ctx.predict(c["z"], c["xnew"])], info


def test_setup_after_setup_equals_a_fresh_context(si):
    order = [(SPEC, SI_F64), (SMALL, SI_F64), (WIDE, SI_F64), (SMALL, SI_F32)]
    want = []
    for c, dtype in order:
        with si.Context(0) as fresh:
            _setup(fresh, c, dtype)
            want.append(_probe(fresh, c))
    assert want[0][1][1], "the first set-up is meant to run the grid loop specialised at run time"
    with si.Context(0) as ctx:
        for (c, dtype), (out_ref, info_ref) in zip(order, want):
            _setup(ctx, c, dtype)
            out, info = _probe(ctx, c)
            assert info == info_ref
            _same(out, out_ref)


@pytest.mark.parametrize("dims,acts,b", [((4, 24, 24, 2), (so.ACT_TANH, R, I), 128), rwmh_audit.MODEL_C],
                         ids=["narrow_head_4_24_24_2", "wide_head_6_40_24_9"])
def test_training_and_inference_setups_agree_on_the_chain(gpu_ctx, dims, acts, b):
    """train_grad over the full batch (mse, batch_max = B) against logdensity_grad with W_swa = w0, P = I, z = 0, sigma_m = 1: the
    two differ by the scale of Delta_L, -2 / (out B).  Both set-ups take fuse_tail and the slot counts from one builder.  The
    tolerance is the one test_gpu_parity.py holds the training gradient to."""
    rng = np.random.default_rng(7)
    table, n = so.layer_table(list(dims), list(acts))
    w0 = (0.3 * rng.standard_normal(n)).astype(np.float32)
    x = np.asfortranarray(rng.standard_normal((dims[0], b)))
    y = np.asfortranarray(rng.standard_normal((dims[-1], b)))
    gpu_ctx.infer_setup(table, n, n, w0.astype(np.float64), np.asfortranarray(np.eye(n)), x, y, 1.0)
    _, g_inf = gpu_ctx.logdensity_grad(np.zeros(n))
    gpu_ctx.train_setup(table, n, w0, x, y, b, 0, 0.1, compute_dtype=_capi.SI_F64)
    gpu_ctx.train_grad(np.arange(b), b)
    g_tr = gpu_ctx.train_grad_get()
    want = (-2.0 / (dims[-1] * b)) * g_inf
    print(dims, "max |want|", np.abs(want).max(), "max |g_tr - want|", np.abs(g_tr - want).max())
    assert np.abs(want).max() > 0.0
    assert np.allclose(g_tr, want, rtol=1e-8, atol=1e-10 * max(1.0, np.abs(want).max()))
