"""Every conv kernel instantiation shapes can reach, held bit for bit on lattice problems (tests/lattice.py): the chains of
tests/conv_routes.py::CASES, each the smallest that reaches the instantiations written next to it there, with the route
table that says so derived from the dispatch and proved complete on the CPU (tests/test_conv_exact_cpu.py: the union of the
cases' routes equals conv_routes.REACHABLE).  profiles/conv_exact_kernel_names.txt is the kernel trace of this file.

Per case, np.array_equal everywhere and lp within 4 ulp of the exact value (only the final combine rounds):
  * the sampling route (ping-pong forward, conv + pool fused without index), fp64 and SI_F32: forward, log-density for both
    targets, predict on new inputs;
  * the gradient route (kept outputs, conv + pool fused WITH the window index), fp64: lp and d lp / d z;
  * the whole weight gradient through si_train_grad: the N-vector, not three numbers of P'g -- a dW element that lands in
    another place of the same layer shows; full batch, shuffled, a subset that is no multiple of 16; then one Descent step;
  * the same call twice gives the same bits (split-K partials are reduced in a fixed order)."""
import numpy as np
import pytest

from oracle import subspace_oracle as so
from tests import conv_routes as cr
from tests import lattice as lat

pytestmark = pytest.mark.gpu

SI_F32, SI_F64 = 0, 1
ETA = 2.0 ** -3


def _setup(ctx, pb, y):
    ctx.infer_setup(pb.table, pb.n, pb.m, pb.w_swa, pb.p, pb.x, y, pb.sigma, compute_dtype=SI_F32 if pb.f32 else SI_F64)


@pytest.mark.parametrize("name", cr.NAMES)
@pytest.mark.parametrize("f32", [False, True])
def test_sampling_route_exact(gpu_ctx, name, f32):
    pb = cr.problem(name, f32)
    for tag, y in (("null", pb.y0), ("r", pb.y1)):
        _setup(gpu_ctx, pb, y)
        for c in range(pb.z.shape[1]):
            lat.assert_exact(gpu_ctx.forward(pb.z[:, c]), pb.yhat[c], "%s forward column %d" % (name, c))
        lp = gpu_ctx.logdensity(pb.z)
        for c, lpe in lat.lp_cases(pb, tag):
            lat.assert_lp(lp[c], lpe)
        assert np.array_equal(lp, gpu_ctx.logdensity(pb.z))
    # predict on new lattice inputs (an fp64 forward in either mode), another batch size: both columns stacked
    xn = np.asfortranarray(np.random.default_rng(7).integers(-2, 3, (pb.x.shape[0], 5)).astype(np.float64))
    out = gpu_ctx.predict(pb.z, xn)
    for c in range(pb.z.shape[1]):
        ref, _, _ = lat.forward_certified(pb.table, pb.w_swa + pb.p @ pb.z[:, c], xn, lat.F64_LIMIT)
        lat.assert_exact(out[:, :, c], ref, "%s predict column %d" % (name, c))


@pytest.mark.parametrize("name", cr.NAMES)
def test_gradient_route_exact(gpu_ctx, name):
    pb = cr.problem(name, False)
    lat.pool_ties_are_exact(pb, 0)      # tied maxima go to the window's first maximum on both sides
    lpe, dz, _ = lat.logdensity_grad_certified(pb, 0, pb.y1)
    _setup(gpu_ctx, pb, pb.y1)
    lp, g = gpu_ctx.logdensity_grad(pb.z[:, 0])
    lat.assert_lp(lp, lpe)
    lat.assert_exact(g, dz, "%s d lp / d z" % name)
    lp2, g2 = gpu_ctx.logdensity_grad(pb.z[:, 0])
    assert lp2 == lp and np.array_equal(g, g2)


def _layer_of(table, i):
    """which row of the table owns element i of the flat vector, and whether it is a weight or a bias (for a failure's message)"""
    for r in lat._param_rows(table):
        ws, bs = lat._row_slices(table[r])
        if ws.start <= i < ws.stop:
            return "row %d weight element %d of %d" % (r, i - ws.start, ws.stop - ws.start)
        if bs.start <= i < bs.stop:
            return "row %d bias %d" % (r, i - bs.start)
    return "?"


def _assert_grad(g, g_ref, table, what):
    if not np.array_equal(g, g_ref):
        bad = np.flatnonzero(g != g_ref)
        raise AssertionError("%s: %d of %d elements differ; first at %d (%s): %r vs exact %r"
                             % (what, bad.size, g.size, bad[0], _layer_of(table, int(bad[0])), g[bad[0]], g_ref[bad[0]]))


@pytest.mark.parametrize("name", cr.NAMES)
def test_train_grad_whole_vector_exact(gpu_ctx, name):
    table, n, w, x, y = cr.train_problem(name)
    b = x.shape[1]
    gpu_ctx.train_setup(table, n, w.astype(np.float32), x, y, b, 0, ETA)
    for idx in cr.train_batches(b):
        sse_ref, g_ref = lat.mse_grad_exact(table, w, x[:, idx], y[:, idx], cr.NB_TOTAL)
        sse = gpu_ctx.train_grad(idx, cr.NB_TOTAL)
        assert sse == sse_ref
        g = gpu_ctx.train_grad_get()
        _assert_grad(g, g_ref, table, "%s train gradient (%d of %d)" % (name, idx.size, b))
        assert gpu_ctx.train_grad(idx, cr.NB_TOTAL) == sse and np.array_equal(gpu_ctx.train_grad_get(), g)
    # one Descent step from the full batch's gradient (scaled by NB_TOTAL: si_train_step would divide by b, which is a power
    # of two in few cases only), read back through train_get_weights
    _, g_ref = lat.mse_grad_exact(table, w, x, y, cr.NB_TOTAL)
    gpu_ctx.train_grad(np.arange(b), cr.NB_TOTAL)
    gpu_ctx.train_apply()
    w32 = w.astype(np.float32)
    so.apply_update(w32, so.optimiser_state(n, ("descent", ETA)), g_ref, ("descent", ETA))
    lat.assert_exact(gpu_ctx.train_get_weights(), w32, "%s weights after one Descent step" % name)
