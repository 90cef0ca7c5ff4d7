"""Every Dense kernel instantiation shapes can reach, held bit for bit on lattice problems (tests/lattice.py): the chains of
tests/dense_routes.py::CASES, each there for the instantiations written next to it, with the route table that says so restated
from the dispatch and proved complete on the CPU (tests/test_dense_exact_cpu.py: the union of the cases' routes equals
dense_routes.REACHABLE).  profiles/dense_exact_kernel_names.txt is the kernel trace of this file.

Per case, np.array_equal everywhere and lp within 4 ulp of the exact value (only the final combine rounds):
  * the sampling route (ping-pong forward), fp64 and SI_F32: forward per column, log-density stacked and one column at a
    time for both targets, predict on new inputs;
  * the gradient route (kept outputs, the reverse sweep), fp64 and SI_F32: lp and d lp / d z through si_logdensity_grad;
  * the whole weight gradient through si_train_grad, fp64 and fp32: the N-vector, not three numbers of P'g -- a dW element that
    lands in another place of the same layer shows; full batch, shuffled, a subset that is no multiple of 16, a smaller batch
    with another split plan; then one Descent step.  (A head of three outputs has no power-of-two mse scale: those two cases are
    held through the gradient route alone.)
  * the same call twice gives the same bits (split-K partials are reduced in a fixed order)."""
import functools

import numpy as np
import pytest

from oracle import subspace_oracle as so
from tests import dense_routes as dr
from tests import lattice as lat

pytestmark = pytest.mark.gpu

SI_F32, SI_F64 = 0, 1
ETA = 2.0 ** -3


def _setup(ctx, pb, y):
    ctx.infer_setup(pb.table, pb.n, pb.m, pb.w_swa, pb.p, pb.x, y, pb.sigma, compute_dtype=SI_F32 if pb.f32 else SI_F64)


@pytest.mark.parametrize("name", dr.NAMES)
@pytest.mark.parametrize("f32", [False, True])
def test_sampling_route_exact(gpu_ctx, name, f32):
    pb = dr.problem(name, f32)
    ncols = pb.z.shape[1]
    for tag, y in (("null", pb.y0), ("r", pb.y1)):
        _setup(gpu_ctx, pb, y)
        for c in range(ncols):
            lat.assert_exact(gpu_ctx.forward(pb.z[:, c]), pb.yhat[c], "%s forward column %d" % (name, c))
        cases = lat.lp_cases(pb, tag)
        lp = gpu_ctx.logdensity(pb.z)                      # every column stacked in one pass (grid.y = chain slot)
        for c, lpe in cases:
            lat.assert_lp(lp[c], lpe)
            lat.assert_lp(gpu_ctx.logdensity(pb.z[:, c:c + 1])[0], lpe)   # and one at a time (the single-chain kernels)
        assert np.array_equal(lp, gpu_ctx.logdensity(pb.z))
    # predict on new lattice inputs (an fp64 forward in either mode), another batch size: both columns stacked
    xn = np.asfortranarray(np.random.default_rng(7).integers(-1, 2, (pb.x.shape[0], dr.PREDICT_B)).astype(np.float64))
    out = gpu_ctx.predict(pb.z, xn)
    for c in range(ncols):
        ref, _, _ = lat.forward_certified(pb.table, pb.w_swa + pb.p @ pb.z[:, c], xn, lat.F64_LIMIT)
        lat.assert_exact(out[:, :, c], ref, "%s predict column %d" % (name, c))


@pytest.mark.parametrize("name", dr.NAMES)
@pytest.mark.parametrize("f32", [False, True])
def test_gradient_route_exact(gpu_ctx, name, f32):
    pb = dr.problem(name, f32)
    lpe, dz, _ = lat.logdensity_grad_certified(pb, 0, pb.y1)
    _setup(gpu_ctx, pb, pb.y1)
    lp, g = gpu_ctx.logdensity_grad(pb.z[:, 0])
    lat.assert_lp(lp, lpe)
    lat.assert_exact(g, dz, "%s d lp / d z" % name)
    lp2, g2 = gpu_ctx.logdensity_grad(pb.z[:, 0])
    assert lp2 == lp and np.array_equal(g, g2)


def _layer_of(table, i):
    """which layer owns element i of the flat vector, and whether it is a weight or a bias (for a failure's message)"""
    for l, (fin, fout, _, w_off, b_off) in enumerate(table):
        if w_off <= i < w_off + fin * fout:
            e = i - w_off
            return "layer %d weight element %d = (row %d, column %d) of %d x %d" % (l, e, e % fout, e // fout, fout, fin)
        if b_off <= i < b_off + fout:
            return "layer %d bias %d" % (l, i - b_off)
    return "?"


def _assert_grad(g, g_ref, table, what):
    if not np.array_equal(g, g_ref):
        bad = np.flatnonzero(g != g_ref)
        raise AssertionError("%s: %d of %d elements differ; first at %d (%s): %r vs exact %r"
                             % (what, bad.size, g.size, bad[0], _layer_of(table, int(bad[0])), g[bad[0]], g_ref[bad[0]]))


@functools.lru_cache(maxsize=2)
def _train_references(name, f32):
    """[(idx, exact sse, exact gradient)] over the index sets of the case, computed once"""
    table, n, w, x, y = dr.train_problem(name, f32)
    limit = lat.F32_LIMIT if f32 else lat.F64_LIMIT
    return [(idx,) + lat.mse_grad_exact(table, w, x[:, idx], y[:, idx], dr.nb_total(name), limit) for idx in dr.train_batches(x.shape[1])]


@pytest.mark.parametrize("name", dr.TRAIN_NAMES)
@pytest.mark.parametrize("f32", [False, True])
def test_train_grad_whole_vector_exact(gpu_ctx, name, f32):
    table, n, w, x, y = dr.train_problem(name, f32)
    b, nbt = x.shape[1], dr.nb_total(name)
    dt = np.float32 if f32 else np.float64
    gpu_ctx.train_setup(table, n, w.astype(np.float32), x.astype(dt), y.astype(dt), b, 0, ETA)
    for idx, sse_ref, g_ref in _train_references(name, f32):
        sse = gpu_ctx.train_grad(idx, nbt)
        assert sse == sse_ref
        g = gpu_ctx.train_grad_get()
        _assert_grad(g, g_ref, table, "%s train gradient (%d of %d)" % (name, idx.size, b))
        assert gpu_ctx.train_grad(idx, nbt) == sse and np.array_equal(gpu_ctx.train_grad_get(), g)
    # one Descent step from the full batch's gradient (scaled by nb_total: si_train_step would divide by b, which is a power
    # of two in few cases only), read back through train_get_weights
    _, _, g_ref = _train_references(name, f32)[0]
    gpu_ctx.train_grad(np.arange(b), nbt)
    gpu_ctx.train_apply()
    w32 = w.astype(np.float32)
    so.apply_update(w32, so.optimiser_state(n, ("descent", ETA)), g_ref.astype(np.float32) if f32 else g_ref, ("descent", ETA))
    lat.assert_exact(gpu_ctx.train_get_weights(), w32, "%s weights after one Descent step" % name)
