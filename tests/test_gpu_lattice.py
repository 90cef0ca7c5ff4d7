"""Bit-exact tests on lattice problems (tests/lattice.py): every operand a small dyadic number, every partial sum certified
below 2^53 (fp64) or 2^24 (compute_dtype = SI_F32), so no kernel rounds anything whatever its summation order, tile split
or split-K -- its result must EQUAL the exact one.  np.array_equal everywhere; lp within 4 ulp of the exact
so.lp_from_sse(S_exact, d, sigma) (only the final combine rounds).  A dropped, doubled or misplaced k-term, a wrong
column of P, a wrong chain slot or a lost bias shows in any element however small.

Which kernel each case reaches (from the dispatch: launch_dense_f64 / launch_dense_f64_fused in kernels_gemm.hip,
dense_small_applies in kernels_gemm_small.hip, dense_panel_applies in kernels_gemm_panel.hip, launch_f32_any in
kernels_gemm_f32.hip, launch_reconstruct in kernels_stream.hip) is written next to it; tests/dense_routes.py restates that
dispatch and tests/test_dense_exact_cpu.py computes what these cases reach from it (the cases here reach 41 of the 87 fp64 Dense
instantiations the table lists; tests/test_gpu_dense_exact.py holds all of them)."""
import functools

import numpy as np
import pytest

from oracle import subspace_oracle as so
from tests import lattice as lat

pytestmark = pytest.mark.gpu

R, I = so.ACT_RELU, so.ACT_IDENTITY
SI_F32, SI_F64 = 0, 1

# ----------------------------------------------------------------------------------------------- Dense problems
# name -> builder (cached).  fp64 problems use dense integer weights; the SI_F32 twins keep the fan-in small
# (sparse weights: w_density, one nonzero per row of P, one-hot z) so every partial sum stays below 2^24 units.
_F32 = dict(f32=True, w_density=0.03, p_nnz=1, z_nnz=1, w_range=2, x_range=1)
_SPECS = {
    # dense_f64_kernel (tile) for layer 1: 2 x 71 feature/batch tiles > 128 -> not the small kernel; ragged out (130), B, in (37).
    # Layer 2 (65 rows, the fused head) has 1 x 71 tiles: the small kernel for one chain, the tile kernel with three stacked
    "tile_ragged": (([37, 130, 65, 3], [R, R, I], 9001), dict(m=4, ncols=3, w_density=0.15)),
    # dense_f64_panel (single chain): layer 1 with in <= 128, even out in 64..1024, 64 x 129 tiles >= 16 x 512 workgroups, W at
    # offset 0, and a stored layer (not the one fused with the head: launch_dense_f64_fused has no panel form)
    "panel_in1": (([1, 1024, 16, 1], [R, R, I], 16400), dict(m=3, ncols=2, w_density=0.3)),
    "panel_in15": (([15, 1024, 16, 1], [R, R, I], 16400), dict(m=3, ncols=2, w_density=0.1)),
    "panel_in17": (([17, 1024, 16, 1], [R, R, I], 16400), dict(m=3, ncols=2, w_density=0.1)),
    "panel_in100": (([100, 1024, 16, 1], [R, R, I], 16400), dict(m=3, ncols=2, w_density=0.05)),
    "panel_in128": (([128, 1024, 16, 1], [I, R, I], 16400), dict(m=3, ncols=2, w_density=0.05)),
    # layer 2 is of the panel's class but its W starts at flat offset 9 (72 bytes, not 16-aligned): the tile kernel
    "panel_unaligned": (([2, 3, 1024, 16, 1], [R, R, R, I], 16400), dict(m=3, ncols=2, w_density=0.3)),
    # dense_small_f64 (<= 128 big tiles) and its fused head (out = 2)
    "small_toy": (([10, 20, 20, 2], [R, R, I], 100), dict(m=3, ncols=9, z_nnz=2)),
    # fused heads out = 1..4 behind the small / tile kernels; a wide last layer (out = 9, un-fused tail)
    "head1": (([4, 100, 1], [R, I], 5000), dict(m=4, ncols=9)),
    "head2": (([12, 256, 130, 2], [R, R, I], 2500), dict(m=7, ncols=3, w_density=0.2)),
    "head3": (([7, 33, 18, 40, 3], [R, R, R, I], 1300), dict(m=5, ncols=3, w_density=0.3)),
    "head4": (([5, 70, 4], [R, R], 777), dict(m=6, ncols=3)),
    "wide_last": (([6, 40, 24, 9], [R, R, I], 900), dict(m=4, ncols=3)),
    # more output tiles than workgroup slots (stored layer + fused tail)
    "many_tiles": (([12, 192, 200, 2], [R, R, I], 33001), dict(m=3, ncols=2, w_density=0.1)),
    # the reference's tutorial MLP (docs nn_example): the narrow chain class
    "nn_example": (([2, 200, 50, 50, 50, 1], [R, R, R, R, I], 1000), dict(m=3, ncols=9, w_density=0.05)),
    # ---- SI_F32 twins
    "f32_dma192": (([16, 960, 960, 1], [R, R, I], 1000), dict(m=32, ncols=5, **_F32)),      # BM 192 (960 = 5 x 192), fused head
    "f32_dma128": (([32, 256, 128, 8], [R, R, I], 257), dict(m=16, ncols=5, **_F32)),       # BM 128, wide last layer
    "f32_tile": (([16, 192, 1], [R, I], 128), dict(m=8, ncols=3, **_F32)),                   # one exact tile of the DMA kernel
    "f32_generic": (([10, 20, 20, 2], [R, R, I], 100), dict(m=4, ncols=9, **_F32)),         # in % 16 != 0: f32_fast_ok false
    "f32_nn_example": (([2, 200, 50, 50, 50, 1], [R, R, R, R, I], 1000), dict(m=16, ncols=9, **_F32)),   # unaligned w_off
    "f32_panel_shape": (([16, 1024, 16, 1], [R, R, I], 16400), dict(m=8, ncols=2, **_F32)),
    # the fp64 list's shapes run with SI_F32 (in % 16 != 0 layers take dense_f32_generic_kernel, the others the DMA kernel)
    "f32_tile_ragged": (([37, 130, 65, 3], [R, R, I], 9001), dict(m=8, ncols=3, **_F32)),
    "f32_head1": (([4, 100, 1], [R, I], 5000), dict(m=8, ncols=9, **_F32)),
    "f32_head2": (([12, 256, 130, 2], [R, R, I], 2500), dict(m=8, ncols=3, **_F32)),
    "f32_head3": (([7, 33, 18, 40, 3], [R, R, R, I], 1300), dict(m=8, ncols=3, **_F32)),
    "f32_head4": (([5, 70, 4], [R, R], 777), dict(m=8, ncols=3, **_F32)),
    "f32_wide_last": (([6, 40, 24, 9], [R, R, I], 900), dict(m=8, ncols=3, **_F32)),
    "f32_many_tiles": (([12, 192, 200, 2], [R, R, I], 33001), dict(m=8, ncols=2, **_F32)),
    # a ragged last feature tile of the DMA kernel on a wide layer: 260 = 2 x 128 + 4 (BM 128), 572 = 2 x 192 + 188 (BM 192)
    "f32_dma128_ragged": (([16, 260, 32, 1], [R, R, I], 2000), dict(m=16, ncols=3, **_F32)),
    "f32_dma192_ragged": (([16, 572, 16, 1], [R, R, I], 1000), dict(m=16, ncols=3, **_F32)),
}


def _builder(name):
    (dims, acts, b), kw = _SPECS[name]
    return functools.lru_cache(maxsize=1)(lambda: lat.dense(dims, acts, b, seed=sum(dims) + b, **kw))


DENSE_PROBLEMS = {name: _builder(name) for name in _SPECS}
CFG2 = ([128, 960, 960, 1], [R, R, I], 100000)


def _setup(ctx, pb, y):
    ctx.infer_setup(pb.table, pb.n, pb.m, pb.w_swa, pb.p, pb.x, y, pb.sigma, compute_dtype=SI_F32 if pb.f32 else SI_F64)


def _check_dense(ctx, pb):
    for tag, y in (("null", pb.y0), ("r", pb.y1)):
        _setup(ctx, pb, y)
        for c in range(pb.z.shape[1]):
            lat.assert_exact(ctx.forward(pb.z[:, c]), pb.yhat[c], "forward column %d" % c)
        cases = lat.lp_cases(pb, tag)
        lp_all = ctx.logdensity(pb.z)                  # every column stacked in one pass (grid.y = chain slot)
        for c, lpe in cases:
            lat.assert_lp(lp_all[c], lpe)
            lat.assert_lp(ctx.logdensity(pb.z[:, c:c + 1])[0], lpe)   # and one at a time (single-chain kernels: panel, small)
        for cols in (1, 2, 3, 4, 5, 8, 9):            # <4>/<2>/<1> groups of K4 and the chain-slot stacking of the density
            if cols <= pb.z.shape[1]:
                lp = ctx.logdensity(pb.z[:, :cols])
                for c, lpe in cases:
                    if c < cols:
                        lat.assert_lp(lp[c], lpe)
    # predict on new lattice inputs (fp64 forward), two columns stacked
    xn = np.asfortranarray(np.random.default_rng(7).integers(-2, 3, (pb.x.shape[0], 37)).astype(np.float64))
    nz = min(2, pb.z.shape[1])
    out = ctx.predict(pb.z[:, :nz], xn)
    for c in range(nz):
        ref, _, _ = lat.forward_certified(pb.table, pb.w_swa + pb.p @ pb.z[:, c], xn, lat.F64_LIMIT)
        lat.assert_exact(out[:, :, c], ref, "predict column %d" % c)


@pytest.mark.parametrize("name", list(_SPECS))
def test_dense_forward_predict_logdensity_exact(gpu_ctx, name):
    _check_dense(gpu_ctx, DENSE_PROBLEMS[name]())


def test_dense_cfg2_full_size_exact(gpu_ctx):
    dims, acts, b = CFG2
    pb = lat.dense(dims, acts, b, m=4, ncols=1, seed=2, w_density=0.05, w_range=1, x_range=1)
    gpu_ctx.infer_setup(pb.table, pb.n, pb.m, pb.w_swa, pb.p, pb.x, pb.y1, pb.sigma)
    lat.assert_exact(gpu_ctx.forward(pb.z[:, 0]), pb.yhat[0], "cfg2 forward")
    lat.assert_lp(gpu_ctx.logdensity(pb.z)[0], lat.lp_exact(pb.sse["r"][0], pb.d, pb.sigma))


# ----------------------------------------------------------------------------------------------- gradients
GRAD_CASES = ["small_toy", "head3", "wide_last", "nn_example", "f32_generic", "f32_dma128", "f32_tile"]


@pytest.mark.parametrize("name", GRAD_CASES)
def test_logdensity_grad_exact(gpu_ctx, name):
    pb = DENSE_PROBLEMS[name]()
    for c, y in ((0, pb.y1), (min(1, pb.z.shape[1] - 1), pb.y0)):
        if pb.sse["r" if y is pb.y1 else "null"][c] is None:
            continue
        lpe, dz, _ = lat.logdensity_grad_certified(pb, c, y)
        _setup(gpu_ctx, pb, y)
        lp, g = gpu_ctx.logdensity_grad(pb.z[:, c])
        lat.assert_lp(lp, lpe)
        lat.assert_exact(g, dz, "d lp / d z, column %d" % c)


# shapes of test_gpu_parity.py::test_weight_gradient_dma_kernel, made lattice.  At every batch used below (nbt, nbt - 37,
# nbt / 2 + 5) plan_dw gives each of their layers 64 x 128 tiles, so they run the register-staged weight gradient
# gemm_f64_kernel<64, 128, .., EPI_RAW> and never the LDS-DMA kernel (tests/test_dense_exact_cpu.py asserts it from the route
# table); dw_f64_dma_kernel<96, 128 | 192> and the 96- and 128-row register-staged tiles are held bit for bit by
# tests/test_gpu_dense_exact.py.
TRAIN_CASES = [
    ([6, 100, 190, 2], 4096),
    ([20, 386, 98, 1], 1024),
    ([64, 192, 96, 4], 256),
    ([30, 130, 258, 2], 2048),
]


def _train_problem(dims, nb, f32, seed):
    rng = np.random.default_rng(seed)
    table, n = so.layer_table(dims, [R, R, I])
    w = lat.lattice_swa(table, n, rng, 1, 0.02 if f32 else 0.3)
    x = np.asfortranarray(rng.integers(-1, 2, (dims[0], nb)).astype(np.float64))
    yh = so.forward(table, w, x)
    y = np.asfortranarray(yh + rng.integers(-2, 3, yh.shape) * lat.out_unit(table))
    return table, n, w, x, y


@pytest.mark.parametrize("dims,nbt", TRAIN_CASES)
@pytest.mark.parametrize("f32", [False, True])
def test_train_grad_exact(si, gpu_ctx, dims, nbt, f32):
    """si_train_grad + si_train_grad_get: the whole N-vector exactly; in-order and shuffled idx, a batch below batch_max that is
    not a multiple of the 16-deep tile (scaled by nb_total, a power of two with out_dim), then one Descent step (eta = 2^-3)"""
    table, n, w, x, y = _train_problem(dims, nbt, f32, seed=sum(dims))
    limit = lat.F32_LIMIT if f32 else lat.F64_LIMIT
    dt = np.float32 if f32 else np.float64
    assert lat.f32_exact(w) and lat.f32_exact(x) and lat.f32_exact(y)
    gpu_ctx.train_setup(table, n, w.astype(np.float32), x.astype(dt), y.astype(dt), nbt, 0, 2.0 ** -3)
    rng = np.random.default_rng(1)
    for idx, nb_total in ((np.arange(nbt), nbt), (rng.permutation(nbt), nbt), (np.sort(rng.choice(nbt, nbt - 37, replace=False)), nbt),
                          (rng.permutation(nbt)[:nbt // 2 + 5], nbt)):
        sse_ref, g_ref = lat.mse_grad_exact(table, w, x[:, idx], y[:, idx], nb_total, limit)
        sse = gpu_ctx.train_grad(idx, nb_total)
        assert sse == sse_ref
        lat.assert_exact(gpu_ctx.train_grad_get(), g_ref, "train gradient (%d of %d)" % (idx.size, nb_total))
    # one Descent step on the full batch, read back through train_get_weights
    _, g_ref = lat.mse_grad_exact(table, w, x, y, nbt, limit)
    gpu_ctx.train_step(np.arange(nbt))
    w32 = w.astype(np.float32)
    so.apply_update(w32, so.optimiser_state(n, ("descent", 2.0 ** -3)), g_ref.astype(np.float32) if f32 else g_ref, ("descent", 2.0 ** -3))
    lat.assert_exact(gpu_ctx.train_get_weights(), w32, "weights after one Descent step")


# ----------------------------------------------------------------------------------------------- Conv
# (these shapes are the ragged ones of tests/test_gpu_conv.py, picked for raggedness and not for dispatch: they reach 32 of the 82
#  conv instantiations.  tests/test_gpu_conv_exact.py holds every reachable one, route by route, with the whole weight gradient.)
def _conv_cases():
    from tests.test_gpu_conv import CASES
    out = []
    for whc, spec, b in CASES:
        # the lattice keeps identity / relu only: every other activation becomes relu (the shapes are what matter here)
        spec2 = []
        for e in spec:
            if e[0] == "conv":
                e = e[:3] + ((e[3] if e[3] in lat.EXACT_ACTS else R),) + e[4:]
            elif e[0] == "dense":
                e = (e[0], e[1], e[2] if e[2] in lat.EXACT_ACTS else R)
            spec2.append(e)
        out.append((whc, spec2, b))
    return out


CONV_CASES = _conv_cases()


def conv_problem(case, f32):
    whc, spec, b = CONV_CASES[case]
    return lat.conv(spec, whc, b, m=3, ncols=2, seed=case, f32=f32, w_density=0.5 if f32 else 1.0)


@pytest.mark.parametrize("case", range(len(CONV_CASES)))
@pytest.mark.parametrize("f32", [False, True])
def test_conv_forward_logdensity_exact(gpu_ctx, case, f32):
    pb = conv_problem(case, f32)
    for tag, y in (("null", pb.y0), ("r", pb.y1)):
        _setup(gpu_ctx, pb, y)
        for c in range(pb.z.shape[1]):
            lat.assert_exact(gpu_ctx.forward(pb.z[:, c]), pb.yhat[c], "conv forward column %d" % c)
        lp = gpu_ctx.logdensity(pb.z)
        for c, lpe in lat.lp_cases(pb, tag):
            lat.assert_lp(lp[c], lpe)
    if not f32:   # the fp64 conv gradient, certified exact.  Integer data tie MaxPool maxima: the gradient then goes to the
        # window's FIRST maximum (NNlib's rule, the oracle's, pinned by test_maxpool_gradient_with_exact_ties), and on the
        # lattice the oracle's isapprox pick is plain equality (lat.pool_ties_are_exact) -- so the comparison stays exact
        _setup(gpu_ctx, pb, pb.y1)
        lpe, dz, _ = lat.logdensity_grad_certified(pb, 0, pb.y1)
        lat.pool_ties_are_exact(pb, 0)
        lp, g = gpu_ctx.logdensity_grad(pb.z[:, 0])
        lat.assert_lp(lp, lpe)
        lat.assert_exact(g, dz, "conv d lp / d z")


# ----------------------------------------------------------------------------------------------- chain loops
@pytest.mark.parametrize("m", [1, 32, 33, 64, 65, 128, 256])
def test_chain_loops_trace_exact_lp(si, gpu_ctx, m):
    """sigma_z = 2^-80 and W_swa nonzero wherever P is: every proposal's weights round back to W_swa, so every lp of every
    chain of si_sample_rwmh is the exact lp.  All five set_chain_loop modes; nchains 1, 8, 64; the narrow class, whose mode-1
    runs of up to 8 chains must take the loop specialised to the chain's shapes at every M (above M = 64 only its tid < M guards
    keep it right)"""
    # (z never moves here and only its size is looked at: the draws, the z + sigma_z eps update, the reject branch and the layout of
    #  the z trace are held, transition by transition at M up to 1025, by tests/test_gpu_rwmh_audit.py)
    dims, acts, b = [2, 200, 50, 50, 50, 1], [R, R, R, R, I], 1000
    pb = lat.dense(dims, acts, b, m=m, ncols=1, seed=m, nonzero_swa=True, w_range=1, x_range=1)
    yh, _, _ = lat.forward_certified(pb.table, pb.w_swa, pb.x, lat.F64_LIMIT)
    y = np.asfortranarray(yh + np.random.default_rng(m).integers(-1, 2, yh.shape) * pb.unit)
    lpe = lat.lp_exact(lat.sse_certified(yh, y, pb.unit), pb.d, pb.sigma)
    gpu_ctx.infer_setup(pb.table, pb.n, m, pb.w_swa, pb.p, pb.x, y, pb.sigma)
    try:
        for mode in (0, 1, 2, 3, 4):
            gpu_ctx.set_chain_loop(mode)
            for nch in (1, 8, 64):
                itr = 6 if nch == 64 else 10
                z, lp, acc = gpu_ctx.sample_rwmh(itr, 2.0 ** -80, seed=5, nchains=nch)
                assert np.all(np.abs(z) < 2.0 ** -70) and np.all(acc >= 0)
                bad = np.abs(lp - lpe) > lat.lp_tol(lpe)
                assert not bad.any(), "mode %d, %d chains: %d of %d lps off the exact %r (first %r)" % (
                    mode, nch, bad.sum(), lp.size, lpe, lp[bad][0])
                if mode == 1 and nch <= 8:   # capi_sample.hip: M <= 256 and this class go to the loop specialised at run time
                    _, loop, msg = gpu_ctx.chain_kernel_info()
                    assert loop, "M = %d, %d chains: the generic grid loop ran (%s)" % (m, nch, msg)
    finally:
        gpu_ctx.set_chain_loop(1)


def test_chain_loop_specialised_kernels_named(si, gpu_ctx):
    """the nn_example class at M = 3: the kernels compiled for the chain's shapes run (and give the exact lp)"""
    pb = DENSE_PROBLEMS["nn_example"]()
    _setup(gpu_ctx, pb, pb.y1)
    gpu_ctx.set_chain_loop(1)
    _, lp, _ = gpu_ctx.sample_rwmh(8, 2.0 ** -80, seed=3, nchains=2)
    d, l, msg = gpu_ctx.chain_kernel_info()
    assert l, msg
    lat.assert_lp(gpu_ctx.logdensity(pb.z[:, :1])[0], lat.lp_cases(pb, "r")[0][1])


def test_rwmh_stepwise_sse_exact_and_shards(si, gpu_ctx):
    """rwmh_begin / rwmh_step_eval: sse_local is the exact SSE; two unequal data shards sum to it exactly"""
    dims, acts, b, m = [6, 40, 3], [R, I], 500, 4
    pb = lat.dense(dims, acts, b, m=m, ncols=1, seed=13, nonzero_swa=True, w_range=1)
    yh, _, _ = lat.forward_certified(pb.table, pb.w_swa, pb.x, lat.F64_LIMIT)
    y = np.asfortranarray(yh + np.random.default_rng(2).integers(-2, 3, yh.shape) * pb.unit)
    sse_e = lat.sse_certified(yh, y, pb.unit)
    gpu_ctx.infer_setup(pb.table, pb.n, m, pb.w_swa, pb.p, pb.x, y, pb.sigma)
    gpu_ctx.rwmh_begin(3, 2.0 ** -80, 7, 0, 2)
    for _ in range(3):
        s = gpu_ctx.rwmh_step_eval()
        assert np.all(s == sse_e), (s, sse_e)
        gpu_ctx.rwmh_step_accept(s)
    gpu_ctx.rwmh_end()
    shards = [si.Context(0), si.Context(0)]
    try:
        for c, (b0, b1) in zip(shards, ((0, 123), (123, 500))):
            c.infer_setup(pb.table, pb.n, m, pb.w_swa, pb.p, np.asfortranarray(pb.x[:, b0:b1]), np.asfortranarray(y[:, b0:b1]), pb.sigma)
            c.rwmh_begin(2, 2.0 ** -80, 7, 0, 2, d_total=y.size)
        for _ in range(2):
            parts = [c.rwmh_step_eval() for c in shards]
            assert np.all(parts[0] + parts[1] == sse_e)
            for c in shards:
                c.rwmh_step_accept(parts[0] + parts[1])
        for c in shards:
            _, lp, _ = c.rwmh_end()
            assert np.all(np.abs(lp - lat.lp_exact(sse_e, y.size, pb.sigma)) <= lat.lp_tol(lat.lp_exact(sse_e, y.size, pb.sigma)))
    finally:
        for c in shards:
            c.close()


# ----------------------------------------------------------------------------------------------- Gram
# (N, K), ragged N, every push path and both storage types.  (These shapes reach 7 of the 26 LDS-DMA instantiations and about a
#  dozen of the 32 panel ones; tests/test_gpu_gram_exact.py holds every reachable one, route by route: tests/gram_routes.py.)
GRAM_CASES = [(1, 1), (31, 15), (33, 16), (4097, 17), (100003, 100), (4097, 128), (33, 129), (4097, 200), (31, 260)]


def gram_problem(n, k):
    """(snapshots, epoch counters, A, exact A'A) of one GRAM_CASES entry.  The epoch counters start at 1: with n_0 = 0 the first
    deviation column is zero, and so are row and column 0 of G (tests/test_gram_exact_cpu.py pins that no column is zero)"""
    snaps, ns, _, a = lat.snapshots(n, k, seed=n + k, ns=[1 + j // 3 for j in range(k)])
    return snaps, ns, a, lat.gram_exact(a).astype(np.float64)


@pytest.mark.parametrize("n,k", GRAM_CASES)
def test_gram_exact(gpu_ctx, n, k):
    import torch
    snaps, ns, _, g_ref = gram_problem(n, k)
    for dtype in (np.float64, np.float32):
        ss = [s.astype(dtype) for s in snaps]
        for path in ("host", "dev", "batch"):
            for storage in ((SI_F64, SI_F32) if path == "host" else (SI_F64,)):
                gpu_ctx.construct_begin(n, k)
                if storage == SI_F32:
                    gpu_ctx.construct_set_storage(SI_F32)
                if path == "host":
                    for w, nn in zip(ss, ns):
                        gpu_ctx.construct_push(w, nn)
                else:
                    dev = torch.from_numpy(np.stack(ss)).cuda()
                    dcode = SI_F32 if dtype == np.float32 else SI_F64
                    if path == "dev":
                        for j, nn in enumerate(ns):
                            gpu_ctx.construct_push_dev(dev[j].data_ptr(), dcode, nn)
                    else:
                        h = k // 2
                        if h:
                            gpu_ctx.construct_push_batch_dev(dev.data_ptr(), dcode, n, ns[:h])
                        gpu_ctx.construct_push_batch_dev(dev[h:].data_ptr(), dcode, n, ns[h:])
                    torch.cuda.synchronize()
                gpu_ctx.construct_gram()
                lat.assert_exact(gpu_ctx.construct_gram_get(), g_ref, "Gram %s %s storage %d" % (path, dtype.__name__, storage))


def test_gram_ring_after_column_shift(gpu_ctx):
    """max_cols ring: after the shift the Gram matrix is A'A of the newest max_cols columns (in ring order)"""
    n, k, mc = 4097, 12, 5
    snaps, ns, means, a = lat.snapshots(n, k, seed=3)
    gpu_ctx.construct_begin(n, k, mc)
    for w, nn in zip(snaps, ns):
        gpu_ctx.construct_push(w, nn)
    gpu_ctx.construct_gram()
    g = gpu_ctx.construct_gram_get()
    a_last = a[:, -mc:]
    # the ring may hold the columns rotated: compare against A'A in the order the library reports through construct_get_A
    a_dev = gpu_ctx.construct_get_A(0, mc)
    assert sorted(map(tuple, a_dev.T)) == sorted(map(tuple, a_last.T))
    lat.assert_exact(g, lat.gram_exact(a_dev).astype(np.float64), "Gram of the ring")


# ----------------------------------------------------------------------------------------------- reconstruct / output map
def test_reconstruct_lattice_c1_to_9(gpu_ctx):
    pb = lat.dense([7, 33, 18, 2], [R, R, I], 50, m=6, ncols=9, seed=4, z_nnz=3, zmax=3)
    gpu_ctx.infer_setup(pb.table, pb.n, pb.m, pb.w_swa, pb.p, pb.x, pb.y1, pb.sigma)
    for cols in range(1, 10):
        lat.assert_exact(gpu_ctx.reconstruct(pb.z[:, :cols]), pb.w_swa[:, None] + pb.p @ pb.z[:, :cols], "reconstruct C=%d" % cols)


def test_sample_rwmh_weights_past_65535_chain_groups(si, gpu_ctx):
    """the output map of a long run: itr * nchains = 4 * 65536 + 4 samples go through ONE launch_reconstruct, whose stacked
    groups of four chains need more than 65535 groups.  P has one nonzero (+-1, +-2) per row, so every W_out column is
    W_swa + p_r z_r rounded once -- what NumPy computes -- whatever z the chain drew."""
    dims, acts, b = [2, 4, 1], [R, I], 16
    table, n = so.layer_table(dims, acts)
    rng = np.random.default_rng(11)
    m = 3
    w_swa = lat.lattice_swa(table, n, rng, 2, nonzero=True)
    p = lat.lattice_p(n, m, rng, 1)
    x = np.asfortranarray(rng.integers(-2, 3, (2, b)).astype(np.float64))
    y = np.asfortranarray(rng.integers(-2, 3, (1, b)).astype(np.float64))
    gpu_ctx.infer_setup(table, n, m, w_swa, p, x, y, 1.0)
    itr, nch = 4097, 64
    ldw = (n + 63) // 64 * 64     # pad_ld(N): the library's wall_elems = pad_ld(N) * itr * C against its 512 MB cap
    assert itr * nch >= 4 * 65536 + 4 and ldw * itr * nch * 8 <= 512 << 20
    out = np.full((n, itr, nch), np.nan, order="F")
    z, lp, acc, w = gpu_ctx.sample_rwmh_weights(itr, 0.05, seed=3, nchains=nch, out=out)
    zz = z.reshape(m, -1, order="F")
    ref = w_swa[:, None] + p @ zz
    lat.assert_exact(w.reshape(n, -1, order="F"), ref, "W_out")
