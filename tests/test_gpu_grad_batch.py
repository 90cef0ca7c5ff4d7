"""si_logdensity_grad_batch: value and gradient of the log-density at C stacked points in one call.

Narrow fp64 Dense chains (identity / relu / tanh / sigmoid, every layer's image in a workgroup's LDS) run the fused forward +
reverse kernel of kernels_chain_grad.hip and one reduction launch per group of points; every other chain walks the columns
through si_logdensity_grad's own code.  Checked here: the oracle (tolerances of test_gpu_parity.py's si_logdensity_grad test:
lp rtol 1e-11, gradient rtol 1e-8 with atol 1e-9 max|g|), lattice problems bit for bit, independence of a point's bits from C /
column / run / grid.y group, the fallback's bits, the state rules, a fixed-seed sweep over the class, and MALA on it."""
import numpy as np
import pytest

from oracle import subspace_oracle as so
from tests import lattice as lat
from tests.test_gpu_chain_grid import NN_EXAMPLE
from tests.test_gpu_conv import CASES as CONV_CASES
from tests.test_gpu_conv import _problem as conv_problem

pytestmark = pytest.mark.gpu

SI_F32, SI_F64 = 0, 1
R, I = so.ACT_RELU, so.ACT_IDENTITY


def _problem(dims, acts, b, m, seed):
    rng = np.random.default_rng(seed)
    table, n = so.layer_table(dims, acts)
    w_swa = 0.3 * rng.standard_normal(n)
    p = np.asfortranarray(0.05 * rng.standard_normal((n, m)))
    x = np.asfortranarray(rng.standard_normal((dims[0], b)))
    y = np.asfortranarray(rng.standard_normal((dims[-1], b)))
    return table, n, w_swa, p, x, y


def _assert_oracle(lp, g, table, w_swa, p, x, y, sigma, z, sigma_p=0.0):
    for c in range(z.shape[1]):
        lp_ref, g_ref, _ = so.logdensity_grad(table, w_swa, p, x, y, sigma, z[:, c])
        if sigma_p > 0.0:   # + logpdf(MvNormal(zeros(N), sigma_p), W_swa + P z), the term si_infer_set_prior switches on
            w = w_swa + p @ z[:, c]
            lp_ref = lp_ref - (w.size * np.log(2.0 * np.pi) + w.size * np.log(sigma_p * sigma_p)) / 2.0 - (w @ w) / (sigma_p * sigma_p) / 2.0
            g_ref = g_ref - p.T @ w / (sigma_p * sigma_p)
        print("column %d: lp %.17g ref %.17g  max|dg| %.3g of max|g| %.3g" % (c, lp[c], lp_ref, np.abs(g[:, c] - g_ref).max(),
                                                                          np.abs(g_ref).max()))
        assert np.isclose(lp[c], lp_ref, rtol=1e-11), (c, lp[c], lp_ref)
        assert np.allclose(g[:, c], g_ref, rtol=1e-8, atol=1e-9 * np.abs(g_ref).max()), (c, g[:, c], g_ref)


def _fused_expected(dims, b):
    """the routing rule restated: 16 observations per workgroup; the images of all L + 1 activations, two Delta buffers of the
    widest produced image and four wave sums, in doubles, within 160 KiB"""
    ld = [((d + 3) // 4) * 4 + 2 for d in dims]
    return 16 * (sum(ld) + 2 * max(ld[1:])) + 4 <= 160 * 1024 // 8


# ----------------------------------------------------------------------------------------------- 1. against the oracle
ORACLE_SHAPES = [
    ([3, 5], [0], 17, 2),                                 # one layer, B one past a tile
    ([7, 33, 18, 40, 3], [2, 1, 3, 0], 130, 5),           # ragged widths, all three activations, a last workgroup of 2 observations
    ([5, 70, 4], [2, 2], 77, 6),                          # activation on the output layer
    ([6, 40, 24, 9], [1, 1, 3], 90, 4),                   # wide last layer
    ([12, 256, 130, 2], [1, 2, 0], 100, 7),               # widest member
    NN_EXAMPLE,
    (NN_EXAMPLE[0], NN_EXAMPLE[1], NN_EXAMPLE[2], 20),
]


@pytest.mark.parametrize("case", range(len(ORACLE_SHAPES)))
def test_batch_matches_oracle(gpu_ctx, case):
    dims, acts, b, m = ORACLE_SHAPES[case]
    table, n, w_swa, p, x, y = _problem(dims, acts, b, m, seed=100 + case)
    gpu_ctx.infer_setup(table, n, m, w_swa, p, x, y, sigma_m=0.9)
    rng = np.random.default_rng(case)
    for c in (1, 3, 9):
        z = np.asfortranarray(0.5 * rng.standard_normal((m, c)))
        lp, g = gpu_ctx.logdensity_grad_batch(z)
        assert lp.shape == (c,) and g.shape == (m, c)
        assert gpu_ctx.grad_kernel_info() == 1
        _assert_oracle(lp, g, table, w_swa, p, x, y, 0.9, z)


def test_batch_with_prior_matches_oracle(gpu_ctx):
    dims, acts, b, m = [7, 33, 18, 40, 3], [2, 1, 3, 0], 130, 5
    table, n, w_swa, p, x, y = _problem(dims, acts, b, m, seed=7)
    gpu_ctx.infer_setup(table, n, m, w_swa, p, x, y, sigma_m=0.9)
    gpu_ctx.set_prior(0.7)
    try:
        z = np.asfortranarray(0.5 * np.random.default_rng(1).standard_normal((m, 3)))
        lp, g = gpu_ctx.logdensity_grad_batch(z)
        assert gpu_ctx.grad_kernel_info() == 1
        _assert_oracle(lp, g, table, w_swa, p, x, y, 0.9, z, sigma_p=0.7)
        lp0 = gpu_ctx.logdensity(z)
        assert np.allclose(lp, lp0, rtol=1e-12)
    finally:
        gpu_ctx.set_prior(0.0)


# ----------------------------------------------------------------------------------------------- 2. exact
LATTICE = [
    # (dims, acts, B, kwargs): B = 17 / 130 / 100 leave a ragged last workgroup (1, 2 and 4 observations)
    (([3, 5], [I], 17), dict(m=2, ncols=3)),
    (([7, 33, 18, 40, 3], [R, R, R, I], 130), dict(m=5, ncols=4, w_density=0.3)),
    (([10, 20, 20, 2], [R, R, I], 100), dict(m=3, ncols=9, z_nnz=2)),
    (([2, 200, 50, 50, 50, 1], [R, R, R, R, I], 1000), dict(m=3, ncols=3, w_density=0.05)),
]


@pytest.mark.parametrize("case", range(len(LATTICE)))
def test_batch_exact_on_lattice(gpu_ctx, case):
    (dims, acts, b), kw = LATTICE[case]
    pb = lat.dense(dims, acts, b, seed=sum(dims) + b, **kw)
    gpu_ctx.infer_setup(pb.table, pb.n, pb.m, pb.w_swa, pb.p, pb.x, pb.y1, pb.sigma)
    ncols = pb.z.shape[1]
    lp, g = gpu_ctx.logdensity_grad_batch(pb.z)
    assert gpu_ctx.grad_kernel_info() == 1
    for c in range(ncols):
        lpe, dz, _ = lat.logdensity_grad_certified(pb, c, pb.y1)
        lat.assert_exact(g[:, c], dz, "batch d lp / d z, column %d" % c)
        lp1, g1 = gpu_ctx.logdensity_grad(pb.z[:, c])
        lat.assert_exact(g[:, c], g1, "batch vs si_logdensity_grad, column %d" % c)
        if pb.sse["r"][c] is not None:   # (an SSE that is itself exact: only the final combine rounds, the same way on both)
            lat.assert_lp(lp[c], lpe)
            assert lp[c] == lp1


# ----------------------------------------------------------------------------------------------- 3. order independence
def test_point_bits_do_not_depend_on_the_call(gpu_ctx):
    dims, acts, b, m = [3, 5], [0], 17, 2
    table, n, w_swa, p, x, y = _problem(dims, acts, b, m, seed=3)
    gpu_ctx.infer_setup(table, n, m, w_swa, p, x, y, sigma_m=0.9)
    rng = np.random.default_rng(0)
    zpt = rng.standard_normal(m)
    lp1, g1 = gpu_ctx.logdensity_grad_batch(zpt.reshape(m, 1))
    z9 = np.asfortranarray(rng.standard_normal((m, 9)))
    z9[:, 5] = zpt
    lp9, g9 = gpu_ctx.logdensity_grad_batch(z9)
    lp9b, g9b = gpu_ctx.logdensity_grad_batch(z9)
    assert np.array_equal(lp9, lp9b) and np.array_equal(g9, g9b)            # two identical calls
    assert lp9[5] == lp1[0] and np.array_equal(g9[:, 5], g1[:, 0])
    big = 70001                                                             # grid.y carries 65535 points: a second group
    zb = np.asfortranarray(rng.standard_normal((m, big)))
    zb[:, 70000] = zpt
    zb[:, 3] = z9[:, 2]
    lpb, gb = gpu_ctx.logdensity_grad_batch(zb)
    assert gpu_ctx.grad_kernel_info() == 1
    assert lpb[70000] == lp1[0] and np.array_equal(gb[:, 70000], g1[:, 0])
    assert lpb[3] == lp9[2] and np.array_equal(gb[:, 3], g9[:, 2])
    assert np.all(np.isfinite(lpb)) and np.all(np.isfinite(gb))
    # a sample of the rest against the stacked density (every column was written by its own point)
    idx = np.array([0, 1, 65534, 65535, 65536, 69999])
    assert np.allclose(lpb[idx], gpu_ctx.logdensity(np.asfortranarray(zb[:, idx])), rtol=1e-12)


# ----------------------------------------------------------------------------------------------- 4. fallback
def _fallback_cases():
    whc, spec, b = CONV_CASES[0]
    table, n, w_swa, p, x, y = conv_problem(whc, spec, b, 3, seed=2)
    yield "conv", (table, n, 3, w_swa, p, x, y), SI_F64
    t2 = _problem([6, 30, 2], [2, 0], 200, 4, seed=8)
    yield "f32", (t2[0], t2[1], 4) + t2[2:], SI_F32
    t3 = _problem([6, 30, 2], [so.ACT_SOFTPLUS, 0], 50, 4, seed=9)
    yield "softplus", (t3[0], t3[1], 4) + t3[2:], SI_F64


@pytest.mark.parametrize("name", ["conv", "f32", "softplus"])
def test_fallback_is_the_single_point_path(gpu_ctx, name):
    (table, n, m, w_swa, p, x, y), cdt = {k: (a, c) for k, a, c in _fallback_cases()}[name]
    gpu_ctx.infer_setup(table, n, m, w_swa, p, x, y, sigma_m=0.8, compute_dtype=cdt)
    z = np.asfortranarray(0.3 * np.random.default_rng(4).standard_normal((m, 4)))
    before = gpu_ctx.logdensity_grad(z[:, 1])
    lp, g = gpu_ctx.logdensity_grad_batch(z)
    assert gpu_ctx.grad_kernel_info() == 0
    for c in range(4):
        lp1, g1 = gpu_ctx.logdensity_grad(z[:, c])
        assert lp[c] == lp1 and np.array_equal(g[:, c], g1), c
    after = gpu_ctx.logdensity_grad(z[:, 1])
    assert before[0] == after[0] and np.array_equal(before[1], after[1])


def test_nothing_shared_is_left_dirty(gpu_ctx):
    dims, acts, b, m = [7, 33, 18, 40, 3], [2, 1, 3, 0], 130, 5
    table, n, w_swa, p, x, y = _problem(dims, acts, b, m, seed=11)
    gpu_ctx.infer_setup(table, n, m, w_swa, p, x, y, sigma_m=0.9)
    z = np.asfortranarray(0.4 * np.random.default_rng(5).standard_normal((m, 6)))
    before = gpu_ctx.logdensity_grad(z[:, 2])
    lp0 = gpu_ctx.logdensity(z)
    lp, g = gpu_ctx.logdensity_grad_batch(z)
    assert gpu_ctx.grad_kernel_info() == 1
    after = gpu_ctx.logdensity_grad(z[:, 2])
    assert before[0] == after[0] and np.array_equal(before[1], after[1])
    assert np.array_equal(gpu_ctx.logdensity(z), lp0) and np.allclose(lp, lp0, rtol=1e-12)
    zs, lps, _ = gpu_ctx.sample_rwmh(8, 0.05, seed=1, nchains=2)
    zr, lpr, _, _ = so.sub_inference(table, x, y, w_swa, p, 0.05, 0.9, 8, seed=1)
    assert np.allclose(zs[:, :, 0], zr, rtol=1e-9, atol=1e-12) and np.allclose(lps[:, 0], lpr, rtol=1e-9)
    xn = np.asfortranarray(np.random.default_rng(6).standard_normal((dims[0], 5)))
    yh = gpu_ctx.predict(z[:, :2], xn)
    assert np.allclose(yh[:, :, 1], so.forward(table, w_swa + p @ z[:, 1], xn), rtol=1e-10, atol=1e-12)
    lp2, g2 = gpu_ctx.logdensity_grad_batch(z)
    assert np.array_equal(lp, lp2) and np.array_equal(g, g2)


# ----------------------------------------------------------------------------------------------- 5. errors
def test_state_rules(si, gpu_ctx):
    m = 2
    fresh = si.Context(0)
    try:
        fresh._m = m
        with pytest.raises(si.SubspaceError) as e:
            fresh.logdensity_grad_batch(np.zeros((m, 2)))
        assert e.value.code == si._capi.SI_ERR_STATE and "si_infer_setup" in str(e.value)
    finally:
        fresh.close()
    table, n, w_swa, p, x, y = _problem([3, 5], [0], 17, m, seed=3)
    gpu_ctx.infer_setup(table, n, m, w_swa, p, x, y, sigma_m=0.9)
    z = np.asfortranarray(np.random.default_rng(0).standard_normal((m, 3)))
    good = gpu_ctx.logdensity_grad_batch(z)
    with pytest.raises(si.SubspaceError) as e:
        gpu_ctx.logdensity_grad_batch(np.zeros((m, 0)))
    assert e.value.code == si._capi.SI_ERR_INVALID
    again = gpu_ctx.logdensity_grad_batch(z)
    assert np.array_equal(good[0], again[0]) and np.array_equal(good[1], again[1])
    gpu_ctx.rwmh_begin(4, 0.1, seed=1)
    try:
        with pytest.raises(si.SubspaceError) as e:
            gpu_ctx.logdensity_grad_batch(z)
        assert e.value.code == si._capi.SI_ERR_STATE and "step-wise RWMH session" in str(e.value)
    finally:
        gpu_ctx.lib.si_rwmh_abort(gpu_ctx.h)
    again = gpu_ctx.logdensity_grad_batch(z)
    assert np.array_equal(good[0], again[0]) and np.array_equal(good[1], again[1])


# ----------------------------------------------------------------------------------------------- 6. fuzz
def test_fixed_seed_sweep_over_the_class(gpu_ctx):
    rng = np.random.default_rng(20261018)
    nfused = 0
    for it in range(20):
        nl = int(rng.integers(1, 6))
        dims = [int(v) for v in rng.integers(1, 257, nl + 1)]
        acts = [int(v) for v in rng.integers(0, 4, nl)]
        b, m, c = int(rng.integers(1, 301)), int(rng.integers(1, 25)), int(rng.integers(1, 6))
        table, n, w_swa, p, x, y = _problem(dims, acts, b, m, seed=1000 + it)
        w_swa *= 0.3   # (wide layers: keep tanh / sigmoid away from saturation, where the oracle's own error grows)
        gpu_ctx.infer_setup(table, n, m, w_swa, p, x, y, sigma_m=1.1)
        z = np.asfortranarray(0.3 * rng.standard_normal((m, c)))
        lp, g = gpu_ctx.logdensity_grad_batch(z)
        fused = gpu_ctx.grad_kernel_info()
        print("member %d: dims %s acts %s B %d M %d C %d fused %d" % (it, dims, acts, b, m, c, fused))
        assert fused == int(_fused_expected(dims, b)), (dims, b)
        nfused += fused
        _assert_oracle(lp, g, table, w_swa, p, x, y, 1.1, z)
    assert nfused >= 1


# ----------------------------------------------------------------------------------------------- 7. MALA
def test_mala_chains_on_the_device_gradient(si, gpu_ctx):
    from subspaceinference_jl_amd import samplers
    dims, acts, b, m = [6, 30, 2], [2, 0], 200, 4
    table, n, w_swa, p, x, y = _problem(dims, acts, b, m, seed=8)
    gpu_ctx.infer_setup(table, n, m, w_swa, p, x, y, sigma_m=1.5)
    zg, lpg, accg = samplers.mala_chains(gpu_ctx.logdensity_grad_batch, m, 40, 0.05, [np.random.default_rng([3, c]) for c in range(3)])
    assert gpu_ctx.grad_kernel_info() == 1
    assert zg.shape == (m, 40, 3) and lpg.shape == (40, 3) and accg.shape == (3,)
    for c in range(3):
        zo, lpo, acco = samplers.mala(lambda z: so.logdensity_grad(table, w_swa, p, x, y, 1.5, z)[:2], m, 40, 0.05,
                                      np.random.default_rng([3, c]))
        assert np.allclose(zg[:, :, c], zo, rtol=1e-7, atol=1e-9) and np.allclose(lpg[:, c], lpo, rtol=1e-9)
        assert abs(accg[c] - acco) < 1e-9 and 0.05 < accg[c] <= 1.0


def test_sub_inference_mala_nchains(si, gpu_ctx):
    from subspaceinference_jl_amd import flux
    rng = np.random.default_rng(0)
    model = flux.Chain(flux.Dense(4, 8, "relu", rng=rng), flux.Dense(8, 1, rng=rng))
    x, y = rng.standard_normal((4, 50)), rng.standard_normal((1, 50))
    data = flux.DataLoader(x, y, batchsize=50)
    _, n = flux.layer_table(model)
    w_swa, p = 0.1 * rng.standard_normal(n), 0.05 * rng.standard_normal((n, 3))
    kw = dict(σ_z=0.05, itr=12, M=3, ctx=gpu_ctx, seed=5, alg=":mala")
    z, lp = si.sub_inference(model, data, w_swa, p, chain_id=1, nchains=3, return_z=True, **kw)
    assert z.shape == (3, 12, 3) and lp.shape == (12, 3)
    for c in range(3):
        z1, lp1 = si.sub_inference(model, data, w_swa, p, chain_id=1 + c, return_z=True, **kw)
        assert np.allclose(z[:, :, c], z1, rtol=1e-7, atol=1e-9) and np.allclose(lp[:, c], lp1, rtol=1e-9)
    chn, lpw = si.sub_inference(model, data, w_swa, p, chain_id=1, nchains=3, **kw)
    assert len(chn) == 3 and len(chn[0]) == 12 and np.allclose(chn[2][5], w_swa + p @ z[:, 5, 2], rtol=1e-13)
    assert np.array_equal(lpw, lp)
    for alg in (":hmc", ":nuts", ":advi"):
        with pytest.raises(si.SubspaceError):
            si.sub_inference(model, data, w_swa, p, itr=5, M=3, ctx=gpu_ctx, alg=alg, nchains=2)
