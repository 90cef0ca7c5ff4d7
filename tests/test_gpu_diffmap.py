"""GPU tests of method = :diffusion (si_construct_finish_diffmap) against the NumPy restatement diffmap.diffmap_dense, which is fed
the deviation columns the device holds (si_construct_get_A).

Tolerances.  An entry of Kn: both sides round a K-term dot product (its error enters the exponent divided by eps) and two
N-term sums, so the entrywise relative bound is r = 2 * (16 K^2 / eps + 4 N + 64) * 2^-53.  P: an eigenvector of a symmetric
matrix perturbed by E moves by ||E|| / gap, the iteration stops at a residual tol, and P = u ./ u_1 divides by entries as small
as min(u_1): max |P_dev - P_ref| <= 10 * (tol + r) / (gap * min(u_1)), gap being computed here from the dense spectrum.
lambda: 10 * (tol + r).

Measured on an MI355X (the tests print every figure with -s): operator, max relative error 9e-16 .. 1.4e-14 against bounds of
1.7e-13 .. 6.7e-12 (at most 0.02 of the bound); result, max |P_dev - P_ref| at most 3.1e-11 on the case list and 1.2e-9 on the
trained toy (M = 5, eps = 10, gap 1.05e-3), at most 4e-3 of the bound everywhere; 5 .. 13 iterations; residuals against the
read-back Kn at most 8.8e-13."""
import numpy as np
import pytest

import diffmap_cases as dc
from oracle import subspace_oracle as so

pytestmark = pytest.mark.gpu
TOL = 1e-12   # the library's default stopping residual
U = 2.0 ** -53


def entry_bound(n, k, eps):
    return 2.0 * (16.0 * k * k / eps + 4.0 * n + 64.0) * U


@pytest.fixture(scope="module")
def dmp(si):
    from subspaceinference_jl_amd import diffmap
    return diffmap


OPERATOR_CASES = [
    # N, K, sign, eps, alpha, rescale, fp32 storage, a constant snapshot
    (77, 5, -1, 1.0, 1.0, True, False, False),
    (77, 5, 1, 0.5, 1.0, False, False, False),
    (200, 1, -1, 1.0, 1.0, True, False, False),          # K = 1: a single k step, three zero rows in it
    (200, 7, 1, 0.5, 0.5, True, False, False),
    (333, 12, -1, 10.0, 1.0, False, False, False),
    (333, 12, 1, 1.0, 1.0, True, True, False),            # fp32 storage of A
    (682, 30, 1, 10.0, 0.5, True, False, True),           # a constant snapshot: 0 * Inf -> 0
    (2051, 37, -1, 1.0, 1.0, True, False, False),         # 33 row blocks: 561 workgroups, 33 row-sum partials per row
    # ---- the operator's edges on real-valued inputs: N at a 64-row tile edge (ldn == Npad == N, a full last tile) and one
    # past it, one 16-row wave patch, the smallest N; K a multiple of 4 (Kp == K); K > N; alpha = 0 and 0.5 at a tile edge
    (64, 4, -1, 1.0, 1.0, True, False, False),
    (64, 8, -1, 1.0, 1.0, True, True, False),             # fp32 storage at a tile edge
    (65, 8, 1, 0.5, 1.0, False, False, False),
    (128, 8, -1, 1.0, 0.0, True, False, False),           # alpha = 0: pow(w, 0) = 1
    (128, 4, 1, 0.5, 0.5, True, False, False),
    (16, 4, -1, 1.0, 1.0, False, False, False),
    (3, 4, 1, 0.5, 1.0, True, False, False),              # the smallest legal N (M = 1)
    (3, 8, -1, 1.0, 0.5, True, False, False),             # K > N
    (20, 30, 1, 10.0, 1.0, True, False, False),           # K > N
]


@pytest.mark.parametrize("n,k,sign,eps,alpha,rescale,f32,const", OPERATOR_CASES)
def test_operator(si, gpu_ctx, dmp, n, k, sign, eps, alpha, rescale, f32, const):
    a = np.array(dc.clustered(n, k, 6, 0))
    if const:
        a[:, 0] = 0.375   # (the first push's deviation column is exactly the column handed in)
    ad = dc.push_columns(gpu_ctx, a, si._capi.SI_F32 if f32 else None)
    if f32:
        assert np.array_equal(ad, ad.astype(np.float32))
    if const:
        assert np.all(ad[:, 0] == 0.375)
    m = min(2, n - 2)   # (N = 3 admits M = 1 only)
    _, p1, lam1, kk = gpu_ctx.construct_finish_diffmap(m, eps, alpha, sign, rescale)
    assert kk == k
    kn, u1 = gpu_ctx.diffmap_get_kernel()
    kn_ref, q = dmp.diffmap_kernel(ad, eps, alpha, sign, rescale)
    r = entry_bound(n, k, eps)
    err = float(np.max(np.abs(kn - kn_ref) / np.abs(kn_ref)))
    print("operator N=%d K=%d: max relative error %.3e, bound %.3e" % (n, k, err, r))
    assert err <= r
    assert np.array_equal(kn, kn.T)
    assert np.max(np.abs(u1 - q / np.linalg.norm(q)) / u1) <= r
    # the bits do not depend on the run
    _, p2, lam2, _ = gpu_ctx.construct_finish_diffmap(m, eps, alpha, sign, rescale)
    kn2, u12 = gpu_ctx.diffmap_get_kernel()
    assert np.array_equal(kn, kn2) and np.array_equal(u1, u12) and np.array_equal(p1, p2) and np.array_equal(lam1, lam2)


def _check_result(gpu_ctx, dmp, ad, m, sign, eps, what):
    n, k = ad.shape
    w, p, lam, _ = gpu_ctx.construct_finish_diffmap(m, eps=eps, kernel_sign=sign)
    p_ref, lam_ref, u1_ref, kn_ref = dmp.diffmap_dense(ad, m, eps=eps, kernel_sign=sign)
    gap = dmp.spectrum_gap(kn_ref, m)
    r = entry_bound(n, k, eps)
    bound = 10.0 * (TOL + r) / (gap * u1_ref.min())
    err = float(np.max(np.abs(p - p_ref)))
    it, res = gpu_ctx.diffmap_info()
    print("%s M=%d sign=%+d eps=%g: %d iterations, residual %.2e, max |P - P_ref| %.3e, bound %.3e, gap %.2e" % (
        what, m, sign, eps, it, res, err, bound, gap))
    assert res <= TOL
    assert err <= bound
    assert lam[0] == 1.0 and np.max(np.abs(lam - lam_ref)) <= 10.0 * (TOL + r)
    return w, p


@pytest.mark.parametrize("sign", dc.SIGNS)
@pytest.mark.parametrize("case", dc.CASES)
def test_result_on_the_case_list(gpu_ctx, dmp, case, sign):
    ad = dc.push_columns(gpu_ctx, dc.clustered(*case))
    for m in dc.MS:
        _check_result(gpu_ctx, dmp, ad, m, sign, 1.0, "case %s" % (case,))


def _push_toy(ctx):
    snaps, ns = dc.trained_toy()[:2]
    ctx.construct_begin(snaps[0].size, len(snaps))
    for wv, nn in zip(snaps, ns):
        ctx.construct_push(wv, nn)
    return ctx.construct_get_A(0, len(snaps))


@pytest.mark.parametrize("sign,eps", [(-1, 1.0), (1, 1.0), (-1, 10.0), (1, 10.0)])
def test_result_on_the_trained_toy(gpu_ctx, dmp, sign, eps):
    ad = _push_toy(gpu_ctx)
    assert np.array_equal(ad, dc.toy_deviations()[1])    # K1 is bit-exact: the device holds the oracle's deviation matrix
    for m in dc.MS:
        _check_result(gpu_ctx, dmp, ad, m, sign, eps, "toy")


@pytest.mark.parametrize("n,k,m,sign", [(2051, 37, 10, -1), (333, 12, 10, 1), (77, 5, 3, -1)])
def test_vectors_without_the_reference(gpu_ctx, n, k, m, sign):
    """M = 10 gives a block of 36 columns: the products and the rotation run on the matrix-core kernels of K3"""
    dc.push_columns(gpu_ctx, dc.clustered(n, k, 6, 0))
    _, p, lam, _ = gpu_ctx.construct_finish_diffmap(m, kernel_sign=sign)
    kn, u1 = gpu_ctx.diffmap_get_kernel()
    u = p * u1[:, None]
    g = u.T @ u
    assert np.max(np.abs(g - np.eye(m))) <= 1e-10
    assert np.max(np.abs(u.T @ u1)) <= 1e-10
    res = np.linalg.norm(kn @ u - u * lam[1:], axis=0)
    print("N=%d M=%d: residuals against the read-back Kn %.2e" % (n, m, res.max()))
    assert res.max() <= 10.0 * TOL
    assert np.all(np.diff(np.abs(lam)) <= 0.0)
    for j in range(m):
        assert p[np.argmax(np.abs(p[:, j])), j] > 0.0


def test_pca_finish_is_untouched(gpu_ctx):
    _push_toy(gpu_ctx)
    w1, p1, s1, _ = gpu_ctx.construct_finish(3)
    wd, pd, lam, _ = gpu_ctx.construct_finish_diffmap(3)
    w3, p3, s3, _ = gpu_ctx.construct_finish(3)
    assert np.array_equal(p1, p3) and np.array_equal(s1, s3) and np.array_equal(w1, w3) and np.array_equal(w1, wd)
    assert not np.array_equal(p1, pd)
    # and the finished construction the ctx holds after a diffusion finish is the diffusion map's
    gpu_ctx.construct_finish_diffmap(3)
    w, p, s = gpu_ctx.construct_get_result()
    assert np.array_equal(p, pd) and np.array_equal(s, np.abs(lam[1:])) and np.array_equal(w, wd)
    assert gpu_ctx.construct_result_ptr()[3] == 3


def test_density_on_the_diffusion_subspace(gpu_ctx):
    _, _, _, x, y = dc.trained_toy()
    _push_toy(gpu_ctx)
    w_swa, p, _, _ = gpu_ctx.construct_finish_diffmap(3)
    table, n = so.layer_table([10, 20, 20, 2], [1, 1, 0])
    assert n == w_swa.size
    gpu_ctx.infer_setup(table, n, 3, None, None, x, y, 0.7)   # W_swa / P taken in place on the device
    zs = np.asfortranarray(0.01 * np.random.default_rng(1).standard_normal((3, 3)))
    lp = gpu_ctx.logdensity(zs)
    lp_ref = np.array([so.logdensity(table, w_swa, p, x, y, 0.7, zs[:, j]) for j in range(3)])
    assert np.allclose(lp, lp_ref, rtol=1e-11)    # test_gpu_parity.py's tolerance for the density


def test_subspace_inference_by_diffusion(si):
    from subspaceinference_jl_amd import flux
    rng = np.random.default_rng(0)
    x, y = rng.random((10, 100)), rng.random((2, 100))
    m = flux.Chain(flux.Dense(10, 20, rng=rng), flux.Dense(20, 20, rng=rng), flux.Dense(20, 2, rng=rng))
    data = flux.DataLoader(x, y, batchsize=10, shuffle=True, rng=rng)
    chn, lp, w_swa = si.subspace_inference(m, flux.mse, data, flux.ADAM(0.01), itr=20, T=3, c=1, M=3, alg=":rwmh",
                                           method=":diffusion", verbose=False)
    assert len(chn) == 20 and lp.shape == (20,) and np.all(np.isfinite(lp))
    assert w_swa.shape == (682,) and all(c.shape == (682,) and np.all(np.isfinite(c)) for c in chn)
    w2, p2 = si.diffusion_subspace(m, flux.mse, data, flux.ADAM(0.01), T=3, M=2, verbose=False, kernel_sign=1, eps=10.0)
    assert p2.shape == (682, 2) and np.all(np.isfinite(p2)) and w2.shape == (682,)


def test_refusals(si, gpu_ctx):
    inv, bounds, state = si._capi.SI_ERR_INVALID, si._capi.SI_ERR_BOUNDS, si._capi.SI_ERR_STATE
    gpu_ctx.construct_begin(40, 3)
    with pytest.raises(si.SubspaceError) as e:
        gpu_ctx.construct_finish_diffmap(2)
    assert e.value.code == state
    a = np.array(dc.clustered(*dc.CASES[0]))
    dc.push_columns(gpu_ctx, a)
    for kw in (dict(m=0), dict(m=2, eps=0.0), dict(m=2, eps=float("nan")), dict(m=2, eps=float("inf")), dict(m=2, alpha=float("inf")),
               dict(m=2, alpha=float("nan")), dict(m=2, kernel_sign=0), dict(m=2, kernel_sign=2)):
        with pytest.raises(si.SubspaceError) as e:
            gpu_ctx.construct_finish_diffmap(**kw)
        assert e.value.code == inv, kw
        assert gpu_ctx.diffmap_info() == (0, 0.0)
    with pytest.raises(si.BoundsError) as e:
        gpu_ctx.construct_finish_diffmap(a.shape[0] - 1)       # M + 1 = N - 1 is the last that fits
    assert e.value.code == bounds
    with pytest.raises(si.SubspaceError, match="not converged after 1 iterations") as e:
        gpu_ctx.construct_finish_diffmap(3, max_iters=1)
    assert e.value.code == inv and gpu_ctx.diffmap_info()[0] == 1
    dc.push_columns(gpu_ctx, 40.0 * a)
    with pytest.raises(si.SubspaceError, match="non-finite") as e:
        gpu_ctx.construct_finish_diffmap(2, kernel_sign=1, rescale=False)    # exp(d / eps) overflows
    assert e.value.code == inv
    gpu_ctx.construct_finish_diffmap(2, kernel_sign=1, rescale=True)         # rescaled: d <= K
    gpu_ctx.construct_begin(65537, 1)
    gpu_ctx.construct_push(np.zeros(65537, dtype=np.float32), 1.0)
    with pytest.raises(si.SubspaceError, match="34 GB") as e:
        gpu_ctx.construct_finish_diffmap(2)
    assert e.value.code == inv
    gpu_ctx.construct_begin(8, 1)   # leave the shared context small
