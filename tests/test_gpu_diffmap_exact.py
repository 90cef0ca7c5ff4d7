"""GPU tests that pin method = :diffusion (si_construct_finish_diffmap) the way the other kernel families are pinned.

1. test_exact_operator: on the 0/1 kernel-matrix family of tests/diffmap_exact.py, Kn and u_1 read back from the device are
   BIT-EQUAL to the helper's restatement of steps 1-3, at every N at and around the 64-row tile edges, below one tile and below one
   16-row wave patch; the finish with M = 1 succeeds on these exactly degenerate operators (eigenvalue 1 once per cluster).
2. test_route_case: every case of tests/diffmap_routes.py::CASES (their routes together are diffmap_routes.REACHABLE) converges,
   passes the reference-free checks of test_gpu_diffmap.py::test_vectors_without_the_reference, and agrees with the dense NumPy
   reference (diffmap.diffmap_dense on the deviation columns the device holds) within the bounds of test_gpu_diffmap.py.
3. test_state_between_calls: finishes of different M and K on one construction equal the same calls on fresh contexts, bit for bit.
profiles/diffmap_exact_kernel_names.txt is the kernel trace of this file.

Measured on an MI355X (every figure is printed with -s): see DESIGN section 16."""
import numpy as np
import pytest

import diffmap_cases as dc
from tests import diffmap_exact as dx
from tests import diffmap_routes as dr
from test_gpu_diffmap import TOL, entry_bound

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dmp(si):
    from subspaceinference_jl_amd import diffmap
    return diffmap


def _where(diff):
    """the 64 x 64 tiles (I, J) a mismatch lies in, for the failure message"""
    i, j = np.nonzero(diff)
    return "%d entries differ, in tiles %s" % (i.size, sorted(set(zip((i // 64).tolist(), (j // 64).tolist())))[:12])


# ---------------------------------------------------------------------------------------------- 1. the exact family
@pytest.mark.parametrize("n,k,family,rescale,alpha,f32", dx.GRID)
def test_exact_operator(si, gpu_ctx, n, k, family, rescale, alpha, f32):
    a, lab = dx.lattice(n, k, family)
    ad = dc.push_columns(gpu_ctx, a, si._capi.SI_F32 if f32 else None)
    assert np.array_equal(ad, a)          # the SWA recurrence and fp32 storage are exact on the lattice
    failure = None
    try:
        _, p, lam, kk = gpu_ctx.construct_finish_diffmap(1, dx.EPS, alpha, dx.SIGN, rescale)
    except si.SubspaceError as e:         # (the read-back below is valid whether or not the iteration converged)
        failure = e
    kn, u1 = gpu_ctx.diffmap_get_kernel()
    kn_ref, _, u1_ref = dx.kernel_of(n, family, alpha)
    assert np.array_equal(kn != 0.0, dx.membership(lab) == 1.0), "exp(-1024) != 0 or a wrong tile: " + _where((kn != 0.0) != (dx.membership(lab) == 1.0))
    assert np.array_equal(kn, kn_ref), _where(kn != kn_ref)
    assert np.array_equal(kn, kn.T)
    assert np.array_equal(u1, u1_ref), "%d entries of u_1 differ" % np.count_nonzero(u1 != u1_ref)
    assert failure is None, failure
    assert kk == k and lam[0] == 1.0
    nc = int(lab.max()) + 1
    it, res = gpu_ctx.diffmap_info()
    print("exact N=%d K=%d %s: %d clusters, %d iterations, residual %.2e, lam[1] - 1 = %.2e" % (n, k, family, nc, it, res, lam[1] - 1.0))
    if nc >= 3:
        assert abs(lam[1] - 1.0) <= 1e-12
    assert res <= 1e-12
    u = p[:, 0] * u1
    for c in range(nc):   # every eigenvector of blockdiag(J_c / c) is constant on every cluster
        assert np.ptp(u[lab == c]) <= 1e-12, c


@pytest.mark.parametrize("n,alpha", [(16, 1000.0), (17, 1000.0), (65, -1000.0)])
def test_non_finite_operator_is_refused(si, gpu_ctx, n, alpha):
    """a finite alpha whose pow over- or underflows (cluster sizes >= 5: w >= 25) makes the normalised operator 0 / 0: the host
    algebra is handed NaN and must refuse it and leave the context whole (the QL sweep of csrc/eig.cpp once ran past its buffers
    on NaN input; tests/native/eig_sanitize_main.cpp holds that directly)"""
    a, lab = dx.lattice(n, 3, "mod3")
    dc.push_columns(gpu_ctx, a)
    with pytest.raises(si.SubspaceError, match="lost its rank") as e:
        gpu_ctx.construct_finish_diffmap(1, dx.EPS, alpha, dx.SIGN, True)
    assert e.value.code == si._capi.SI_ERR_INVALID
    kn, _ = gpu_ctx.diffmap_get_kernel()
    assert not np.all(np.isfinite(kn))
    gpu_ctx.construct_finish_diffmap(1, dx.EPS, 1.0, dx.SIGN, True)     # and the context is whole afterwards
    assert np.array_equal(gpu_ctx.diffmap_get_kernel()[0], dx.kernel_of(n, "mod3", 1.0)[0])


# ---------------------------------------------------------------------------------------------- 2. the route table
def _case_id(c):
    return "N%d-K%d-M%d-%s%s-s%d" % (c[0], c[1], c[2], "plus" if c[3] == 1 else "minus", "-f32" if c[5][0] == "uniform32" else "", c[5][1])


@pytest.mark.parametrize("case", dr.CASES, ids=_case_id)
def test_route_case(si, gpu_ctx, dmp, case):
    n, k, m, sign, eps, (gen, _) = case
    ad = dc.push_columns(gpu_ctx, dr.case_input(case), si._capi.SI_F32 if gen == "uniform32" else None)
    if gen == "uniform32":
        assert np.array_equal(ad, ad.astype(np.float32))
    _, p, lam, kk = gpu_ctx.construct_finish_diffmap(m, eps=eps, kernel_sign=sign)     # converges, or raises
    it, res = gpu_ctx.diffmap_info()
    assert kk == k and res <= TOL
    assert it >= 2 or dr.block_sizes(n, k, m)["b"] == n - 1      # the next-block product ran (diffmap_routes.case_routes counts on it)
    kn, u1 = gpu_ctx.diffmap_get_kernel()
    # the reference-free checks of test_vectors_without_the_reference
    u = p * u1[:, None]
    assert np.max(np.abs(u.T @ u - np.eye(m))) <= 1e-10
    assert np.max(np.abs(u.T @ u1)) <= 1e-10
    rk = np.linalg.norm(kn @ u - u * lam[1:], axis=0).max()
    assert rk <= 10.0 * TOL
    assert np.all(np.diff(np.abs(lam)) <= 0.0)
    for j in range(m):
        assert p[np.argmax(np.abs(p[:, j])), j] > 0.0
    # the dense reference on what the device holds
    p_ref, lam_ref, u1_ref, kn_ref = dmp.diffmap_dense(ad, m, eps=eps, kernel_sign=sign)
    r = entry_bound(n, k, eps)
    lam_err, lam_bound = float(np.max(np.abs(lam - lam_ref))), 10.0 * (TOL + r)
    gap = dmp.spectrum_gap(kn_ref, m)
    free = dr.exempt(n, m, sign)
    line = "route N=%d K=%d M=%d sign=%+d: %d iterations, residual %.2e (against Kn %.2e), max |lam - lam_ref| %.3e of %.3e, gap %.2e" % (
        n, k, m, sign, it, res, rk, lam_err, lam_bound, gap)
    if gap >= dr.GAP_MIN:
        err, bound = float(np.max(np.abs(p - p_ref))), 10.0 * (TOL + r) / (gap * u1_ref.min())
        line += ", max |P - P_ref| %.3e of %.3e (ratio %.2e)" % (err, bound, err / bound)
    print(line)
    assert lam[0] == 1.0 and lam_err <= lam_bound
    assert free or gap >= dr.GAP_MIN      # (tests/test_diffmap_routes_cpu.py holds this on the generated input)
    if gap >= dr.GAP_MIN:
        assert err <= bound


# ---------------------------------------------------------------------------------------------- 3. state between calls
STATE_N, STATE_K0, STATE_K1 = 129, 7, 9    # K crosses a multiple of 4: Kp = 8, then 12


def _push_range(ctx, a, s, j0, j1):
    for j in range(j0, j1):
        ctx.construct_push(s + 2.0 * a[:, j], 1.0)    # (as diffmap_cases.push_columns)
        s = s + a[:, j]
    return s


def _begin_and_push(ctx, a, k):
    ctx.construct_begin(a.shape[0], a.shape[1])
    return _push_range(ctx, a, np.zeros(a.shape[0]), 0, k)


def _finish(ctx, m):
    _, p, lam, kk = ctx.construct_finish_diffmap(m, eps=0.25)
    kn, u1 = ctx.diffmap_get_kernel()
    return dict(p=p, lam=lam, kn=kn, u1=u1, k=kk, iters=ctx.diffmap_info()[0], residual=ctx.diffmap_info()[1])


def _same(x, y, what):
    assert x.keys() == y.keys()
    for key in x:
        assert np.array_equal(x[key], y[key]), "%s: %s differs from the fresh context's" % (what, key)


def test_state_between_calls(si, gpu_ctx):
    a = dr.uniform(STATE_N, STATE_K1, 4)
    s = _begin_and_push(gpu_ctx, a, STATE_K0)
    got = [(25, STATE_K0, _finish(gpu_ctx, 25)), (2, STATE_K0, _finish(gpu_ctx, 2))]
    _push_range(gpu_ctx, a, s, STATE_K0, STATE_K1)
    got += [(2, STATE_K1, _finish(gpu_ctx, 2)), (25, STATE_K1, _finish(gpu_ctx, 25))]
    pca = gpu_ctx.construct_finish(3)
    for m, k, res in got:
        assert res["k"] == k and res["residual"] <= TOL
        with si.Context(0) as fresh:
            _begin_and_push(fresh, a, k)
            _same(res, _finish(fresh, m), "M = %d at K = %d" % (m, k))
    with si.Context(0) as fresh:
        _begin_and_push(fresh, a, STATE_K1)
        for x, y in zip(pca, fresh.construct_finish(3)):
            assert np.array_equal(x, y)
    assert not np.array_equal(got[0][2]["kn"], got[3][2]["kn"])     # the two K are different operators
    gpu_ctx.construct_begin(8, 1)   # leave the shared context small
