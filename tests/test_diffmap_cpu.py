"""CPU tests of method = :diffusion: identities of the NumPy restatement (diffmap.diffmap_dense) that hold whether or not the
restatement of ManifoldLearning 0.6.2 is right, the boundary (exported symbols, API names), and the condition under which the
GPU tests' comparisons mean something: every case's leading eigenvalues are separated (spectrum_gap >= 1e-3)."""
import numpy as np
import pytest

import diffmap_cases as dc


@pytest.fixture(scope="module")
def dmp(si):
    from subspaceinference_jl_amd import diffmap
    return diffmap


@pytest.mark.parametrize("sign", dc.SIGNS)
@pytest.mark.parametrize("rescale", [True, False])
def test_kernel_identities(dmp, sign, rescale):
    a = dc.clustered(*dc.CASES[0])
    p, lam, u1, kn = dmp.diffmap_dense(a, 3, eps=2.0, alpha=0.5, kernel_sign=sign, rescale=rescale)
    assert np.array_equal(kn, kn.T)
    assert abs(lam[0] - 1.0) <= 1e-12
    _, q = dmp.diffmap_kernel(a, eps=2.0, alpha=0.5, kernel_sign=sign, rescale=rescale)
    assert np.array_equal(u1, q / np.linalg.norm(q)) and np.all(u1 > 0.0)
    assert np.linalg.norm(kn @ u1 - u1) <= 1e-13                      # the Perron pair
    assert np.all(np.abs(lam[1:]) <= 1.0 + 1e-12) and np.all(np.diff(np.abs(lam)) <= 1e-15)
    u = p * u1[:, None]                                               # the vectors back from the projection
    assert np.allclose(u.T @ u, np.eye(3), atol=1e-12) and np.allclose(u.T @ u1, 0.0, atol=1e-12)
    assert np.allclose(kn @ u, u * lam[1:], atol=1e-12)
    for j in range(3):                                                # the sign convention
        assert p[np.argmax(np.abs(p[:, j])), j] > 0.0


def test_constant_snapshot_rescales_to_zeros(dmp):
    a = np.array(dc.clustered(*dc.CASES[0]))
    a[:, 2] = 0.375
    xr = dmp.rescale_unit_range(np.ascontiguousarray(a.T))
    assert np.array_equal(xr[2], np.zeros(a.shape[0]))
    assert xr.min() == 0.0 and xr.max() == 1.0 and np.all(np.isfinite(xr))
    b = np.delete(a, 2, axis=1)                                       # a snapshot of zeros adds nothing to any distance
    assert np.allclose(dmp.diffmap_kernel(a)[0], dmp.diffmap_kernel(b)[0], rtol=1e-13, atol=0.0)   # (BLAS sums K terms in another order)


def test_permuting_the_weights_permutes_the_rows_of_p(dmp):
    a = dc.clustered(*dc.CASES[0])
    perm = np.random.default_rng(5).permutation(a.shape[0])
    p = dmp.diffmap_dense(a, 3)[0]
    pp = dmp.diffmap_dense(a[perm], 3)[0]
    gap = dmp.spectrum_gap(dmp.diffmap_kernel(a)[0], 3)
    assert np.max(np.abs(pp - p[perm])) <= 1e-12 / gap


def test_overflow_is_reported(dmp, si):
    a = 40.0 * np.array(dc.clustered(*dc.CASES[0]))
    with pytest.raises(si.SubspaceError, match="non-finite"):
        dmp.diffmap_dense(a, 2, kernel_sign=1, rescale=False)
    kn = dmp.diffmap_dense(a, 2, kernel_sign=1, rescale=True)[3]      # rescaled distances are <= K: no overflow
    assert np.all(np.isfinite(kn))
    for bad in (dict(kernel_sign=0), dict(eps=0.0), dict(eps=np.nan), dict(alpha=np.inf)):
        with pytest.raises(si.SubspaceError):
            dmp.diffmap_dense(a, 2, **bad)
    with pytest.raises(IndexError):
        dmp.diffmap_dense(a[:6], 5)


def test_library_and_api_have_the_route(si):
    lib = si.load()
    for name in ("si_construct_finish_diffmap", "si_diffmap_info", "si_diffmap_get_kernel"):
        assert hasattr(lib, name) and name in si._capi.SIGNATURES
    assert callable(si.diffusion_subspace) and "diffusion_subspace" in si.__all__
    assert hasattr(si.Context, "construct_finish_diffmap")
    from subspaceinference_jl_amd import flux
    m = flux.Chain(flux.Dense(3, 2))
    data = flux.DataLoader(np.zeros((3, 4)), np.zeros((2, 4)))
    with pytest.raises(si.SubspaceError, match="No method found"):
        si.subspace_inference(m, flux.mse, data, flux.Descent(0.1), method=":x")


@pytest.mark.parametrize("case", dc.CASES)
def test_case_list_is_well_separated(dmp, case):
    a = dc.clustered(*case)
    for sign in dc.SIGNS:
        kn = dmp.diffmap_kernel(a, kernel_sign=sign)[0]
        for m in dc.MS:
            assert dmp.spectrum_gap(kn, m) >= 1e-3, (case, sign, m)


def test_trained_toy_is_well_separated(dmp):
    _, a = dc.toy_deviations()
    assert a.shape == (682, 30)
    for sign in dc.SIGNS:
        for eps in (1.0, 10.0):
            kn = dmp.diffmap_kernel(a, eps=eps, kernel_sign=sign)[0]
            for m in dc.MS:
                assert dmp.spectrum_gap(kn, m) >= 1e-3, (sign, eps, m)
