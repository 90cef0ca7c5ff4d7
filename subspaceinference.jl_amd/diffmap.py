"""The diffusion map of `diffusion_subspace` (reference src/subspace_construction.jl:202-206) restated in plain NumPy.

The reference calls ManifoldLearning 0.6.2: `diff_M = fit(DiffMap, A', maxoutdim = M); P = transform(diff_M)` and returns
`(W_swa, P')`.  Neither that package nor Julia is available to this build, so everything below is

    [upstream, from memory, unverifiable offline]

and every point where memory may be wrong is a named parameter (`eps`, `alpha`, `kernel_sign`, `rescale`): a maintainer
with Julia matches upstream by changing a default, not a kernel (tests/golden/make_golden_diffmap.jl writes the data to
compare against).  This file is to si_construct_finish_diffmap what samplers.py is to the device samplers: the definition
the device result is tested against.  It is dense and O(N^3): use it for tests only.
"""
import numpy as np

from ._capi import SubspaceError


def rescale_unit_range(X):
    """StatsBase `fit(UnitRangeTransform, X; dims = 2)` + `transform` as ManifoldLearning's DiffMap applies it to the K x N
    data: per ROW k (one snapshot) (x - min_k) * (1 / (max_k - min_k)); a NaN (constant row: 0 * Inf) becomes 0."""
    mn = X.min(axis=1, keepdims=True)
    mx = X.max(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        sc = 1.0 / (mx - mn)
        Xr = (X - mn) * sc
    Xr[np.isnan(Xr)] = 0.0
    return Xr


def sign_convention(P):
    """each column's entry of largest magnitude is positive (lowest index on a tie), as in si_construct_finish"""
    P = np.array(P, dtype=np.float64, order="F")
    for j in range(P.shape[1]):
        i = int(np.argmax(np.abs(P[:, j])))   # (argmax returns the first of equal maxima)
        if P[i, j] < 0.0:
            P[:, j] = -P[:, j]
    return P


def diffmap_kernel(A, eps=1.0, alpha=1.0, kernel_sign=-1, rescale=True):
    """Steps 1-3 of the definition: the normalised symmetric kernel matrix Kn (N x N) and q (Kn's Perron vector, unnormalised)
    of the N x K deviation matrix A (column k = snapshot k, as si_construct_get_A returns it)."""
    A = np.asarray(A, dtype=np.float64)
    if A.ndim != 2:
        raise SubspaceError("diffmap: A must be the N x K deviation matrix")
    if kernel_sign not in (1, -1):
        raise SubspaceError("diffmap: kernel_sign must be +1 or -1")
    if not (np.isfinite(eps) and np.isfinite(alpha) and eps > 0.0):
        raise SubspaceError("diffmap: eps must be positive and finite, alpha finite")
    X = np.ascontiguousarray(A.T)   # reference :204: fit(DiffMap, A', ...): K x N, column i = the K deviations of weight i
    # 1. rescale (DiffMap's transform of the data before the kernel)
    Xr = rescale_unit_range(X) if rescale else X
    # 2. kernel: pairwise squared distances from the Gram matrix (upstream: pairwise(SqEuclidean(), X, dims = 2)), then
    #    exp(kernel_sign * d / eps); kernel_sign = -1 is the Gaussian kernel of upstream's docstring, +1 what 0.6.2's source is
    #    remembered to compute
    s = np.sum(Xr * Xr, axis=0)
    S = Xr.T @ Xr
    S = 0.5 * (S + S.T)   # (BLAS gives S_ij and S_ji the same bits in practice; made certain)
    d = (s[:, None] + s[None, :]) - 2.0 * S
    with np.errstate(over="ignore"):
        Kmat = np.exp(kernel_sign * d / eps)
    if not np.all(np.isfinite(Kmat)):
        raise SubspaceError("diffmap: the kernel matrix has a non-finite entry (exp overflows: kernel_sign = +1 with "
                            "distances / eps beyond 709)")
    # 3. normalise: upstream's `normalize!(L, alpha)` with t = 1, then the symmetric conjugate of the Markov matrix
    p = Kmat.sum(axis=1)
    Kmat = Kmat / (np.outer(p, p) ** alpha)
    q = np.sqrt(Kmat.sum(axis=1))
    Kn = Kmat / np.outer(q, q)
    return Kn, q


def diffmap_dense(A, M, eps=1.0, alpha=1.0, kernel_sign=-1, rescale=True):
    """(P, lam, u1, Kn): P (N x M) the reference's projection matrix, lam the M + 1 leading eigenvalues of Kn ordered by
    |lambda| descending (lam[0] = 1), u1 = q / ||q|| and Kn itself."""
    Kn, q = diffmap_kernel(A, eps, alpha, kernel_sign, rescale)
    N = Kn.shape[0]
    if M < 1:
        raise SubspaceError("diffmap: M must be positive")
    if M + 1 > N - 1:
        raise IndexError("BoundsError: diffmap needs M + 1 <= N - 1")
    # 4. spectrum: svd(Kn) of a symmetric matrix = its eigenvectors ordered by |lambda| descending
    w, U = np.linalg.eigh(Kn)
    order = np.argsort(-np.abs(w), kind="stable")
    w, U = w[order], U[:, order]
    u1 = q / np.linalg.norm(q)
    # lambda_1 = 1 with the Perron vector: take it analytically (eigh's copy of it has an arbitrary sign)
    lead = int(np.argmax(np.abs(U.T @ u1)))
    rest = [i for i in range(N) if i != lead][:M]
    # 5. projection (upstream's transform: the non-trivial vectors over the trivial one), reference :205-206
    Y = U[:, rest] / u1[:, None]
    lam = np.concatenate(([w[lead]], w[rest]))
    return sign_convention(Y), lam, u1, Kn


def spectrum_gap(Kn, M):
    """min | |lambda_j| - |lambda_i| | over j among the leading M + 1 and i any other eigenvalue: where it is small the
    compared vectors are not well defined and a case is of no use"""
    a = np.sort(np.abs(np.linalg.eigvalsh(Kn)))[::-1]
    lead, gap = a[:M + 1], np.inf
    for j in range(M + 1):
        others = np.delete(a, j)
        gap = min(gap, float(np.min(np.abs(others - lead[j]))))
    return gap
