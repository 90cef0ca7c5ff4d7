"""The helpers of tests/test_gpu_finish_exact.py, certified without a GPU: project_exact equals a restatement in exact
rationals; assert_projection passes every legitimate fp64 evaluation of A V and fails the errors the GPU tests are meant to
catch; finish_v_reference restates the ladder of csrc/capi.hip (held by a text check of the statements it mirrors) and is
deterministic; the recorded table of the diagonal-G legs and the sign-margin conditions hold for the chosen seeds."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import lattice as lat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_AV = [(n, k, m) for n, k, m, _ in lat.FINISH_F64 + lat.FINISH_F32]


def _case(n, k, m, seed=0):
    """integer A and a V of full-width doubles (orthonormal columns), as the finish routes meet them"""
    rng = np.random.default_rng(seed + n + k + m)
    a = np.asfortranarray(rng.integers(-2000, 2001, (n, k)).astype(np.float64))
    v, _ = np.linalg.qr(rng.standard_normal((k, max(k, m))))
    return a, np.asfortranarray(v[:, :m])


# ----------------------------------------------------------------------------------------------- project_exact
@pytest.mark.parametrize("n,k,m,float_a", [(7, 1, 1, False), (9, 5, 3, False), (6, 17, 4, False), (5, 33, 2, True), (4, 6, 6, True)])
def test_project_exact_equals_fractions(n, k, m, float_a):
    a, v = _case(n, k, m)
    if float_a:   # a non-integer A (the graded-spectrum problem): both operands are split
        a = a * np.logspace(0, -12, k)[None, :] / 3.0
    v[0, 0] = 2.0 ** -130 * (1.0 + 2.0 ** -52)   # dust of the size the fast solver route leaves
    p, s = lat.project_exact(a, v)
    fr = lat.project_fraction(a, v)
    for i in range(n):
        for j in range(m):
            assert p[i, j] == float(fr[i][j])                       # float(Fraction) rounds correctly: the product rounded ONCE
            s_fr = sum(abs(Fraction(float(a[i, t])) * Fraction(float(v[t, j]))) for t in range(k))
            assert abs(Fraction(float(s[i, j])) - s_fr) <= Fraction(float(lat.gamma(k))) * s_fr
    # a plain fp64 product is NOT that reference in general (53-bit v times a multi-bit a rounds)
    rows = np.array([1, n - 1])
    assert np.array_equal(lat.project_exact(a, v, rows)[0], p[rows])


def test_split26_is_exact_and_certifies_itself():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.standard_normal(1000) * 10.0 ** rng.integers(-40, 5, 1000), [0.0, 1.0, -2.0 ** -30, 1.0 - 2.0 ** -53,
                                                                                            2.0 ** 26 + 1, 3.0 * 2.0 ** -27 + 2.0 ** -80]])
    hi, lo = lat.split26(x)
    for xv, h, l in zip(x, hi, lo):
        assert Fraction(float(h)) + Fraction(float(l)) == Fraction(float(xv))
        for part in (h, l):
            num = abs(Fraction(float(part)).numerator)
            assert num.bit_length() <= 26 or num & (num - 1) == 0
    with pytest.raises(AssertionError):
        lat.split26(np.array([1e-300]))


# ----------------------------------------------------------------------------------------------- assert_projection
def _pairwise(t):
    while t.shape[-1] > 1:
        if t.shape[-1] % 2:
            t = np.concatenate([t[..., :-2], t[..., -2:-1] + t[..., -1:]], axis=-1)
        t = t[..., 0::2] + t[..., 1::2]
    return t[..., 0]


def _ordered(a, v, order):
    """A V with every element's k-sum taken sequentially in fp64 in the given order"""
    p = np.zeros((a.shape[0], v.shape[1]))
    for t in order:
        p = p + a[:, t][:, None] * v[t][None, :]
    return p


@pytest.mark.parametrize("n,k,m", [(70, 100, 20), (40, 260, 33), (33, 17, 8), (65, 1, 1), (50, 128, 128)])
def test_checker_passes_every_fp64_evaluation(n, k, m):
    a, v = _case(n, k, m)
    worst = {}
    worst["blas"] = lat.assert_projection(a @ v, a, v)
    worst["forward"] = lat.assert_projection(_ordered(a, v, range(k)), a, v)
    worst["reversed"] = lat.assert_projection(_ordered(a, v, range(k - 1, -1, -1)), a, v)
    worst["pairwise"] = lat.assert_projection(_pairwise(a[:, None, :] * v.T[None, :, :]), a, v)
    assert lat.assert_projection(lat.project_exact(a, v)[0], a, v) == 0.0
    assert lat.assert_projection_rest(a @ v, a, v, np.arange(5)) <= 1.0
    assert max(worst.values()) < 0.5, worst     # a K-term fp64 sum sits far inside its worst-case bound


@pytest.mark.parametrize("n,k,m", [(70, 100, 20), (40, 260, 33), (33, 17, 8)])
def test_checker_catches_the_errors_it_is_for(n, k, m):
    a, v = _case(n, k, m)
    good = a @ v
    lat.assert_projection(good, a, v)
    # (i) the product accumulated in fp32
    p32 = np.zeros((n, m), dtype=np.float32)
    for t in range(k):
        p32 = p32 + (a[:, t][:, None] * v[t][None, :]).astype(np.float32)
    with pytest.raises(AssertionError, match="times the bound"):
        lat.assert_projection(p32.astype(np.float64), a, v)
    # (ii) ONE element of A rounded through float16 and back (2049 -> 2048: a once-rounded operand)
    i, t = n // 2, k // 3
    a2 = a.copy()
    a2[i, t] = 2049.0
    assert float(np.float16(a2[i, t])) != a2[i, t]
    bad = a2 @ v
    a16 = a2.copy()
    a16[i, t] = float(np.float16(a2[i, t]))
    with pytest.raises(AssertionError, match="row % 64 = " + str(i % 64) + ","):
        lat.assert_projection(a16 @ v, a2, v)
    lat.assert_projection(bad, a2, v)
    # (iii) one k-term dropped where |v| >= 1e-6
    j = m - 1
    t = int(np.argmin(np.where(np.abs(v[:, j]) >= 1e-6, np.abs(v[:, j]), np.inf)))
    ii = int(np.argmax(np.abs(a[:, t])))
    assert abs(v[t, j]) >= 1e-6 and a[ii, t] != 0
    p = good.copy()
    p[ii, j] -= a[ii, t] * v[t, j]
    with pytest.raises(AssertionError, match="column % 8 = " + str(j % 8) + r"\]"):
        lat.assert_projection(p, a, v)
    # (iv) one element shifted by 64 ulp of |P|: 128 u |P|, against a bound of K u S with S = sum |a||v| >= |P| -- outside the bound
    # (and caught) while K S / |P| < 128, i.e. at K = 17 here; at K >= 100 such a shift is a legitimate fp64 result of SOME
    # summation order and no sound test can reject it.  There the smallest shift that must be caught is held instead:
    # twice the element's bound (the unshifted error is below once the bound).
    big = np.unravel_index(int(np.argmax(np.abs(good))), good.shape)
    bound = lat.projection_bound(lat.project_exact(a, v, [big[0]])[1], k)[0, big[1]]
    shift = 64.0 * np.spacing(abs(good[big]))
    if k * 1.6 < 128:
        assert shift > 2.0 * bound
    p = good.copy()
    p[big] += max(shift, 2.0 * bound)
    with pytest.raises(AssertionError):
        lat.assert_projection(p, a, v)
    # and the same shift in a row outside the exactly checked sample is caught by the 2x leg
    with pytest.raises(AssertionError, match="TWICE"):
        lat.assert_projection_rest(p, a, v, np.setdiff1d(np.arange(n), [big[0]]))


def test_exact_rows_cover_the_edges():
    for n in (100003, 20001):
        r = lat.exact_rows(n, 1)
        assert len(r) >= 4096 and set(range(192)) <= set(r) and set(range(n - 192, n)) <= set(r)
        assert set(range(n - n % 64, n)) <= set(r) and r.max() == n - 1 and len(np.unique(r)) == len(r)
    assert np.array_equal(lat.exact_rows(4097, 1), np.arange(4097))


# ----------------------------------------------------------------------------------------------- the ladder
def _squeeze(text):
    return re.sub(r"\s+", "", text)


def test_ladder_text_still_what_the_helper_restates():
    """finish_v_reference / finish_eig_top / wide_reference / refine_reference restate these statements of csrc/capi.hip;
    a change of the ladder must fail here and not as a mystery on the GPU"""
    src = _squeeze(open(os.path.join(ROOT, "subspaceinference.jl_amd", "csrc", "capi.hip")).read())

    def body(start, end):
        i = src.index(_squeeze(start))
        return src[i:src.index(_squeeze(end), i)]

    top = body("static int32_t top_eigen(", "static int32_t fetch_G(")
    for stmt in ("if (sym_eig_top((int)K, G, (int)M, wtop.data(), Vtop.data()) != 0) {",
                 "erc = sym_eig((int)K, G, lam.data());",
                 "wtop[(size_t)m] = lam[(size_t)(K - 1 - m)];",
                 "std::copy(G + (size_t)(K - 1 - m) * K, G + (size_t)(K - m) * K, Vtop.data() + (size_t)m * K);"):
        assert _squeeze(stmt) in top, stmt
    refine = body("int32_t si_construct_refine(si_ctx* ctx) {", "static int32_t alloc_P(")
    for stmt in ("const int erc = sym_eig((int)K, G, lam.data());",
                 "std::copy(G + (size_t)(K - 1 - j) * K, G + (size_t)(K - j) * K, ctx->vfull.data() + (size_t)j * K);",
                 "launch_project(ctx->stream, ctx->d_A, ctx->ldA, N, K, ctx->d_V, (int32_t)K, Kpad, ctx->d_B,",
                 "launch_gram(ctx->stream, ctx->d_B, ctx->ldA, N, K, ctx->d_Gpart, ctx->d_G, ctx->num_cu, ctx);"):
        assert _squeeze(stmt) in refine, stmt
    wide = body("static int32_t finish_wide(", "int32_t si_construct_finish(")
    for stmt in ("if ((rc = top_eigen(ctx, N, M, wtop, U)) != SI_OK) return rc;",
                 "ctx->svals[(size_t)m] = std::sqrt(wtop[(size_t)m]);",
                 "if (std::fabs(v[k]) > std::fabs(v[imax])) imax = k;",
                 "const double f = (v[imax] < 0.0 ? -1.0 : 1.0) * ctx->svals[(size_t)m];",
                 "Ph[(size_t)m * N + n] = f * U[(size_t)m * N + n];"):
        assert _squeeze(stmt) in wide, stmt
    fin = body("int32_t si_construct_finish(si_ctx* ctx, int32_t M,", "int32_t si_construct_get_result(")
    for stmt in ("if (wtop[(size_t)M - 1] > SI_GRAM_ROUTE_MIN * wtop[0]) {",
                 "for (int m = 0; m < M; ++m) ctx->svals[(size_t)m] = std::sqrt(wtop[(size_t)m]);",
                 "const int jrc = jacobi_eig_psd((int)K, ctx->h_pin, lam2.data(), W.data());",
                 "for (int m = 0; m < M; ++m) ctx->svals[(size_t)m] = std::sqrt(lam2[(size_t)m]);",
                 "std::copy(W.begin(), W.begin() + (size_t)K * M, vcols.begin());",
                 "for (int64_t k = 0; k < K; ++k) dst[k] += vj[k] * wjm;",
                 "const double* vs = (vsign.empty() ? vcols.data() : vsign.data()) + (size_t)m * K;",
                 "if (std::fabs(vs[k]) > std::fabs(vs[imax])) imax = k;",
                 "const double sgn = vs[imax] < 0.0 ? -1.0 : 1.0;",
                 "for (int64_t k = 0; k < K; ++k) V[(size_t)k * Mpad + m] = sgn * v[k];"):
        assert _squeeze(stmt) in fin, stmt
    assert "staticconstexprdoubleSI_GRAM_ROUTE_MIN=1e-9;" in src


# which branch of top_eigen every case of FINISH_F64 / FINISH_F32 takes on its lattice G: the fast route is tried for K >= 8 and
# 3 M <= K (csrc/eig.cpp) and may still decline when its own verification fails -- recorded: it never does on these cases
FAST_ROUTE = {(n, k, m) for n, k, m in ALL_AV if 3 * m <= k and k >= 8}


@pytest.mark.parametrize("n,k,m", sorted(set(ALL_AV)))
def test_ladder_on_every_lattice_case(si, n, k, m):
    a = lat.finish_problem(n, k)[3]
    g = lat.gram_exact_f64(a)
    w, v, branch = lat.finish_v_reference(si, g, m, with_branch=True)
    w2, v2, branch2 = lat.finish_v_reference(si, g.copy(), m, with_branch=True)
    assert branch == branch2 and np.array_equal(w, w2) and np.array_equal(v, v2)        # deterministic call to call
    print("(N, K, M) = (%d, %d, %d): %s" % (n, k, m, branch))
    assert (branch == "fast") == ((n, k, m) in FAST_ROUTE)
    assert np.all(np.diff(w) <= 0) and w[-1] > 1e-9 * w[0] > 0                          # the Gram route keeps the case
    assert np.abs(v.T @ g @ v - np.diag(w)).max() <= k * np.finfo(np.float64).eps * w[0]
    assert not any(lat.argmax_tie(v)), "a tie in argmax |v|: the sign rule would depend on the scan order"
    for j in range(m):
        assert v[int(np.argmax(np.abs(v[:, j]))), j] > 0


def test_ladder_fallback_takes_the_top_columns_reversed(si):
    """the fallback restated once more from the full solver's documented output (ascending eigenvalues, eigenvectors in columns)"""
    a = lat.finish_problem(65, 47)[3]
    g = lat.gram_exact_f64(a)
    assert si.host_sym_eig_top(g, 40) is None
    lam, vec = si.host_sym_eig(g)
    w, v, branch = lat.finish_eig_top(si, g, 40)
    assert branch == "fallback" and np.array_equal(w, lam[::-1][:40]) and np.array_equal(v, vec[:, ::-1][:, :40])
    assert np.all(np.diff(lam) >= 0)
    assert lat.finish_eig_top(si, g, 3)[2] == "fast"   # 3 M <= K: the other branch, on the same matrix


# ----------------------------------------------------------------------------------------------- injected Gram matrices
@pytest.mark.parametrize("n,k,m,f32,kernel,exact", lat.FINISH_DIAG)
def test_diag_gram_table(si, n, k, m, f32, kernel, exact):
    g, d, perm = lat.diag_gram(k, seed=k + m)
    assert len(set(d)) == k and np.all(d > 0) and np.array_equal(np.diag(g), d)
    w, v, branch = lat.finish_v_reference(si, g, m, with_branch=True)
    assert np.array_equal(w, d[perm[:m]])              # eigenvalues returned exactly
    got_exact, dust = lat.unit_columns(v, perm)
    assert dust is not None, "a column is not a unit vector (+ dust)"
    print("diag (K, M) = (%d, %d): %s, dust %.3g" % (k, m, branch, dust))
    assert got_exact == exact == (branch == "fallback")
    # dust: K max|A| dust stays below half an ulp of 1 by a wide margin, so a nonzero integer A[i, perm[m]] is reproduced exactly
    a_max = float(np.abs(lat.finish_problem(n, k)[3]).max())
    assert k * a_max * dust < 2.0 ** -100


@pytest.mark.parametrize("n,k,m,f32,kernel", lat.FINISH_PAIRED)
def test_paired_gram_is_near_degenerate(si, n, k, m, f32, kernel):
    g = lat.paired_gram(k, seed=k + m)
    w, v = lat.finish_v_reference(si, g, m)
    assert np.array_equal(g, g.T) and np.abs(v.T @ g @ v - np.diag(w)).max() <= k * np.finfo(np.float64).eps * w[0]
    gaps = np.abs(np.diff(w)) / w[:-1]
    assert gaps.min() <= 2.0 ** -28 and w[-1] > 1e-9 * w[0]
    assert np.allclose(np.sort(np.abs(v), axis=0)[-2:], np.sqrt(0.5), rtol=0, atol=1e-6) or k % 2   # (1, +-1) / sqrt 2


# ----------------------------------------------------------------------------------------------- K > N
def test_wide_sign_margins(si):
    """the sign of a finish_wide column is read from the device's fp64 A'u: pinned where the exact winner beats the runner-up by
    more than both bounds.  Condition of the GPU leg: at most 1 column in 20 over the whole list is not pinned."""
    total = unpinned = 0
    for n, k, m, _ in lat.FINISH_WIDE:
        a = lat.finish_problem(n, k)[3]
        assert k > n >= m
        s, p_ref, pinned = lat.wide_reference(si, a, m)
        assert s[-1] ** 2 > 1e-9 * s[0] ** 2 > 0           # finish_wide keeps the case (no fall-through to the K x K route)
        assert np.allclose(np.sum(p_ref * p_ref, axis=0), s * s, rtol=1e-12)
        total += m
        unpinned += m - sum(pinned)
    print("finish_wide sign check: %d of %d columns not pinned" % (unpinned, total))
    assert 20 * unpinned <= total


@pytest.mark.parametrize("n,k,m,kernel", lat.FINISH_REFINE)
def test_refine_reference_on_the_host(si, n, k, m, kernel):
    """the two-stage reference, replayed with NumPy's fp64 products in the device's place: both must sit inside the composed bounds"""
    a = lat.finish_problem(n, k)[3]
    g = lat.gram_exact_f64(a)
    v_full, b_ref, d = lat.refine_reference(si, a, g)
    b_np = a @ v_full
    assert np.all(np.abs(b_np - b_ref) <= d)
    g2_np = b_np.T @ b_np
    g2_ref, _ = lat.project_exact(b_ref.T, b_ref)
    bound2 = lat.gram2_bound(b_ref, d)
    assert np.all(np.abs(g2_np - g2_ref) <= bound2)
    assert np.abs(g2_np - g2_ref).max() / bound2.max() < 0.5
    s, wm, ok = lat.second_stage_reference(si, v_full, g2_np, m)
    assert all(ok), "a second-stage sign is not pinned for this seed"
    lat.assert_projection(b_np @ wm, b_ref, wm, extra=d @ np.abs(wm))
    assert np.allclose(s, np.sqrt(np.sort(np.linalg.eigvalsh(g))[::-1][:m]), rtol=1e-9)
