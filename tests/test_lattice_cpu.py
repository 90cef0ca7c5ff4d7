"""The lattice problems of tests/lattice.py, checked without a GPU: the oracle equals a plain restatement in exact rationals
(no NumPy arithmetic) on them, every certificate holds, and the comparison helpers fail on the smallest error the GPU tests
are meant to catch -- one lattice unit in one element."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import subspace_oracle as so
from tests import lattice as lat

R, I = so.ACT_RELU, so.ACT_IDENTITY

SMALL_DENSE = [
    ([3, 5, 4, 2], [R, R, I], 7, 3),
    ([4, 6, 1], [I, I], 5, 2),
    ([2, 9, 7, 5, 3], [R, R, R, I], 4, 4),
]


@pytest.mark.parametrize("dims,acts,b,m", SMALL_DENSE)
def test_oracle_forward_equals_exact_rationals(dims, acts, b, m):
    pb = lat.dense(dims, acts, b, m=m, ncols=3, seed=sum(dims), z_nnz=2)
    for c in range(3):
        w = pb.w_swa + pb.p @ pb.z[:, c]
        exact = lat.dense_forward_fraction(pb.table, w, pb.x)
        assert all(Fraction(float(pb.yhat[c][i, t])) == exact[i][t] for i in range(dims[-1]) for t in range(b))
        assert np.array_equal(so.forward(pb.table, w, pb.x), pb.yhat[c])
    # the targets: a null residual for column 0 and an integer one of exactly the recorded SSE
    assert pb.sse["null"][0] == 0.0
    r = (pb.y1 - pb.yhat[0]) / pb.unit
    assert np.array_equal(r, np.round(r)) and pb.sse["r"][0] == float(sum(int(v) ** 2 for v in r.ravel())) * pb.unit ** 2


@pytest.mark.parametrize("dims,acts,b,m", SMALL_DENSE)
def test_oracle_gradient_equals_exact_rationals(dims, acts, b, m):
    pb = lat.dense(dims, acts, b, m=m, ncols=2, seed=sum(dims) + 1, z_nnz=2)
    for c, y in ((0, pb.y1), (1, pb.y0)):
        lp, dz, gw = lat.logdensity_grad_certified(pb, c, y)
        w = pb.w_swa + pb.p @ pb.z[:, c]
        exact = lat.dense_gw_fraction(pb.table, w, pb.x, y, pb.sigma)
        assert [Fraction(float(v)) for v in gw] == exact
        pz = [sum(Fraction(float(pb.p[i, j])) * exact[i] for i in range(pb.n)) for j in range(m)]
        assert [Fraction(float(v)) for v in dz] == pz


def test_no_pre_activation_is_zero():
    """the bias fractions keep every pre-activation off 0 (relu'(0) never arises)"""
    pb = lat.dense([5, 30, 20, 1], [R, R, I], 50, m=3, ncols=4, seed=3, z_nnz=2)
    for c in range(4):
        w = pb.w_swa + pb.p @ pb.z[:, c]
        h = pb.x
        for fin, fout, act, w_off, b_off in pb.table:
            pre = w[w_off:w_off + fin * fout].reshape((fout, fin), order="F") @ h + w[b_off:b_off + fout][:, None]
            assert np.all(pre != 0)
            h = np.maximum(pre, 0) if act == R else pre


def test_oracle_conv_forward_equals_brute_force():
    spec = [("conv", (3, 2), 3, R, (2, 1), (1, 0), (1, 2)), ("maxpool", (2, 2)), ("flatten",), ("dense", 2, I)]
    pb = lat.conv(spec, (7, 8, 2), 3, m=2, ncols=2, seed=5)
    row = pb.table[0]
    _, (kw, kh, cin, cout), (wi, hi), stride, pad, dil, act, w_off, b_off = row
    for c in range(2):
        w = pb.w_swa + pb.p @ pb.z[:, c]
        w4 = w[w_off:w_off + kw * kh * cin * cout].reshape((kw, kh, cin, cout), order="F")
        x4 = pb.x.reshape((wi, hi, cin, 3), order="F")
        y_int = lat.conv_forward_int(x4, w4, w[b_off:b_off + cout], stride, pad, dil)
        y_or = so.conv_forward(x4, w4, w[b_off:b_off + cout], stride, pad, dil)
        assert all(Fraction(float(a)) == b for a, b in zip(y_or.ravel(), y_int.ravel()))


@pytest.mark.parametrize("ns", [list(range(9)), [0, 0, 1, 1, 2, 2, 3, 3], [0, 3, 3, 7, 8, 20]])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_construction_snapshots_exact(ns, dtype):
    k = len(ns)
    snaps, nsf, means, a = lat.snapshots(37, k, seed=len(ns), ns=ns, dtype=dtype)
    w_ref, a_ref = so.construct_stream(snaps, nsf)
    assert np.array_equal(a_ref, a) and np.array_equal(w_ref, means[-1])
    # the integer restatement: column j = n_j (m_j - m_{j-1}) with m_{-1} = 0
    prev = np.zeros(37, dtype=np.int64)
    for j, nj in enumerate(ns):
        mj = means[j].astype(np.int64)
        assert np.array_equal(a[:, j].astype(np.int64), nj * (mj - prev))
        prev = mj
    g = lat.gram_exact(a)
    assert np.array_equal(g.astype(np.float64), a.T @ a)


# -------------------------------------------------------------------- the certificates the GPU file relies on
def _gpu_dense_problems():
    from tests import test_gpu_lattice as g
    return [(name, builder) for name, builder in g.DENSE_PROBLEMS.items()]


@pytest.mark.parametrize("name", [n for n, _ in _gpu_dense_problems()])
def test_gpu_dense_cases_are_certified_and_detect_one_unit(name):
    from tests import test_gpu_lattice as g
    pb = g.DENSE_PROBLEMS[name]()   # the builder asserts the forward and SSE certificates
    assert pb.bound_bits < (24 if pb.f32 else 53)
    for tag in ("null", "r"):
        assert lat.detect_margin(pb, tag) > 1e3, (name, tag)
    _checker_sees_one_unit(pb)


@pytest.mark.parametrize("case", range(len(__import__("tests.test_gpu_lattice", fromlist=["CONV_CASES"]).CONV_CASES)))
@pytest.mark.parametrize("f32", [False, True])
def test_gpu_conv_cases_are_certified(case, f32):
    from tests import test_gpu_lattice as g
    pb = g.conv_problem(case, f32=f32)   # forward and SSE certificates
    assert lat.detect_margin(pb, "r") > 1e3
    _checker_sees_one_unit(pb)
    if not f32:   # what the GPU file compares of the fp64 conv gradient
        lat.logdensity_grad_certified(pb, 0, pb.y1)
        lat.pool_ties_are_exact(pb, 0)


def _checker_sees_one_unit(pb):
    """assert_exact fails on a copy perturbed by one unit in one (the smallest) element; an lp shifted by one unit's
    worth of SSE fails assert_lp"""
    yh = pb.yhat[0]
    k = np.unravel_index(np.argmin(np.abs(yh)), yh.shape)
    bad = yh.copy()
    bad[k] += pb.unit
    lat.assert_exact(yh, yh)
    with pytest.raises(AssertionError):
        lat.assert_exact(bad, yh)
    for tag, y in (("null", pb.y0), ("r", pb.y1)):
        lp = lat.lp_exact(pb.sse[tag][0], pb.d, pb.sigma)
        lp_bad = lat.lp_exact(lat.sse_certified(bad, y, pb.unit), pb.d, pb.sigma)
        lat.assert_lp(lp, lp)
        with pytest.raises(AssertionError):
            lat.assert_lp(lp_bad, lp)
        assert abs(lp_bad - lp) >= lat.lp_one_unit_shift(pb.unit, pb.sigma) * (1 - 1e-12) or tag == "r"


def test_gram_cases_are_certified():
    """the GPU file's Gram problems themselves: gram_exact asserts every entry of A'A below 2^53, and A is an integer matrix"""
    from tests import test_gpu_lattice as g
    for n, k in g.GRAM_CASES:
        snaps, ns, a, g_ref = g.gram_problem(n, k)
        assert a.shape == (n, k) and np.array_equal(a, np.round(a)) and np.abs(g_ref).max() < 2 ** 53
        for dtype in (np.float64, np.float32):
            assert all(np.array_equal(s.astype(dtype).astype(np.float64), s) for s in snaps)


def test_certificate_refuses_a_problem_that_would_round():
    with pytest.raises(AssertionError):
        lat.dense([64, 512, 512, 512, 1], [R, R, R, I], 50, m=4, f32=True, seed=1, w_range=3, p_nnz=2, z_nnz=4, zmax=2)
    with pytest.raises(AssertionError):
        lat.dense([4, 8, 1], [so.ACT_TANH, I], 5)


def test_gpu_gradient_cases_are_certified():
    """the reverse sweeps the GPU file compares bit for bit: every partial sum within its certificate"""
    from tests import test_gpu_lattice as g
    for name in g.GRAD_CASES:
        pb = g.DENSE_PROBLEMS[name]()
        lat.logdensity_grad_certified(pb, 0, pb.y1)
        lat.logdensity_grad_certified(pb, min(1, pb.z.shape[1] - 1), pb.y0)
    for dims, nbt in g.TRAIN_CASES:
        for f32 in (False, True):
            table, n, w, x, y = g._train_problem(dims, nbt, f32, seed=sum(dims))
            assert lat.f32_exact(w) and lat.f32_exact(x) and lat.f32_exact(y)
            lat.mse_grad_exact(table, w, x, y, nbt, lat.F32_LIMIT if f32 else lat.F64_LIMIT)
