"""Lattice problems: model, data and subspace whose every operand is a small dyadic number, chosen so that no operation of
the forward pass, the reverse sweep, the SSE or the construction rounds -- whatever the summation order, tile split or
split-K.  On such a problem a kernel's result must equal the exact result BIT FOR BIT: a dropped, doubled or misplaced term
shows in any element, however small.  Each builder carries its exactness certificate (asserted when the problem is built):
every partial sum, measured in the unit of its grid, stays below 2^53 (fp64) or 2^24 (cases run with compute_dtype = SI_F32).

The scheme (a helper module for the tests, not a conftest):
  * X: integers.  Dense / Conv weights: integers (W_swa integer, P entries in {0, +-1, +-2} with no all-zero row, z integer).
  * the bias of the l-th parametrised layer (l = 0, 1, ...) is an integer plus +-2^-(l+1): the layer's output lies on the grid
    2^-(l+1) and no pre-activation is ever exactly 0, so relu'(0) never arises.  (That convention is not pinned here: the
    oracle uses h > 0, the reference's gradient backend may differ; the lattice tests stay clear of it.)
  * only identity and relu are exact; the other activations stay with the tolerance tests.
  * sigma_m is a power of two (2^-4 by default) so the SSE's 1 / sigma^2 scale is exact and a one-unit error is amplified.
"""
import math
from fractions import Fraction

import numpy as np

from oracle import subspace_oracle as so

F64_LIMIT, F32_LIMIT = 2.0 ** 53, 2.0 ** 24
SIGMA_M = 2.0 ** -4
EXACT_ACTS = (so.ACT_IDENTITY, so.ACT_RELU)


class Problem:
    """a plain record; fields are set by the builders below"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


# --------------------------------------------------------------------------- parameters
def _param_rows(table):
    """indices of the table rows that own weights (Dense or Conv), in order"""
    return [i for i, r in enumerate(table) if r[0] not in ("maxpool", "flatten")]


def _row_slices(row):
    """(weight slice, bias slice) of a Dense or Conv row in the flat vector"""
    if row[0] == "conv":
        (kw, kh, cin, cout), w_off, b_off = row[1], row[7], row[8]
        return slice(w_off, w_off + kw * kh * cin * cout), slice(b_off, b_off + cout)
    fin, fout, _, w_off, b_off = row
    return slice(w_off, w_off + fin * fout), slice(b_off, b_off + fout)


def _acts(table):
    return [r[6] if r[0] == "conv" else r[2] for r in (table[i] for i in _param_rows(table))]


def lattice_swa(table, n, rng, w_range=2, density=1.0, nonzero=False):
    """W_swa: integer weights in [-w_range, w_range] (a fraction `density` of them nonzero; all nonzero when `nonzero`),
    biases of the l-th parametrised layer = integer +- 2^-(l+1)"""
    w = np.zeros(n)
    for l, i in enumerate(_param_rows(table)):
        ws, bs = _row_slices(table[i])
        k = ws.stop - ws.start
        if nonzero:
            v = rng.integers(1, w_range + 1, k) * rng.choice([-1, 1], k)
        else:
            v = rng.integers(-w_range, w_range + 1, k) * (rng.random(k) < density)
        w[ws] = v
        nb = bs.stop - bs.start
        w[bs] = rng.integers(-1, 2, nb) + rng.choice([-1.0, 1.0], nb) * 2.0 ** -(l + 1)
    return w


def lattice_p(n, m, rng, nnz=1):
    """N x M, entries in {0, +-1, +-2}, exactly `nnz` nonzeros in every row (no row is all zero)"""
    p = np.zeros((n, m))
    for j in range(min(nnz, m)):
        cols = (rng.integers(0, m, n) + j) % m if j == 0 else (cols + 1) % m   # distinct columns per row
        p[np.arange(n), cols] = rng.choice([-2.0, -1.0, 1.0, 2.0], n)
    return np.asfortranarray(p)


def lattice_z(m, ncols, rng, nnz=1, zmax=1):
    """M x C integer z: `nnz` nonzero entries in [-zmax, zmax] per column, at random rows"""
    z = np.zeros((m, ncols))
    for c in range(ncols):
        idx = rng.choice(m, min(nnz, m), replace=False)
        z[idx, c] = rng.integers(1, zmax + 1, idx.size) * rng.choice([-1.0, 1.0], idx.size)
    return np.asfortranarray(z)


# --------------------------------------------------------------------------- certificate
def forward_certified(table, wflat, x, limit):
    """the oracle's forward, each parametrised layer checked: its output lies on the grid 2^-(l+1), and the bound
    sum |W| |a| + |b| of every output element, in that unit, stays below `limit`.  Returns (yhat, hs, bound_bits) --
    bound_bits the largest log2 of a bound in units (so the margin is visible)."""
    hs, h, l, worst = [x], x, 0, 0.0
    pr = set(_param_rows(table))
    for i, row in enumerate(table):
        nh = so._layer_forward(row, wflat, h)
        if i in pr:
            if row[0] == "conv":
                arow = row[:6] + (so.ACT_IDENTITY,) + row[7:]
            else:
                arow = row[:2] + (so.ACT_IDENTITY,) + row[3:]
            bound = so._layer_forward(arow, np.abs(wflat), np.abs(h))
            scale = 2.0 ** (l + 1)
            b_units = float(np.max(bound)) * scale if bound.size else 0.0
            assert b_units < limit, "layer %d: bound %.3g units exceeds the certificate's %.3g" % (l, b_units, limit)
            assert np.all(np.mod(nh * scale, 1.0) == 0), "layer %d output off its grid 2^-%d" % (l, l + 1)
            worst = max(worst, b_units)
            l += 1
        hs.append(nh)
        h = nh
    return h, hs, math.log2(worst) if worst > 0 else 0.0


def out_unit(table):
    return 2.0 ** -len(_param_rows(table))


def sse_certified(yhat, y, unit, limit=F64_LIMIT):
    """exact SSE of y - yhat; asserts every square and every partial sum of squares is an integer below `limit` in unit^2"""
    r = (y - yhat).reshape(-1) / unit
    assert np.all(np.mod(r, 1.0) == 0) and np.max(np.abs(r), initial=0.0) < 2.0 ** 26
    s_units = float(np.dot(r, r))
    assert s_units < limit
    return s_units * unit * unit


def lp_exact(sse, d, sigma=SIGMA_M):
    return so.lp_from_sse(sse, d, sigma)


def lp_tol(lp):
    """the lp comparison: only the final combine rounds -- 4 ulp of |lp|"""
    return 4.0 * np.spacing(abs(lp))


def lp_one_unit_shift(unit, sigma=SIGMA_M):
    """the smallest lp change one lattice unit of error in one output element causes against a null residual"""
    return unit * unit / (2.0 * sigma * sigma)


def assert_lp(lp, lp_ref):
    assert abs(lp - lp_ref) <= lp_tol(lp_ref), "lp %r vs exact %r (%.3g ulp)" % (lp, lp_ref, abs(lp - lp_ref) / np.spacing(abs(lp_ref)))


def assert_exact(a, ref, what=""):
    a, ref = np.asarray(a), np.asarray(ref)
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    if not np.array_equal(a, ref):
        bad = np.argwhere(a != ref)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d elements differ; first at %s: %r vs exact %r"
                             % (what, len(bad), a.size, i, a[i], ref[i]))


def f32_exact(a):
    a = np.asarray(a, dtype=np.float64)
    return bool(np.all(a.astype(np.float32).astype(np.float64) == a))


# --------------------------------------------------------------------------- Dense / Conv problems
def dense(dims, acts, b, m=4, ncols=1, seed=0, f32=False, w_range=2, w_density=1.0, p_nnz=1, z_nnz=1, zmax=1, x_range=2,
          nonzero_swa=False, r_max=2, sigma=SIGMA_M):
    table, n = so.layer_table(dims, acts)
    return _build(table, n, dims[0], b, m, ncols, seed, f32, w_range, w_density, p_nnz, z_nnz, zmax, x_range, nonzero_swa, r_max,
                  sigma)


def conv(spec, whc, b, m=3, ncols=1, seed=0, f32=False, **kw):
    table, n = so.conv_table(spec, whc)
    return _build(table, n, whc[0] * whc[1] * whc[2], b, m, ncols, seed, f32, kw.get("w_range", 1), kw.get("w_density", 1.0),
                  kw.get("p_nnz", 1), kw.get("z_nnz", 1), kw.get("zmax", 1), kw.get("x_range", 2), False, kw.get("r_max", 2),
                  kw.get("sigma", SIGMA_M))


def _build(table, n, in_dim, b, m, ncols, seed, f32, w_range, w_density, p_nnz, z_nnz, zmax, x_range, nonzero_swa, r_max, sigma):
    for a in _acts(table):
        assert a in EXACT_ACTS, "only identity and relu are exact"
    rng = np.random.default_rng(seed)
    limit = F32_LIMIT if f32 else F64_LIMIT
    x = np.asfortranarray(rng.integers(-x_range, x_range + 1, (in_dim, b)).astype(np.float64))
    w_swa = lattice_swa(table, n, rng, w_range, w_density, nonzero_swa)
    p = lattice_p(n, m, rng, p_nnz)
    z = lattice_z(m, ncols, rng, z_nnz, zmax)
    unit = out_unit(table)
    yhats, bits = [], 0.0
    for c in range(ncols):
        w = w_swa + p @ z[:, c]
        assert np.all(np.mod(w * 2.0 ** len(_param_rows(table)), 1.0) == 0)
        yh, _, bb = forward_certified(table, w, x, limit)
        if f32:
            assert f32_exact(w) and f32_exact(x), "fp32 operand not representable"
        yhats.append(yh)
        bits = max(bits, bb)
    y0 = np.asfortranarray(yhats[0])                                              # the null residual of column 0
    y1 = np.asfortranarray(yhats[0] + rng.integers(-r_max, r_max + 1, yhats[0].shape) * unit)   # small integer residuals
    d = y0.size
    sse = {}
    for tag, y in (("null", y0), ("r", y1)):
        s = []
        for c in range(ncols):
            try:
                s.append(sse_certified(yhats[c], y, unit))
            except AssertionError:
                s.append(None)   # this column's SSE would round: its lp is not compared exactly
        sse[tag] = s
    assert sse["null"][0] == 0.0 and sse["r"][0] is not None
    return Problem(table=table, n=n, m=m, x=x, w_swa=w_swa, p=p, z=z, yhat=yhats, y0=y0, y1=y1, sse=sse, d=d, unit=unit,
                   sigma=sigma, f32=f32, bound_bits=bits, limit=limit)


def lp_cases(pb, tag):
    """[(column, exact lp)] for the columns whose SSE is certified exact against target `tag` ("null" / "r")"""
    return [(c, lp_exact(s, pb.d, pb.sigma)) for c, s in enumerate(pb.sse[tag]) if s is not None]


def detect_margin(pb, tag):
    """how many times the one-unit lp shift exceeds the lp tolerance at column 0, the column the targets are built around
    (the other columns are held bit for bit through their forward outputs; their lp only re-checks the stacking).  Against
    a residual r the one-unit change of r^2 is |2 r u +- u^2| >= u^2 as well (r is a multiple of u)."""
    shift = lp_one_unit_shift(pb.unit, pb.sigma)
    return shift / lp_tol(lp_exact(pb.sse[tag][0], pb.d, pb.sigma))


# --------------------------------------------------------------------------- gradients
def logdensity_grad_certified(pb, c, y, limit=None):
    """the oracle's (lp, dz, gw) at column c against target y, with the reverse sweep certified exact: every partial sum of
    the abs-value sweep (|g|, |W|, |h|), in the finest unit the sweep reaches, stays below the limit"""
    limit = pb.limit if limit is None else limit
    w = pb.w_swa + pb.p @ pb.z[:, c]
    lp, dz, gw = so.logdensity_grad(pb.table, pb.w_swa, pb.p, pb.x, y, pb.sigma, pb.z[:, c])
    # (P' g is formed in fp64 on both paths: the SI_F32 reverse sweep hands its fp32 gradient to an fp64 projection)
    _certify_backward(pb.table, w, pb.x, (y - pb.yhat[c]) / pb.sigma ** 2, pb.unit / pb.sigma ** 2, limit, p=pb.p, p_limit=F64_LIMIT)
    return lp, dz, gw


def _certify_backward(table, w, x, g_last, g_unit, limit, p=None, p_limit=None):
    hs = [x]
    for row in table:
        hs.append(so._layer_forward(row, w, hs[-1]))
    L = len(_param_rows(table))
    # finest unit: delta carries g_unit through integer weights; gw of layer l multiplies by the grid of its input 2^-l
    fine = g_unit * 2.0 ** -(L - 1)
    gb = np.zeros_like(w)
    g = np.abs(g_last)
    aw = np.abs(w)
    for i in range(len(table) - 1, -1, -1):
        # (a MaxPool row routes each window's |g| to the input its real values pick: it is given the real input)
        h_in = hs[i] if table[i][0] == "maxpool" else np.abs(hs[i])
        g = np.abs(so._layer_backward(table[i], aw, h_in, hs[i + 1], g, gb))
        assert float(np.max(g, initial=0.0)) / fine < limit
    assert float(np.max(gb, initial=0.0)) / fine < limit, "gradient bound %.3g units" % (np.max(gb) / fine)
    if p is not None:
        assert float(np.max(np.abs(p).T @ gb, initial=0.0)) / fine < (limit if p_limit is None else p_limit)
    return gb


def pool_ties_are_exact(pb, c):
    """the oracle's MaxPool gradient picks each window's first input `isapprox` (rtol sqrt(eps)) to the maximum; on the lattice
    that is plain equality when rtol * max|input| stays below the input's grid unit (values one unit apart never pass).
    Asserts it for every MaxPool row at column c, so tied maxima are resolved by the exact first-maximum rule."""
    w = pb.w_swa + pb.p @ pb.z[:, c]
    h, l = pb.x, 0
    rtol = math.sqrt(np.finfo(np.float64).eps)
    for row in pb.table:
        if row[0] == "maxpool":
            assert rtol * float(np.max(np.abs(h), initial=0.0)) < 2.0 ** -l
        elif row[0] != "flatten":
            l += 1
        h = so._layer_forward(row, w, h)


def mse_grad_exact(table, w, x, y, nb_total, limit=F64_LIMIT):
    """the training gradient of si_train_grad: d/dw of sum((f(x) - y)^2) / (out * nb_total) over the observations in x
    (the rank's share of a batch of nb_total).  out * nb_total must be a power of two so the scale is exact.
    Returns (sse, gradient), certified exact."""
    out = y.shape[0]
    scale = 2.0 / (out * nb_total)
    assert math.log2(out * nb_total).is_integer()
    hs = [x]
    for row in table:
        hs.append(so._layer_forward(row, w, hs[-1]))
    unit = out_unit(table)
    sse = sse_certified(hs[-1], y, unit, limit)
    gw = np.zeros_like(w)
    g = scale * (hs[-1] - y)
    for i in range(len(table) - 1, -1, -1):
        g = so._layer_backward(table[i], w, hs[i], hs[i + 1], g, gw)
    _certify_backward(table, w, x, scale * (hs[-1] - y), scale * unit, limit)
    return sse, gw


# --------------------------------------------------------------------------- construction snapshots
def snapshots(n, k, seed, ns=None, mmax=4, dtype=np.float64):
    """snapshots whose running mean is an integer sequence m_0, m_1, ...: w_j = (n_j + 1) m_j - n_j m_{j-1} with integer
    epoch counters n_j (so.swa_dev_push: t = n s; u = t + w; s' = u / (n + 1) = m_j, exactly).  Every deviation column
    n_j (m_j - m_{j-1}) is an integer, so A and G = A'A are exact integer matrices.  Returns (snaps, ns, means, A)."""
    rng = np.random.default_rng(seed)
    ns = list(range(k)) if ns is None else list(ns)
    assert len(ns) == k and all(float(v).is_integer() and v >= 0 for v in ns)
    prev = np.zeros(n)   # Q1: the mean starts at zero
    snaps, means, cols = [], [], []
    for nj in ns:
        mj = rng.integers(-mmax, mmax + 1, n).astype(np.float64)
        w = (nj + 1) * mj - nj * prev
        assert np.max(np.abs(w)) < (2 ** 24 if dtype == np.float32 else 2 ** 53)
        snaps.append(w.astype(dtype))
        cols.append(w - mj)
        means.append(mj)
        prev = mj
    a = np.asfortranarray(np.stack(cols, axis=1))
    return snaps, [float(v) for v in ns], means, a


def gram_exact(a):
    """A'A in int64 (the certificate: every entry below 2^53)"""
    ai = a.astype(np.int64)
    assert np.array_equal(ai.astype(np.float64), a)
    g = ai.T @ ai
    assert np.abs(ai).max(initial=0) ** 2 * a.shape[0] < 2 ** 53
    return g


# --------------------------------------------------------------------------- plain integer restatements (CPU tests)
def _fr(v):
    return Fraction(float(v))


def dense_forward_fraction(table, w, x):
    """Dense forward in exact rationals, no NumPy arithmetic: the restatement the oracle is checked against"""
    h = [[_fr(v) for v in row] for row in np.asarray(x)]
    for fin, fout, act, w_off, b_off in table:
        W = [[_fr(w[w_off + i + j * fout]) for j in range(fin)] for i in range(fout)]
        bias = [_fr(w[b_off + i]) for i in range(fout)]
        nb = len(h[0])
        out = []
        for i in range(fout):
            row = []
            for t in range(nb):
                s = bias[i] + sum(W[i][j] * h[j][t] for j in range(fin))
                row.append(max(s, Fraction(0)) if act == so.ACT_RELU else s)
            out.append(row)
        h = out
    return h


def dense_gw_fraction(table, w, x, y, sigma):
    """gradient of the Gaussian log-likelihood wrt the flat weights, in exact rationals (relu' = [pre-activation > 0];
    the lattice never puts a pre-activation at 0)"""
    hs = [[[_fr(v) for v in row] for row in np.asarray(x)]]
    pre = []
    for fin, fout, act, w_off, b_off in table:
        h = hs[-1]
        nb = len(h[0])
        zs = [[_fr(w[b_off + i]) + sum(_fr(w[w_off + i + j * fout]) * h[j][t] for j in range(fin)) for t in range(nb)]
              for i in range(fout)]
        pre.append(zs)
        hs.append([[max(v, Fraction(0)) if act == so.ACT_RELU else v for v in r] for r in zs])
    s2 = _fr(sigma) ** 2
    g = [[(_fr(y[i, t]) - hs[-1][i][t]) / s2 for t in range(len(hs[-1][0]))] for i in range(len(hs[-1]))]
    gw = [Fraction(0)] * len(w)
    for li in range(len(table) - 1, -1, -1):
        fin, fout, act, w_off, b_off = table[li]
        delta = [[g[i][t] if (act != so.ACT_RELU or pre[li][i][t] > 0) else Fraction(0) for t in range(len(g[0]))]
                 for i in range(fout)]
        h = hs[li]
        for i in range(fout):
            gw[b_off + i] = sum(delta[i])
            for j in range(fin):
                gw[w_off + i + j * fout] = sum(delta[i][t] * h[j][t] for t in range(len(h[0])))
        g = [[sum(_fr(w[w_off + i + j * fout]) * delta[i][t] for i in range(fout)) for t in range(len(h[0]))] for j in range(fin)]
    return gw


def conv_forward_int(x4, w4, b, stride, pad, dil):
    """NNlib's true convolution (kernel index reversed) by brute force over Python numbers: x4 (W, H, CIN, N),
    w4 (KW, KH, CIN, COUT)"""
    kw, kh, cin, cout = w4.shape
    wi, hi, _, nn = x4.shape
    wo, ho = so.conv_out_size(wi, kw, stride[0], pad[0], dil[0]), so.conv_out_size(hi, kh, stride[1], pad[1], dil[1])
    y = np.empty((wo, ho, cout, nn), dtype=object)
    for o in range(cout):
        for s in range(nn):
            for i in range(wo):
                for j in range(ho):
                    acc = _fr(b[o])
                    for a in range(kw):
                        for c in range(kh):
                            xi, xj = i * stride[0] - pad[0] + a * dil[0], j * stride[1] - pad[1] + c * dil[1]
                            if 0 <= xi < wi and 0 <= xj < hi:
                                for ci in range(cin):
                                    acc += _fr(x4[xi, xj, ci, s]) * _fr(w4[kw - 1 - a, kh - 1 - c, ci, o])
                    y[i, j, o, s] = acc
    return y
