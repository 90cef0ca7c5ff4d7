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


def pool_tie_count(pb, c):
    """(windows whose maximum is attained by more than one input, windows) over every MaxPool row at column c"""
    w = pb.w_swa + pb.p @ pb.z[:, c]
    h, ties, wins = pb.x, 0, 0
    for row in pb.table:
        if row[0] == "maxpool":
            _, win, ch, (wi, hi), stride = row
            x4 = h.reshape((wi, hi, ch, -1), order="F")
            y = so.maxpool_forward(x4, win, stride)
            wo, ho = y.shape[:2]
            cnt = np.zeros(y.shape)
            for a in range(win[0]):
                for d in range(win[1]):
                    cnt += x4[a: a + (wo - 1) * stride[0] + 1: stride[0], d: d + (ho - 1) * stride[1] + 1: stride[1]] == y
            ties += int(np.sum(cnt > 1))
            wins += y.size
        h = so._layer_forward(row, w, h)
    return ties, wins


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


def gram_exact_certified(a):
    """A'A by the fp64 matrix product, with its certificate: A is an integer matrix and sum_i |a_ik| |a_il| < 2^53 for every
    (k, l) -- then every partial sum of every entry, in ANY order, is an integer below 2^53, nothing rounds, and the fp64
    product is itself the exact reference (a third of the int64 product's time at 49257 x 208).  The bound is asserted through
    its largest member: by Cauchy-Schwarz sum_i |a_ik| |a_il| <= max_k sum_i a_ik^2, the largest diagonal entry, itself an
    exact integer sum when it is below 2^53 (and at least 2^53 as computed when it is not: a sum of non-negative terms rounds
    monotonically)."""
    a = np.asarray(a, dtype=np.float64)
    assert np.array_equal(a, np.rint(a)), "A is not an integer matrix"
    amax = float(np.max(np.abs(a), initial=0.0))
    assert amax < 2.0 ** 26                          # every square is exact
    diag = np.einsum("ij,ij->j", a, a)
    assert float(np.max(diag, initial=0.0)) < F64_LIMIT, "sum_i a_ik^2 reaches 2^53"
    g = np.asfortranarray(a.T @ a)
    assert np.array_equal(np.diag(g), diag)
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


# --------------------------------------------------------------------------- the finish routes against an exact product
# si_construct_finish computes P = A V_M with V_M taken from a HOST eigensolver the library also exports.  On a lattice
# problem G = A'A is exact on the device, so the test can hand the same bits to the same solver, rebuild the V the library
# uploads, form A V exactly and hold the device kernel to the forward error bound of a K-term fp64 dot product:
#     |P[i, m] - (A V)[i, m]| <= gamma_K * sum_k |A[i, k]| |V[k, m]|,   gamma_K = K u / (1 - K u),  u = 2^-53
# (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: valid for ANY summation order, with or without
# FMA).  No eigenvector perturbation, no sign alignment and no gap condition enter the comparison.
U_ROUND = 2.0 ** -53


def gamma(k):
    """gamma_k = k u / (1 - k u)"""
    return k * U_ROUND / (1.0 - k * U_ROUND)


def finish_v_reference(si, g, m, with_branch=False):
    """The ladder of top_eigen (csrc/capi.hip) on a host copy of G, then the sign rule of si_construct_finish:
    host_sym_eig_top(g, m); where it declines, host_sym_eig(g) (ascending) with eigenpair K-1-j taken as the j-th;
    column m multiplied by -1 when its largest-magnitude entry (first index on ties) is negative.
    Returns (w_top descending, V_signed K x m) [, "fast" | "fallback"]."""
    w, v, branch = finish_eig_top(si, g, m)
    v = np.array(v, dtype=np.float64, order="F")
    for j in range(m):
        imax = int(np.argmax(np.abs(v[:, j])))     # first index of the maximum, as the strict > of the C loop keeps it
        if v[imax, j] < 0.0:
            v[:, j] = -v[:, j]
    return (w, v, branch) if with_branch else (w, v)


def finish_eig_top(si, g, m):
    """top_eigen without the sign rule (finish_wide reads its signs from A'U instead): (w_top, V K x m, branch)"""
    g = np.array(g, dtype=np.float64, order="F")
    k = g.shape[0]
    assert g.shape == (k, k) and 0 < m <= k
    r = si.host_sym_eig_top(g, m)
    if r is not None:
        return r[0], r[1], "fast"
    lam, vec = si.host_sym_eig(g)
    idx = [k - 1 - j for j in range(m)]
    return lam[idx].copy(), np.asfortranarray(vec[:, idx]), "fallback"


def argmax_tie(v):
    """True when a column's largest |entry| is attained twice (the sign rule would depend on the scan order)"""
    av = np.abs(np.asarray(v))
    return [int(np.sum(av[:, j] == av[:, j].max())) > 1 for j in range(av.shape[1])]


def split26(x):
    """x = hi + lo exactly, hi and lo with at most 26 significant bits each (hi = x rounded to 26 bits; the remainder is at
    most half a unit of hi's last place and lies on x's 53-bit grid: 26 bits, or the single bit 2^26).  Products of two
    such halves are exact in fp64 (<= 52 bits).  Asserted, not assumed."""
    x = np.asarray(x, dtype=np.float64)
    assert np.all(np.isfinite(x))
    mant, ex = np.frexp(x)
    hi = np.ldexp(np.rint(np.ldexp(mant, 26)), ex - 26)
    lo = x - hi
    assert np.array_equal(hi + lo, x)
    for part in (hi, lo):
        pm, _ = np.frexp(part)
        assert np.array_equal(np.ldexp(pm, 26), np.rint(np.ldexp(pm, 26))), "a half has more than 26 significant bits"
    tiny = (x != 0) & (np.abs(x) < 2.0 ** -900)
    assert not np.any(tiny), "operand too close to the subnormal range for exact products"
    return hi, lo


def project_exact(a, v, rows=None):
    """A V correctly rounded (the exact product rounded once), and sum_k |A||V| for the bound: (P_ref, S).
    Every operand is split into two 26-bit halves (split26); the <= 4 K partial products of an element are exact fp64
    numbers and math.fsum adds them without error, rounding once at the end.  An integer A below 2^26 has no low half,
    which leaves 2 K terms.  `rows` restricts the work to those rows of A."""
    a = np.asarray(a, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    if rows is not None:
        a = a[np.asarray(rows)]
    n, k = a.shape
    assert v.shape[0] == k
    m = v.shape[1]
    if np.all(a == np.rint(a)) and np.max(np.abs(a), initial=0.0) < 2.0 ** 26:
        a_parts = [a]
    else:
        a_hi, a_lo = split26(a)
        a_parts = [a_hi, a_lo]
    v_hi, v_lo = split26(v)
    v_parts = [v_hi] if not np.any(v_lo) else [v_hi, v_lo]
    out = np.empty((n, m), order="F")
    for j in range(m):
        terms = np.concatenate([ap * vp[:, j][None, :] for ap in a_parts for vp in v_parts], axis=1)
        nz = terms != 0
        assert np.all(np.abs(terms[nz]) > 2.0 ** -1000) and np.all(np.isfinite(terms)), "a partial product left the exact range"
        out[:, j] = [math.fsum(r) for r in terms.tolist()]
    return out, np.abs(a) @ np.abs(v)


def project_fraction(a, v):
    """A V in exact rationals (object array of Fractions): the restatement project_exact is checked against"""
    a, v = np.asarray(a, dtype=np.float64), np.asarray(v, dtype=np.float64)
    return [[sum((Fraction(float(a[i, t])) * Fraction(float(v[t, j])) for t in range(a.shape[1])), Fraction(0))
             for j in range(v.shape[1])] for i in range(a.shape[0])]


def projection_bound(s, k, extra=None):
    """gamma_K * S elementwise (S = |A| |V| as project_exact returns it), evaluated so that the fp64 rounding of S and of the
    product can only make it SMALLER than the real-number bound (factor 1 - 2 gamma_{K+2})."""
    b = gamma(k) * s * (1.0 - 2.0 * gamma(k + 2))
    return b if extra is None else b + extra


def projection_ratio(p, p_ref, bound):
    """(worst |p - p_ref| / bound, (row, column)); an element with bound 0 must be equal (ratio inf otherwise)"""
    err = np.abs(np.asarray(p) - p_ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    if ratio.size == 0:
        return 0.0, (0, 0)
    i, j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[i, j]), (int(i), int(j))


def assert_projection(p, a, v, rows=None, what="P", extra=None, factor=1.0):
    """|P - A V| <= factor * (gamma_K |A| |V| + extra) on `rows` (default: all), against the exact product.  Returns the worst
    error as a multiple of the bound; a failure names the element, its row % 64 and column % 8."""
    rows = np.arange(np.asarray(a).shape[0]) if rows is None else np.asarray(rows)
    p_ref, s = project_exact(a, v, rows)
    bound = projection_bound(s, np.asarray(a).shape[1], None if extra is None else np.asarray(extra)[rows])
    worst, (i, j) = projection_ratio(np.asarray(p)[rows], p_ref, bound)
    if not worst <= factor:
        r = int(rows[i])
        raise AssertionError("%s: element (%d, %d) [row %% 64 = %d, column %% 8 = %d] is %r, exact %r: %.4g times the bound %.3g"
                             % (what, r, j, r % 64, j % 8, np.asarray(p)[r, j], p_ref[i, j], worst, bound[i, j]))
    return worst


def assert_projection_rest(p, a, v, rows_done, what="P"):
    """the rows NOT held to the exact product: against NumPy's fp64 a @ v at twice the bound (NumPy's product is itself within
    once the bound of the exact one, by the same theorem)"""
    a, v, p = np.asarray(a), np.asarray(v), np.asarray(p)
    rest = np.setdiff1d(np.arange(a.shape[0]), rows_done)
    if rest.size == 0:
        return 0.0
    bound = 2.0 * projection_bound(np.abs(a[rest]) @ np.abs(v), a.shape[1])
    worst, (i, j) = projection_ratio(p[rest], a[rest] @ v, bound)
    if not worst <= 1.0:
        r = int(rest[i])
        raise AssertionError("%s: element (%d, %d) [row %% 64 = %d, column %% 8 = %d] is %.4g times TWICE the bound (fp64 a @ v)"
                             % (what, r, j, r % 64, j % 8, worst))
    return 2.0 * worst


def exact_rows(n, seed, sample=4096, edge=192):
    """rows held to the exact product when N is large: a random sample, the first and last `edge` rows and the whole last
    partial 64-row slab; all rows when that is no saving"""
    if n <= sample + 2 * edge + 64:
        return np.arange(n)
    rng = np.random.default_rng(seed)
    tail = n - max(edge, n % 64)
    return np.unique(np.concatenate([rng.choice(n, sample, replace=False), np.arange(edge), np.arange(tail, n)]))


# ---- injected Gram matrices with known eigenvectors (si_construct_gram_set)
def diag_gram(k, seed):
    """G = diag(d), d a shuffle of distinct positive integers: eigenvalue number j (descending) is d[perm[j]] with the unit
    vector e_perm[j].  Returns (G, d, perm)."""
    rng = np.random.default_rng(seed)
    d = rng.permutation(np.arange(1, k + 1) * 3 + 7).astype(np.float64)
    perm = np.argsort(-d, kind="stable")
    return np.asfortranarray(np.diag(d)), d, perm


def unit_columns(v, perm):
    """(exact, dust): whether V's column j is exactly the unit vector e_perm[j]; else the largest |entry| off that place
    (None when a column is not a unit vector up to dust: the place itself must hold exactly +1)"""
    v = np.asarray(v)
    off = np.array(v, copy=True)
    for j in range(v.shape[1]):
        if v[perm[j], j] != 1.0:
            return False, None
        off[perm[j], j] = 0.0
    dust = float(np.max(np.abs(off), initial=0.0))
    return dust == 0.0, dust


def paired_gram(k, seed, eps=2.0 ** -30):
    """block-diagonal G of 2 x 2 blocks [[a, b], [b, a]], b = eps * a (eigenvalues a (1 +- eps), eigenvectors (1, +-1)/sqrt 2:
    near-degenerate pairs with a relative gap 2 eps), distinct integers a, the blocks at shuffled places; odd K: a last
    1 x 1 block.  Not exactly representable eigenvectors: for the bound, never for equality."""
    rng = np.random.default_rng(seed)
    place = rng.permutation(k)
    g = np.zeros((k, k))
    for b in range(k // 2):
        i, j = place[2 * b], place[2 * b + 1]
        a = float(3 * b + 5)
        g[i, i] = g[j, j] = a
        g[i, j] = g[j, i] = eps * a
    if k % 2:
        g[place[-1], place[-1]] = 2.0
    return np.asfortranarray(g)


# ---- the two-stage route (si_construct_refine, then the second-stage finish)
def refine_reference(si, a, g, rows=None):
    """V_full as si_construct_refine builds it (host_sym_eig ascending, column j <- eigenvector K-1-j) and B_ref = A V_full
    correctly rounded.  Returns (V_full, B_ref, D) with D the elementwise bound on |B_device - B_ref|:
        B* = A V exactly;  |B_device - B*| <= gamma_K S  (the projection kernel),  |B_ref - B*| <= u S  (one rounding), S = |A||V|
        =>  D = (gamma_K + u) S."""
    k = np.asarray(g).shape[0]
    _, vec = si.host_sym_eig(np.array(g, dtype=np.float64, order="F"))
    v_full = np.asfortranarray(vec[:, ::-1])
    b_ref, s = project_exact(a, v_full, rows)
    return v_full, b_ref, (gamma(k) + U_ROUND) * s * (1.0 + 4.0 * gamma(k))


def gram2_bound(b_ref, d):
    """Elementwise bound on |G2_device - B_ref' B_ref| (the latter correctly rounded), G2_device = fl(B^' B^) over N rows:
        |B^| <= |B_ref| + D =: Bu;   fl error of an N-term dot product: gamma_N Bu' Bu;
        B^'B^ - B_ref'B_ref = d'B_ref + B_ref'd + d'd with |d| <= D:  D'|B_ref| + |B_ref|'D + D'D;
        rounding of the reference itself: u |B_ref|'|B_ref|.
    Composed, not tuned; the (1 + 4 gamma_N) covers the fp64 evaluation of this expression."""
    n = b_ref.shape[0]
    ab = np.abs(b_ref)
    bu = ab + d
    t = gamma(n) * (bu.T @ bu) + d.T @ ab + ab.T @ d + d.T @ d + U_ROUND * (ab.T @ ab)
    return t * (1.0 + 4.0 * gamma(n))


def second_stage_reference(si, v_full, g2, m):
    """The second-stage finish on the DEVICE's G2 (bit-identical input to host_jacobi_eig_psd): (s, W_signed K x m, margin_ok).
    Signs as capi.hip reads them from V_full W_M; that product is formed in fp64 there (in an order and with a contraction
    the compiler chooses), so a column's sign is only pinned when its largest |entry| beats the runner-up and zero by more
    than the K-term bound 2 gamma_K |V_full||W|: margin_ok[j] says so."""
    lam2, w = si._capi.host_jacobi_eig_psd(np.array(g2, dtype=np.float64, order="F"))
    k = v_full.shape[0]
    wm = np.array(w[:, :m], dtype=np.float64, order="F")
    vs = v_full @ wm
    tol = 2.0 * gamma(k) * (np.abs(v_full) @ np.abs(wm))
    ok = []
    for j in range(m):
        av = np.abs(vs[:, j])
        order = np.argsort(-av, kind="stable")
        i0 = int(np.argmax(av))
        second = av[order[1]] + tol[order[1], j] if k > 1 else 0.0
        ok.append(bool(av[i0] - tol[i0, j] > second))
        if vs[i0, j] < 0.0:
            wm[:, j] = -wm[:, j]
    return np.sqrt(lam2[:m]), wm, ok


# ---- the K > N route (finish_wide)
def gram_wide_exact(a):
    """A A' in int64 (certificate: every entry below 2^53)"""
    ai = a.astype(np.int64)
    assert np.array_equal(ai.astype(np.float64), a)
    assert int(np.abs(ai).max(initial=0)) ** 2 * a.shape[1] < 2 ** 53
    return ai @ ai.T


def wide_reference(si, a, m):
    """finish_wide replayed on the host: U, w from the ladder on the exact A A'; the sign of column j from the
    largest-magnitude entry of R = A' u_j, which the DEVICE forms in fp64 -- so it is pinned only where, on the exact R, the
    winner beats the runner-up by more than both entries' bounds gamma_N |A'||U|.  Returns (s, P_ref = +-s_j u_j, pinned[j])."""
    n = a.shape[0]
    w, u, _ = finish_eig_top(si, gram_wide_exact(a).astype(np.float64), m)
    s = np.sqrt(w)
    r, sabs = project_exact(a.T, u)
    tol = gamma(n) * sabs
    p_ref = np.empty((n, m), order="F")
    pinned = []
    for j in range(m):
        av = np.abs(r[:, j])
        i0 = int(np.argmax(av))
        order = np.argsort(-av, kind="stable")
        second = order[1] if order[0] == i0 else order[0]
        pinned.append(bool(a.shape[1] == 1 or av[i0] - tol[i0, j] > av[second] + tol[second, j]))
        f = (-1.0 if r[i0, j] < 0.0 else 1.0) * s[j]
        p_ref[:, j] = f * u[:, j]
    return s, p_ref, pinned


def gram_exact_f64(a):
    """A'A by the fp64 BLAS: exact under gram_exact's certificate (every partial sum is an integer below 2^53 in any order)"""
    assert np.array_equal(a, np.rint(a)) and float(np.max(np.abs(a), initial=0.0)) ** 2 * a.shape[0] < 2.0 ** 53
    return np.asfortranarray(a.T @ a)


def finish_problem(n, k):
    """the lattice construction problem of a FINISH_* case: (snapshots, epoch counters, means, A).  The epoch counters start at
    1: with n_0 = 0 the first deviation column is zero and A has rank K - 1, which would send every M = K case to the
    two-stage route and from there to BoundsError."""
    return snapshots(n, k, seed=n + k, ns=range(1, k + 1))


# ---- the shapes of tests/test_gpu_finish_exact.py, shared with its CPU certificate (tests/test_finish_exact_cpu.py).
# (N, K, M, kernel reached).  M <= min(N, K) is the API's own limit (BoundsError), so:
#   * the slab-stream kernels (M > 32, K <= 128) cannot be reached with NT = ceil(K / 16) < 3 nor with N below two 32-row
#     slabs; NT = 3 .. 8 are, each at K = 16 NT, 16 NT - 1 and 16 NT - 15;
#   * project_glds_kernel<NT, NB, 1> (one workgroup per CU) is selected only by a development-build knob: shapes reach OCC = 2.
# Several slabs per workgroup need more than 2 * 256 slabs: N = 20001 (626 slabs, the last of 1 row), 100003.
FINISH_F64 = [
    (1, 1, 1, "project_kernel<8, double>"),
    (63, 15, 3, "project_kernel<8, double>"),
    (64, 16, 8, "project_kernel<8, double>"),
    (65, 17, 9, "project_kernel<16, double>"),
    (511, 100, 16, "project_kernel<16, double>"),
    (513, 128, 17, "project_kernel<24, double>"),
    (4097, 129, 24, "project_kernel<24, double>"),
    (100003, 100, 25, "project_kernel<32, double>"),
    (4097, 200, 32, "project_kernel<32, double>"),
    (513, 260, 25, "project_kernel<32, double>"),
    (33, 33, 33, "project_glds_kernel<3>"),
    (65, 47, 40, "project_glds_kernel<3>"),
    (4097, 48, 33, "project_glds_kernel<3>"),
    (127, 49, 40, "project_glds_kernel<4>"),
    (20001, 63, 33, "project_glds_kernel<4>"),
    (513, 64, 64, "project_glds_kernel<4>"),
    (129, 65, 65, "project_glds_kernel<5>"),
    (4097, 79, 70, "project_glds_kernel<5>"),
    (128, 80, 64, "project_glds_kernel<5>"),
    (4097, 81, 33, "project_glds_kernel<6>"),
    (511, 95, 65, "project_glds_kernel<6>"),
    (20001, 96, 40, "project_glds_kernel<6>"),
    (513, 97, 70, "project_glds_kernel<7>"),
    (4097, 111, 100, "project_glds_kernel<7>"),
    (64, 112, 64, "project_glds_kernel<7>"),
    (4097, 113, 100, "project_glds_kernel<8>"),
    (129, 127, 65, "project_glds_kernel<8>"),
    (4097, 128, 128, "project_glds_kernel<8>"),
    (100003, 128, 64, "project_glds_kernel<8>"),
    (127, 129, 33, "gemm_f64_kernel<128, 64>"),
    (128, 130, 64, "gemm_f64_kernel<128, 64>"),
    (129, 143, 65, "gemm_f64_kernel<128, 64>"),
    (4097, 144, 128, "gemm_f64_kernel<128, 64>"),
    (20001, 145, 33, "gemm_f64_kernel<128, 64>"),
    (129, 200, 129, "gemm_f64_kernel<128, 64>"),
    (4097, 200, 64, "gemm_f64_kernel<128, 64>"),
    (513, 260, 200, "gemm_f64_kernel<128, 64>"),
]
# fp32 storage (si_construct_set_storage(SI_F32)); M > 32 with K > 128 walks project_valu's 32 / 24 / 16 / 8 passes
FINISH_F32 = [
    (63, 15, 8, "project_kernel<8, float>"),
    (513, 100, 16, "project_kernel<16, float>"),
    (4097, 128, 24, "project_kernel<24, float>"),
    (65, 200, 32, "project_kernel<32, float>"),
    (513, 129, 33, "project_kernel<32 + 8, float>"),
    (4097, 200, 65, "project_kernel<32 + 32 + 8, float>"),
    (127, 260, 50, "project_kernel<32 + 24, float>"),
    (129, 143, 44, "project_kernel<32 + 16, float>"),
    (65, 33, 33, "project_glds_f32_kernel<3>"),
    (4097, 48, 40, "project_glds_f32_kernel<3>"),
    (513, 64, 64, "project_glds_f32_kernel<4>"),
    (129, 80, 65, "project_glds_f32_kernel<5>"),
    (20001, 95, 33, "project_glds_f32_kernel<6>"),
    (4097, 111, 100, "project_glds_f32_kernel<7>"),
    (127, 127, 70, "project_glds_f32_kernel<8>"),
    (4097, 128, 128, "project_glds_f32_kernel<8>"),
]
# injected diagonal G: (N, K, M, fp32 storage, kernel, solver returns exact unit vectors).  The last field is RECORDED from the host
# solver (tests/test_finish_exact_cpu.py::test_diag_gram_table holds it); the fallback solver returns exact unit vectors,
# the fast route unit vectors plus dust far below 2^-100 in the other places.
FINISH_DIAG = [
    (513, 16, 8, False, "project_kernel<8, double>", True),
    (65, 12, 3, False, "project_kernel<8, double>", False),
    (4097, 100, 20, False, "project_kernel<24, double>", False),
    (4097, 200, 32, False, "project_kernel<32, double>", False),
    (513, 48, 33, False, "project_glds_kernel<3>", True),
    (129, 81, 65, False, "project_glds_kernel<6>", True),
    (20001, 100, 70, False, "project_glds_kernel<7>", True),
    (4097, 128, 64, False, "project_glds_kernel<8>", True),
    (129, 200, 33, False, "gemm_f64_kernel<128, 64>", False),
    (513, 145, 129, False, "gemm_f64_kernel<128, 64>", True),
    (4097, 260, 130, False, "gemm_f64_kernel<128, 64>", True),
    (65, 17, 9, True, "project_kernel<16, float>", True),
    (4097, 200, 65, True, "project_kernel<32 + 32 + 8, float>", False),
    (513, 64, 40, True, "project_glds_f32_kernel<4>", True),
]
# near-degenerate pairs (relative gap 2^-29): (N, K, M, fp32 storage, kernel)
FINISH_PAIRED = [
    (4097, 100, 20, False, "project_kernel<24, double>"),
    (513, 128, 64, False, "project_glds_kernel<8>"),
    (4097, 200, 33, False, "gemm_f64_kernel<128, 64>"),
    (129, 64, 33, True, "project_glds_f32_kernel<4>"),
]
# two-stage route on a lattice A, driven explicitly: (N, K, M of the finish, kernel of B = A V_full with M = K)
FINISH_REFINE = [
    (1025, 24, 5, "project_kernel<24, double>"),
    (4097, 40, 33, "project_glds_kernel<3>"),
    (513, 130, 64, "gemm_f64_kernel<128, 64>"),
]
# K > N: (N, K, M, projection kernel of R = A'U with N in the role of K)
FINISH_WIDE = [
    (5, 6, 1, "project_kernel<8, double>"),
    (5, 1000, 3, "project_kernel<8, double>"),
    (64, 65, 20, "project_kernel<24, double>"),
    (64, 128, 33, "project_glds_kernel<4>"),
    (100, 101, 3, "project_kernel<8, double>"),
    (100, 200, 64, "project_glds_kernel<7>"),
    (128, 1000, 33, "project_glds_kernel<8>"),
    (129, 130, 64, "gemm_f64_kernel<128, 64>"),
    (129, 258, 20, "project_kernel<24, double>"),
    (200, 201, 33, "gemm_f64_kernel<128, 64>"),
    (200, 1000, 64, "gemm_f64_kernel<128, 64>"),
    (682, 683, 64, "gemm_f64_kernel<128, 64>"),
    (682, 1000, 20, "project_kernel<24, double>"),
    (682, 1364, 33, "gemm_f64_kernel<128, 64>"),
]
