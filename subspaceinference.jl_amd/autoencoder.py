"""The decoder of the autoencoder route (reference src/space_inference.jl:238-318, `auto_inference`: the density at
`W_swa + decoder(z)` instead of `W_swa + P*z`) restated in plain NumPy.

This file is to si_infer_set_decoder / si_decode what diffmap.py is to the diffusion route: the definition the device result is
tested against.  A decoder is a Dense-only layer table (`flux.layer_table` of the decoder chain: rows (in, out, act, w_off,
b_off), M -> h_1 -> ... -> h_{D-1} -> N) with its flat parameter vector `wdec` in Flux.destructure order ([vec(W_l); b_l] per
layer, W_l column-major out x in), Float32 (Flux's default) or Float64.

All arithmetic is fp64; Float32 parameters are widened, which is exact -- what Julia's promotion does with a Float64 z.
Per layer u = W a + b: the sum over the input index ascending from 0.0, every product and every sum rounded, the bias added
last; then a = act(u).  In the two Jacobian products act' is rebuilt from the stored layer OUTPUT (the project's convention,
dact_from_output in the kernels), so all eight SI_ACT_* are allowed.
"""
import numpy as np

from . import flux
from ._capi import SubspaceError

_SELU_L, _SELU_A = flux._SELU_L, flux._SELU_A


def dact_from_output(h, kind):
    """act'(x) expressed through the output h = act(x), as csrc/kernels_gemm.h: dact_full"""
    if kind == flux.identity:
        return np.ones_like(h)
    if kind == flux.relu:
        return np.where(h > 0.0, 1.0, 0.0)
    if kind == flux.tanh:
        return 1.0 - h * h
    if kind == flux.sigmoid:
        return h * (1.0 - h)
    if kind == flux.leakyrelu:
        return np.where(h > 0.0, 1.0, 0.01)
    if kind == flux.elu:
        return np.where(h >= 0.0, 1.0, h + 1.0)
    if kind == flux.softplus:
        return 1.0 - np.exp(-h)
    if kind == flux.selu:
        return np.where(h > 0.0, _SELU_L, h + _SELU_L * _SELU_A)
    raise SubspaceError("Error: activation %r is not available" % (kind,))


def check_table(table, wdec, m=None, n=None):
    """The refusals of si_infer_set_decoder that need no device; returns (M, N) of the decoder."""
    if len(table) < 1:
        raise SubspaceError("a decoder needs at least one Dense layer")
    wdec = np.asarray(wdec)
    if wdec.ndim != 1 or wdec.dtype not in (np.float32, np.float64):
        raise SubspaceError("decoder parameters must be a flat Float32 or Float64 vector")
    prev = None
    for row in table:
        if isinstance(row[0], str):
            raise SubspaceError("every decoder layer must be Dense")
        fin, fout, act, w_off, b_off = (int(v) for v in row[:5])
        if not 0 <= act < 8:
            raise SubspaceError("unknown activation %d" % act)
        if prev is not None and fin != prev:
            raise SubspaceError("DimensionMismatch: consecutive decoder widths do not chain (%d after %d)" % (fin, prev))
        if w_off < 0 or w_off + fin * fout > wdec.size or b_off < 0 or b_off + fout > wdec.size:
            raise SubspaceError("a decoder layer's offset range falls outside the parameter vector")
        prev = fout
    m_dec, n_dec = int(table[0][0]), int(table[-1][1])
    if m is not None and m_dec != m:
        raise SubspaceError("DimensionMismatch: the decoder takes %d inputs but M = %d" % (m_dec, m))
    if n is not None and n_dec != n:
        raise SubspaceError("DimensionMismatch: the decoder returns %d values but the model has %d parameters" % (n_dec, n))
    return m_dec, n_dec


def _layers(table, wdec):
    wdec = np.asarray(wdec)
    for fin, fout, act, w_off, b_off in (tuple(int(v) for v in row[:5]) for row in table):
        W = wdec[w_off:w_off + fin * fout].astype(np.float64).reshape((fout, fin), order="F")
        b = wdec[b_off:b_off + fout].astype(np.float64)
        yield W, b, act


def _forward(table, wdec, z):
    """every layer's output, a_0 = z first; z is (M,) or (M, C)"""
    a = np.array(z, dtype=np.float64)
    outs = [a]
    for W, b, act in _layers(table, wdec):
        u = np.zeros((W.shape[0],) + a.shape[1:])
        for i in range(W.shape[1]):            # ascending input index, from 0.0; every product and sum rounded
            u = u + (W[:, i] * a[i] if a.ndim == 1 else W[:, i:i + 1] * a[i:i + 1])
        u = u + (b if a.ndim == 1 else b[:, None])
        a = flux._act_fwd(u, act)
        outs.append(a)
    return outs


def decode(table, wdec, z):
    """y = decoder(z): (N,) for a vector z, (N, C) for an M x C matrix"""
    return _forward(table, wdec, z)[-1]


def weights(w_swa, table, wdec, z):
    """W_swa + decoder(z), W_swa first (reference :247)"""
    y = decode(table, wdec, z)
    w_swa = np.asarray(w_swa, dtype=np.float64)
    return (w_swa if y.ndim == 1 else w_swa[:, None]) + y


def decode_jvp(table, wdec, z, dz):
    """J(z) dz for a vector z"""
    outs = _forward(table, wdec, np.asarray(z, dtype=np.float64).reshape(-1))
    t = np.array(dz, dtype=np.float64).reshape(-1)
    for (W, _, act), a in zip(_layers(table, wdec), outs[1:]):
        t = dact_from_output(a, act) * (W @ t)
    return t


def decode_vjp(table, wdec, z, gy):
    """J(z)' gy for a vector z: per layer, from the last, delta = g .* act'(a_l); g = W_l' delta with the sum over the output
    index ascending from 0.0"""
    outs = _forward(table, wdec, np.asarray(z, dtype=np.float64).reshape(-1))
    g = np.array(gy, dtype=np.float64).reshape(-1)
    for (W, _, act), a in reversed(list(zip(_layers(table, wdec), outs[1:]))):
        delta = g * dact_from_output(a, act)
        g = np.zeros(W.shape[1])
        for j in range(W.shape[0]):
            g = g + W[j, :] * delta[j]
    return g


# ---------------------------------------------------------------------------------------------------------------------------------
# Training Chain(encoder, decoder) on the deviation columns (reference src/subspace_construction.jl:125-140): the definition of
# si_ae_train_step / si_ae_train_loss (csrc/kernels_ae_train.hip).  `table` is the Dense-only layer table of the whole
# autoencoder N -> e_1 -> ... -> M -> ... -> H -> N, `w` its flat parameters in flux.params order, `xb` the N x nb batch.
#
# Three sums run over the N rows: the first layer's forward, the last layer's pull-back W_D' delta, and sum r^2 (with
# `penalty`, the rows' shares of sum w^2 as well).  `order` names how they are taken: "ascending" (the default: the written
# order of this file), "pairwise", or "blocked" -- the device's order, which depends on N alone: row n belongs to row block
# n // AE_ROWS, row block rb to workgroup rb % G with G = min(row blocks, AE_GRID); per row block a shuffle-down tree over each
# wave's 64 rows and (w0 + w1) + (w2 + w3) over the four waves; a workgroup adds its row blocks in ascending order from 0.0,
# and the G workgroup sums are added in ascending order from 0.0.  Every other sum is ascending from 0.0.
AE_ROWS, AE_GRID = 256, 1024   # the kernels' constants of the same names (tests/test_ae_train_cpu.py compares them)


def _nsum(t, order="ascending"):
    """sum over axis 0 of t (N x ...) in the named order"""
    t = np.asarray(t, dtype=np.float64)
    n = t.shape[0]
    if order == "ascending":
        return np.cumsum(t, axis=0)[-1]          # (cumsum adds one element after the other)
    if order == "pairwise":
        while t.shape[0] > 1:
            if t.shape[0] & 1:
                t = np.concatenate([t, np.zeros((1,) + t.shape[1:])], axis=0)
            t = t[0::2] + t[1::2]
        return t[0]
    if order != "blocked":
        raise SubspaceError("unknown summation order %r" % (order,))
    nblk = -(-n // AE_ROWS)
    g = min(nblk, AE_GRID)
    passes = -(-nblk // g)
    pad = passes * g * AE_ROWS - n
    if pad:
        t = np.concatenate([t, np.zeros((pad,) + t.shape[1:])], axis=0)
    t = t.reshape((passes, g, AE_ROWS // 64, 64) + t.shape[1:])
    off = 32
    while off > 0:
        t = t[:, :, :, :off] + t[:, :, :, off:2 * off]
        off >>= 1
    t = t[:, :, :, 0]
    t = (t[:, :, 0] + t[:, :, 1]) + (t[:, :, 2] + t[:, :, 3])
    acc = np.zeros(t.shape[1:])
    for p in range(passes):
        acc = acc + t[p]
    return np.cumsum(np.concatenate([np.zeros((1,) + acc.shape[1:]), acc], axis=0), axis=0)[-1]


def check_train_table(table, w, n=None):
    """the refusals of si_ae_train_setup that need no device; returns N"""
    check_table(table, w)
    big = int(table[0][0])
    if int(table[-1][1]) != big or (n is not None and big != n):
        raise SubspaceError("DimensionMismatch: the autoencoder must take and return N values")
    if len(table) < 2:
        raise SubspaceError("an autoencoder needs an encoder and a decoder layer")
    if any(int(r[1]) > 256 for r in table[:-1]):
        raise SubspaceError("a hidden width above 256")
    return big


def _train_forward(table, w, xb, order):
    xb = np.asarray(xb, dtype=np.float64)
    xb = xb.reshape(xb.shape[0], -1)
    lay = list(_layers(table, w))
    outs = [xb]
    W, b, act = lay[0]
    u = _nsum(W.T[:, :, None] * xb[:, None, :], order) + b[:, None]      # terms[n, j, b] = W_1[j, n] x[n, b]
    outs.append(flux._act_fwd(u, act))
    for W, b, act in lay[1:]:
        a = outs[-1]
        u = np.zeros((W.shape[0], a.shape[1]))
        for i in range(W.shape[1]):
            u = u + W[:, i:i + 1] * a[i:i + 1]
        outs.append(flux._act_fwd(u + b[:, None], act))
    return lay, outs


def _penalty(table, w, order):
    """sum w^2 as the device takes it: (first layer's rows + the small arrays in flat order) + last layer's rows"""
    lay = list(_layers(table, w))
    w64 = np.asarray(w).astype(np.float64)
    W1, WD, bD = lay[0][0], lay[-1][0], lay[-1][1]
    q1 = np.zeros(W1.shape[1])
    for j in range(W1.shape[0]):
        q1 = q1 + W1[j, :] * W1[j, :]
    qd = np.zeros(WD.shape[0])
    for h in range(WD.shape[1]):
        qd = qd + WD[:, h] * WD[:, h]
    qd = qd + bD * bD
    lo, hi = int(table[0][4]), int(table[-1][3])          # b_1 and every middle array: one contiguous flat range
    mid = 0.0
    for x in w64[lo:hi]:
        mid = mid + x * x
    return (float(_nsum(q1, order)) + mid) + float(_nsum(qd, order))


def train_loss(table, w, x, penalty=False, order="ascending"):
    """autoloss(re_weight) (reference :129,137): (sum r^2 over ALL columns) / (N K), one division; + sum w^2 with `penalty`.
    sum r^2 of a row is taken over the columns ascending, the rows as `order` says (the device: chunk after chunk of batch_max
    columns, the chunks' sums added in ascending order -- on the integer lattice the same number)"""
    lay, outs = _train_forward(table, w, x, order)
    r = outs[-1] - outs[0]
    q = np.zeros(r.shape[0])
    for b in range(r.shape[1]):
        q = q + r[:, b] * r[:, b]
    loss = float(_nsum(q, order)) / float(r.shape[0] * r.shape[1])
    return loss + _penalty(table, w, order) if penalty else loss


def train_value_and_grad(table, w, xb, penalty=False, order="ascending"):
    """(loss, g): loss = (sum r^2) / (N nb), r = sae(xb) - xb, and its gradient w.r.t. the flat parameters, Float64.

    The reverse sweep carries the UNSCALED cotangent: dt_L = r .* act'(a_L); per layer, from the last, G_l = dt_l a_{l-1}',
    gb_l = sum_batch dt_l (both over the batch index ascending from 0.0), dt_{l-1} = (W_l' dt_l) .* act'(a_{l-1}) (the sum over
    the output index ascending from 0.0; the last layer's over its N rows as `order` says).  The factor s = 2.0 / (N nb) enters
    once per gradient element, g = s * G; with `penalty`, g += 2 w and the loss gains sum w^2.  flux.MSE.value_and_grad scales
    the cotangent first: the two differ by rounding only."""
    w = np.asarray(w)
    lay, outs = _train_forward(table, w, xb, order)
    big, nb = outs[0].shape
    r = outs[-1] - outs[0]
    q = np.zeros(big)
    for b in range(nb):
        q = q + r[:, b] * r[:, b]
    loss = float(_nsum(q, order)) / float(big * nb)
    s = 2.0 / float(big * nb)
    g = np.zeros(w.size)
    dt = r * dact_from_output(outs[-1], lay[-1][2])
    for l in range(len(lay) - 1, -1, -1):
        W, _, _ = lay[l]
        _, fout, _, w_off, b_off = (int(v) for v in table[l][:5])
        a = outs[l]
        G = np.zeros(W.shape)
        gb = np.zeros(fout)
        for b in range(nb):
            G = G + dt[:, b:b + 1] * a[:, b][None, :]
            gb = gb + dt[:, b]
        g[w_off:w_off + W.size] = (s * G).reshape(-1, order="F")
        g[b_off:b_off + fout] = s * gb
        if l > 0:
            if l == len(lay) - 1:
                back = _nsum(W[:, :, None] * dt[:, None, :], order)       # terms[n, h, b] = W_D[n, h] dt[n, b]
            else:
                back = np.zeros((W.shape[1], nb))
                for j in range(W.shape[0]):
                    back = back + W[j, :][:, None] * dt[j:j + 1, :]
            dt = back * dact_from_output(a, lay[l - 1][2])
    if penalty:
        g = g + 2.0 * w.astype(np.float64)
        loss = loss + _penalty(table, w, order)
    return loss, g


def optimiser_update(w, m, v, g, opt, beta_pows):
    """csrc/optimiser_update.h on whole arrays for a Float64 gradient: Float64 arithmetic, the state and the parameters rounded
    once on the store into their own element type.  opt = (kind, eta, p1, p2); returns (w, m, v) -- new arrays"""
    kind, eta, p1, p2 = opt
    T = w.dtype.type
    w64, m64, v64 = w.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    if kind == 0:
        step = g * eta
    elif kind == 1:
        m = (p1 * m64 - eta * g).astype(T)
        step = -m.astype(np.float64)
    else:
        m = (p1 * m64 + (1.0 - p1) * g).astype(T)
        v = (p2 * v64 + (1.0 - p2) * (g * g)).astype(T)
        step = m.astype(np.float64) / (1.0 - beta_pows[0]) / (np.sqrt(v.astype(np.float64) / (1.0 - beta_pows[1])) + 1e-8) * eta
    return (w64 - step).astype(T), m.copy(), v.copy()


def train_step(table, w, m, v, beta_pows, xb, opt, penalty=False, order="ascending"):
    """one step: the gradient at w, then the update -> (loss, w, m, v, beta_pows), the loss that of the batch BEFORE the update.
    w, m, v share an element type (Float32 or Float64: Flux keeps zero(x) as state); the beta powers advance once per ADAM step"""
    loss, g = train_value_and_grad(table, w, xb, penalty, order)
    w2, m2, v2 = optimiser_update(np.asarray(w), np.asarray(m), np.asarray(v), g, opt, beta_pows)
    bp = [beta_pows[0] * opt[2], beta_pows[1] * opt[3]] if opt[0] == 2 else list(beta_pows)
    return loss, w2, m2, v2, bp
