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
