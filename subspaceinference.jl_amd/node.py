"""The NeuralODE density (reference src/space_inference.jl:96-101, `model_re` at src/libs.jl:36-54; docs/src/node_example.md)
restated in plain NumPy: Tsit5 with its free interpolant, the PI step controller, the Hairer-Wanner starting step, the save rule
of `saveat` without `tstops`, and the sum of squared errors over the saved states.

This file is to si_infer_setup_node / si_node_solve what diffmap.py and autoencoder.py are to their routes: the definition the
device result is tested against.  All arithmetic is fp64, every product and every sum is rounded on its own, and the WRITTEN
ORDER of every expression below is the definition: csrc/kernels_node.hip (built without contraction of a*b+c) repeats it
operator by operator.  The trajectories of one weight vector are advanced side by side (one column each, every column with its
own t, h and controller state); all operations are elementwise over the columns, so a trajectory's bits do not depend on which
others run beside it.

Right-hand side: a_0 = u, or (u*u)*u with pre_power = 3 (Julia's literal x^3, the tutorial's `x -> x.^3`); then Dense layers as
autoencoder.decode evaluates them: the sum over the input index ascending from 0.0, the bias last, act from the eight SI_ACT_*.

`nudge` (a Nudge, or None) moves the result of every transcendental call (tanh / exp / log1p, the controller's and the starting
step's pow) by +-k ulp following a seeded sign pattern: the tests use it to measure how far a few ulp of libm move a result.
"""
from dataclasses import dataclass

import numpy as np

from . import flux
from ._capi import SubspaceError

# ---- Tsit5 (Tsitouras 2011): seven stages, FSAL, b = a_7. ---------------------------------------------------------------------
C = (0.0, 0.161, 0.327, 0.9, 0.9800255409045097, 1.0, 1.0)
A = ((),
     (0.161,),
     (-0.008480655492356989, 0.335480655492357),
     (2.8971530571054935, -6.359448489975075, 4.3622954328695815),
     (5.325864828439257, -11.748883564062828, 7.4955393428898365, -0.09249506636175525),
     (5.86145544294642, -12.92096931784711, 8.159367898576159, -0.071584973281401, -0.028269050394068383),
     (0.09646076681806523, 0.01, 0.4798896504144996, 1.379008574103742, -3.290069515436081, 2.324710524099774))
BT = (-0.00178001105222577714, -0.0008164344596567469, 0.007880878010261995, -0.1447110071732629, 0.5823571654525552,
      -0.45808210592918697, 0.015151515151515152)
# the interpolant's constants, b_j(theta) as written in interp_weights below
B1 = (-1.0530884977290216, 1.3299890189751412, 1.4364028541716351, 0.7139816917074209)
B2 = (0.1017, 2.1966568338249754, 1.2949852507374631)
B3 = (2.490627285651252793, 2.38535645472061657, 1.57803468208092486)
B4 = (-16.54810288924490272, 1.21712927295533244, 0.61620406037800089)
B5 = (47.37952196281928122, 1.203071208372362603, 0.658047292653547382)
B6 = (-34.87065786149660974, 1.2, 0.666666666666666667)
B7 = (2.5, 1.0, 0.6)
# what si_node_tableau writes: c (7), a row by row (21), b~ (7), B1 .. B7 (4 + 6 * 3)
TABLEAU = np.array(list(C) + [v for row in A for v in row] + list(BT) + list(B1 + B2 + B3 + B4 + B5 + B6 + B7), dtype=np.float64)

# the PI controller (OrdinaryDiffEq's defaults for Tsit5, from memory: README "parity is unpinned")
BETA1, BETA2, GAMMA, QMIN_INV, QMAX_INV, QOLD0 = 7.0 / 50.0, 2.0 / 25.0, 9.0 / 10.0, 5.0, 0.1, 1e-4
MAX_STEPS_DEFAULT, MAX_STEPS_LIMIT = 100000, 1000000
MAX_LAYERS, MAX_D, MAX_WIDTH, MAX_N, MAX_S = 8, 8, 256, 8192, 4096


def interp_weights(th):
    """b_1(theta) .. b_7(theta); th may be an array"""
    th2 = th * th
    return (B1[0] * th * (th - B1[1]) * (th2 - B1[2] * th + B1[3]),
            B2[0] * th2 * (th2 - B2[1] * th + B2[2]),
            B3[0] * th2 * (th2 - B3[1] * th + B3[2]),
            B4[0] * (th - B4[1]) * (th - B4[2]) * th2,
            B5[0] * (th - B5[1]) * (th - B5[2]) * th2,
            B6[0] * (th - B6[1]) * (th - B6[2]) * th2,
            B7[0] * (th - B7[1]) * (th - B7[2]) * th2)


@dataclass
class Opts:
    t0: float = 0.0
    reltol: float = 1e-3
    abstol: float = 1e-6
    dt: float = 0.0
    adaptive: int = 1
    max_steps: int = MAX_STEPS_DEFAULT
    pre_power: int = 1


class Nudge:
    """moves every value it is given by +-k ulp; the signs come from one seeded stream"""

    def __init__(self, k, seed=0):
        self.k, self.rng = int(k), np.random.default_rng(seed)

    def __call__(self, v):
        v = np.asarray(v, dtype=np.float64)
        if self.k == 0:
            return v
        up = self.rng.integers(0, 2, size=v.shape).astype(bool)
        out = v.copy()
        for _ in range(self.k):
            out = np.where(up, np.nextafter(out, np.inf), np.nextafter(out, -np.inf))
        return np.where(np.isfinite(v), out, v)


def _same(v):
    return v


def act(v, kind, nudge=_same):
    """the eight activations as csrc/kernels_gemm.h: act_full writes them"""
    if kind == flux.identity:
        return v
    if kind == flux.relu:
        return np.where(v > 0.0, v, 0.0)
    if kind == flux.tanh:
        return nudge(np.tanh(v))
    if kind == flux.sigmoid:
        return 1.0 / (1.0 + nudge(np.exp(-v)))
    if kind == flux.leakyrelu:
        return np.where(v > 0.01 * v, v, 0.01 * v)
    if kind == flux.elu:
        return np.where(v >= 0.0, v, nudge(np.exp(np.minimum(v, 0.0))) - 1.0)
    if kind == flux.softplus:
        t = nudge(np.log1p(nudge(np.exp(-np.abs(v)))))
        return np.where(v > 0.0, v + t, t)
    if kind == flux.selu:
        return flux._SELU_L * np.where(v > 0.0, v, flux._SELU_A * (nudge(np.exp(np.minimum(v, 0.0))) - 1.0))
    raise SubspaceError("Error: activation %r is not available" % (kind,))


def check(table, n, d, ts, opts):
    """the refusals of si_infer_setup_node that need no device"""
    def bad(what):
        raise SubspaceError("si_infer_setup_node: " + what)
    if not 1 <= len(table) <= MAX_LAYERS:
        bad("a NeuralODE right-hand side has 1 to %d Dense layers" % MAX_LAYERS)
    if not 1 <= d <= MAX_D:
        bad("the state dimension d must be 1 to %d" % MAX_D)
    if not 1 <= n <= MAX_N:
        bad("N must be 1 to %d" % MAX_N)
    prev = d
    for row in table:
        if isinstance(row[0], str):
            bad("every layer of the right-hand side must be Dense")
        fin, fout, a, w_off, b_off = (int(v) for v in row[:5])
        if not 0 <= a < 8:
            bad("unknown activation")
        if fin != prev:
            bad("consecutive layer widths do not chain from d")
        if not 1 <= fout <= MAX_WIDTH:
            bad("layer widths must be 1 to %d" % MAX_WIDTH)
        if w_off < 0 or w_off + fin * fout > n or b_off < 0 or b_off + fout > n:
            bad("a layer's offset range falls outside [0, N)")
        prev = fout
    if prev != d:
        bad("the right-hand side must map d to d")
    ts = np.asarray(ts, dtype=np.float64).reshape(-1)
    if not 1 <= ts.size <= MAX_S:
        bad("the number of save times S must be 1 to %d" % MAX_S)
    if not (np.all(np.isfinite(ts)) and np.isfinite(opts.t0) and np.all(np.diff(ts) > 0.0) and ts[0] >= opts.t0):
        bad("the save times must be finite, strictly ascending and not before t0")
    if opts.pre_power not in (1, 3):
        bad("pre_power must be 1 or 3")
    if not 0 <= opts.max_steps <= MAX_STEPS_LIMIT:
        bad("max_steps must be 1 to %d (0: %d)" % (MAX_STEPS_LIMIT, MAX_STEPS_DEFAULT))
    if opts.adaptive:
        if not (np.isfinite(opts.reltol) and opts.reltol > 0.0 and np.isfinite(opts.abstol) and opts.abstol > 0.0):
            bad("reltol and abstol must be finite and positive in adaptive mode")
        if not (np.isfinite(opts.dt) and opts.dt >= 0.0):
            bad("dt must be finite and >= 0 (0: the starting-step rule)")
    elif not (np.isfinite(opts.dt) and opts.dt > 0.0):
        bad("dt must be finite and positive in fixed-step mode")


def group_lanes(table):
    """G of si_node_info: the lanes that share one trajectory -- the smallest power of two >= the widest layer, capped at 64"""
    g, widest = 1, max(int(row[1]) for row in table)
    while g < widest and g < 64:
        g *= 2
    return g


def rhs(table, w, u, pre_power=1, nudge=_same):
    """f(u) for the columns of u (d x n)"""
    a = (u * u) * u if pre_power == 3 else u
    for fin, fout, kind, w_off, b_off in (tuple(int(v) for v in row[:5]) for row in table):
        W = w[w_off:w_off + fin * fout].reshape((fout, fin), order="F")
        acc = np.zeros((fout, a.shape[1]))
        for i in range(fin):
            acc = acc + W[:, i:i + 1] * a[i:i + 1]
        acc = acc + w[b_off:b_off + fout][:, None]
        a = act(acc, kind, nudge)
    return a


def _comb(coefs, ks):
    """c_1 k_1 + c_2 k_2 + ..., terms ascending"""
    s = coefs[0] * ks[0]
    for c, k in zip(coefs[1:], ks[1:]):
        s = s + c * k
    return s


def _rms(v):
    """sqrt(mean_i v_i^2), the sum ascending from 0.0"""
    acc = np.zeros(v.shape[1])
    for i in range(v.shape[0]):
        acc = acc + v[i] * v[i]
    return np.sqrt(acc / v.shape[0])


@dataclass
class Solution:
    U: np.ndarray          # d*S x f in Y's layout (row i*S + s: state i at save time s); NaN where a failed trajectory saved nothing
    sse: np.ndarray        # f; +Inf for a failed trajectory (zeros without Y)
    naccept: np.ndarray    # f
    nreject: np.ndarray    # f
    status: np.ndarray     # f: 0 done, 1 max_steps reached, 2 non-finite state or error / t + h == t
    min_margin: float      # the smallest |err - 1| over all accept / reject decisions (inf in fixed-step mode)
    record: list = None    # solve(record=True): per trajectory its accepted steps (t_n, hs_n, h_n, u_n), see Steps


@dataclass
class Steps:
    """the accepted steps of one trajectory, the shortened last step included: step n starts at t[n] in u[:, n] and is hs[n] long.
    It ends at t[n + 1], the last one at tend.  h[n] is the controller's step before it was shortened to hs[n] (the device does
    not record it: only a mutant of tests/node_grad_cases.py reads it)."""
    t: np.ndarray
    hs: np.ndarray
    h: np.ndarray
    u: np.ndarray          # d x n
    status: int = 0        # the trajectory's status: the gradient is defined for 0 alone


def solve(table, w, u0, ts, opts, y=None, nudge=None, record=False):
    """all columns of u0 (d x f) through the right-hand side with the flat weights w"""
    nudge = nudge if nudge is not None else _same
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    u0 = np.asarray(u0, dtype=np.float64)
    u0 = u0.reshape(u0.shape[0], -1)
    ts = np.asarray(ts, dtype=np.float64).reshape(-1)
    d, f = u0.shape
    S = ts.size
    check(table, w.size, d, ts, opts)
    if y is not None:
        y = np.asarray(y, dtype=np.float64).reshape(d * S, f)
    tend = ts[-1]
    max_steps = opts.max_steps if opts.max_steps != 0 else MAX_STEPS_DEFAULT   # (0: the default, as si_infer_setup_node takes it)
    adaptive = bool(opts.adaptive)
    U = np.full((d * S, f), np.nan)
    sse = np.zeros(f)
    nacc, nrej, status = np.zeros(f, np.int64), np.zeros(f, np.int64), np.zeros(f, np.int64)
    snext = np.zeros(f, np.int64)
    min_margin = np.inf
    rows = np.arange(d) * S
    rec = [([], [], [], []) for _ in range(f)] if record else None

    def fn(u):
        return rhs(table, w, u, opts.pre_power, nudge)

    def save(p, s, us):
        U[rows + s, p] = us
        if y is not None:
            for i in range(d):
                r = us[i] - y[i * S + s, p]
                sse[p] = sse[p] + r * r

    with np.errstate(all="ignore"):
        t = np.full(f, float(opts.t0))
        u = u0.copy()
        k1 = fn(u)
        if ts[0] == opts.t0:
            for p in range(f):
                save(p, 0, u[:, p])
            snext[:] = 1
        done = snext >= S
        # ---- the starting step (Hairer, Norsett, Wanner II.4, order 5), or the caller's dt
        if adaptive and not opts.dt > 0.0:
            sk = opts.abstol + opts.reltol * np.abs(u)
            d0, d1 = _rms(u / sk), _rms(k1 / sk)
            h0 = np.where((d0 < 1e-5) | (d1 < 1e-5), 1e-6, 0.01 * (d0 / d1))
            h0 = np.minimum(h0, tend - t)
            f1 = fn(u + h0 * k1)
            d2 = _rms((f1 - k1) / sk) / h0
            dm = np.maximum(d1, d2)
            h1 = np.where(dm <= 1e-15, np.maximum(1e-6, h0 * 1e-3), nudge(np.power(0.01 / dm, 1.0 / 6.0)))
            h = np.minimum(100.0 * h0, h1)
        else:
            h = np.full(f, float(opts.dt))
        qold = np.full(f, QOLD0)
        bad0 = ~done & ~(np.isfinite(h) & np.all(np.isfinite(k1), axis=0))
        status[bad0] = 2
        live = ~done & ~bad0
        while np.any(live):
            out_of_steps = live & (nacc + nrej >= max_steps)
            status[out_of_steps] = 1
            live &= ~out_of_steps
            ix = np.flatnonzero(live)
            if ix.size == 0:
                break
            tt, uu, hh = t[ix], u[:, ix], h[ix]
            last = tt + hh >= tend
            hs = np.where(last, tend - tt, hh)
            stuck = tt + hs == tt
            ks = [k1[:, ix]]
            for i in range(1, 6):
                ks.append(fn(uu + hs * _comb(A[i], ks)))
            un = uu + hs * _comb(A[6], ks)
            ks.append(fn(un))
            fine = np.all(np.isfinite(un), axis=0) & ~stuck
            if adaptive:
                e = hs * _comb(BT, ks)
                err = _rms(e / (opts.abstol + opts.reltol * np.maximum(np.abs(uu), np.abs(un))))
                fine &= np.isfinite(err)
                accept = fine & (err <= 1.0)
                if np.any(fine):
                    min_margin = min(min_margin, float(np.min(np.abs(err[fine] - 1.0))))
                q11 = nudge(np.power(err, BETA1))
                q = np.maximum(QMAX_INV, np.minimum(QMIN_INV, (q11 / nudge(np.power(qold[ix], BETA2))) / GAMMA))
                hnew = np.where(accept, hs / q, hs / np.minimum(QMIN_INV, q11 / GAMMA))
                qnew = np.where(accept, np.maximum(err, 1e-4), qold[ix])
            else:
                accept, hnew, qnew = fine, hh, qold[ix]
            tn = np.where(last, tend, tt + hs)
            for j, p in enumerate(ix):
                if not fine[j]:
                    status[p] = 2
                    live[p] = False
                    continue
                if not accept[j]:
                    nrej[p] += 1
                    h[p] = hnew[j]
                    continue
                nacc[p] += 1
                if rec is not None:
                    for lst, v in zip(rec[p], (tt[j], hs[j], hh[j], uu[:, j].copy())):
                        lst.append(v)
                while snext[p] < S and ts[snext[p]] <= tn[j]:
                    s = snext[p]
                    if ts[s] == tn[j]:
                        us = un[:, j]
                    else:
                        bw = interp_weights((ts[s] - tt[j]) / hs[j])
                        us = uu[:, j] + hs[j] * _comb(bw, [k[:, j] for k in ks])
                    save(p, s, us)
                    snext[p] += 1
                t[p], u[:, p], k1[:, p], h[p], qold[p] = tn[j], un[:, j], ks[6][:, j], hnew[j], qnew[j]
                if snext[p] >= S:
                    live[p] = False
    sse[status != 0] = np.inf
    if y is None:
        sse[status == 0] = 0.0
    if rec is not None:
        rec = [Steps(np.array(r[0]), np.array(r[1]), np.array(r[2]), np.array(r[3]).reshape(-1, d).T, int(status[p]))
               for p, r in enumerate(rec)]
    return Solution(U, sse, nacc, nrej, status, min_margin, rec)


def sum_squares(w):
    """||w||^2 in the order of the device's two-stage reduction (csrc/kernels_stream.hip: one element per thread of 256-thread
    blocks, shuffle-down wave sums, (r0 + r1) + (r2 + r3), the block sums the same way); N <= 8192 is at most 32 blocks"""
    def wave(v):
        v = v.copy()
        for off in (32, 16, 8, 4, 2, 1):
            v[:off] = v[:off] + v[off:2 * off]
        return v[0]

    def block(v):
        r = [wave(v[64 * i:64 * i + 64]) for i in range(4)]
        return (r[0] + r[1]) + (r[2] + r[3])
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    if w.size > 256 * 256:
        raise SubspaceError("sum_squares restates the reduction for N <= 65536")
    nb = (w.size + 255) // 256
    sq = np.zeros(nb * 256)
    sq[:w.size] = w * w
    parts = np.zeros(256)
    for b in range(nb):
        parts[b] = block(sq[256 * b:256 * b + 256])
    return block(parts)


def sse_total(sse_p):
    """the per-trajectory sums in ascending p, from 0.0 (the reference's loop order)"""
    acc = 0.0
    for v in np.asarray(sse_p, dtype=np.float64).reshape(-1):
        acc = acc + v
    return acc


def logdensity(table, w, u0, y, ts, opts, nudge=None):
    """lp = -sum_p ||sol_p - Y_p||^2 - ||w||^2 (src/space_inference.jl:96-101; sigma_m and sigma_p are unused there too)"""
    sol = solve(table, w, u0, ts, opts, y=y, nudge=nudge)
    return (0.0 - (sse_total(sol.sse) / 0.5) / 2.0) + (0.0 - (sum_squares(w) / 0.5) / 2.0)


# ---- the gradient through the solver: the discrete adjoint of the integration above with its accepted steps frozen -----------------
# For a trajectory that ended with status 0 take its accepted steps (t_n, hs_n, u_n), the shortened last step included.  d lp / d W
# is the exact derivative of W -> -sum_s ||us_s - y_s||^2 built from those steps with hs_n and every theta_s = (ts_s - t_n) / hs_n
# held constant: rejected steps, the starting-step evaluations and the controller do not enter.  This is NOT what ForwardDiff gives
# through OrdinaryDiffEq in the reference, where the partials enter the error norm and move the steps [upstream, from memory,
# unverifiable offline]; the two agree to the order of the tolerance.  As everywhere in this file every product and sum is rounded on
# its own and the written order is the definition (csrc/kernels_node.hip: node_grad_kernel repeats it).
GRAD_MAX_WIDTH = 64        # si_node_set_grad: every lane of a group owns one unit per layer
MUTANTS = ("interp-k7-dropped", "k1-dropped", "h-for-hs", "theta-of-wrong-step", "cube-derivative-missing", "end-save-twice")


def dact(h, kind, nudge=_same):
    """act'(x) through the output h = act(x), as the Chain reverse sweep defines it (csrc/kernels_gemm.h: dact_full)"""
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
        return 1.0 - nudge(np.exp(-h))
    if kind == flux.selu:
        return np.where(h > 0.0, flux._SELU_L, h + flux._SELU_L * flux._SELU_A)
    raise SubspaceError("Error: activation %r is not available" % (kind,))


def _step_end(st, n, tend):
    return st.t[n + 1] if n + 1 < st.t.size else tend


def _stages(fn, u, hs):
    """the seven stage values of the step from u (d x 1) and its end state, as `solve` forms them; k_1 = f(u) is the FSAL value"""
    ks = [fn(u)]
    for i in range(1, 6):
        ks.append(fn(u + hs * _comb(A[i], ks)))
    un = u + hs * _comb(A[6], ks)
    ks.append(fn(un))
    return ks, un


def replay(table, w, u0, ts, opts, record, y=None, nudge=None):
    """the arithmetic of `solve` on the given steps: U and sse of `solve(..., record=True)` again, bit for bit.  Only t_n and hs_n are read:
    the state is carried from u0, so that this is the function of W whose derivative grad_w is (its u_n are the recorded ones
    at the recorded W).  A trajectory whose record is that of a failed integration keeps the saves of its steps and sse = +Inf."""
    nudge = nudge if nudge is not None else _same
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    u0 = np.asarray(u0, dtype=np.float64)
    u0 = u0.reshape(u0.shape[0], -1)
    ts = np.asarray(ts, dtype=np.float64).reshape(-1)
    d, f = u0.shape
    S = ts.size
    check(table, w.size, d, ts, opts)
    if y is not None:
        y = np.asarray(y, dtype=np.float64).reshape(d * S, f)
    tend = ts[-1]
    U = np.full((d * S, f), np.nan)
    sse = np.zeros(f)
    rows = np.arange(d) * S

    def fn(u):
        return rhs(table, w, u, opts.pre_power, nudge)

    def save(p, s, us):
        U[rows + s, p] = us
        if y is not None:
            for i in range(d):
                r = us[i] - y[i * S + s, p]
                sse[p] = sse[p] + r * r

    with np.errstate(all="ignore"):
        for p in range(f):
            st = record[p]
            s = 0
            if ts[0] == opts.t0:
                save(p, 0, u0[:, p])
                s = 1
            u = u0[:, p:p + 1]
            for n in range(st.t.size):
                t, hs = st.t[n], st.hs[n]
                ks, un = _stages(fn, u, hs)
                tn = _step_end(st, n, tend)
                while s < S and ts[s] <= tn:
                    if ts[s] == tn:
                        us = un[:, 0]
                    else:
                        bw = interp_weights((ts[s] - t) / hs)
                        us = (u + hs * _comb(bw, ks))[:, 0]
                    save(p, s, us)
                    s += 1
                u = un
            if st.status != 0:
                sse[p] = np.inf
    if y is None:
        sse[np.isfinite(sse)] = 0.0
    return U, sse


def _vjp(table, w, x, kbar, pre_power, gw, nudge, no_cube=False):
    """J_u' kbar of f at x (both d x 1); J_W' kbar is added into gw, one contribution per weight element"""
    a = (x * x) * x if pre_power == 3 else x
    rows = [tuple(int(v) for v in row[:5]) for row in table]
    outs = [a]
    for fin, fout, kind, w_off, b_off in rows:
        W = w[w_off:w_off + fin * fout].reshape((fout, fin), order="F")
        acc = np.zeros((fout, 1))
        for i in range(fin):
            acc = acc + W[:, i:i + 1] * a[i:i + 1]
        acc = acc + w[b_off:b_off + fout][:, None]
        a = act(acc, kind, nudge)
        outs.append(a)
    g = kbar
    for l in range(len(rows) - 1, -1, -1):
        fin, fout, kind, w_off, b_off = rows[l]
        W = w[w_off:w_off + fin * fout].reshape((fout, fin), order="F")
        delta = g * dact(outs[l + 1], kind, nudge)
        gw[b_off:b_off + fout] = gw[b_off:b_off + fout] + delta[:, 0]
        for i in range(fin):
            gw[w_off + fout * i:w_off + fout * (i + 1)] = gw[w_off + fout * i:w_off + fout * (i + 1)] + delta[:, 0] * outs[l][i, 0]
        g = np.zeros((fin, 1))
        for j in range(fout):                                  # the transposed product: the output index ascending, from 0.0
            g = g + W[j:j + 1, :].T * delta[j:j + 1]
    if pre_power == 3 and not no_cube:
        g = (3.0 * (x * x)) * g
    return g


def grad_slices(table, w, u0, ts, opts, y, record, nudge=None, mutant=None):
    """N x f: column p is d(-sse_p) / dW of trajectory p over its recorded steps, contributions added from 0.0 in sweep order (steps
    descending; within a step k_7, then the stages 6 .. 1).  A trajectory whose record carries status != 0 (a failed
    integration) gives NaN.  `mutant` (one of MUTANTS) breaks one rule, for the tests' catalogue."""
    nudge = nudge if nudge is not None else _same
    if mutant is not None and mutant not in MUTANTS:
        raise SubspaceError("unknown mutant %r" % (mutant,))
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    u0 = np.asarray(u0, dtype=np.float64)
    u0 = u0.reshape(u0.shape[0], -1)
    ts = np.asarray(ts, dtype=np.float64).reshape(-1)
    d, f = u0.shape
    S = ts.size
    check(table, w.size, d, ts, opts)
    y = np.asarray(y, dtype=np.float64).reshape(d * S, f)
    tend = ts[-1]
    out = np.zeros((w.size, f))

    def fn(u):
        return rhs(table, w, u, opts.pre_power, nudge)

    def vjp(x, kbar, gw):
        return _vjp(table, w, x, kbar, opts.pre_power, gw, nudge, no_cube=mutant == "cube-derivative-missing")

    with np.errstate(all="ignore"):
        for p in range(f):
            st = record[p]
            nsteps = st.t.size
            if st.status != 0:
                out[:, p] = np.nan
                continue
            gw = out[:, p]
            lam = np.zeros((d, 1))
            s = S - 1
            for n in range(nsteps - 1, -1, -1):
                t, hs, u = st.t[n], st.hs[n], st.u[:, n:n + 1]
                if mutant == "h-for-hs":
                    hs = st.h[n]
                ks, un = _stages(fn, u, hs)
                tn = _step_end(st, n, tend)
                ub = np.zeros((d, 1))
                kb = [np.zeros((d, 1)) for _ in range(7)]
                while s >= 0 and ts[s] > t:                    # 1. the saves of the step, descending
                    ys = y[np.arange(d) * S + s, p][:, None]
                    if ts[s] == tn:
                        r = -2.0 * (un - ys)
                        lam = lam + r
                        if mutant == "end-save-twice":
                            lam = lam + r
                    else:
                        bw = interp_weights((ts[s] - t) / hs)
                        us = u + hs * _comb(bw, ks)
                        if mutant == "theta-of-wrong-step":    # (measured from the start of step n + 1)
                            bw = interp_weights((ts[s] - tn) / hs)
                        r = -2.0 * (us - ys)
                        ub = ub + r
                        for j in range(6 if mutant == "interp-k7-dropped" else 7):
                            kb[j] = kb[j] + (hs * bw[j]) * r
                    s -= 1
                lam = lam + vjp(un, kb[6], gw)                 # 2. k_7 = f(u_{n+1})
                ub = ub + lam                                  # 3. u_{n+1} = u_n + hs sum_j a_7j k_j
                for j in range(6):
                    kb[j] = kb[j] + (hs * A[6][j]) * lam
                for i in range(5, 0, -1):                      # 4. the stages 6 .. 2
                    g = vjp(u + hs * _comb(A[i], ks), kb[i], gw)
                    ub = ub + g
                    for j in range(i):
                        kb[j] = kb[j] + (hs * A[i][j]) * g
                if mutant != "k1-dropped":                     # 5. k_1 = f(u_n)
                    ub = ub + vjp(u, kb[0], gw)
                lam = ub                                       # 6.
    return out


def grad_w(table, w, u0, ts, opts, y, record, nudge=None, mutant=None):
    """d(-sum_p sse_p) / dW: the trajectories' slices added in ascending p, from 0.0"""
    sl = grad_slices(table, w, u0, ts, opts, y, record, nudge=nudge, mutant=mutant)
    acc = np.zeros(sl.shape[0])
    with np.errstate(all="ignore"):
        for p in range(sl.shape[1]):
            acc = acc + sl[:, p]
    return acc


def logdensity_grad(table, w, u0, y, ts, opts, nudge=None):
    """(lp, d lp / dW): `logdensity`'s value; grad_w over the steps of that very integration, then -2 W (the prior term's gradient,
    g - w * 2 as launch_prior_grad forms it).  A failed trajectory: lp = -Inf and NaN in every component."""
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    sol = solve(table, w, u0, ts, opts, y=y, nudge=nudge, record=True)
    lp = (0.0 - (sse_total(sol.sse) / 0.5) / 2.0) + (0.0 - (sum_squares(w) / 0.5) / 2.0)
    if np.any(sol.status != 0):
        return lp, np.full(w.size, np.nan)
    return lp, grad_w(table, w, u0, ts, opts, y, sol.record, nudge=nudge) - w * 2.0


# ---- the training step of a NeuralODE (si_train_setup_node; flux.NodeSSE is the cost) ------------------------------------------------
# loss(W) = sum_{p in batch} ||sol_p(W) - Y_p||^2 + ||W||^2 / penalty_div: at one column and penalty_div = 100 the tutorial's
#     L1(m, x, y) = sum(abs2, m(vec(x)) .- reshape(y[:,1], :,2)') + sum(sqnorm, Flux.params(m))/100      (docs/src/node_example.md:272)
# The gradient is the frozen-step discrete adjoint above (grad_slices) -- NOT what Zygote gives through DiffEqFlux's NeuralODE, which
# differentiates with a continuous adjoint by default [upstream, from memory, unverifiable offline]: the two agree to the order of the
# tolerances, not to rounding.  `sum(sqnorm, params)` adds array by array in the reference; here ||W||^2 is sum_squares over the flat
# vector.  Only the printed loss depends on that order (the penalty's gradient is elementwise), and it is not reproduced.
def train_value_and_grad(table, w, u0_b, y_b, ts, opts, penalty_div, nudge=None):
    """(loss, g) of the batch columns u0_b (d x nb), y_b (d*S x nb) at the flat weights w; penalty_div None drops the penalty.
    Per weight element acc = the batch's slices added from 0.0 in batch order; g = (w * 2.0) / penalty_div - acc, or 0.0 - acc.
    A trajectory that ends with status != 0 raises (si_train_step: the step leaves the weights as they were)."""
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    sol = solve(table, w, u0_b, ts, opts, y=y_b, nudge=nudge, record=True)
    for p, st in enumerate(sol.status):
        if st != 0:
            raise SubspaceError("NeuralODE training: trajectory %d of the batch ended with status %d (1: max_steps reached, 2: a "
                                "non-finite state)" % (p, int(st)))
    sl = grad_slices(table, w, u0_b, ts, opts, y_b, sol.record, nudge=nudge)
    acc = np.zeros(w.size)
    for p in range(sl.shape[1]):
        acc = acc + sl[:, p]
    loss = sse_total(sol.sse)
    if penalty_div is None:
        return loss, 0.0 - acc
    return loss + sum_squares(w) / penalty_div, (w * 2.0) / penalty_div - acc
