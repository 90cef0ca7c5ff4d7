"""Bit-for-bit audit of the `Flux.update!` stage (reference src/subspace_construction.jl:43, Flux 0.11.2 Descent / Momentum /
ADAM; the device's optimiser_kernel / train_apply in csrc/capi_train.hip) -- TEST INFRASTRUCTURE, no GPU needed.

Three parts:

  * `true_element`: the three rules restated ELEMENT BY ELEMENT on Python floats (IEEE doubles, no fused multiply-add, no
    vectorised NumPy cast), every store into a Float32 array rounded by `f32`, in both gradient forms (a Float64 gradient:
    x - step rounded once; a Float32 gradient, `g32`: the step rounded into the Float32 gradient array, then a Float32
    subtraction).  It shares no array code with oracle.subspace_oracle.apply_update, which it is held against.
  * `MUTANTS`: the near-miss rules -- every one a plausible refactor of the kernel that today's tolerance tests would pass -- in
    the same scalar style.  tests/test_optimiser_audit_cpu.py requires each of them to differ from the true rule in at least one
    bit on the input set; that is a condition on the inputs.
  * `inputs` / `specials`: the seeded input set.  Random data alone cannot tell most mutants from the rule: a difference in the
    last bits of a Float64 intermediate survives the rounding into Float32 once in 2^29 elements.  So the builder SEARCHES: the
    stored value is a monotone function of the injected gradient, `_split` bisects for the gradient at which the true rule and
    a mutant cross a Float32 rounding boundary at different places, and that element goes into the set ("trigger" elements,
    first in every array, so that even the smallest device problem holds some).

`same_bits` compares bit patterns (NaNs equal where both are NaN) and names the first differing element.
"""
import functools
import math
import struct
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

STEPS = 6
KINDS = ("descent", "momentum", "adam")
KIND_ID = {"descent": 0, "momentum": 1, "adam": 2}

# hyper-parameters: (eta,) | (eta, rho) | (eta, beta1, beta2)
HYPER = {
    "flux": {"descent": (0.1,), "momentum": (0.01, 0.9), "adam": (0.001, 0.9, 0.999)},          # Flux 0.11.2's defaults
    # tests/golden/make_golden.py trains with Flux's defaults for Momentum and ADAM; this set takes the values of the other device
    # training tests (tests/test_gpu_parity.py) where the fixture's coincide with the defaults
    "fixture": {"descent": (0.05,), "momentum": (0.05, 0.9), "adam": (0.01, 0.9, 0.999)},
    "dyadic": {"descent": (0.125,), "momentum": (0.125, 0.5), "adam": (0.125, 0.5, 0.75)},
}


def oracle_opt(kind, hp):
    return (kind,) + tuple(hp)


# ----------------------------------------------------------------------------------------------- scalar IEEE helpers
def f32(x):
    """round a double to the nearest Float32 (ties to even), returned as the double of that value"""
    try:
        return struct.unpack("<f", struct.pack("<f", x))[0]
    except OverflowError:
        return math.copysign(math.inf, x)


def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _sqrt(x):
    if x != x:
        return x
    return math.sqrt(x) if x >= 0.0 else math.nan


def fma(a, b, c):
    """a * b + c rounded ONCE: exact in rationals, then one rounding (int / int in CPython is correctly rounded)"""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:
        return a * b + c
    try:
        return r.numerator / r.denominator
    except OverflowError:
        return math.inf if r > 0 else -math.inf


def _ftz32(x):
    return math.copysign(0.0, x) if x != 0.0 and abs(x) < 2.0 ** -126 else x


def bits32(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def bits64(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _from_bits64(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def _from_bits32(b):
    return struct.unpack("<f", struct.pack("<I", b))[0]


# ----------------------------------------------------------------------------------------------- the rule
def _finish(w, step, g32):
    return f32(w - f32(step)) if g32 else f32(w - step)


def true_element(kind, hp, w, m, v, bp, g, g32):
    """One element of `x .-= apply!(opt, x, g)`; w, m, v: Float32 values held in doubles; returns the new (w, m, v)."""
    eta = hp[0]
    if kind == "descent":
        step = g * eta
    elif kind == "momentum":
        m = f32(hp[1] * m - eta * g)
        step = -m
    else:
        b1, b2 = hp[1], hp[2]
        m = f32(b1 * m + (1.0 - b1) * g)
        v = f32(b2 * v + (1.0 - b2) * (g * g))
        step = _div(_div(m, 1.0 - bp[0]), _sqrt(_div(v, 1.0 - bp[1])) + 1e-8) * eta
    return _finish(w, step, g32), m, v


def _bp0(kind, hp):
    return [hp[1], hp[2]] if kind == "adam" else None


def _bp_next(kind, hp, bp, t):
    return [bp[0] * hp[1], bp[1] * hp[2]] if kind == "adam" else None


@dataclass(frozen=True)
class Rule:
    name: str
    what: str
    kinds: tuple
    element: object = true_element
    bp0: object = _bp0
    bp_next: object = _bp_next


TRUE = Rule("true", "Flux 0.11.2", KINDS)


# ----------------------------------------------------------------------------------------------- the mutants
def _adam_state(hp, m, v, g):
    b1, b2 = hp[1], hp[2]
    return f32(b1 * m + (1.0 - b1) * g), f32(b2 * v + (1.0 - b2) * (g * g))


def _adam_step(hp, m, v, bp):
    return _div(_div(m, 1.0 - bp[0]), _sqrt(_div(v, 1.0 - bp[1])) + 1e-8) * hp[0]


def _m_eps_inside(kind, hp, w, m, v, bp, g, g32):
    m, v = _adam_state(hp, m, v, g)
    step = _div(_div(m, 1.0 - bp[0]), _sqrt(_div(v, 1.0 - bp[1]) + 1e-8)) * hp[0]
    return _finish(w, step, g32), m, v


def _m_eps_before_correction(kind, hp, w, m, v, bp, g, g32):
    m, v = _adam_state(hp, m, v, g)
    step = _div(_div(m, 1.0 - bp[0]), _div(_sqrt(v), _sqrt(1.0 - bp[1])) + 1e-8) * hp[0]
    return _finish(w, step, g32), m, v


def _m_adam_unrounded(kind, hp, w, m, v, bp, g, g32):
    b1, b2 = hp[1], hp[2]
    mu = b1 * m + (1.0 - b1) * g
    vu = b2 * v + (1.0 - b2) * (g * g)
    return _finish(w, _adam_step(hp, mu, vu, bp), g32), f32(mu), f32(vu)


def _m_eta_first(kind, hp, w, m, v, bp, g, g32):
    m, v = _adam_state(hp, m, v, g)
    step = _div(_div(hp[0] * m, 1.0 - bp[0]), _sqrt(_div(v, 1.0 - bp[1])) + 1e-8)
    return _finish(w, step, g32), m, v


def _adam_with(m_of, v_of):
    def element(kind, hp, w, m, v, bp, g, g32):
        b1, b2 = hp[1], hp[2]
        m, v = f32(m_of(b1, m, g)), f32(v_of(b2, v, g))
        return _finish(w, _adam_step(hp, m, v, bp), g32), m, v
    return element


def _m_plain(b1, m, g):
    return b1 * m + (1.0 - b1) * g


def _v_plain(b2, v, g):
    return b2 * v + (1.0 - b2) * (g * g)


def _m_momentum_unrounded(kind, hp, w, m, v, bp, g, g32):
    mu = hp[1] * m - hp[0] * g
    return _finish(w, -mu, g32), f32(mu), v


def _m_momentum_fma_state(kind, hp, w, m, v, bp, g, g32):
    m = f32(fma(hp[1], m, -(hp[0] * g)))
    return _finish(w, -m, g32), m, v


def _m_momentum_fma_grad(kind, hp, w, m, v, bp, g, g32):
    m = f32(fma(-hp[0], g, hp[1] * m))
    return _finish(w, -m, g32), m, v


def _m_descent_fma(kind, hp, w, m, v, bp, g, g32):
    if g32:
        return f32(w - f32(g * hp[0])), m, v
    return f32(fma(-g, hp[0], w)), m, v


def _m_adam_weight_fma(kind, hp, w, m, v, bp, g, g32):
    m, v = _adam_state(hp, m, v, g)
    if g32:
        return _finish(w, _adam_step(hp, m, v, bp), g32), m, v
    q = _div(_div(m, 1.0 - bp[0]), _sqrt(_div(v, 1.0 - bp[1])) + 1e-8)
    return f32(fma(-q, hp[0], w)), m, v


def _m_always_g32(kind, hp, w, m, v, bp, g, g32):
    return true_element(kind, hp, w, m, v, bp, g, True)


def _m_never_g32(kind, hp, w, m, v, bp, g, g32):
    return true_element(kind, hp, w, m, v, bp, g, False)


def _m_float32(kind, hp, w, m, v, bp, g, g32):
    """every operand and every operation in Float32 (of two Float32 operands, +, -, *, / and sqrt through a double and one more
    rounding give the correctly rounded Float32 result)"""
    h = [f32(p) for p in hp]
    g = f32(g)
    if kind == "descent":
        step = f32(g * h[0])
    elif kind == "momentum":
        m = f32(f32(h[1] * m) - f32(h[0] * g))
        step = -m
    else:
        one1, one2 = f32(1.0 - h[1]), f32(1.0 - h[2])
        m = f32(f32(h[1] * m) + f32(one1 * g))
        v = f32(f32(h[2] * v) + f32(one2 * f32(g * g)))
        c1, c2 = f32(1.0 - f32(bp[0])), f32(1.0 - f32(bp[1]))
        den = f32(f32(_sqrt(f32(_div(v, c2)))) + f32(1e-8))
        step = f32(f32(_div(f32(_div(m, c1)), den)) * h[0])
    return f32(w - step), m, v


def _m_descent_float32_product(kind, hp, w, m, v, bp, g, g32):
    return _finish(w, f32(g) * f32(hp[0]), g32), m, v


def _m_flush(kind, hp, w, m, v, bp, g, g32):
    w, m, v = true_element(kind, hp, w, m, v, bp, g, g32)
    return _ftz32(w), _ftz32(m), _ftz32(v)


A, M_, D = ("adam",), ("momentum",), ("descent",)
MUTANTS = [
    Rule("a-eps-inside-sqrt", "sqrt(v^ + eps)", A, _m_eps_inside),
    Rule("b-eps-before-bias-correction", "sqrt(vt) / sqrt(1 - bp2) + eps", A, _m_eps_before_correction),
    Rule("c-beta-powers-from-1", "beta powers start at 1", A, bp0=lambda kind, hp: [1.0, 1.0]),
    Rule("c-beta-powers-from-beta2", "beta powers start at beta^2", A, bp0=lambda kind, hp: [hp[1] * hp[1], hp[2] * hp[2]]),
    Rule("c-beta-powers-by-pow", "beta powers as beta ** t", A, bp_next=lambda kind, hp, bp, t: [hp[1] ** (t + 2), hp[2] ** (t + 2)]),
    Rule("d-step-from-unrounded-moments", "ADAM's step from the Float64 mt, vt", A, _m_adam_unrounded),
    Rule("e-eta-first", "eta * mt / (1 - bp1) / (...)", A, _m_eta_first),
    Rule("f-m-fma-state", "mt = fma(b1, mt, (1 - b1) g)", A, _adam_with(lambda b1, m, g: fma(b1, m, (1.0 - b1) * g), _v_plain)),
    Rule("f-m-fma-grad", "mt = fma(1 - b1, g, b1 mt)", A, _adam_with(lambda b1, m, g: fma(1.0 - b1, g, b1 * m), _v_plain)),
    Rule("f-v-fma-state", "vt = fma(b2, vt, (1 - b2) g^2)", A, _adam_with(_m_plain, lambda b2, v, g: fma(b2, v, (1.0 - b2) * (g * g)))),
    Rule("f-v-fma-grad", "vt = fma(1 - b2, g^2, b2 vt)", A, _adam_with(_m_plain, lambda b2, v, g: fma(1.0 - b2, g * g, b2 * v))),
    Rule("f-momentum-fma-state", "v = fma(rho, v, -(eta g))", M_, _m_momentum_fma_state),
    Rule("f-momentum-fma-grad", "v = fma(-eta, g, rho v)", M_, _m_momentum_fma_grad),
    Rule("f-descent-weight-fma", "x = fma(-g, eta, x)", D, _m_descent_fma),
    Rule("f-adam-weight-fma", "x = fma(-(mt / .. / ..), eta, x)", A, _m_adam_weight_fma),
    Rule("g-momentum-step-from-unrounded-velocity", "Momentum's step from the Float64 velocity", M_, _m_momentum_unrounded),
    Rule("h-g32-form-on-a-Float64-gradient", "step rounded to Float32 although g is Float64", KINDS, _m_always_g32),
    Rule("h-f64-form-on-a-Float32-gradient", "x - step rounded once although g is Float32", KINDS, _m_never_g32),
    Rule("i-float32-arithmetic", "every operation in Float32", KINDS, _m_float32),
    Rule("j-descent-float32-product", "float32(g) * float32(eta)", D, _m_descent_float32_product),
    Rule("k-flush-float32-subnormals", "subnormal w, m, v stored as zero", KINDS, _m_flush),
]
MUTANT_BY_NAME = {r.name: r for r in MUTANTS}


# ----------------------------------------------------------------------------------------------- running a rule
def run(rule, kind, hp, w0, grads, g32, state=None):
    """grads: steps x n.  Returns a list, one entry per step, of (w, m, v, bp): Float32 arrays and the beta powers AFTER that
    step.  state = (m, v, bp) to continue from, None = the fresh optimiser."""
    n = len(w0)
    w = [float(x) for x in w0]
    if state is None:
        m, v, bp = [0.0] * n, [0.0] * n, rule.bp0(kind, hp)
    else:
        m, v, bp = [float(x) for x in state[0]], [float(x) for x in state[1]], (list(state[2]) if state[2] is not None else None)
    out = []
    for t, gt in enumerate(grads):
        for i in range(n):
            w[i], m[i], v[i] = rule.element(kind, hp, w[i], m[i], v[i], bp, float(gt[i]), g32)
        bp = rule.bp_next(kind, hp, bp, t)
        out.append((np.array(w, dtype=np.float32), np.array(m, dtype=np.float32), np.array(v, dtype=np.float32),
                    None if bp is None else list(bp)))
    return out


def run_oracle(kind, hp, w0, grads, g32, state=None):
    """the same through oracle.subspace_oracle.apply_update (vectorised NumPy)"""
    from oracle import subspace_oracle as so
    opt = oracle_opt(kind, hp)
    w = np.array(w0, dtype=np.float32)
    if state is None:
        st = so.optimiser_state(w.size, opt)
    else:
        st = {"m": np.array(state[0], dtype=np.float32), "v": np.array(state[1], dtype=np.float32),
              "bp": None if state[2] is None else list(state[2])}
    out = []
    for gt in grads:
        g = np.asarray(gt, dtype=np.float64)
        so.apply_update(w, st, g.astype(np.float32) if g32 else g, opt)
        out.append((w.copy(), st["m"].copy(), st["v"].copy(), None if st["bp"] is None else list(st["bp"])))
    return out


# ----------------------------------------------------------------------------------------------- comparison
def _view(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return a.view(np.uint32)
    if a.dtype == np.float64:
        return a.view(np.uint64)
    raise TypeError("same_bits compares Float32 or Float64 arrays, got %s" % a.dtype)


def differing(got, want):
    """indices at which the bit patterns differ (two NaNs count as equal)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        raise AssertionError("dtype / shape: got %s %s, expected %s %s" % (got.dtype, got.shape, want.dtype, want.shape))
    ne = (_view(got) != _view(want)) & ~(np.isnan(got) & np.isnan(want))
    return np.flatnonzero(ne.reshape(-1))


def same_bits(got, want, what, **inputs):
    """assert bit identity; the message names the first differing index, both bit patterns and the inputs there
    (inputs: name = array of the same length, or a scalar)"""
    bad = differing(got, want)
    if bad.size == 0:
        return
    i = int(bad[0])
    g, w = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    width = 8 if g.dtype == np.float32 else 16
    at = []
    for k, a in inputs.items():
        a = np.asarray(a)
        x = a.reshape(-1)[i] if a.ndim and a.size == g.size else a
        at.append("%s = %r" % (k, x.tolist() if hasattr(x, "tolist") else x))
    raise AssertionError("%s: %d of %d elements differ, first at index %d: got %r (0x%0*x), expected %r (0x%0*x); %s" % (
        what, bad.size, g.size, i, g[i].item(), width, int(_view(g)[i]), w[i].item(), width, int(_view(w)[i]), ", ".join(at)))


def same_powers(got, want, what):
    if want is None:
        return
    same_bits(np.array(got, dtype=np.float64), np.array(want, dtype=np.float64), what)


# ----------------------------------------------------------------------------------------------- trigger search
def _ordered(x):
    """an integer that orders the doubles as the reals do"""
    b = bits64(x)
    return -(b & 0x7FFFFFFFFFFFFFFF) if b >> 63 else b


def _unordered(k):
    return _from_bits64(k) if k >= 0 else _from_bits64((-k) | (1 << 63))


def _ordered32(x):
    b = bits32(x)
    return -(b & 0x7FFFFFFF) if b >> 31 else b


def _unordered32(k):
    return _from_bits32(k) if k >= 0 else _from_bits32((-k) | (1 << 31))


def _first(f, y, lo, hi, up, single):
    """f monotone over the gradients lo..hi (ordered integers): the first gradient at which f has reached y"""
    dec = _unordered32 if single else _unordered
    reached = (lambda x: f(x) >= y) if up else (lambda x: f(x) <= y)
    if not reached(dec(hi)):
        return None
    while lo < hi:
        mid = (lo + hi) // 2
        if reached(dec(mid)):
            hi = mid
        else:
            lo = mid + 1
    return dec(lo)


def _split(f_true, f_mut, g_lo, g_hi, single, boundaries=16):
    """a gradient in [g_lo, g_hi] at which the two monotone Float32-valued functions differ, or None"""
    enc = _ordered32 if single else _ordered
    lo, hi = enc(g_lo), enc(g_hi)
    y0, y1 = f_true(g_lo), f_true(g_hi)
    if not (math.isfinite(y0) and math.isfinite(y1)) or y0 == y1:
        return None
    up = y1 > y0
    k = _ordered32(y0)
    for j in range(1, boundaries + 1):
        y = _unordered32(k + j if up else k - j)
        if (y >= y1) if up else (y <= y1):
            break
        a, b = _first(f_true, y, lo, hi, up, single), _first(f_mut, y, lo, hi, up, single)
        if a is not None and b is not None and a != b:
            g = min(a, b)
            if f_true(g) != f_mut(g):
                return g
    return None


def _cancelling(kind, hp, rule, g_lo, g_hi, trials=6000):
    """ADAM's Float64 step is a function of the stored Float32 (mt, vt) alone, so no gradient steers it onto a rounding boundary.
    Where a mutant moves the step by an ulp of Float64, a weight equal to the step's own leading 24 bits shows it: w - step then
    cancels to the step's low 29 bits, and one Float64 ulp of the step is 2^-5 of a Float32 ulp of the difference.  A few
    hundred gradients are enough to find one whose difference rounds the other way.  (Float64 form only: with a Float32
    gradient the step is rounded to Float32 first and the last bits of Float64 never reach the weight.)"""
    bp = _bp0(kind, hp)
    for j in range(trials):
        g = g_lo + (g_hi - g_lo) * ((j * 0.6180339887498949) % 1.0)
        w0 = f32(true_element(kind, hp, 0.0, 0.0, 0.0, bp, g, False)[0] * -1.0)
        if true_element(kind, hp, w0, 0.0, 0.0, bp, g, False)[0] != rule.element(kind, hp, w0, 0.0, 0.0, bp, g, False)[0]:
            return w0, g
    return None


# mutants that random data cannot tell from the rule.  (watched index into (w, m, v); the step at which the trigger fires; the
# window of gradients searched); watched None: the cancelling-weight search above
_WATCH = {
    "b-eps-before-bias-correction": (None, 0, (3e-7, 6e-7)),
    "e-eta-first": (None, 0, (3e-7, 6e-7)),
    "f-adam-weight-fma": (None, 0, (3e-7, 6e-7)),
    "f-m-fma-state": (1, 1, (1e-4, 2e-4)),
    "f-m-fma-grad": (1, 1, (0.25, 0.5)),
    "f-v-fma-state": (2, 1, (1e-3, 2e-3)),
    "f-v-fma-grad": (2, 1, (0.25, 0.5)),
    "f-momentum-fma-state": (1, 1, (1e-4, 2e-4)),
    "f-momentum-fma-grad": (1, 1, (0.25, 0.5)),
    "f-descent-weight-fma": (0, 0, (1e-3, 2e-3)),
}
_TRIGGER_W0 = {0: (0.7421875, 0.0), 1: (0.3,), 2: (0.3,)}
_WARM_G = (0.37, 0.41, 0.29, 0.53, 0.61, 0.23, 0.47, 0.19)   # gradients of the step before a trigger that fires at step 1: they leave a state to fuse with


@functools.lru_cache(maxsize=None)
def triggers(kind, hpname, g32):
    """[(mutant name, w0, [g_0 .. g_5])]: elements built so that the named mutant and the true rule part ways"""
    hp = HYPER[hpname][kind]
    out = []
    for rule in MUTANTS:
        if kind not in rule.kinds or rule.name not in _WATCH:
            continue
        watch, at, (g_lo, g_hi) = _WATCH[rule.name]
        if watch is None:
            hit = None if g32 else _cancelling(kind, hp, rule, g_lo, g_hi)
            if hit is not None:
                out.append((rule.name, hit[0], [hit[1], 0.5 * hit[1], -0.25 * hit[1], 0.0, hit[1], -hit[1]]))
            continue
        # (the products of one state with the gradients of one binade leave residues on a short lattice, the same at every
        # rounding boundary: where one warm-up state finds nothing, another does)
        for w0, warm in [(a, b) for b in _WARM_G for a in _TRIGGER_W0[watch]]:
            w, m, v, bp = f32(w0), 0.0, 0.0, _bp0(kind, hp)
            warm = f32(warm) if g32 else warm
            pre = []
            for t in range(at):
                w, m, v = true_element(kind, hp, w, m, v, bp, warm, g32)
                bp = _bp_next(kind, hp, bp, t)
                pre.append(warm)
            lo, hi = (f32(g_lo), f32(g_hi)) if g32 else (g_lo, g_hi)
            g = _split(lambda x: true_element(kind, hp, w, m, v, bp, x, g32)[watch],
                       lambda x: rule.element(kind, hp, w, m, v, bp, x, g32)[watch], lo, hi, g32)
            if g is not None:
                rest = [0.5 * g, -0.25 * g, 0.0, g, -g][: STEPS - at - 1]
                out.append((rule.name, w0, pre + [g] + rest))
                break
    return tuple(out)


# ----------------------------------------------------------------------------------------------- the input set
def _bulk(rng, n, hpname, g32):
    """w of magnitude 1e-6 .. 1 (log-uniform: a step of 1e-3 must meet weights of its own size, where the order of the roundings
    shows) with exact zeros and +-1; gradients of magnitude 1e-8 .. 1e3, both signs, one in sixteen an exact zero"""
    if hpname == "dyadic":
        w = rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(-20, 1, n) * rng.integers(1, 16, n) / 16.0
        g = rng.choice([-1.0, 1.0], (STEPS, n)) * 2.0 ** rng.integers(-26, 11, (STEPS, n))
    else:
        w = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6.0, 0.0, n)
        g = rng.choice([-1.0, 1.0], (STEPS, n)) * 10.0 ** rng.uniform(-8.0, 3.0, (STEPS, n))
    w[rng.random(n) < 1.0 / 16.0] = 0.0
    w[rng.random(n) < 1.0 / 32.0] = 1.0
    w[rng.random(n) < 1.0 / 32.0] = -1.0
    g[rng.random((STEPS, n)) < 1.0 / 16.0] = 0.0
    if g32:
        g = g.astype(np.float32).astype(np.float64)
    return w.astype(np.float32), g


def inputs(kind, hpname, g32, n, seed=0):
    """(w0 Float32[n], grads Float64[STEPS, n], names of the mutants whose trigger elements the set holds): trigger elements
    first, seeded bulk after them.  With g32 every gradient is Float32-representable."""
    rng = np.random.default_rng([seed, KIND_ID[kind], sorted(HYPER).index(hpname), int(g32)])
    w, g = _bulk(rng, n, hpname, g32)
    held = []
    for i, (name, w0, gs) in enumerate(triggers(kind, hpname, g32)[:n]):
        w[i] = w0
        g[:, i] = gs
        held.append(name)
    return w, g, held


def _solve(f, target, lo, hi):
    """f monotone over [lo, hi] (positive doubles): the gradient at which f first reaches the target, if it hits it exactly"""
    up = f(hi) > f(lo)
    g = _first(f, target, _ordered(lo), _ordered(hi), up, False)
    return g if g is not None and f(g) == target else None


@functools.lru_cache(maxsize=None)
def specials(kind, hpname, g32):
    """[(label, w0, [g_0 .. g_5])]: the gradients and states at which an implementation leaves IEEE behind first"""
    hp = HYPER[hpname][kind]
    eta = hp[0]
    rows = []
    tail = [0.3, -0.2, 0.0, 0.1, 0.05]
    for label, s in (("+0", 0.0), ("-0", -0.0), ("+inf", math.inf), ("-inf", -math.inf), ("nan", math.nan),
                     ("+1e200", 1e200), ("-1e200", -1e200), ("+1e-310", 1e-310), ("-1e-310", -1e-310)):
        rows.append(("g = " + label, 0.4375, [s] + tail))
        rows.append(("g = " + label + " at step 2", -0.8125, [0.3, -0.2, s, 0.1, 0.0, s]))
    # Float32-subnormal state: m near 1e-40 and v near 1e-42, then left to decay under zero gradients
    if kind == "momentum":
        rows.append(("velocity near 1e-40", 0.25, [1e-40 / eta, 0.0, 0.0, -3e-41 / eta, 0.0, 0.0]))
    if kind == "adam":
        gm = 1e-40 / (1.0 - hp[1])
        gv = math.sqrt(1e-42 / (1.0 - hp[2]))
        rows.append(("m near 1e-40", 0.25, [gm, 0.0, -0.5 * gm, 0.0, 0.0, gm]))
        rows.append(("v near 1e-42", 0.25, [gv, 0.0, -0.5 * gv, 0.0, 0.0, gv]))
        rows.append(("m near 1e-40, w = 0", 0.0, [-gm, 0.0, 0.0, gm, 0.0, 0.0]))
    # a subnormal weight and a subnormal step: the Float32 subtraction of the g32 form must not flush either
    if kind == "adam":   # (ADAM's step is eta m^ / (sqrt(v^) + eps): it is small only where m is next to the smallest Float32)
        rows.append(("subnormal weight", 1e-40, [0.0, 1.4e-44, 0.0, 0.0, -1.4e-44, 0.0]))
        rows.append(("weight lands in the subnormals", 2.0 ** -126, [0.0, 1.4e-44, 0.0, 0.0, 0.0, 0.0]))
    else:
        rows.append(("subnormal weight", 1e-40, [3e-40 / eta, -1e-40 / eta, 0.0, 2e-41 / eta, 0.0, -5e-40 / eta]))
        rows.append(("weight lands in the subnormals", 2.0 ** -126, [2.0 ** -127 / eta, 0.0, 0.0, 0.0, 0.0, 0.0]))
    # w - step exactly half way between two Float32: 1 - 2^-25 lies between 1 - 2^-24 (odd) and 1 (even)
    fresh = _bp0(kind, hp)
    pre = (lambda g: 1.0 - f32(true_step(kind, hp, g, fresh))) if g32 else (lambda g: 1.0 - true_step(kind, hp, g, fresh))
    tie = _solve(pre, 1.0 - 2.0 ** -25, 1e-16, 1e-3)
    if tie is not None and not g32:
        rows.append(("rounding tie", 1.0, [tie, 0.0, 0.0, 0.0, 0.0, 0.0]))
    if g32:   # the step is rounded first: a Float32 step of 2^-25 exactly
        tie = _first(lambda g: f32(true_step(kind, hp, g, fresh)), 2.0 ** -25, _ordered32(f32(1e-16)), _ordered32(f32(1e-3)), True, True)
        if tie is not None and f32(true_step(kind, hp, tie, fresh)) == 2.0 ** -25:
            rows.append(("rounding tie", 1.0, [tie, 0.0, 0.0, 0.0, 0.0, 0.0]))
    if g32:
        rows = [(label, w0, [f32(g) for g in gs]) for label, w0, gs in rows]
    return tuple(rows)


def true_step(kind, hp, g, bp):
    """the Float64 step of a FRESH state for the gradient g (what `apply!` returns before `x .-= step`)"""
    if kind == "descent":
        return g * hp[0]
    if kind == "momentum":
        return -f32(hp[1] * 0.0 - hp[0] * g)
    m, v = _adam_state(hp, 0.0, 0.0, g)
    return _adam_step(hp, m, v, bp)


def special_arrays(kind, hpname, g32):
    rows = specials(kind, hpname, g32)
    w = np.array([r[1] for r in rows], dtype=np.float32)
    g = np.array([r[2] for r in rows], dtype=np.float64).T.copy()
    return w, g, [r[0] for r in rows]
