"""The optimiser audit (tests/optimiser_audit.py) on the host alone -- no GPU.

  * oracle.subspace_oracle.apply_update, the reference tests/test_gpu_optimiser_audit.py holds the device to, equals the scalar
    restatement of Flux 0.11.2's Descent / Momentum / ADAM bit for bit: three kinds, three hyper-parameter sets, both gradient
    forms, six consecutive steps from the fresh state and six more from the state they leave, and the special values;
  * every catalogued near-miss rule differs from the true rule in at least one bit of (w, m, v, beta powers) on that input set --
    a condition on the inputs: the audit can only catch on the device what its inputs can tell apart on the host;
  * the beta powers are the running product, at a t where beta ** (t + 1) is another number;
  * the device states the rule once (csrc/optimiser_update.h), and both kernels that apply it call that function.
"""
import functools
import math
import os
import re

import numpy as np
import pytest

from tests import optimiser_audit as oa

N_BULK = 320
FORMS = [False, True]
COMBOS = [(k, h, f) for k in oa.KINDS for h in oa.HYPER for f in FORMS]


def _id(c):
    return "%s-%s-%s" % (c[0], c[1], "g32" if c[2] else "g64")


@functools.lru_cache(maxsize=None)
def _set(kind, hpname, g32):
    """the whole input set of one combination: trigger elements, bulk, special rows -- (w0, grads, labels)"""
    w, g, held = oa.inputs(kind, hpname, g32, N_BULK)
    ws, gs, labels = oa.special_arrays(kind, hpname, g32)
    w, g = np.concatenate([w, ws]), np.concatenate([g, gs], axis=1)
    names = ["trigger " + h for h in held] + ["bulk"] * (N_BULK - len(held)) + labels
    w.setflags(write=False)
    g.setflags(write=False)
    return w, g, names


@functools.lru_cache(maxsize=None)
def _true_run(kind, hpname, g32):
    w, g, _ = _set(kind, hpname, g32)
    return oa.run(oa.TRUE, kind, oa.HYPER[hpname][kind], w, g, g32)


def _compare(kind, got, want, g, names, tag):
    for t, (a, b) in enumerate(zip(got, want)):
        for what, x, y in zip("wmv", a[:3], b[:3]):
            oa.same_bits(x, y, "%s, step %d, %s" % (tag, t, what), g=g[t], row=np.array(names, dtype=object))
        assert (a[3] is None) == (b[3] is None) == (kind != "adam")
        oa.same_powers(a[3], b[3], "%s, step %d, beta powers" % (tag, t))


@pytest.mark.parametrize("combo", COMBOS, ids=_id)
def test_apply_update_equals_the_scalar_restatement(combo):
    kind, hpname, g32 = combo
    hp = oa.HYPER[hpname][kind]
    w, g, names = _set(kind, hpname, g32)
    with np.errstate(all="ignore"):
        want = _true_run(kind, hpname, g32)
        got = oa.run_oracle(kind, hp, w, g, g32)
        _compare(kind, got, want, g, names, _id(combo) + " from the fresh state")
        # ... and from a state reached after six steps, with the gradients in another order
        state = want[-1][1:]
        g2 = g[::-1]
        _compare(kind, oa.run_oracle(kind, hp, want[-1][0], g2, g32, state), oa.run(oa.TRUE, kind, hp, want[-1][0], g2, g32, state), g2,
                 names, _id(combo) + " continued")
    # the set is what the builder promises
    nb = slice(0, N_BULK)
    assert np.any(w[nb] == 0.0) and np.abs(w[nb]).max() <= 1.0 and np.any(g[:, nb] == 0.0)
    assert np.any(g[:, nb] > 0.0) and np.any(g[:, nb] < 0.0)
    mag = np.abs(g[:, nb][g[:, nb] != 0.0])
    assert mag.min() < 1e-7 and mag.max() > 1e2
    if g32:
        assert np.array_equal(g.astype(np.float32).astype(np.float64), g, equal_nan=True)   # Float32-representable, every one


def _first_difference(rule, kind, hpname, g32):
    hp = oa.HYPER[hpname][kind]
    w, g, names = _set(kind, hpname, g32)
    mut = oa.run(rule, kind, hp, w, g, g32)
    for t, (a, b) in enumerate(zip(mut, _true_run(kind, hpname, g32))):
        for what, x, y in zip("wmv", a[:3], b[:3]):
            bad = oa.differing(x, y)
            if bad.size:
                i = int(bad[0])
                return "step %d, %s[%d] (%s): %r instead of %r, %d elements" % (t, what, i, names[i], x[i], y[i], bad.size)
        if a[3] is not None and oa.differing(np.array(a[3]), np.array(b[3])).size:
            return "step %d, beta powers %r instead of %r" % (t, a[3], b[3])
    return None


@pytest.mark.parametrize("rule", oa.MUTANTS, ids=lambda r: r.name)
def test_every_mutant_differs_from_the_rule(rule):
    """within six steps on the input set; the Float64 form is tried first, every combination that tells the mutant apart is listed"""
    found = []
    with np.errstate(all="ignore"):
        for kind, hpname, g32 in COMBOS:
            if kind in rule.kinds:
                d = _first_difference(rule, kind, hpname, g32)
                if d:
                    found.append("%s: %s" % (_id((kind, hpname, g32)), d))
    print("%s (%s): distinguished in %d combinations" % (rule.name, rule.what, len(found)))
    for line in found:
        print("   " + line)
    assert found, "%s (%s) is bit-identical to the true rule on the whole input set: extend the builder" % (rule.name, rule.what)
    # a mutant of the Float64 path must show in the Float64 form, which is where the device audit looks for it
    if rule.name != "h-f64-form-on-a-Float32-gradient":
        assert any("-g64:" in line for line in found), found


def test_the_trigger_elements_are_there():
    """every mutant that random data cannot tell from the rule has an element built for it, in the Float64 form of both
    non-dyadic sets (products with dyadic hyper-parameters are exact: nothing to fuse)"""
    for kind in oa.KINDS:
        need = {n for n in oa._WATCH if kind in oa.MUTANT_BY_NAME[n].kinds}
        for hpname in ("flux", "fixture"):
            assert {t[0] for t in oa.triggers(kind, hpname, False)} == need, (kind, hpname)


def test_the_special_rows_reach_what_they_name():
    with np.errstate(all="ignore"):
        for kind, hpname, g32 in COMBOS:
            w, g, names = _set(kind, hpname, g32)
            out = _true_run(kind, hpname, g32)
            sub = lambda a: (a != 0.0) & (np.abs(a) < 2.0 ** -126)
            ws, ms, vs = (np.stack([o[j] for o in out]) for j in range(3))
            assert np.any(sub(ws)), _id((kind, hpname, g32))                       # a subnormal weight is stored
            assert np.any(np.isnan(ws)) and np.any(np.isinf(ws) | np.isnan(ws))
            if kind != "descent":
                assert np.any(sub(ms)) and np.any(np.isinf(ms))                    # m near 1e-40; the Float32 store overflows
                i = names.index("velocity near 1e-40" if kind == "momentum" else "m near 1e-40")
                assert 5e-41 < abs(ms[0, i]) < 2e-40
            if kind == "adam":
                i = names.index("v near 1e-42")
                assert 5e-43 < vs[0, i] < 2e-42 and np.any(np.isinf(vs))
            if kind != "adam":   # (ADAM's Float64 step is a function of the Float32 moments alone: it cannot be steered onto a tie)
                i = names.index("rounding tie")
                hp = oa.HYPER[hpname][kind]
                step = oa.true_step(kind, hp, float(g[0, i]), None)
                half_way = oa.f32(step) == 2.0 ** -25 if g32 else 1.0 - step == 1.0 - 2.0 ** -25   # (1 - step: a Float64, no rounding yet)
                assert w[i] == 1.0 and half_way and ws[0, i] == 1.0                                  # ties to even: 1.0


def test_the_dyadic_first_step_has_an_exact_square_root():
    hp = oa.HYPER["dyadic"]["adam"]
    for g32 in FORMS:
        w, g, _ = oa.inputs("adam", "dyadic", g32, N_BULK)
        _, m, v, _ = oa.run(oa.TRUE, "adam", hp, w, g[:1], g32)[0]
        for gi, vi in zip(g[0], v):
            vhat = float(vi) / (1.0 - hp[2])
            assert vhat == gi * gi and math.sqrt(vhat) == abs(gi)


def test_beta_powers_are_the_running_product():
    for beta in (0.9, 0.999, 0.75):
        prod, ts = beta, []
        for t in range(1, 2001):       # after t applies the power is beta^(t + 1), multiplied up one factor at a time
            prod *= beta
            if prod != beta ** (t + 1):
                ts.append(t)
        if beta == 0.75:
            assert not ts or ts[0] > 6   # (dyadic: exact while the product fits 53 bits)
            continue
        assert ts, "beta = %r: the running product equals beta ** (t + 1) up to t = 2000" % beta
    t = 12   # (the fixture's length)
    hp = oa.HYPER["flux"]["adam"]
    g = np.zeros((t, 2))
    bp_scalar = oa.run(oa.TRUE, "adam", hp, np.zeros(2, np.float32), g, False)[-1][3]
    bp_oracle = oa.run_oracle("adam", hp, np.zeros(2, np.float32), g, False)[-1][3]
    want = [hp[1], hp[2]]
    for _ in range(t):
        want = [want[0] * hp[1], want[1] * hp[2]]
    oa.same_powers(bp_scalar, want, "scalar restatement")
    oa.same_powers(bp_oracle, want, "apply_update")
    assert want[0] != hp[1] ** (t + 1) or want[1] != hp[2] ** (t + 1), "t = %d does not tell pow from the running product" % t


def test_the_update_rule_is_written_once():
    """csrc/optimiser_update.h holds the Descent / Momentum / ADAM arithmetic, with its own contraction pragma; optimiser_kernel and
    the NeuralODE step's tail kernel call it, and no other file of csrc/ states the ADAM or the Momentum step"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "subspaceinference.jl_amd", "csrc")
    text = {f: re.sub(r"\s+", " ", open(os.path.join(csrc, f)).read()) for f in sorted(os.listdir(csrc))
            if os.path.isfile(os.path.join(csrc, f))}
    for expr in ("/ (1.0 - bp1) / (sqrt(", "(float)(p1 * (double)m[i] - eta * gi)"):
        assert {f: t.count(expr) for f, t in text.items() if expr in t} == {"optimiser_update.h": 1}, expr
    rule = text["optimiser_update.h"]
    body = rule[rule.index("float optimiser_update("):]
    assert body[body.index("{"):].startswith("{ #pragma clang fp contract(off) ")
    for f, kernel, call in (("capi_train.hip", "void optimiser_kernel(", "optimiser_update(w, m, v, i, g[i], "),
                            ("kernels_node_train.hip", "void node_train_tail_kernel(", "a.w64[i] = (double)optimiser_update(a.w32, ")):
        raw = open(os.path.join(csrc, f)).read()
        assert '#include "optimiser_update.h"' in raw
        body = raw[raw.index(kernel):]
        assert call in body[:body.index("\n}\n")], f        # (up to the closing brace of the kernel)


def test_same_bits_names_the_first_difference():
    a = np.array([1.0, np.nan, -0.0, 3.0], dtype=np.float32)
    b = a.copy()
    b[1] = np.float32(np.nan)
    oa.same_bits(a, b, "equal")                                            # NaN against NaN
    b[2] = 0.0                                                             # -0 against +0: other bits
    b[3] = np.nextafter(np.float32(3.0), np.float32(4.0))
    with pytest.raises(AssertionError, match=r"2 of 4 elements differ, first at index 2: got -0.0 \(0x80000000\), expected 0.0 \(0x00000000\); g = 7.0"):
        oa.same_bits(a, b, "w", g=np.array([5.0, 6.0, 7.0, 8.0]))
    with pytest.raises(AssertionError, match="0x3ff0000000000001"):
        oa.same_bits(np.array([1.0]), np.array([np.nextafter(1.0, 2.0)]), "bp")
    with pytest.raises(AssertionError, match="first at index 0"):
        oa.same_bits(np.array([np.nan], dtype=np.float32), np.array([1.0], dtype=np.float32), "nan against a number")
