"""The case lists of NeuralODE training (si_train_setup_node; node.train_value_and_grad is the definition of a step's loss and
gradient, tests/optimiser_audit.run_oracle of its update), shared by tests/test_node_train_cpu.py (the definition alone) and
tests/test_gpu_node_train.py (the device) -- TEST INFRASTRUCTURE, no GPU needed.

The problems are those of tests/node_grad_cases.py with the weights rounded to Float32 (the device keeps Float32 weights), the
smallest shapes at which the new code can go wrong: N = 4 (one trajectory, far below one block of the tail kernel), N = 77 (below
one block), N = 322 with G = 64 (two blocks of the tail kernel; four trajectories per workgroup of the solver, so a batch of 7
spans two workgroups), d = 8, two hidden layers behind the cube, several saves inside one step, one transcendental case and two
adaptive ones.  Every run takes STEPS = 4 steps, for Descent, Momentum and ADAM, with penalty_div 100.0 and without a penalty.

The batching patterns (together: one trajectory per step, a partial last batch smaller than batch_max, out-of-order indices):
  "one"       batchsize 1
  "three"     batchsize 3 in order: f = 7 gives batches of 3, 3, 1 (f = 5: 3, 2)
  "full"      batchsize f: the one batch the device uses in place
  "shuffled"  batchsize 3 (2 where f = 3) over a seeded permutation per epoch: the index path, a partial last batch
A run's four steps walk through as many epochs as they need.

`trace` is the definition's run; with `mutant` it breaks one rule (MUTANTS), for the catalogue that certifies that the device
tests' bit comparisons are not hollow: test_node_train_cpu.py requires every mutant to change a bit of the trace -- w, m, v after
a step, the step's gradient or its loss -- on at least one fixed-step case.
"""
import functools

import numpy as np

from subspaceinference_jl_amd import node
from tests import node_grad_cases as gc
from tests import optimiser_audit as oa

STEPS = 4
PENALTIES = (100.0, None)
KINDS = oa.KINDS
# steps small enough that four of them keep every case near the weights its parent case was certified at (the tutorial's ADAM(0.1)
# moves every weight by 0.1 per step: on these problems the adaptive cases' step decisions then come within 4e-4 of err = 1,
# measured on the definition).  ADAM(0.1) itself runs in the API tests.
HYPER = {"descent": (0.01,), "momentum": (0.005, 0.9), "adam": (0.01, 0.9, 0.999)}

FIXED = [("g-w1-d1-f1", "one"), ("g-w15", "one"), ("g-w15", "shuffled"), ("g-w64", "three"), ("g-w64", "full"), ("g-d8", "full"),
         ("g-d8", "shuffled"), ("g-3x5-cube", "one"), ("g-saves-in-step", "shuffled")]
AUDITED = [("g-tr-deep", "three"), ("g-tr-deep", "one"), ("g-ad-tanh-cube", "three"), ("g-ad-tanh-cube", "shuffled"),
           ("g-ad-relu", "full"), ("g-ad-relu", "one")]
MUTANTS = ("stale-float64-weights", "penalty-without-factor-2", "penalty-at-updated-weights", "last-trajectory-dropped",
           "batch-descending", "beta-powers-not-advanced", "loss-after-update")
# The spread (node_cases.spread) of the definition's training gradient under node.Nudge at +-2 ulp over every state of the AUDITED
# runs, measured by test_node_train_cpu.py::test_spread_of_the_training_gradient (seeded, so deterministic):
#   g-tr-deep 2.4e-15, g-ad-tanh-cube 2.66e-13: at or below node_grad_cases.MEASURED_GRAD_SPREAD (4.0e-13) -> they reuse GRAD_TOL;
#   g-ad-relu 4.31e-09, with identical step counts: above it.  An adaptive step size moves by 1e-9 of itself under the nudges (the
#   error estimate cancels: tests/node_cases.py), and relu's derivative jumps where a unit's stage argument changes sign, which
#   the rounded and then trained weights meet and the parent's unrounded ones did not.  Recorded as TRAIN_GRAD_SPREAD, bound 8 x it.
TRAIN_GRAD_SPREAD = 4.4e-09            # measured 4.31e-09 (g-ad-relu, "full", ADAM without a penalty, step 4)
GRAD_TOL = {"g-tr-deep": gc.GRAD_TOL, "g-ad-tanh-cube": gc.GRAD_TOL, "g-ad-relu": 8 * TRAIN_GRAD_SPREAD}


def case_of(name):
    return gc.CASE_BY_NAME[name]


def batch_size(case, pattern):
    return {"one": 1, "three": min(3, case.f), "full": case.f, "shuffled": 2 if case.f <= 3 else 3}[pattern]


@functools.lru_cache(maxsize=None)
def batches(name, pattern, steps=STEPS):
    """the index batches of the run's steps, epoch after epoch (int64 arrays)"""
    case = case_of(name)
    bs = batch_size(case, pattern)
    rng = np.random.default_rng(900 + case.seed)
    out = []
    while len(out) < steps:
        idx = rng.permutation(case.f) if pattern == "shuffled" else np.arange(case.f)
        out += [idx[i:i + bs].astype(np.int64) for i in range(0, case.f, bs)]
    return tuple(out[:steps])


def w0_of(name):
    return gc.weights(case_of(name)).astype(np.float32)


def value_and_grad(case, w, ids, penalty, mutant=None, nudge=None):
    """node.train_value_and_grad on the batch `ids`, restated so that a mutant can break one rule (no mutant: its bits, which
    test_node_train_cpu.py holds it to)"""
    pb = gc.problem(case)
    u0, y = pb.u0[:, ids], pb.y[:, ids]
    if mutant is None:
        return node.train_value_and_grad(pb.table, w, u0, y, pb.ts, case.opts(), penalty, nudge=nudge)
    w = np.asarray(w, dtype=np.float64)
    sol = node.solve(pb.table, w, u0, pb.ts, case.opts(), y=y, record=True)
    assert not sol.status.any()
    sl = node.grad_slices(pb.table, w, u0, pb.ts, case.opts(), y, sol.record)
    order = list(range(sl.shape[1]))
    if mutant == "last-trajectory-dropped":
        order = order[:-1]
    if mutant == "batch-descending":
        order = order[::-1]
    acc = np.zeros(w.size)
    for p in order:
        acc = acc + sl[:, p]
    loss = node.sse_total(sol.sse)
    if penalty is None:
        return loss, 0.0 - acc
    two = 1.0 if mutant == "penalty-without-factor-2" else 2.0
    return loss + node.sum_squares(w) / penalty, (w * two) / penalty - acc


@functools.lru_cache(maxsize=None)
def trace(name, pattern, kind, penalty, mutant=None):
    """the run's steps: a list of dicts with the batch `ids`, the weights `w_in` the step started from, its `loss` and gradient `g`,
    and w, m, v (Float32) and the beta powers `bp` after it"""
    case = case_of(name)
    hp = HYPER[kind]
    w32, state, out = w0_of(name), None, []
    prev_in = w32
    for k, ids in enumerate(batches(name, pattern)):
        w_in = w32
        w_solve = prev_in if mutant == "stale-float64-weights" else w_in
        inner = mutant if mutant in ("penalty-without-factor-2", "last-trajectory-dropped", "batch-descending") else None
        loss, g = value_and_grad(case, w_solve.astype(np.float64), ids, penalty, inner)
        if mutant == "penalty-at-updated-weights" and penalty is not None:
            # the update is applied with the penalty-free gradient first, and the penalty is then read from the new weights
            acc = (w_solve.astype(np.float64) * 2.0) / penalty - g
            w_new = oa.run_oracle(kind, hp, w_in, [0.0 - acc], False, state)[-1][0]
            g = (w_new.astype(np.float64) * 2.0) / penalty - acc
        if mutant == "beta-powers-not-advanced" and state is not None and state[2] is not None:
            state = (state[0], state[1], oa._bp0(kind, hp))
        w32, m, v, bp = oa.run_oracle(kind, hp, w_in, [g], False, state)[-1]
        if mutant == "loss-after-update":
            loss = value_and_grad(case, w32.astype(np.float64), ids, penalty)[0]
        state = (m, v, bp)
        out.append(dict(ids=ids, w_in=w_in, loss=loss, g=g, w=w32, m=m, v=v, bp=bp))
        prev_in = w_in
    return out


def same_trace(a, b):
    """bit equality of two traces in w, m, v, g and the loss"""
    return all(np.array_equal(x[k], y[k]) for x, y in zip(a, b) for k in ("w", "m", "v", "g")) and all(x["loss"] == y["loss"] for x, y in zip(a, b))
