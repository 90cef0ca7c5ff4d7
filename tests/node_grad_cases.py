"""The case lists of the gradient through the NeuralODE solver (si_node_set_grad; node.logdensity_grad is the definition), shared by
tests/test_node_grad_cpu.py (the definition alone) and tests/test_gpu_node_grad.py (the device) -- TEST INFRASTRUCTURE, no GPU needed.

Shapes are the smallest at which the reverse kernel can still go wrong, all with f <= 7, S <= 6 and at most 40 steps: widths 1,
3 -> 5 (two hidden layers of different width), 15 (G = 16 with an idle lane) and 64 (G = 64); d = 1 and d = 8; f = 1 and f that
are no multiple of 256 / G; S = 1 with ts[0] = t0 (the gradient is -2 W exactly); several save times inside one step, saves
exactly at step ends, a shortened last step; pre_power = 3; C = 4 over two passes of launches (d = 8, f = 7 and max_steps = 10^6
make the step record of one chain 560 MB, so the 2 GiB budget carries three chains per pass).

Three kinds of constants, all measured on the CPU on the definition alone (test_node_grad_cpu.py re-measures each and holds it
within 10 % above the fresh figure; everything is seeded, so the measurements are deterministic):

FD_TOL[name]   the bound on |grad_w . v - finite differences| for the case: 8 x FD_DISAGREEMENT[name], the disagreement of the two
               finest levels of the Richardson-extrapolated central differences of the replayed lp along v, in units of
               1 + |finite differences|.  That is the finite-difference reference's own error with a margin for its error constant.
GRAD_TOL       the bound on device gradients where a transcendental function is involved: the largest spread of gw (metric
               node_cases.spread) under node.Nudge at +-2 ulp over TRANS_CASES + ADAPTIVE_CASES, times 8.
"""
import functools

import numpy as np

from subspaceinference_jl_amd import node
from tests.node_cases import Case, I, R, T, SG, LR, E, SP, SE, problem, spread  # noqa: F401 (re-exported for the two test files)

EXACT_CASES = [
    Case("g-w1-d1-f1", 1, (1,), (R, I), 3, 1, 1, dt=0.13, seed=1),
    Case("g-3x5-cube", 2, (3, 5), (LR, R, I), 4, 3, 2, pre_power=3, dt=0.11, wscale=0.5, seed=2),
    Case("g-w15", 2, (15,), (R, I), 5, 5, 1, dt=0.07, t_first=0.11, seed=3),
    Case("g-w64", 2, (64,), (LR, I), 2, 7, 1, dt=0.2, seed=4),
    Case("g-d8", 8, (15,), (I, I), 3, 3, 3, dt=0.1, wscale=0.4, seed=5),
    Case("g-s1-at-t0", 2, (3,), (R, I), 1, 3, 2, t_last=0.0, seed=6),                       # nothing is integrated: gw = -2 W
    Case("g-saves-in-step", 2, (15,), (R, I), 6, 3, 2, pre_power=3, dt=0.5, wscale=0.5, seed=7),   # 0.2, 0.4 | 0.6, 0.8, 1.0 at the end
    Case("g-saves-at-ends", 2, (3,), (LR, I), 5, 3, 1, dt=0.25, seed=8),                    # every save exactly at a step end
    Case("g-one-step", 1, (3,), (LR, I), 5, 1, 1, dt=2.0, seed=9),                          # one shortened step, every save inside it
]
# d = 8, f = 7 and max_steps = 10^6: three chains per pass of launches under the budget, so C = 4 takes two passes
PASS_SPLIT = Case("g-pass-split", 8, (15,), (R, I), 2, 7, 4, dt=0.25, wscale=0.4, max_steps=1000000, seed=10)
TRANS_CASES = [Case("g-tr-%d" % a, 2, (15,), (a, I), 5, 3, 2, pre_power=1 + 2 * (a % 2), dt=0.1, seed=20 + a) for a in (T, SG, E, SP, SE)] + [
    Case("g-tr-deep", 3, (5, 3), (T, SG, I), 4, 5, 1, dt=0.1, seed=28)]
ADAPTIVE_CASES = [
    Case("g-ad-tanh-cube", 2, (15,), (T, I), 6, 7, 1, pre_power=3, adaptive=True, dt=0.0, reltol=1e-5, abstol=1e-7, seed=30),
    Case("g-ad-d1", 1, (3,), (T, I), 2, 5, 1, adaptive=True, dt=0.0, t_first=0.2, seed=31),
    Case("g-ad-relu", 2, (16,), (R, I), 5, 3, 2, adaptive=True, dt=0.0, seed=32),
    Case("g-ad-w64", 2, (64,), (SG, I), 3, 5, 1, adaptive=True, dt=0.0, reltol=1e-4, abstol=1e-6, seed=33),
]
ALL_CASES = EXACT_CASES + [PASS_SPLIT] + TRANS_CASES + ADAPTIVE_CASES
CASE_BY_NAME = {c.name: c for c in ALL_CASES}
# the samplers' problem: a certified adaptive tanh case whose trajectories all integrate around the chains' paths
SAMPLER = Case("g-sampler-tanh", 2, (3,), (T, I), 4, 3, 1, adaptive=True, dt=0.0, seed=10)
# ... and its fixed-step twin: no step decision, so device and definition take the same steps wherever a sampler's tree wanders
SAMPLER_FIXED = Case("g-sampler-fixed-tanh", 2, (3,), (T, I), 4, 3, 1, dt=0.1, seed=10)
MAX_STEPS_SEEN = 40

# ---- the measured constants (see the module's docstring) ---------------------------------------------------------------------------
# The central differences' steps h, h / 2, h / 4.  Where every activation is smooth the steps are large, so that the differences'
# truncation error (not their rounding error, eps / h) is what the extrapolation removes and what its levels disagree by.  relu,
# leakyrelu, elu and selu have a kink: lp is smooth only between kinks, so the steps are small enough that none is crossed and the
# differences are at their rounding error, which the disagreement of two levels measures just as well.
FD_LEVELS_SMOOTH, FD_LEVELS_KINKED = (4e-2, 2e-2, 1e-2), (4e-5, 2e-5, 1e-5)
FD_SEEDS = (0, 1)                     # the directions v
# (For the cases with a kink the figure is the differences' rounding noise: it is tied to the NumPy / libm build the suite is pinned
# to.  Another build may move it by more than the 10 % the CPU test allows above a fresh measurement; the constants are then
# re-measured, the bound's rule -- 8 x the disagreement -- stays.)
FD_DISAGREEMENT = {   # measured (fd_error's second value), rounded up in the third digit
    "g-w1-d1-f1": 1.02e-12, "g-3x5-cube": 9.30e-12, "g-w15": 1.05e-11, "g-w64": 6.68e-11, "g-d8": 6.18e-10, "g-s1-at-t0": 0.0,
    "g-saves-in-step": 6.65e-12, "g-saves-at-ends": 3.33e-12, "g-one-step": 4.03e-13, "g-pass-split": 8.85e-12,
    "g-tr-2": 8.18e-09, "g-tr-3": 1.45e-08, "g-tr-5": 5.54e-12, "g-tr-6": 2.24e-08, "g-tr-7": 6.62e-12, "g-tr-deep": 2.57e-09,
    "g-ad-tanh-cube": 7.86e-06, "g-ad-d1": 3.97e-08, "g-ad-relu": 5.39e-12, "g-ad-w64": 2.94e-11,
}
FD_TOL = {name: 8 * v for name, v in FD_DISAGREEMENT.items()}
MEASURED_GRAD_SPREAD = 4.0e-13        # measured 3.93e-13 (g-ad-w64; the fixed-step cases give 9e-15 at most)
GRAD_TOL = 8 * MEASURED_GRAD_SPREAD
MUTANT_FACTOR = 100.0                 # every mutant exceeds a case's FD_TOL by at least this factor on at least one case


def weights(case, c=0):
    pb = problem(case)
    return pb.weights(pb.z[:, c])


@functools.lru_cache(maxsize=None)
def recorded(case, c=0):
    """the definition's integration at column c with its step record"""
    pb = problem(case)
    return node.solve(pb.table, weights(case, c), pb.u0, pb.ts, case.opts(), y=pb.y, record=True)


def replayed_lp(case, w, record):
    """-sum_p sse_p over the frozen steps: the function grad_w differentiates"""
    pb = problem(case)
    return 0.0 - node.sse_total(node.replay(pb.table, w, pb.u0, pb.ts, case.opts(), record, y=pb.y)[1])


def direction(case, seed):
    v = np.random.default_rng(500 + seed).standard_normal(problem(case).n)
    return v / np.sqrt(v @ v)


def richardson(case, v, record):
    """d lp(w + h v) / dh at 0: central differences at h, h / 2, h / 4, extrapolated once (their h^2 term removed) at the two
    finest pairs -> (the finest extrapolated value, its disagreement with the coarser one)"""
    w = weights(case)
    levels = FD_LEVELS_KINKED if any(a in (R, LR, E, SE) for a in case.acts) else FD_LEVELS_SMOOTH
    d = [(replayed_lp(case, w + h * v, record) - replayed_lp(case, w - h * v, record)) / (2.0 * h) for h in levels]
    r = [(4.0 * d[i + 1] - d[i]) / 3.0 for i in range(2)]
    return r[1], abs(r[1] - r[0])


def fd_error(case, mutant=None):
    """(the largest |grad_w . v - fd| / (1 + |fd|) over the directions, the largest disagreement of the two finest levels likewise)"""
    pb = problem(case)
    sol = recorded(case)
    g = node.grad_w(pb.table, weights(case), pb.u0, pb.ts, case.opts(), pb.y, sol.record, mutant=mutant)
    err, dis = 0.0, 0.0
    for seed in FD_SEEDS:
        v = direction(case, seed)
        fd, d = richardson(case, v, sol.record)
        err = max(err, abs(g @ v - fd) / (1.0 + abs(fd)))
        dis = max(dis, d / (1.0 + abs(fd)))
    return err, dis


def definition(case, pb=None):
    """lp (C) and gw (N, C) of node.logdensity_grad at every column of the case's z"""
    pb = problem(case) if pb is None else pb
    out = [node.logdensity_grad(pb.table, pb.weights(pb.z[:, c]), pb.u0, pb.y, pb.ts, case.opts()) for c in range(case.C)]
    return np.array([o[0] for o in out]), np.stack([o[1] for o in out], axis=1)
