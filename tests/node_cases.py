"""The NeuralODE case lists shared by tests/test_node_cpu.py (which certifies them on the definition alone) and
tests/test_gpu_node.py (which runs them on the device) -- TEST INFRASTRUCTURE, no GPU needed.

Shapes are the smallest at which the kernel can still go wrong: d in {1, 2, 3}; L in {1, 2, 3}; widths around the lane-group
edges {1, 3, 15, 16, 17, 65} (G = 1, 4, 16, 16, 32, 64 with a second round of output units at 65); S in {1, 2, 5, 30} with
ts[0] = t0, ts[0] > t0 and several save times inside one step; f in {1, 3, 64, 65} (a last workgroup partly filled);
C in {1, 2, 9}; both pre_power; all eight activations.

VALUE_TOL is the bound on device values where a transcendental function is involved (tanh / exp / log1p / pow differ from the
host's libm by a few ulp).  It is measured on the CPU, never on the code under test: the largest spread of the definition under
`node.Nudge` at +-2 ulp over TRANS_CASES + ADAPTIVE_CASES, in the metric `spread` below, times 8 -- the device's functions may
each be a few ulp from libm where the nudge moves one call by two.  Measured spread: 9.4e-11 (case ad-loose; the tutorial's
shape and tolerances give 1.7e-12, the fixed-step cases 5e-16), held here as 9.5e-11, so VALUE_TOL = 7.6e-10;
test_node_cpu.py::test_value_tolerance_is_the_measured_spread_times_eight re-measures it (the nudges are seeded, so the
measurement is deterministic) and holds the constant to it within its rounding.
The spread is far above a few ulp because the error estimate h * sum(b~_j k_j) cancels: where a step is much shorter than the
tolerance asks for (the first steps after the starting-step rule) its relative error is 1e-8, the controller passes a seventh
of that on to the next step size, and a solution that is only as accurate as a loose tolerance moves with its step sizes.
"""
import functools
from dataclasses import dataclass

import numpy as np

from subspaceinference_jl_amd import flux, node

I, R, T, SG, LR, E, SP, SE = flux.identity, flux.relu, flux.tanh, flux.sigmoid, flux.leakyrelu, flux.elu, flux.softplus, flux.selu

MEASURED_SPREAD = 9.5e-11
VALUE_TOL = 8 * MEASURED_SPREAD
MIN_MARGIN = 1e-3          # every accept / reject decision of a certified adaptive case has |err - 1| >= this


@dataclass(frozen=True)
class Case:
    name: str
    d: int
    hidden: tuple           # hidden widths: L = len(hidden) + 1
    acts: tuple             # one activation per layer
    S: int
    f: int
    C: int = 1
    pre_power: int = 1
    adaptive: bool = False
    dt: float = 0.07
    reltol: float = 1e-6
    abstol: float = 1e-8
    t0: float = 0.0
    t_first: float = 0.0    # ts[0]
    t_last: float = 1.0
    max_steps: int = 100000
    m: int = 2
    wscale: float = 0.8
    seed: int = 0

    def opts(self):
        return node.Opts(t0=self.t0, reltol=self.reltol, abstol=self.abstol, dt=self.dt, adaptive=1 if self.adaptive else 0,
                         max_steps=self.max_steps, pre_power=self.pre_power)

    def setup_kwargs(self):
        o = self.opts()
        return dict(t0=o.t0, reltol=o.reltol, abstol=o.abstol, dt=o.dt, adaptive=bool(o.adaptive), max_steps=o.max_steps, pre_power=o.pre_power)


@dataclass(frozen=True)
class Problem:
    table: list
    n: int
    w_swa: np.ndarray
    p: np.ndarray
    u0: np.ndarray
    y: np.ndarray
    ts: np.ndarray
    z: np.ndarray           # M x C: the points the case is evaluated at

    def weights(self, z):
        acc = np.zeros(self.n)    # W_swa + P z as K4 forms it: P z from 0.0 with the columns ascending, every product and sum rounded
        for j in range(self.p.shape[1]):
            acc = acc + self.p[:, j] * z[j]
        return self.w_swa + acc


@functools.lru_cache(maxsize=None)
def problem(case):
    rng = np.random.default_rng(1000 + case.seed + 7 * case.d + 13 * sum(case.hidden) + case.S + case.f)
    dims = (case.d,) + tuple(case.hidden) + (case.d,)
    table, off = [], 0
    w = []
    for l, (fin, fout) in enumerate(zip(dims[:-1], dims[1:])):
        table.append((fin, fout, case.acts[l], off, off + fin * fout))
        off += fin * fout + fout
        w += [case.wscale / np.sqrt(fin) * rng.standard_normal(fin * fout), 0.1 * rng.standard_normal(fout)]
    w_swa = np.concatenate(w)
    p = np.asfortranarray(0.05 * rng.standard_normal((off, case.m)))
    u0 = np.asfortranarray(rng.uniform(-1.0, 1.0, (case.d, case.f)))
    ts = np.linspace(case.t_first, case.t_last, case.S) if case.S > 1 else np.array([case.t_last])
    z = np.asfortranarray(0.5 * rng.standard_normal((case.m, case.C)))
    # the observations: the trajectories at W_swa plus noise, in fixed steps (cheap, and good enough for data)
    sol = node.solve(table, w_swa, u0, ts, node.Opts(t0=case.t0, adaptive=0, dt=0.05, pre_power=case.pre_power))
    y = np.asfortranarray(np.where(np.isfinite(sol.U), sol.U, 0.0) + 0.05 * rng.standard_normal(sol.U.shape))
    for a in (w_swa, p, u0, y, ts, z):
        a.setflags(write=False)
    return Problem(table, off, w_swa, p, u0, y, ts, z)


def spread(a, b):
    """the metric of VALUE_TOL: the largest |a - b| / (1 + |a|)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / (1.0 + np.abs(a)))) if a.size else 0.0


def _exact_cases():
    out = []
    # fixed steps, no transcendental function anywhere: the device result is the definition's, bit for bit
    for k, (d, hidden, acts) in enumerate([(1, (), (I,)), (2, (1,), (R, I)), (3, (3,), (LR, I)), (2, (15,), (R, I)), (2, (16,), (LR, R)),
                                           (3, (17,), (R, I)), (2, (65,), (R, I)), (2, (17, 3), (R, LR, I)), (1, (16, 15), (I, R, I))]):
        for pre in (1, 3):
            S = (1, 2, 5, 30)[(k + pre) % 4]
            f = (1, 3, 64, 65)[(k + 2 * pre) % 4]
            C = (1, 2, 9)[(k + pre) % 3]
            out.append(Case("ex-d%d-h%s-p%d" % (d, "x".join(map(str, hidden)) or "0", pre), d, hidden, acts, S, f, C, pre_power=pre,
                            t_first=0.0 if (k + pre) % 2 else 0.11, dt=0.07 if S != 30 else 0.13, seed=3 * k + pre,
                            wscale=0.8 if pre == 1 else 0.5))   # (the cube grows fast: smaller weights keep every trajectory finite)
    # many save times inside one step, and a step that ends exactly on a save time (dt = 0.25 hits t = 0.5 and 1.0)
    out.append(Case("ex-saves-in-step", 2, (15,), (R, I), 30, 3, 2, pre_power=3, dt=0.25))
    out.append(Case("ex-one-step", 2, (3,), (LR, I), 5, 3, 1, dt=2.0))
    return out


def _trans_cases():
    # fixed steps with the five transcendental activations: step counts and statuses equal, values within VALUE_TOL
    return [Case("tr-%d" % a, 2, (15,), (a, I), 5, 3, 2, pre_power=1 + 2 * (a % 2), seed=a) for a in (T, SG, E, SP, SE)] + [
        Case("tr-deep", 3, (17, 16), (T, SG, I), 5, 65, 1, seed=3)]


def _adaptive_cases():
    out = [Case("ad-tutorial", 2, (15,), (T, I), 30, 100, 1, pre_power=3, adaptive=True, dt=0.0, reltol=1e-7, abstol=1e-9, t_last=1.5, seed=1)]
    out.append(Case("ad-relu", 2, (16,), (R, I), 5, 3, 2, adaptive=True, dt=0.0, seed=20))
    out.append(Case("ad-d1", 1, (3,), (T, I), 2, 64, 1, adaptive=True, dt=0.0, t_first=0.2, seed=3))
    out.append(Case("ad-d3-wide", 3, (65,), (T, I), 5, 3, 9, adaptive=True, dt=0.0, reltol=1e-5, abstol=1e-7, seed=4))
    out.append(Case("ad-dt-given", 2, (15,), (SG, I), 30, 3, 1, pre_power=3, adaptive=True, dt=0.1, seed=5))
    out.append(Case("ad-loose", 2, (17,), (SE, I), 1, 65, 1, adaptive=True, dt=0.0, reltol=1e-3, abstol=1e-6, t_last=2.0, seed=6))
    return out


EXACT_CASES = _exact_cases()
TRANS_CASES = _trans_cases()
ADAPTIVE_CASES = _adaptive_cases()
ALL_CASES = EXACT_CASES + TRANS_CASES + ADAPTIVE_CASES
CASE_BY_NAME = {c.name: c for c in ALL_CASES}

# the failure paths: status 1 (max_steps = 50 at tolerances that ask for well over a hundred steps) and status 2 (a cube
# right-hand side with large weights blows up in finite time).  Neither is on the certified list: the tests hold their statuses,
# sums and densities to the definition, not their step counts.
FAIL_STEPS = Case("fail-max-steps", 2, (15,), (T, I), 5, 3, 2, pre_power=3, adaptive=True, dt=0.0, reltol=1e-12, abstol=1e-14, t_last=8.0, max_steps=50, seed=7)
FAIL_BLOWUP = Case("fail-blow-up", 1, (), (I,), 5, 3, 2, pre_power=3, adaptive=True, dt=0.0, t_last=50.0, wscale=40.0, seed=8)
# a chain that starts where every trajectory integrates and meets proposals that fail: du/dt = w u^3 + b with w = -0.5 + 3 z.
# For w > 0 the solution leaves every bound at t = 1 / (2 w u0^2): at u0 = 0.9 before t = 1 once z > 0.37, and the solver then
# runs into max_steps = 50 (status 1) or a non-finite state (status 2) on its way there.
FAIL_PROPOSAL = Case("fail-proposal", 1, (), (I,), 4, 3, 1, pre_power=3, adaptive=True, dt=0.0, max_steps=50, m=1)
FAIL_PROPOSAL_RWMH = dict(itr=40, sigma_z=0.35, seed=11, chain_id0=2)


@functools.lru_cache(maxsize=None)
def fail_proposal_problem():
    case = FAIL_PROPOSAL
    w_swa, p = np.array([-0.5, 0.0]), np.asfortranarray([[3.0], [0.0]])
    u0 = np.asfortranarray([[0.9, -0.8, 0.5]])
    ts = np.linspace(0.0, 1.0, case.S)
    table = [(1, 1, I, 0, 1)]
    sol = node.solve(table, w_swa, u0, ts, case.opts())
    y = np.asfortranarray(sol.U + 0.05 * np.random.default_rng(5).standard_normal(sol.U.shape))
    z = np.zeros((1, 1), order="F")
    for a in (w_swa, p, u0, y, ts, z):
        a.setflags(write=False)
    return Problem(table, 2, w_swa, p, u0, y, ts, z)

# the RWMH audit's problem (f = 3, S = 4, H = 3, fixed-step relu) and the adaptive tanh one
RWMH_FIXED = Case("rwmh-fixed-relu", 2, (3,), (R, I), 4, 3, 1, dt=0.1, seed=9)
RWMH_ADAPTIVE = Case("rwmh-adaptive-tanh", 2, (3,), (T, I), 4, 3, 1, adaptive=True, dt=0.0, seed=10)
RWMH = dict(itr=30, sigma_z=2.0, seed=11, chain_id0=2)


def definition_at(case, pb, z, nudge=None):
    """node.solve at W_swa + P z"""
    return node.solve(pb.table, pb.weights(z), pb.u0, pb.ts, case.opts(), y=pb.y, nudge=nudge)


def density(case, pb):
    def lp(z):
        return node.logdensity(pb.table, pb.weights(np.asarray(z, dtype=np.float64).reshape(-1)), pb.u0, pb.y, pb.ts, case.opts())
    return lp
