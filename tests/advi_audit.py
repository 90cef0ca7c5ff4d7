"""Per-update audit of a finished ADVI trace (reference src/space_inference.jl:126-138; the step of si_fit_advi, whose contract is
the header comment in include/subspace_hip.h, restated on the build's Philox stream, oracle/philox.py) -- TEST INFRASTRUCTURE, no
GPU needed.  The manner of tests/mala_audit.py: the audit takes the trace's OWN theta_t and points as given and checks every step
by itself, so that one ulp of libm difference in exp cannot compound over the fit.  With theta = [mu; omega], sigma = exp(omega),
nblk = ceil(M / 2), eta_k the M normals of (chain, purpose 3, step t, blocks k nblk ..) and (lp_k, g_k) the ORACLE's value and
gradient at the trace's own points[:, k, t]:

  theta_0   within 16 2^-53 sigma_z |n| of sigma_z n, n = the 2M normals of (purpose 2, step 0)
  points    |points[m, k, t] - (mu + sigma eta_k)[m]| <= 16 2^-53 (|mu| + sigma |eta_k|) + 4 2^-52 sigma |eta_k|
            (rwmh_audit's 16 ulp for the normals and the two roundings; exp: 3 ulp on the device by the OpenCL fp64 limit, 1 ulp
            for the host libm)
  update    dmu = -(sum_k g_k) / S, domega = -(sum_k g_k eta_k sigma) / S - 1, s = the sum of d^2 over the last W steps, all from
            the oracle.  theta_{t+1} - theta_t must equal -d eta_opt / (tau + sqrt(s)) within the first-order effect of the
            project's stated gradient tolerances: with e_k = g_rtol |g_k| + g_atol max|g_k|,
              delta_dmu = sum_k e_k / S,  delta_domega = sum_k e_k |eta_k| sigma / S + 20 2^-52 sum_k |g_k eta_k sigma| / S
              (the second term: eta and sigma as the device has them), both + 16 2^-53 (sum_k |term_k| / S + 1) for the roundings;
              delta_s = sum over the window of 2 |d| delta_d + delta_d^2;  delta_sqrt = min(delta_s / (2 sqrt s), sqrt(delta_s));
              tol = c delta_d + |d| c delta_sqrt / (tau + sqrt s) + 16 2^-53 (|theta_t| + |d| c),  c = eta_opt / (tau + sqrt s)
            -- nothing is taken from the device
  elbo_t    within lp_rtol (relative) of ((lp_0 / S + H) + lp_1 / S + ...), H = M (log 2 pi + 1) / 2 + sum_m omega_m
  final     theta equals the last trace column bit for bit
  draws     Z[:, i] within the points' bound of mu_T + exp(omega_T) n_i, n_i = the M normals of (purpose 4, step i)

oracle_trace(case) is the Philox-driven host ADVI; MUTANTS names the wrong kernels it can imitate.  The audit must reject each on at
least one case (tests/test_advi_audit_cpu.py) -- except ring_slot_next: writing d^2 to slot (t + 1) mod W and summing all W slots
adds the SAME W values in another order, so no tolerance can tell it from the definition; what tells it is the bit-for-bit
restatement of the update (mu_replay below, which tests/test_gpu_advi.py holds on the device's traces), and the CPU test demands
that instead.  CASES is certified there on the oracle alone.
"""
import functools
from dataclasses import dataclass

import numpy as np

from oracle import philox
from oracle import subspace_oracle as so
from tests import mala_audit as ma
from tests.rwmh_audit import EPS, Z_ULPS, AuditFailure, _bits, _same_bits

LP_RTOL_F64, LP_RTOL_F32 = ma.LP_RTOL_F64, ma.LP_RTOL_F32
G_RTOL_F64, G_ATOL_F64 = ma.G_RTOL_F64, ma.G_ATOL_F64
G_RTOL_F32, G_ATOL_F32 = ma.G_RTOL_F32, ma.G_ATOL_F32
EXP_ULPS = 4.0                      # device exp within 3 ulp (OpenCL fp64), host libm within 1
LOG_2PI = 1.8378770664093453        # the literal of kernels_advi.hip
P_INIT, P_STEP, P_DRAW = 2, 3, 4    # Philox purposes (0 and 1 are RWMH's and MALA's)


def normals(seed, chain, step, purpose, block0, nblk):
    """the 2 nblk normals of blocks block0 .. block0 + nblk - 1 of (chain, step, purpose): block j gives components 2j, 2j + 1"""
    ctr = np.stack([philox._ctr(step, chain, purpose, block0 + j) for j in range(nblk)])
    x = philox.philox4x32(ctr, np.broadcast_to(philox._key(seed), (nblk, 2)))
    u1, u2 = philox._u53(x[:, 1], x[:, 0]), philox._u53(x[:, 3], x[:, 2])
    r = np.sqrt(-2.0 * np.log(u1))
    t = (2.0 * np.pi) * u2
    out = np.empty(2 * nblk)
    out[0::2] = r * np.cos(t)
    out[1::2] = r * np.sin(t)
    return out


def step_normals(seed, chain, t, m, s, purpose=P_STEP):
    """eta[:, k] for k = 0 .. S-1 (M x S)"""
    nblk = (m + 1) // 2
    return np.stack([normals(seed, chain, t, purpose, k * nblk, nblk)[:m] for k in range(s)], axis=1)


def sum_omega(om):
    """sum_m omega_m in the kernel's order: thread i of 256 adds its components 2j, 2j + 1 for j = i, i + 256, ...; every wave of 64
    folds its upper half onto its lower (32, 16, 8, 4, 2, 1); the four wave sums are added as (r0 + r1) + (r2 + r3)"""
    m = om.size
    nblk = (m + 1) // 2
    part = np.zeros(256)
    for i in range(min(256, nblk)):
        acc = 0.0
        for j in range(i, nblk, 256):
            for c in (0, 1):
                if 2 * j + c < m:
                    acc = acc + float(om[2 * j + c])
        part[i] = acc
    r = []
    for w in range(4):
        v = part[64 * w:64 * w + 64].copy()
        for h in (32, 16, 8, 4, 2, 1):
            v = v[:h] + v[h:2 * h]
        r.append(float(v[0]))
    return (r[0] + r[1]) + (r[2] + r[3])


def entropy(om):
    return (om.size * (LOG_2PI + 1.0)) / 2.0 + sum_omega(om)


def elbo_of(lp, h):
    """(((lp_0 / S + H) + lp_1 / S) + ...) + lp_{S-1} / S"""
    s = float(len(lp))
    e = float(lp[0]) / s + h
    for k in range(1, len(lp)):
        e = e + float(lp[k]) / s
    return e


class Ring:
    """TruncatedADAGrad's window as the kernel keeps it: slot t mod W of every component holds d^2, s is the sum of the W slots in
    slot order from 0.0, unwritten slots are 0; step(t, d) returns d (eta_opt / (tau + sqrt(s))).  Only +, *, / and sqrt: the host's
    bits are the device's."""

    def __init__(self, ncomp, w, eta_opt, tau, mutant=None):
        self.slots, self.w, self.eta, self.tau, self.mutant = np.zeros((w, ncomp)), w, eta_opt, tau, mutant
        self.total = np.zeros(ncomp)

    def step(self, t, d):
        slot = ((t + 1) if self.mutant == "ring_slot_next" else t) % self.w
        d2 = d * d
        if self.mutant == "s_without_current":
            s = self._sum()
            self.slots[slot] = d2
        else:
            self.slots[slot] = d2
            s = self._sum()
        if self.mutant == "ring_never_wraps":
            self.total = self.total + d2
            s = self.total
        root = s if self.mutant == "no_sqrt" else np.sqrt(s)
        return d * (self.eta / (self.tau + root))

    def _sum(self):
        s = np.zeros(self.slots.shape[1])
        for w in range(self.w):
            s = s + self.slots[w]
        return s


def grad_mu(g, s):
    """dmu = -(sum_k g_k) / S, k ascending from 0.0 (g: M x S)"""
    acc = np.zeros(g.shape[0])
    for k in range(g.shape[1]):
        acc = acc + g[:, k]
    return -(acc / float(s))


def grad_omega(g, eta, sigma, s):
    acc = np.zeros(g.shape[0])
    for k in range(g.shape[1]):
        acc = acc + (g[:, k] * eta[:, k]) * sigma
    return -(acc / float(s)) - 1.0


def mu_replay(theta_trace, lp_g_of_step, s, w, eta_opt, tau, mutant=None):
    """the mu half of every theta_{t+1} of one run (2M x (T+1)) from theta_t and the step's gradients g (M x S), bit for bit: dmu, the
    ring, s and the update use only +, *, / and sqrt.  lp_g_of_step(t) -> (lp[S], g[M, S]) as the update kernel was given them.
    Raises AuditFailure at the first step whose bits differ."""
    m = theta_trace.shape[0] // 2
    ring = Ring(m, w, eta_opt, tau, mutant)
    for t in range(theta_trace.shape[1] - 1):
        _, g = lp_g_of_step(t)
        want = theta_trace[:m, t] - ring.step(t, grad_mu(g, s))
        if not _same_bits(want, theta_trace[:m, t + 1]):
            i = int(np.flatnonzero(_bits(want) != _bits(theta_trace[:m, t + 1]))[0])
            raise AuditFailure("step %d: mu[%d] is %r, the restated update gives %r" % (t, i, theta_trace[i, t + 1], want[i]))


# ----------------------------------------------------------------------------------------------- the audit
@dataclass
class Report:
    steps: int = 0
    worst_theta0_ratio: float = 0.0
    worst_point_ratio: float = 0.0
    worst_update_ratio: float = 0.0
    worst_elbo_rel: float = 0.0
    worst_draw_ratio: float = 0.0

    def line(self):
        return "steps %d, worst ratios: theta_0 %.3f, points %.3f, update %.3g, draws %.3f; worst elbo rel %.2e" % (
            self.steps, self.worst_theta0_ratio, self.worst_point_ratio, self.worst_update_ratio, self.worst_draw_ratio, self.worst_elbo_rel)


def _ratio(err, bound):
    return float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0.0))) if err.size else 0.0


def audit(theta_trace, points, elbo, theta, Z, value_grad, sigma_z, seed, chain_id0, eta_opt=0.1, tau=1.0, window=100,
          lp_rtol=LP_RTOL_F64, g_rtol=G_RTOL_F64, g_atol=G_ATOL_F64):
    """theta_trace: 2M x (T+1) x R, points: M x S x T x R, elbo: T x R, theta: 2M x R, Z: M x D x R.  value_grad(z) -> (lp, g): the
    host fp64 oracle.  Raises AuditFailure naming run, step and the first offending component; returns a Report."""
    theta_trace, points, elbo, theta, Z = (np.asarray(a, dtype=np.float64) for a in (theta_trace, points, elbo, theta, Z))
    if (theta_trace.ndim != 3 or points.ndim != 4 or Z.ndim != 3 or theta_trace.shape[0] != 2 * points.shape[0]
            or theta_trace.shape[1] != points.shape[2] + 1 or elbo.shape != (points.shape[2], points.shape[3])
            or theta.shape != (theta_trace.shape[0], theta_trace.shape[2]) or Z.shape[0] != points.shape[0]
            or not (theta_trace.shape[2] == points.shape[3] == Z.shape[2])):
        raise AuditFailure("shapes: theta_trace %s, points %s, elbo %s, theta %s, Z %s" % (
            theta_trace.shape, points.shape, elbo.shape, theta.shape, Z.shape))
    nm, ns, nt, nr = points.shape
    sd = float(ns)
    rep = Report()

    def fail(r, t, what):
        raise AuditFailure("run %d (Philox chain %d), step %d: %s" % (r, chain_id0 + r, t, what))

    def check(r, t, got, target, bound, what):
        err = np.abs(got - target)
        bad = np.flatnonzero(~(err <= bound))
        if bad.size:
            i = int(bad[0])
            fail(r, t, "%s component %d is %r, expected %r: off by %.3g of its bound (%d of %d components off)"
                 % (what, i, got[i], target[i], err[i] / bound[i] if bound[i] > 0 else np.inf, bad.size, got.size))
        return _ratio(err, bound)

    def point_bound(mu, sig, eta):
        return Z_ULPS * EPS * (np.abs(mu) + sig * np.abs(eta)) + EXP_ULPS * 2.0 * EPS * sig * np.abs(eta)

    for r in range(nr):
        chain = chain_id0 + r
        n0 = sigma_z * normals(seed, chain, 0, P_INIT, 0, nm)
        rep.worst_theta0_ratio = max(rep.worst_theta0_ratio, check(r, 0, theta_trace[:, 0, r], n0, Z_ULPS * EPS * np.abs(n0), "theta_0"))
        ring_d2, ring_dd = np.zeros((window, 2 * nm)), np.zeros((window, 2 * nm))
        for t in range(nt):
            th = theta_trace[:, t, r]
            mu, om = th[:nm], th[nm:]
            sig = np.exp(om)
            eta = step_normals(seed, chain, t, nm, ns)
            lps, g, e = np.empty(ns), np.empty((nm, ns)), np.empty((nm, ns))
            for k in range(ns):
                rep.worst_point_ratio = max(rep.worst_point_ratio, check(
                    r, t, points[:, k, t, r], mu + sig * eta[:, k], point_bound(mu, sig, eta[:, k]), "point %d:" % k))
                lps[k], g[:, k] = value_grad(points[:, k, t, r])
                e[:, k] = g_rtol * np.abs(g[:, k]) + g_atol * np.max(np.abs(g[:, k]))
            d = np.concatenate([grad_mu(g, ns), grad_omega(g, eta, sig, ns)])
            terms_mu = np.sum(np.abs(g), axis=1) / sd
            terms_om = np.sum(np.abs(g * eta) * sig[:, None], axis=1) / sd
            dd = np.concatenate([
                np.sum(e, axis=1) / sd + Z_ULPS * EPS * (terms_mu + 1.0),
                np.sum(e * np.abs(eta), axis=1) * sig / sd + (Z_ULPS + EXP_ULPS) * 2.0 * EPS * terms_om + Z_ULPS * EPS * (terms_om + 1.0)])
            ring_d2[t % window], ring_dd[t % window] = d * d, 2.0 * np.abs(d) * dd + dd * dd
            s, ds = np.zeros(2 * nm), np.zeros(2 * nm)
            for w in range(window):
                s, ds = s + ring_d2[w], ds + ring_dd[w]
            root = np.sqrt(s)
            dsqrt = np.minimum(np.divide(ds, 2.0 * root, out=np.full_like(ds, np.inf), where=root > 0.0), np.sqrt(ds))
            c = eta_opt / (tau + root)
            delta = -(d * c)
            tol = c * dd + np.abs(d) * c * dsqrt / (tau + root) + Z_ULPS * EPS * (np.abs(th) + np.abs(delta))
            rep.worst_update_ratio = max(rep.worst_update_ratio, check(
                r, t, theta_trace[:, t + 1, r] - th, delta, tol, "the update theta_{t+1} - theta_t,"))
            ref = elbo_of(lps, entropy(om))
            rel = abs(elbo[t, r] - ref) / abs(ref) if ref != 0.0 else abs(elbo[t, r])
            if not rel <= lp_rtol:
                fail(r, t, "elbo is %r, its restatement is %r: relative error %.3e > %g" % (elbo[t, r], ref, rel, lp_rtol))
            rep.worst_elbo_rel = max(rep.worst_elbo_rel, float(rel))
            rep.steps += 1
        if not _same_bits(theta[:, r], theta_trace[:, nt, r]):
            i = int(np.flatnonzero(_bits(theta[:, r]) != _bits(theta_trace[:, nt, r]))[0])
            fail(r, nt, "theta component %d is %r, the last trace column holds %r" % (i, theta[i, r], theta_trace[i, nt, r]))
        mu, sig = theta[:nm, r], np.exp(theta[nm:, r])
        for i in range(Z.shape[1]):
            n = normals(seed, chain, i, P_DRAW, 0, (nm + 1) // 2)[:nm]
            rep.worst_draw_ratio = max(rep.worst_draw_ratio, check(r, nt, Z[:, i, r], mu + sig * n, point_bound(mu, sig, n), "draw %d:" % i))
    return rep


# ----------------------------------------------------------------------------------------------- problems and cases
T_, R_, I_ = so.ACT_TANH, so.ACT_RELU, so.ACT_IDENTITY


@dataclass(frozen=True)
class Case:
    name: str
    model: tuple            # (dims, acts, B), or ("conv", name of a spec in rwmh_audit.CONV_MODELS)
    m: int
    fused: bool             # the route si_fit_advi must report
    t: int                  # T, steps
    s: int = 10             # S, points per step
    w: int = 100            # W, the optimiser's window
    nruns: int = 1
    chain_id0: int = 0
    ndraws: int = 3
    sigma_z: float = 0.3
    eta: float = 0.1
    tau: float = 1.0
    sigma_m: float = 0.8
    seed: int = 11
    prior: float = 0.0
    f32: bool = False

    @property
    def tols(self):
        return (LP_RTOL_F32, G_RTOL_F32, G_ATOL_F32) if self.f32 else (LP_RTOL_F64, G_RTOL_F64, G_ATOL_F64)


def problem(case):
    return ma.problem(case)


def value_grad_of(pb):
    return ma.value_grad_of(pb)


TINY = ((3, 4, 2), (T_, I_), 17)        # N = 26
SMALL = ((5, 9, 6, 3), (T_, R_, I_), 37)   # B no multiple of the 16-observation tile, three workgroups per point

CASES = [
    Case("M1-S1", TINY, 1, True, 5, s=1),                       # one Philox block, half used; one point per step
    Case("M3-S10", TINY, 3, True, 4),                           # a ragged last block
    Case("M33-W4-T11", SMALL, 33, True, 11, s=3, w=4),          # the ring wraps
    Case("M33-W100-T7", SMALL, 33, True, 7, s=3),               # T < W: unwritten slots are summed
    Case("M300-S2", SMALL, 300, True, 3, s=2),                  # 2M > 512: a second lap of the thread-strided loops
    Case("M3-R3", TINY, 3, True, 5, s=3, nruns=3, chain_id0=2),
    Case("M33-prior", SMALL, 33, True, 4, s=3, prior=0.7),
    # the second route, on mala_audit's problems
    Case("conv-f64", ("conv", "conv0"), 5, False, 4, s=2, ndraws=2),
    Case("dense-f32", ma.F32_DENSE, 4, False, 5, s=3, f32=True),
    Case("softplus", ma.SOFTPLUS, 4, False, 6, s=3),
]
CASE_BY_NAME = {c.name: c for c in CASES}

MUTANTS = ("no_minus_one", "no_sigma", "eta0_reused", "no_over_s", "ring_slot_next", "s_without_current", "ring_never_wraps", "no_sqrt",
           "update_sign", "draws_purpose0", "final_from_prev_theta", "omega0_zero")
BIT_ONLY_MUTANTS = ("ring_slot_next",)    # the same W addends in another order: see the module's header


def oracle_trace(case, value_grad=None, mutant=None):
    """the definition on the case's Philox chains: (theta_trace 2M x (T+1) x R, points M x S x T x R, elbo T x R, theta 2M x R,
    Z M x D x R), si_fit_advi's shapes.  mutant: one of MUTANTS -- the trace a kernel with that mistake would produce."""
    assert mutant is None or mutant in MUTANTS, mutant
    vg = value_grad_of(problem(case)) if value_grad is None else value_grad
    m, nt, ns, nr, nd = case.m, case.t, case.s, case.nruns, case.ndraws
    trace = np.empty((2 * m, nt + 1, nr), order="F")
    points = np.empty((m, ns, nt, nr), order="F")
    elbo = np.empty((nt, nr), order="F")
    theta_out = np.empty((2 * m, nr), order="F")
    Z = np.empty((m, nd, nr), order="F")
    for r in range(nr):
        chain = case.chain_id0 + r
        th = case.sigma_z * normals(case.seed, chain, 0, P_INIT, 0, m)
        if mutant == "omega0_zero":
            th[m:] = 0.0
        trace[:, 0, r] = th
        ring = Ring(2 * m, case.w, case.eta, case.tau, mutant)
        prev = th
        for t in range(nt):
            mu, om = th[:m], th[m:]
            sig = np.exp(om)
            eta = step_normals(case.seed, chain, t, m, ns, purpose=0 if mutant == "draws_purpose0" else P_STEP)
            if mutant == "eta0_reused":
                eta = np.repeat(eta[:, :1], ns, axis=1)
            lps, g = np.empty(ns), np.empty((m, ns))
            for k in range(ns):
                points[:, k, t, r] = mu + sig * eta[:, k]
                lps[k], g[:, k] = vg(points[:, k, t, r])
            elbo[t, r] = elbo_of(lps, entropy(om))
            div = 1 if mutant == "no_over_s" else ns
            dom = grad_omega(g, eta, np.ones(m) if mutant == "no_sigma" else sig, div)
            if mutant == "no_minus_one":
                dom = dom + 1.0
            step = ring.step(t, np.concatenate([grad_mu(g, div), dom]))
            prev, th = th, (th + step if mutant == "update_sign" else th - step)
            trace[:, t + 1, r] = th
        theta_out[:, r] = th
        src = prev if mutant == "final_from_prev_theta" else th
        for i in range(nd):
            Z[:, i, r] = src[:m] + np.exp(src[m:]) * normals(case.seed, chain, i, P_DRAW, 0, (m + 1) // 2)[:m]
    return trace, points, elbo, theta_out, Z


@functools.lru_cache(maxsize=None)
def cached_oracle_trace(case):
    out = oracle_trace(case)
    for a in out:
        a.setflags(write=False)
    return out


def audit_case(case, theta_trace, points, elbo, theta, Z, value_grad=None):
    lp_rtol, g_rtol, g_atol = case.tols
    return audit(theta_trace, points, elbo, theta, Z, value_grad_of(problem(case)) if value_grad is None else value_grad,
                 case.sigma_z, case.seed, case.chain_id0, case.eta, case.tau, case.w, lp_rtol, g_rtol, g_atol)
