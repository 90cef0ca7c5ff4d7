"""Per-transition audit of a finished HMC trace (reference src/space_inference.jl:139-160; samplers.hmc + samplers.StanAdaptor +
samplers.find_good_stepsize -- the project's restatement of AdvancedHMC 0.2.27 [upstream, unverifiable offline] -- on the build's
Philox stream, oracle/philox.py) -- TEST INFRASTRUCTURE, no GPU needed.  The manner of tests/mala_audit.py: the audit takes the
trace's OWN previous column (z, lp, g, eps, Minv) as given and checks every transition and every adaptor update by itself.

Streams of chain c (Philox chain chain_id0 + c): purpose 0, step 0 = n_0 (MALA's z_0); purpose 1, step t, block 0 = the uniform
u_t = u53(x1, x0), EXACT on the host; purpose 5, step t = the momentum normals n_t; purpose 6, step 0 = the search's momentum rho.

  column 0  Z[:, 0] within 16 2^-53 sigma_z |n_0| of sigma_z n_0 (rwmh_audit's bound); lp[0] / G[:, 0] within (lp_rtol) / (g_rtol,
            g_atol max|g|) of the oracle at Z[:, 0]; Minv[:, 0] == 1; alpha[0] == 0
  step t    with z, lp, g = column t - 1, eps = eps[t], Minv = Minv[:, t] (those USED by transition t), all the trace's own:
            r = n_t / sqrt(Minv), rh = r + (eps / 2) g, zp = z + eps (Minv rh) on the host.  Exactly one of
    reject    Z[:, t], lp[t], G[:, t] are bit copies of column t - 1
    accept    |Z[m, t] - zp[m]| <= 24 2^-53 (|z| + |eps Minv r| + |eps Minv (eps / 2) g|)[m] for every m; lp[t], G[:, t] within the
              tolerances of the oracle at Z[:, t].  The 24: rwmh_audit's 16 for the normals (device log / sin / cos against the
              host libm), then six operations that both sides round once each and whose results may differ by one unit when
              their inputs do -- the quotient n / sqrt(Minv) (the square root is correctly rounded), (eps / 2) g, the sum rh,
              Minv rh, eps (.), the sum with z -- and two units of headroom.
  decision  accepted exactly when u_t < alpha[t], the host's exact u_t against the DEVICE's alpha[t]: no undecidable step
  alpha[t]  against a_ref from the oracle's (lpp, gp) at the host's zp:  K0 = 1/2 sum (Minv r) r, rp = rh + (eps / 2) gp,
            K1 = 1/2 sum (Minv rp) rp, dH = (lpp - K1) - (lp - K0), a(dH) = 0 if lpp - K1 is not finite, 1 if dH >= 0, else exp(dH).
            tol = lp_rtol (|lpp| + |lp|) + sum_m |eps / 2 Minv_m rp_m| (g_rtol |gp_m| + g_atol max|gp|)
                  + (2 24 + M + 8) 2^-53 (|K0| + |K1| + |lp| + |lpp|)
            the first-order effect of the stated tolerances (d dH / d gp_m = -eps / 2 Minv_m rp_m), and for the sums: a square
            doubles the 24 units of its argument, M positive terms added in any order differ by at most M units of their sum, 8
            units for the remaining roundings.  Nothing is taken from the device.  Required:
            a(dH - tol) (1 - 16 2^-53) <= alpha[t] <= a(dH + tol) (1 + 16 2^-53)   (the exp: 3 units on the device, 1 on the host)
  adaptor   samplers.StanAdaptor replayed from the trace's own alpha and Z (class Adaptor below, the same statements).  With k the
            dual-averaging count since the last restart (the restart takes the trace's own eps):
            |log eps[t+1] - log eps_replay| <= LOGEPS_BOUND(k, mu) = 2^-53 ((sqrt(k) / gamma) (6 k + 4) + 8 |mu| + 8)
            -- hbar is a convex combination of itself and delta - a, both at most 1 in magnitude, so rounding does not amplify:
            six roundings per step, at most 6 k 2^-53 after k steps; log eps = mu - sqrt(k) / gamma hbar carries it times
            sqrt(k) / gamma, plus four roundings of that product and difference, the logarithm in mu (3 + 1 units, doubled for
            headroom) and 8 units for the exponential that makes eps.  After step n_adapts eps = exp(log_eps_bar), a convex
            combination of the log eps so far: LOGEPS_BAR_BOUND(k, mu, L) = max_{j <= k} LOGEPS_BOUND(j, mu) + 8 k 2^-53 L with
            L = max |log eps| of the run (the weight k^-0.75 comes from pow: 8 units per step of what it multiplies).
            Minv[:, t+1] is a bit copy of Minv[:, t], except after a window's close: there it is held against
            n / (n + 5) var + 1e-3 5 / (n + 5) with var the two-pass longdouble variance of the window's columns of Z, within
            MINV_BOUND = n / (n + 5) 8 2^-53 (n var + 2 / (n - 1) sum_i |z_i - mean| (|z_i| + |mean|)) + 4 2^-53 Minv
            (Welford: every update rounds dlt, the mean and the product a few times -- an error of 2^-53 (|z_i| + |mean|) in dlt
            enters m2 times 2 |dlt|, and m2 itself takes a few roundings per step, n steps).  After n_adapts both are frozen bit
            for bit.  tests/test_hmc_audit_cpu.py certifies both bounds: on every case the float64 replay against a longdouble
            replay sits under a quarter of the bound.  Worst ratios measured there: log eps 0.021, Minv 0.062.
  search    find_good_stepsize replayed with the oracle from the trace's own column 0 and rho.  Every candidate eps is exact
            arithmetic (doublings, halvings, midpoints of 0.1), so eps[0] must equal the replay's result bit for bit whenever
            every comparison of the replay is decidable: |dH - log threshold| > the dH tolerance above (Minv = 1, thresholds 0.5
            while crossing, 0.25 and 0.75 while bisecting).  Otherwise the chain's search is undecidable: counted, skipped.
  count     mean_alpha[c] = mean of alpha[1:, c], what the host sampler reports as its acceptance statistic

oracle_trace(case, mutant=None) is the Philox-driven host HMC; MUTANTS names the wrong kernels it can imitate, each of which the audit
must reject on at least one case (tests/test_hmc_audit_cpu.py).  CASES is certified there on the oracle alone, so that
tests/test_gpu_hmc.py can hold the same conditions on the device's traces.
"""
import functools
import math
from dataclasses import dataclass, field

import numpy as np

from oracle import philox
from tests import mala_audit as ma
from tests import rwmh_audit as ra
from tests.advi_audit import normals as _purpose_normals
from tests.rwmh_audit import EPS, Z_ULPS, AuditFailure, _bits, _same_bits

P_MOMENTUM, P_SEARCH = 5, 6
ZP_ULPS = 24.0
EXP_ULPS = 16.0
GAMMA, T0, KAPPA = 0.05, 10.0, 0.75


def momentum_normals(seed, chain, step, m, purpose=P_MOMENTUM):
    return _purpose_normals(seed, chain, step, purpose, 0, (m + 1) // 2)[:m]


def uniform(seed, chain, step, purpose=1):
    x = philox.philox4x32(philox._ctr(step, chain, purpose, 0)[None, :], philox._key(seed)[None, :])
    return float(philox._u53(x[:, 1], x[:, 0])[0])


def n_adapts_of(itr, n_adapts=None):
    return int(round(itr / 2)) if n_adapts is None else int(n_adapts)


# ----------------------------------------------------------------------------------------------- the adaptor, restated for replay
class Adaptor:
    """samplers.StanAdaptor statement by statement (tests/test_hmc_audit_cpu.py holds the two bit for bit), in the number type `ft`
    (float or np.longdouble), with the switches the mutants need"""

    def __init__(self, m, n_adapts, eps, delta=0.8, ft=float, mutant=None):
        from subspaceinference_jl_amd import samplers
        ref = samplers.StanAdaptor(1, n_adapts, 0.1)
        self.window_start, self.window_end, self.window_splits = ref.window_start, ref.window_end, list(ref.window_splits)
        if mutant == "close_off_by_one":
            self.window_splits = [s + 1 for s in self.window_splits]
            self.window_end += 1
        self.m, self.n_adapts, self.ft, self.mutant = m, int(n_adapts), ft, mutant
        self.delta = ft(0.65 if mutant == "delta_065" else delta)
        self.i = 0
        self.minv = np.ones(m, dtype=ft)
        self.eps = ft(eps)
        self.restart(self.eps)
        self.wn, self.wmean, self.wm2 = 0, np.zeros(m, dtype=ft), np.zeros(m, dtype=ft)
        self.max_abs_log_eps = 0.0
        self.closed = False

    def _log(self, v):
        return math.log(v) if self.ft is float else np.log(v)

    def _exp(self, v):
        return math.exp(v) if self.ft is float else np.exp(v)

    def restart(self, eps):
        ft = self.ft
        self.mu = self._log(ft(eps)) if self.mutant == "mu_log_eps" else self._log(ft(10.0) * ft(eps))
        self.hbar, self.log_eps_bar, self.t = ft(0.0), ft(0.0), 0
        self.log_eps = self._log(ft(eps))

    def adapt(self, z, accept, z_proposed=None):
        """after adaptation step i (1-based).  Sets self.closed when this step closed a window."""
        ft = self.ft
        self.closed = False
        if self.i >= self.n_adapts and self.mutant != "adapt_after_n_adapts":
            return
        self.i += 1
        gamma, t0, kappa = ft(GAMMA), ft(T0), ft(KAPPA)
        self.t += 1
        t = ft(self.t)
        a = ft(accept) if accept < 1.0 else ft(1.0)
        self.hbar = (ft(1.0) - ft(1.0) / (t + t0)) * self.hbar + (self.delta - a) / (t + t0)
        sq = math.sqrt(self.t) if ft is float else np.sqrt(t)
        log_eps = self.mu - sq / gamma * self.hbar
        eta = self.t ** (-KAPPA) if ft is float else np.power(t, -kappa)
        self.log_eps_bar = eta * log_eps + (ft(1.0) - eta) * self.log_eps_bar
        self.log_eps = log_eps
        self.max_abs_log_eps = max(self.max_abs_log_eps, abs(float(log_eps)))
        self.eps = self._exp(min(log_eps, ft(700.0)))
        inside = self.window_start <= self.i <= self.window_end
        if inside or (self.mutant == "welford_outside_window" and self.i <= self.window_end):
            zz = np.asarray(z_proposed if (self.mutant == "welford_proposed" and z_proposed is not None) else z, dtype=ft)
            self.wn += 1
            dlt = zz - self.wmean
            self.wmean = self.wmean + dlt / ft(self.wn)
            self.wm2 = self.wm2 + dlt * (zz - self.wmean)
            if self.i in self.window_splits:
                n = self.wn
                if n >= 2:
                    var = self.wm2 / ft(n - 1)
                    if self.mutant == "var_unregularised":
                        self.minv = var
                    else:
                        self.minv = (ft(n) / (ft(n) + ft(5.0))) * var + ft(1e-3) * (ft(5.0) / (ft(n) + ft(5.0)))
                self.wn, self.wmean, self.wm2 = 0, np.zeros(self.m, dtype=ft), np.zeros(self.m, dtype=ft)
                self.closed = True
                if self.mutant != "da_no_restart":
                    self.restart(self.eps)
        if self.i == self.n_adapts:
            if self.t > 0 and self.mutant != "final_eps_not_average":
                self.eps = self._exp(min(self.log_eps_bar, ft(700.0)))


def logeps_bound(k, mu):
    return EPS * ((math.sqrt(k) / GAMMA) * (6.0 * k + 4.0) + 8.0 * abs(mu) + 8.0)


def logeps_bar_bound(k, mu, max_abs_log_eps):
    return logeps_bound(k, mu) + 8.0 * k * EPS * max_abs_log_eps     # (logeps_bound grows with k: its maximum over j <= k is at k)


def window_minv(zwin):
    """(Minv, bound) of a window's columns zwin (M x n): the regularised two-pass longdouble variance and MINV_BOUND"""
    zl = np.asarray(zwin, dtype=np.longdouble)
    n = zl.shape[1]
    mean = zl.sum(axis=1) / n
    dev = zl - mean[:, None]
    var = (dev * dev).sum(axis=1) / (n - 1)
    minv = (np.longdouble(n) / (n + 5)) * var + np.longdouble(1e-3) * (np.longdouble(5) / (n + 5))
    spread = (np.abs(dev) * (np.abs(zl) + np.abs(mean)[:, None])).sum(axis=1)
    bound = (n / (n + 5.0)) * 8.0 * EPS * (n * var + 2.0 / (n - 1) * spread) + 4.0 * EPS * minv
    return minv, bound.astype(np.float64)


# ----------------------------------------------------------------------------------------------- one leapfrog step on the host
def kinetic(r, minv):
    return 0.5 * float(np.sum(minv * r * r))


def half_kick_drift(z, r, g, eps, minv):
    rh = r + 0.5 * eps * g
    return rh, z + eps * (minv * rh)


def dh_tolerance(lp, lpp, gp, rp, eps, minv, k0, k1, tols, m):
    lp_rtol, g_rtol, g_atol = tols
    gmax = float(np.max(np.abs(gp))) if gp.size else 0.0
    return (lp_rtol * (abs(lpp) + abs(lp)) + float(np.sum(np.abs(0.5 * eps * minv * rp) * (g_rtol * np.abs(gp) + g_atol * gmax)))
            + (2.0 * ZP_ULPS + m + 8.0) * EPS * (abs(k0) + abs(k1) + abs(lp) + abs(lpp)))


def alpha_of(h1, dh):
    if not np.isfinite(h1):
        return 0.0
    return 1.0 if dh >= 0.0 else math.exp(dh)


def search(vg, z, lp, g, rho, tols, a_cross=0.5, eval_next=False, eps=0.1, max_iter=100):
    """samplers.find_good_stepsize with rho in place of the generator's draw (tests/test_hmc_audit_cpu.py holds the two bit for
    bit).  Returns (eps_0, decidable, evaluations): decidable = every comparison was further from its threshold than the dH
    tolerance.  a_cross / eval_next: the two search mutants."""
    m = z.size
    one = np.ones(m)
    k0 = 0.5 * float(rho @ rho)
    h0 = lp - k0
    state = dict(decidable=True, evals=0)

    def delta_h(e, thresholds):
        rh, zp = half_kick_drift(z, rho, g, e, 1.0)
        lpp, gp = vg(zp)
        rp = rh + 0.5 * e * gp
        k1 = 0.5 * float(rp @ rp)
        d = lpp - k1 - h0
        state["evals"] += 1
        if np.isfinite(d):
            tol = dh_tolerance(lp, lpp, gp, rp, e, one, k0, k1, tols, m)
            if any(abs(d - th) <= tol for th in thresholds):
                state["decidable"] = False
        return d

    log_cross = math.log(a_cross)
    direction = 1 if delta_h(eps, (log_cross,)) > log_cross else -1
    eps_next = eps
    for _ in range(max_iter):
        eps_next = 2.0 * eps if direction == 1 else 0.5 * eps
        d = delta_h(eps_next if eval_next else eps, (log_cross,))
        if direction == 1 and not d > log_cross:
            break
        if direction == -1 and not d < log_cross:
            break
        eps = eps_next
    lo, hi = (eps, eps_next) if eps < eps_next else (eps_next, eps)
    for _ in range(max_iter):
        mid = 0.5 * (lo + hi)
        d = delta_h(mid, (math.log(0.25), math.log(0.75)))
        try:
            a = math.exp(d)
        except OverflowError:
            a = math.inf
        if a > 0.75:
            lo = mid
        elif a < 0.25:
            hi = mid
        else:
            lo = mid
            break
    return lo, state["decidable"], state["evals"]


# ----------------------------------------------------------------------------------------------- the audit
@dataclass
class Report:
    accepts: int = 0
    rejects: int = 0
    undecidable: int = 0             # chains whose step-size search has a comparison inside its tolerance
    worst_z_ratio: float = 0.0
    worst_lp_rel: float = 0.0
    worst_g_ratio: float = 0.0
    worst_alpha_ratio: float = 0.0   # |dH(alpha) - dH_ref| / tol over the steps with 0 < alpha < 1
    worst_logeps_ratio: float = 0.0
    worst_minv_ratio: float = 0.0
    closes: int = 0
    chain_accepts: list = field(default_factory=list)
    chain_rejects: list = field(default_factory=list)
    mean_alpha: list = field(default_factory=list)
    search_evals: list = field(default_factory=list)

    @property
    def steps(self):
        return self.accepts + self.rejects

    def line(self):
        return ("accepts %s, rejects %s, undecidable searches %d, window closes %d, worst ratios: z %.3f, lp rel %.2e, g %.2e, alpha %.2e, "
                "log eps %.2e, Minv %.2e" % (
                    self.chain_accepts if len(self.chain_accepts) <= 8 else self.accepts,
                    self.chain_rejects if len(self.chain_rejects) <= 8 else self.rejects, self.undecidable, self.closes,
                    self.worst_z_ratio, self.worst_lp_rel, self.worst_g_ratio, self.worst_alpha_ratio, self.worst_logeps_ratio,
                    self.worst_minv_ratio))


def _ratio(err, bound):
    return float(np.max(np.divide(err, bound, out=np.where(err > 0.0, np.inf, 0.0), where=bound > 0.0))) if np.size(err) else 0.0


def audit(Z, lp, alpha, eps, G, Minv, value_grad, sigma_z, seed, chain_id0, n_adapts, delta=0.8, tols=None):
    """Z, G, Minv: M x (itr+1) x C; lp, alpha, eps: (itr+1) x C.  value_grad(z) -> (lp, g): the host fp64 oracle.  Raises
    AuditFailure naming chain, step and the first offending component; returns a Report."""
    Z, lp, alpha, eps, G, Minv = (np.asarray(a, dtype=np.float64) for a in (Z, lp, alpha, eps, G, Minv))
    if Z.ndim != 3 or G.shape != Z.shape or Minv.shape != Z.shape or any(a.shape != Z.shape[1:] for a in (lp, alpha, eps)):
        raise AuditFailure("shapes: Z %s, lp %s, alpha %s, eps %s, G %s, Minv %s" % (Z.shape, lp.shape, alpha.shape, eps.shape, G.shape, Minv.shape))
    tols = (ma.LP_RTOL_F64, ma.G_RTOL_F64, ma.G_ATOL_F64) if tols is None else tols
    lp_rtol, g_rtol, g_atol = tols
    nm, cols, nch = Z.shape
    itr = cols - 1
    rep = Report()

    def fail(c, t, what):
        raise AuditFailure("chain %d (Philox chain %d), step %d: %s" % (c, chain_id0 + c, t, what))

    def check_z(c, t, zt, target, scale, ulps, what):
        err, bound = np.abs(zt - target), ulps * EPS * scale
        bad = np.flatnonzero(~(err <= bound))
        if bad.size:
            m = int(bad[0])
            fail(c, t, "component %d is %r, expected %s = %r: off by %.3g of the %g-unit bound (%d of %d components off)"
                 % (m, zt[m], what, target[m], err[m] / bound[m] if bound[m] > 0 else np.inf, ulps, bad.size, nm))
        rep.worst_z_ratio = max(rep.worst_z_ratio, _ratio(err, bound))

    def check_lp_g(c, t, ref, what):
        lp_ref, g_ref = ref
        rel = abs(lp[t, c] - lp_ref) / abs(lp_ref) if lp_ref != 0.0 else abs(lp[t, c])
        if not rel <= lp_rtol:
            fail(c, t, "lp is %r, the value at %s is %r: relative error %.3e > %g" % (lp[t, c], what, lp_ref, rel, lp_rtol))
        rep.worst_lp_rel = max(rep.worst_lp_rel, float(rel))
        err, bound = np.abs(G[:, t, c] - g_ref), g_rtol * np.abs(g_ref) + g_atol * np.max(np.abs(g_ref))
        bad = np.flatnonzero(~(err <= bound))
        if bad.size:
            m = int(bad[0])
            fail(c, t, "gradient component %d is %r, the gradient at %s has %r: off by %.3g of its bound (%d of %d components off)"
                 % (m, G[m, t, c], what, g_ref[m], err[m] / bound[m] if bound[m] > 0 else np.inf, bad.size, nm))
        rep.worst_g_ratio = max(rep.worst_g_ratio, _ratio(err, bound))

    for c in range(nch):
        chain = chain_id0 + c
        n0 = sigma_z * philox.normals(seed, chain, 0, nm)
        check_z(c, 0, Z[:, 0, c], n0, np.abs(n0), Z_ULPS, "sigma_z n_0")
        check_lp_g(c, 0, value_grad(Z[:, 0, c]), "Z[:, 0]")
        if not np.all(Minv[:, 0, c] == 1.0):
            fail(c, 0, "Minv[:, 0] is not 1: %r" % (Minv[:, 0, c],))
        if alpha[0, c] != 0.0:
            fail(c, 0, "alpha[0] is %r, not 0" % alpha[0, c])
        # the step-size search from the trace's own column 0
        rho = momentum_normals(seed, chain, 0, nm, P_SEARCH)
        eps0, decidable, evals = search(value_grad, Z[:, 0, c], lp[0, c], G[:, 0, c], rho, tols)
        rep.search_evals.append(evals)
        if not decidable:
            rep.undecidable += 1
        elif _bits(eps[0:1, c])[0] != _bits(np.array([eps0]))[0]:
            fail(c, 0, "eps[0] is %r, the step-size search replayed from column 0 gives %r (%d evaluations, every comparison decidable)"
                 % (eps[0, c], eps0, evals))
        ad = Adaptor(nm, n_adapts, eps[0, c], delta)
        win_first = None      # first column of the window that is open
        n_acc = n_rej = k_before = 0
        for t in range(1, cols):
            z, g, zt, e, mi = Z[:, t - 1, c], G[:, t - 1, c], Z[:, t, c], eps[t, c], Minv[:, t, c]
            if not (e > 0.0 and np.isfinite(e)):
                fail(c, t, "eps[t] is %r" % e)
            if not np.all((mi > 0.0) & np.isfinite(mi)):
                fail(c, t, "Minv[:, t] is not positive and finite")
            r = momentum_normals(seed, chain, t, nm) / np.sqrt(mi)
            rh, zp = half_kick_drift(z, r, g, e, mi)
            if _same_bits(zt, z):
                if _bits(lp[t:t + 1, c])[0] != _bits(lp[t - 1:t, c])[0]:
                    fail(c, t, "Z[:, t] is a bit copy of Z[:, t-1] (a reject) but lp changed from %r to %r" % (lp[t - 1, c], lp[t, c]))
                if not _same_bits(G[:, t, c], g):
                    m = int(np.flatnonzero(_bits(G[:, t, c]) != _bits(g))[0])
                    fail(c, t, "Z[:, t] is a bit copy of Z[:, t-1] (a reject) but gradient component %d changed from %r to %r"
                         % (m, g[m], G[m, t, c]))
                accepted = False
                n_rej += 1
            else:
                check_z(c, t, zt, zp, np.abs(z) + np.abs(e * (mi * r)) + np.abs(e * (mi * (0.5 * e * g))), ZP_ULPS,
                        "z + eps (Minv (r + eps / 2 g))")
                accepted = True
                n_acc += 1
            lpp, gp = value_grad(zp)
            if accepted:
                check_lp_g(c, t, (lpp, gp) if _same_bits(zt, zp) else value_grad(zt), "Z[:, t]")
            # the decision: exact
            u = uniform(seed, chain, t)
            if accepted != (u < alpha[t, c]):
                fail(c, t, "the trace %s, but u_t = %r and alpha[t] = %r say %s" % (
                    "accepted" if accepted else "rejected", u, alpha[t, c], "accept" if u < alpha[t, c] else "reject"))
            # alpha[t] against the oracle
            k0 = kinetic(r, mi)
            rp = rh + 0.5 * e * gp
            k1 = kinetic(rp, mi)
            h1 = lpp - k1
            dh = h1 - (lp[t - 1, c] - k0)
            if not np.isfinite(h1):
                if alpha[t, c] != 0.0:
                    fail(c, t, "lpp - K1 = %r is not finite, alpha[t] must be 0 and is %r" % (h1, alpha[t, c]))
            else:
                tol = dh_tolerance(lp[t - 1, c], lpp, gp, rp, e, mi, k0, k1, tols, nm)
                a_lo, a_hi = alpha_of(h1, dh - tol) * (1.0 - EXP_ULPS * EPS), min(1.0, alpha_of(h1, dh + tol) * (1.0 + EXP_ULPS * EPS))
                if not a_lo <= alpha[t, c] <= a_hi:
                    fail(c, t, "alpha[t] is %r; (lpp - K1) - (lp - K0) = (%r - %r) - (%r - %r) = %r (tolerance %.3g) allows [%r, %r]" % (
                        alpha[t, c], lpp, k1, lp[t - 1, c], k0, dh, tol, a_lo, a_hi))
                if 1e-300 < alpha[t, c] < 1.0:
                    rep.worst_alpha_ratio = max(rep.worst_alpha_ratio, abs(math.log(alpha[t, c]) - dh) / tol)
            # the adaptor's update after transition t, against column t + 1
            if t <= n_adapts and ad.window_start <= t <= ad.window_end and win_first is None:
                win_first = t
            mu_used = float(ad.mu)
            ad.adapt(zt, alpha[t, c])
            if t + 1 >= cols:
                continue
            e1, mi1 = eps[t + 1, c], Minv[:, t + 1, c]
            if t > n_adapts:
                if _bits(eps[t + 1:t + 2, c])[0] != _bits(eps[t:t + 1, c])[0] or not _same_bits(mi1, mi):
                    fail(c, t, "adaptation ended after step %d, but eps or Minv changed from column %d to %d (eps %r -> %r)" % (
                        n_adapts, t, t + 1, e, e1))
                continue
            if not (e1 > 0.0 and np.isfinite(e1)):
                fail(c, t + 1, "eps[t] is %r" % e1)
            if t == n_adapts and ad.t > 0:
                bound = logeps_bar_bound(ad.t, mu_used, ad.max_abs_log_eps) + 8.0 * EPS
                want = float(ad.log_eps_bar)
            else:
                k = ad.t if not ad.closed else k_before + 1
                bound = logeps_bound(k, mu_used)
                want = math.log(float(ad.eps))
            err = abs(math.log(e1) - want)
            if not err <= bound:
                fail(c, t, "after this step's update eps is %r (column %d), the adaptor replayed from the trace's alpha gives %r: "
                     "log eps off by %.3g of its bound %.3g" % (e1, t + 1, math.exp(want), err / bound, bound))
            rep.worst_logeps_ratio = max(rep.worst_logeps_ratio, err / bound)
            if ad.closed:
                rep.closes += 1
                want_minv, mbound = window_minv(Z[:, win_first:t + 1, c])
                merr = np.abs(mi1 - want_minv.astype(np.float64))
                bad = np.flatnonzero(~(merr <= mbound))
                if bad.size:
                    m = int(bad[0])
                    fail(c, t, "a window closed (columns %d .. %d): Minv[%d] is %r in column %d, the regularised variance of the window is %r: "
                         "off by %.3g of its bound" % (win_first, t, m, mi1[m], t + 1, float(want_minv[m]), merr[m] / mbound[m]))
                rep.worst_minv_ratio = max(rep.worst_minv_ratio, _ratio(merr, mbound))
                win_first = None
                ad.minv = mi1.copy()
                ad.eps = e1
                ad.restart(e1)          # (the restart takes the trace's own eps)
            elif not _same_bits(mi1, mi):
                m = int(np.flatnonzero(_bits(mi1) != _bits(mi))[0])
                fail(c, t, "no window closed at this step, but Minv[%d] changed from %r to %r" % (m, mi[m], mi1[m]))
            k_before = ad.t
        rep.accepts += n_acc
        rep.rejects += n_rej
        rep.chain_accepts.append(n_acc)
        rep.chain_rejects.append(n_rej)
        rep.mean_alpha.append(float(alpha[1:, c].mean()) if itr > 0 else 0.0)
    return rep


# ----------------------------------------------------------------------------------------------- problems and cases
problem, value_grad_of = ma.problem, ma.value_grad_of
SMALL, RAGGED, F32_DENSE, SOFTPLUS, MODEL_A, MODEL_B = ma.SMALL, ma.RAGGED, ma.F32_DENSE, ma.SOFTPLUS, ma.MODEL_A, ma.MODEL_B


@dataclass(frozen=True)
class Case:
    name: str
    model: tuple            # mala_audit's models
    m: int
    sigma_z: float
    fused: bool             # the route si_sample_hmc must report
    nchains: int = 2
    itr: int = 60
    n_adapts: int = -1      # -1: the reference's round(itr / 2)
    delta: float = 0.8
    sigma_m: float = 0.8
    seed: int = 11
    chain_id0: int = 2
    prior: float = 0.0
    f32: bool = False
    per_chain: bool = True  # both branches in EVERY chain; False: in the case as a whole

    @property
    def tols(self):
        return (ma.LP_RTOL_F32, ma.G_RTOL_F32, ma.G_ATOL_F32) if self.f32 else (ma.LP_RTOL_F64, ma.G_RTOL_F64, ma.G_ATOL_F64)

    @property
    def adapts(self):
        return n_adapts_of(self.itr, None if self.n_adapts < 0 else self.n_adapts)


MUTANTS = ("no_second_kick", "drift_no_minv", "momentum_unscaled", "kinetic_no_minv", "g_stale", "lp_stale", "momentum_purpose0",
           "momentum_next_step", "momentum_prev_step", "momentum_next_chain", "u_from_purpose0", "a_uncapped", "delta_065",
           "da_no_restart", "mu_log_eps", "final_eps_not_average", "var_unregularised", "welford_outside_window", "welford_proposed",
           "close_off_by_one", "adapt_after_n_adapts", "search_cross_08", "search_eval_next")


def oracle_trace(case, value_grad=None, mutant=None):
    """samplers.hmc on the case's Philox chains: (Z, lp, alpha, eps, G, Minv) in si_sample_hmc's shapes (itr + 1 columns).  mutant:
    one of MUTANTS -- the trace a kernel with that mistake would produce."""
    assert mutant is None or mutant in MUTANTS, mutant
    vg = value_grad_of(problem(case)) if value_grad is None else value_grad
    m, itr, s, nc = case.m, case.itr, case.sigma_z, case.nchains
    Z, G, MI = (np.empty((m, itr + 1, nc), order="F") for _ in range(3))
    lps, al, ep = (np.empty((itr + 1, nc), order="F") for _ in range(3))
    for c in range(nc):
        chain = case.chain_id0 + c

        def normals(t):
            if mutant == "momentum_purpose0":
                return philox.normals(case.seed, chain, t, m)
            if mutant == "momentum_next_step":
                return momentum_normals(case.seed, chain, t + 1, m)
            if mutant == "momentum_prev_step":
                return momentum_normals(case.seed, chain, t - 1, m)
            if mutant == "momentum_next_chain":
                return momentum_normals(case.seed, chain + 1, t, m)
            return momentum_normals(case.seed, chain, t, m)
        z = s * philox.normals(case.seed, chain, 0, m)
        lp, g = vg(z)
        eps0 = search(vg, z, lp, g, momentum_normals(case.seed, chain, 0, m, P_SEARCH), case.tols,
                      a_cross=0.8 if mutant == "search_cross_08" else 0.5, eval_next=mutant == "search_eval_next")[0]
        ad = Adaptor(m, case.adapts, eps0, case.delta, mutant=mutant)
        Z[:, 0, c], lps[0, c], G[:, 0, c], al[0, c], ep[0, c], MI[:, 0, c] = z, lp, g, 0.0, eps0, 1.0
        for t in range(1, itr + 1):
            minv, eps = np.array(ad.minv, dtype=np.float64), float(ad.eps)
            n = normals(t)
            r = n if mutant == "momentum_unscaled" else n / np.sqrt(minv)
            k0 = 0.5 * float(np.sum(r * r)) if mutant == "kinetic_no_minv" else kinetic(r, minv)
            rh, zp = half_kick_drift(z, r, g, eps, 1.0 if mutant == "drift_no_minv" else minv)
            lpp, gp = vg(zp)
            rp = rh if mutant == "no_second_kick" else rh + 0.5 * eps * gp
            k1 = 0.5 * float(np.sum(rp * rp)) if mutant == "kinetic_no_minv" else kinetic(rp, minv)
            h1 = lpp - k1
            dh = h1 - (lp - k0)
            a = alpha_of(h1, dh)
            if mutant == "a_uncapped" and np.isfinite(h1):
                a = math.exp(min(dh, 700.0))
            u = uniform(case.seed, chain, t, 0 if mutant == "u_from_purpose0" else 1)
            if u < a:
                z = zp
                if mutant != "lp_stale":
                    lp = lpp
                if mutant != "g_stale":
                    g = gp
            Z[:, t, c], lps[t, c], G[:, t, c], al[t, c], ep[t, c], MI[:, t, c] = z, lp, g, a, eps, minv
            ad.adapt(z, a, zp)
    return Z, lps, al, ep, G, MI


@functools.lru_cache(maxsize=None)
def cached_oracle_trace(case):
    out = oracle_trace(case)
    for a in out:
        a.setflags(write=False)
    return out


def audit_case(case, Z, lp, alpha, eps, G, Minv, value_grad=None):
    return audit(Z, lp, alpha, eps, G, Minv, value_grad_of(problem(case)) if value_grad is None else value_grad, case.sigma_z, case.seed,
                 case.chain_id0, case.adapts, case.delta, case.tols)


SHORT = 8   # cases of at most this many transitions are exempt from the both-branches condition: too few steps to demand a reject


def check_caps(case, rep):
    """conditions on a case, not measurements: both branches in every chain (per_chain = False: in the case as a whole; itr <= 8
    with per_chain: exempt); no undecidable search in fp64, at most F32_UNDECIDABLE_CAP of the chains with SI_F32"""
    if case.itr > SHORT or not case.per_chain:
        if case.per_chain:
            for c, (a, r) in enumerate(zip(rep.chain_accepts, rep.chain_rejects)):
                assert a >= 1 and r >= 1, "chain %d has %d accepts and %d rejects: the case must reach both branches in every chain" % (c, a, r)
        else:
            assert rep.accepts >= 1 and rep.rejects >= 1, "the case has %d accepts and %d rejects" % (rep.accepts, rep.rejects)
    cap = ra.F32_UNDECIDABLE_CAP * case.nchains if case.f32 else 0
    assert rep.undecidable <= cap, "%d undecidable searches of %d chains (cap %g)" % (rep.undecidable, case.nchains, cap)
    assert rep.steps == case.itr * case.nchains


# sigma_z only places the initial point: the step size is the search's and the adaptor's.  Values are mala_audit's for the same
# models, where its chains stay in the region the oracle's gradient tolerances were stated for.
CASES = [
    # itr = 400, n_adapts = 200: the standard schedule, windows close at 100 and 150, two restarts of the dual averaging
    Case("small-M2-adapt200", SMALL, 2, 1.0, True, itr=400),
    Case("small-M1", SMALL, 1, 0.5, True),                       # itr = 60, n_adapts = 30: rescaled schedule, one close at 27
    Case("ragged-M5", RAGGED, 5, 0.2, True),
    Case("A-M33", MODEL_A, 33, 0.2, True, nchains=3),
    Case("A-M65", MODEL_A, 65, 0.2, True),
    Case("A-M33-prior", MODEL_A, 33, 0.2, True, prior=0.7),
    Case("A-M2-high-words", MODEL_A, 2, 0.2, True, seed=2 ** 40 + 7, chain_id0=2 ** 24 + 5),
    Case("A-M2-itr1", MODEL_A, 2, 0.2, True, itr=1),             # n_adapts = 0
    Case("A-M2-itr5", MODEL_A, 2, 0.2, True, itr=5),             # n_adapts = round(2.5) = 2, ties to even
    Case("A-M5-itr8", MODEL_A, 5, 0.2, True, itr=8),             # n_adapts = 4: no window
    Case("small-M2-adapt-all", SMALL, 2, 1.0, True, itr=40, n_adapts=40),   # explicit n_adapts = itr: the last column is the last update
    # (seed 49: in both chains one doubling of the search lands between the acceptances 0.5 and 0.8, which tells the crossing threshold)
    Case("small-M2-search", SMALL, 2, 1.0, True, itr=8, seed=49),
    Case("small-M513", SMALL, 513, 0.2, True, itr=8),            # 257 Philox blocks: the 256-thread sweep runs twice
    Case("A-M33x64", MODEL_A, 33, 0.2, True, nchains=64, itr=8, seed=12, per_chain=False),
    Case("conv-f64", ("conv", "conv0"), 5, 1.0, False, itr=40),
    Case("dense-f32", F32_DENSE, 4, 0.15, False, itr=40, f32=True),
    Case("softplus", SOFTPLUS, 4, 0.2, False, itr=40),
]
CASE_BY_NAME = {c.name: c for c in CASES}
