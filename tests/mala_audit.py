"""Per-transition audit of a finished MALA trace (reference src/space_inference.jl:117-120; samplers.mala restated on the build's
Philox stream, oracle/philox.py) -- TEST INFRASTRUCTURE, no GPU needed.  The manner of tests/rwmh_audit.py: the audit takes the
trace's OWN previous (z, lp, g) as given and checks every transition by itself, so that no decision has to stay in lockstep with
another chain.  With h = sigma_z^2 / 2, n_t the M normals of (chain, step t, purpose 0) and e_t the Exp(1) draw of purpose 1:

  step 0    Z[:, 0] = sigma_z n_0 within 16 2^-53 sigma_z |n_0|; lp[0] within lp_rtol and G[:, 0] within (g_rtol, g_atol max|g|) of
            the oracle's value and gradient at Z[:, 0]
  step t    exactly one of
    reject    Z[:, t], lp[t] and G[:, t] are bit copies of step t - 1
    accept    |Z[m, t] - (z + h g + sigma_z n_t)[m]| <= 16 2^-53 (|z[m]| + h |g[m]| + sigma_z |n_t[m]|) for EVERY m, with z = Z[:, t-1]
              and g = G[:, t-1], the trace's own; lp[t] and G[:, t] within the tolerances above of the oracle at Z[:, t]
  decision  with zp = z + h g + sigma_z n_t on the host and the oracle's (lpp, gp) at zp: fwd = zp - z - h g, bwd = z - zp - h gp,
            logq = -(bwd.bwd - fwd.fwd) / (2 sigma_z^2), margin = lpp - lp[t-1] + logq + e_t,
            tol = lp_rtol (|lpp| + |lp[t-1]|) + 1/2 sum_m |bwd_m| (g_rtol |gp_m| + g_atol max|gp|) + 16 2^-53 e_t
            -- the first-order effect of the stated lp and gradient tolerances (d logq / d gp_m = bwd_m / 2), nothing taken from the
            device.  |margin| > tol => accepted exactly when margin > 0; otherwise the step is undecidable (counted, skipped here)
  count     acc[c] (itr - 1) == number of accept-classified steps, exactly (itr == 1: acc == 0)

The z bound is rwmh_audit's 16 ulp (the normals: log, sin / cos, sqrt within the OpenCL fp64 limits against the host libm, then the
roundings of h g, sigma_z n and two adds), scaled by the three terms that are added.

oracle_trace(case) is the Philox-driven host MALA; MUTANTS names the wrong kernels it can imitate, each of which the audit must
reject on at least one case (tests/test_mala_audit_cpu.py).  CASES is certified there on the oracle alone -- both branches in every
chain, no undecidable step in fp64 -- so that tests/test_gpu_mala.py can hold the same conditions on the device's traces.
"""
import functools
from dataclasses import dataclass, field

import numpy as np

from oracle import philox
from oracle import subspace_oracle as so
from tests import rwmh_audit as ra
from tests.rwmh_audit import EPS, Z_ULPS, AuditFailure, _bits, _same_bits

LP_RTOL_F64, LP_RTOL_F32 = ra.LP_RTOL_F64, ra.LP_RTOL_F32
G_RTOL_F64, G_ATOL_F64 = 1e-8, 1e-9      # tests/test_gpu_grad_batch.py, test_gpu_parity.py: rtol 1e-8, atol 1e-9 max|g|
G_RTOL_F32, G_ATOL_F32 = 0.0, 2e-5       # tests/test_gpu_f32.py: max|g - g_ref| <= 2e-5 max|g_ref|
F32_UNDECIDABLE_CAP = ra.F32_UNDECIDABLE_CAP


@dataclass
class Report:
    accepts: int = 0
    rejects: int = 0
    undecidable: int = 0
    worst_z_ratio: float = 0.0
    worst_lp_rel: float = 0.0
    worst_g_ratio: float = 0.0
    min_margin_over_tol: float = np.inf
    chain_accepts: list = field(default_factory=list)
    chain_rejects: list = field(default_factory=list)

    @property
    def steps(self):
        return self.accepts + self.rejects

    def line(self):
        return ("accepts %s, rejects %s, undecidable %d, worst z ratio %.3f, worst lp rel %.2e, worst g ratio %.2e, min |margin| / tol %.2e"
                % (self.chain_accepts if len(self.chain_accepts) <= 8 else self.accepts,
                   self.chain_rejects if len(self.chain_rejects) <= 8 else self.rejects, self.undecidable, self.worst_z_ratio,
                   self.worst_lp_rel, self.worst_g_ratio, self.min_margin_over_tol))


def logq_terms(z, g, zp, gp, h, sigma_z):
    fwd = zp - z - h * g
    bwd = z - zp - h * gp
    return -(float(bwd @ bwd) - float(fwd @ fwd)) / (2.0 * sigma_z * sigma_z), bwd


def audit(Z, lp, acc, G, value_grad, sigma_z, seed, chain_id0, lp_rtol=LP_RTOL_F64, g_rtol=G_RTOL_F64, g_atol=G_ATOL_F64):
    """Z, G: M x itr x C, lp: itr x C, acc: C.  value_grad(z) -> (lp, g): the host fp64 oracle.  Raises AuditFailure naming chain,
    step and the first offending component; returns a Report."""
    Z, lp, acc, G = (np.asarray(a, dtype=np.float64) for a in (Z, lp, acc, G))
    if Z.ndim != 3 or G.shape != Z.shape or lp.shape != Z.shape[1:] or acc.shape != (Z.shape[2],):
        raise AuditFailure("shapes: Z %s, lp %s, acc %s, G %s" % (Z.shape, lp.shape, acc.shape, G.shape))
    nm, itr, nch = Z.shape
    h = 0.5 * sigma_z * sigma_z
    rep = Report()

    def fail(c, t, what):
        raise AuditFailure("chain %d (Philox chain %d), step %d: %s" % (c, chain_id0 + c, t, what))

    def check_z(c, t, zt, zprev, drift, noise):
        target = zprev + drift + noise
        err, bound = np.abs(zt - target), Z_ULPS * EPS * (np.abs(zprev) + np.abs(drift) + np.abs(noise))
        bad = np.flatnonzero(~(err <= bound))
        if bad.size:
            m = int(bad[0])
            fail(c, t, "component %d is %r, expected z + h g + sigma_z n = %r + %r + %r = %r: off by %.3g of the %g-ulp bound (%d of %d components off)"
                 % (m, zt[m], zprev[m], drift[m], noise[m], target[m], err[m] / bound[m] if bound[m] > 0 else np.inf, Z_ULPS, bad.size, nm))
        rep.worst_z_ratio = max(rep.worst_z_ratio, float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0.0))))

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
        rep.worst_g_ratio = max(rep.worst_g_ratio, float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0.0))))

    for c in range(nch):
        chain = chain_id0 + c
        zero = np.zeros(nm)
        check_z(c, 0, Z[:, 0, c], zero, zero, sigma_z * philox.normals(seed, chain, 0, nm))
        check_lp_g(c, 0, value_grad(Z[:, 0, c]), "Z[:, 0]")
        n_acc = n_rej = 0
        for t in range(1, itr):
            zprev, gprev, zt = Z[:, t - 1, c], G[:, t - 1, c], Z[:, t, c]
            noise = sigma_z * philox.normals(seed, chain, t, nm)
            if _same_bits(zt, zprev):
                if _bits(lp[t:t + 1, c])[0] != _bits(lp[t - 1:t, c])[0]:
                    fail(c, t, "Z[:, t] is a bit copy of Z[:, t-1] (a reject) but lp changed from %r to %r" % (lp[t - 1, c], lp[t, c]))
                if not _same_bits(G[:, t, c], gprev):
                    m = int(np.flatnonzero(_bits(G[:, t, c]) != _bits(gprev))[0])
                    fail(c, t, "Z[:, t] is a bit copy of Z[:, t-1] (a reject) but gradient component %d changed from %r to %r"
                         % (m, gprev[m], G[m, t, c]))
                accepted = False
                n_rej += 1
            else:
                check_z(c, t, zt, zprev, h * gprev, noise)
                accepted = True
                n_acc += 1
            zp = zprev + h * gprev + noise
            lpp, gp = value_grad(zp)
            if accepted:
                check_lp_g(c, t, (lpp, gp) if _same_bits(zt, zp) else value_grad(zt), "Z[:, t]")
            logq, bwd = logq_terms(zprev, gprev, zp, gp, h, sigma_z)
            e_t = philox.randexp(seed, chain, t)
            margin = lpp - lp[t - 1, c] + logq + e_t
            tol = (lp_rtol * (abs(lpp) + abs(lp[t - 1, c])) + 0.5 * float(np.sum(np.abs(bwd) * (g_rtol * np.abs(gp) + g_atol * np.max(np.abs(gp)))))
                   + Z_ULPS * EPS * e_t)
            if abs(margin) > tol:
                rep.min_margin_over_tol = min(rep.min_margin_over_tol, abs(margin) / tol)
                if accepted != (margin > 0.0):
                    fail(c, t, "the trace %s, but lpp - lp[t-1] + logq + e_t = %r - %r + %r + %r = %r (tolerance %.3g) says %s" % (
                        "accepted" if accepted else "rejected", lpp, lp[t - 1, c], logq, e_t, margin, tol, "accept" if margin > 0.0 else "reject"))
            elif not np.isnan(margin):
                rep.undecidable += 1
            else:
                fail(c, t, "the decision margin is NaN (lpp = %r, lp[t-1] = %r, logq = %r)" % (lpp, lp[t - 1, c], logq))
        want = n_acc / (itr - 1) if itr > 1 else 0.0
        if acc[c] != want:
            raise AuditFailure("chain %d (Philox chain %d): acc is %r, the trace holds %d accepted of %d steps (%r)" % (
                c, chain, acc[c], n_acc, itr - 1, want))
        rep.accepts += n_acc
        rep.rejects += n_rej
        rep.chain_accepts.append(n_acc)
        rep.chain_rejects.append(n_rej)
    return rep


# ----------------------------------------------------------------------------------------------- problems and cases
R, T, S, I = ra.R, ra.T, ra.S, ra.I
SP = so.ACT_SOFTPLUS
MODEL_A, MODEL_B = ra.MODEL_A, ra.MODEL_B


@dataclass(frozen=True)
class Case:
    name: str
    model: tuple            # (dims, acts, B), or ("conv", name of a spec in rwmh_audit.CONV_MODELS)
    m: int
    sigma_z: float
    fused: bool             # the route si_sample_mala must report: the device-resident one, or the per-point one
    nchains: int = 3
    itr: int = 40
    sigma_m: float = 0.8
    seed: int = 11
    chain_id0: int = 2
    prior: float = 0.0      # set_prior(sigma_p); 0 = off
    f32: bool = False       # compute_dtype = SI_F32
    per_chain: bool = True  # both branches in EVERY chain; False: in the case as a whole (many short chains)

    @property
    def tols(self):
        return (LP_RTOL_F32, G_RTOL_F32, G_ATOL_F32) if self.f32 else (LP_RTOL_F64, G_RTOL_F64, G_ATOL_F64)


def problem(case):
    return ra._problem(case.model, case.m, case.sigma_m, case.prior)


def value_grad_of(pb):
    """z -> (lp, d lp / d z) of the fp64 oracle, with the optional prior term"""
    def f(z):
        lp, g, _ = so.logdensity_grad(pb.table, pb.w, pb.p, pb.x, pb.y, pb.sigma_m, z)
        if pb.prior > 0.0:
            w = pb.w + pb.p @ z
            lp += so.log_prior(w, pb.prior)
            g = g - pb.p.T @ w / (pb.prior * pb.prior)
        return lp, g
    return f


MUTANTS = ("h_is_sigma2", "no_logq", "fwd_bwd_swapped", "g_stale", "lp_stale", "normals_next_step", "normals_prev_step",
           "normals_next_chain", "e_from_purpose0", "acc_over_itr")


def _randexp_purpose0(seed, chain, step):
    x = philox.philox4x32(philox._ctr(step, chain, 0, 0)[None, :], philox._key(seed)[None, :])
    return float(-np.log(philox._u53(x[:, 1], x[:, 0]))[0])


def oracle_trace(case, value_grad=None, mutant=None):
    """the transition of samplers.mala on the case's Philox chains: (Z M x itr x C, lp itr x C, acc C, G M x itr x C), the shapes and
    the acc of si_sample_mala.  mutant: one of MUTANTS -- the chain a kernel with that mistake would produce."""
    assert mutant is None or mutant in MUTANTS, mutant
    vg = value_grad_of(problem(case)) if value_grad is None else value_grad
    m, itr, s = case.m, case.itr, case.sigma_z
    h = s * s if mutant == "h_is_sigma2" else 0.5 * s * s
    Z = np.empty((m, itr, case.nchains), order="F")
    G = np.empty((m, itr, case.nchains), order="F")
    lps = np.empty((itr, case.nchains), order="F")
    acc = np.empty(case.nchains)
    for c in range(case.nchains):
        chain = case.chain_id0 + c

        def normals(t):
            if mutant == "normals_next_step":
                return philox.normals(case.seed, chain, t + 1, m)
            if mutant == "normals_prev_step" and t > 0:
                return philox.normals(case.seed, chain, t - 1, m)
            if mutant == "normals_next_chain":
                return philox.normals(case.seed, chain + 1, t, m)
            return philox.normals(case.seed, chain, t, m)
        z = s * normals(0)
        lp, g = vg(z)
        Z[:, 0, c], lps[0, c], G[:, 0, c] = z, lp, g
        nacc = 0
        for t in range(1, itr):
            zp = z + h * g + s * normals(t)
            lpp, gp = vg(zp)
            logq = logq_terms(z, g, zp, gp, h, s)[0]
            if mutant == "no_logq":
                logq = 0.0
            elif mutant == "fwd_bwd_swapped":
                logq = -logq
            e_t = _randexp_purpose0(case.seed, chain, t) if mutant == "e_from_purpose0" else philox.randexp(case.seed, chain, t)
            if -e_t < lpp - lp + logq:
                z = zp
                if mutant != "lp_stale":
                    lp = lpp
                if mutant != "g_stale":
                    g = gp
                nacc += 1
            Z[:, t, c], lps[t, c], G[:, t, c] = z, lp, g
        acc[c] = (nacc / itr if mutant == "acc_over_itr" else nacc / (itr - 1)) if itr > 1 else 0.0
    return Z, lps, acc, G


@functools.lru_cache(maxsize=None)
def cached_oracle_trace(case):
    out = oracle_trace(case)
    for a in out:
        a.setflags(write=False)
    return out


def audit_case(case, Z, lp, acc, G, value_grad=None):
    lp_rtol, g_rtol, g_atol = case.tols
    return audit(Z, lp, acc, G, value_grad_of(problem(case)) if value_grad is None else value_grad, case.sigma_z, case.seed,
                 case.chain_id0, lp_rtol, g_rtol, g_atol)


def check_caps(case, rep):
    """conditions on a case, not measurements: both branches in every chain (per_chain = False: in the case as a whole); no
    undecidable step in fp64, at most 5 % with SI_F32"""
    if case.itr > 1:
        if case.per_chain:
            for c, (a, r) in enumerate(zip(rep.chain_accepts, rep.chain_rejects)):
                assert a >= 1 and r >= 1, "chain %d has %d accepts and %d rejects: the case must reach both branches in every chain" % (c, a, r)
        else:
            assert rep.accepts >= 1 and rep.rejects >= 1, "the case has %d accepts and %d rejects" % (rep.accepts, rep.rejects)
    cap = F32_UNDECIDABLE_CAP * rep.steps if case.f32 else 0
    assert rep.undecidable <= cap, "%d undecidable steps of %d (cap %g)" % (rep.undecidable, rep.steps, cap)
    assert rep.steps == (case.itr - 1) * case.nchains


# sigma_z: chosen on the CPU with the oracle alone so that every chain both accepts and rejects.  0.05, the RWMH default, never
# rejects on the small models and never accepts on MODEL_B.
SMALL = ((3, 5), (I,), 17)
RAGGED = ((7, 33, 18, 40, 3), (T, R, S, I), 130)
F32_DENSE = ((6, 30, 2), (T, I), 200)          # the SI_F32 member of tests/test_gpu_grad_batch.py's fallback cases
SOFTPLUS = ((6, 30, 2), (SP, I), 50)           # ... and its softplus member

CASES = [
    Case("small-M2", SMALL, 2, 1.0, True),
    Case("small-M1", SMALL, 1, 0.5, True),
    Case("ragged-M5", RAGGED, 5, 0.2, True),
    Case("A-M33", MODEL_A, 33, 0.2, True),
    Case("A-M65", MODEL_A, 65, 0.2, True),
    Case("A-M33-prior", MODEL_A, 33, 0.2, True, prior=0.7),
    Case("A-M2-high-words", MODEL_A, 2, 0.2, True, seed=2 ** 40 + 7, chain_id0=2 ** 24 + 5),
    Case("B-M3", MODEL_B, 3, 0.005, True, nchains=2, itr=30),
    # (M = 20 accepts every step at 0.01 and rejects nearly every step from 0.011 on)
    Case("B-M20", MODEL_B, 20, 0.0104, True, nchains=2, itr=30),
    Case("A-M2-itr1", MODEL_A, 2, 0.2, True, itr=1),
    # 64 chains of 7 transitions: both branches in the case as a whole, not in every chain
    Case("A-M33x64", MODEL_A, 33, 0.2, True, nchains=64, itr=8, seed=12, per_chain=False),
    # 257 Philox blocks: the 256-thread sweep runs twice.  (sigma_z: 20 weights leave most of the 513 directions flat, so every chain
    #  accepts all 7 steps up to 0.8 and chain 0 up to 1.3; from 1.4 to 3.0 every chain does both, and 2.0 lies in the middle)
    Case("small-M513", SMALL, 513, 2.0, True, itr=8),
    # (14 observations pin the posterior loosely and large steps are accepted.  sigma_z = 1.0 is the largest of 0.5 / 0.8 / 1.0 / 1.2
    #  whose chains stay where the tanh units ahead of the MaxPool are not saturated: at 1.2 a chain reaches |z| = 15, pooling windows
    #  hold several values within sqrt(eps) of each other, the reference's `y ≈ x` rule no longer singles out the maximum and the
    #  oracle's own gradient moves by 1.2 of the tolerance when the rule is replaced by the exact maximum;
    #  tests/test_mala_audit_cpu.py holds that this does not happen at any state of this case)
    Case("conv-f64", ("conv", "conv0"), 5, 1.0, False, nchains=2),
    # (SI_F32 on a Dense chain: the library refuses the gradient of a Conv chain set up with SI_F32)
    Case("dense-f32", F32_DENSE, 4, 0.15, False, nchains=2, f32=True),
    Case("softplus", SOFTPLUS, 4, 0.2, False, nchains=2),
]
CASE_BY_NAME = {c.name: c for c in CASES}
