"""Per-transition audit of a finished elliptical-slice trace (si_sample_ess; samplers.ess_iter restated on the build's Philox stream,
oracle/philox.py) -- TEST INFRASTRUCTURE, no GPU needed.  The sampler is not in the reference.  The manner of tests/rwmh_audit.py:
the audit takes the trace's OWN previous column (z, lp) as given and checks every transition by itself.  With n_0 the M normals of
(chain, step 0, purpose 0), e_t the Exp(1) draw of purpose 1, n_t the M normals of (chain, step t, purpose 9), v_j = u53(x1, x0) of
(chain, step t, purpose 10, block j), nu = sigma_z n_t and logy = lp[t-1] - e_t:

  column 0  Z[:, 0] = sigma_z n_0 within rwmh_audit's 16 2^-53 sigma_z |n_0|; lp[0] within lp_rtol of the oracle at Z[:, 0];
            nev[0] = 1, theta[0] = 0
  stuck     (nev[t] < 0)  nev[t] = -max_evals, theta[t] = 0, Z[:, t] and lp[t] are bit copies of column t - 1
  kept      1 <= nev[t] <= max_evals, and with the DEVICE's own theta[t]
    ellipse   |Z[m, t] - (z cos theta + nu sin theta)[m]| <= K 2^-53 (|z cos theta| + |nu sin theta|)[m] for EVERY m, K = 32
    value     lp[t] within lp_rtol of the oracle at Z[:, t]
    slice     lp[t] > logy - tol(lp[t])
  replay    the bracket on the host: theta_0 = 2 pi v_0, lo = theta_0 - 2 pi, hi = theta_0; zp_j = z cos theta_j + nu sin theta_j,
            lpp_j = the oracle at the HOST's zp_j; after a reject theta_j < 0 ? lo = theta_j : hi = theta_j and
            theta_{j+1} = lo + (hi - lo) v_{j+1}.  A comparison with |lpp_j - logy| > tol(lpp_j) is decidable and must be the
            device's: a reject for j < nev - 1 (for every j < max_evals on a stuck step), a keep at j = nev - 1.  A NaN lpp_j is a
            decidable reject.  While all are decidable theta[t] equals theta_{nev-1} BIT FOR BIT and nev[t] is the replay's count.
            From the first undecidable comparison on only the ellipse, value and slice conditions are held for that transition; it
            is counted (Report.undecidable).
  tol(v)    lp_rtol (|v| + |lp[t-1]|) + 16 2^-53 e_t: rwmh_audit's decision tolerance

K = 32.  Host and device form every angle from identical bits (plain IEEE arithmetic on exact uniforms, no contraction), so theta is
the same double on both sides.  nu = sigma_z n_t is within rwmh_audit's 16 units of 2^-53 (the normals' log, sin / cos and sqrt
against the host libm, the product's rounding).  The device's sin theta and cos theta are within 4 ulp = 8 units (the OpenCL fp64
limit), the host libm's within 1 ulp = 2 units: 10 units each.  Three operations follow that both sides round once each, a unit a
side: z cos theta, nu sin theta and their sum.  The nu term carries 16 + 10 + 2 = 28 units, the z term 10 + 2 = 12, the sum adds 2 of
|z cos theta| + |nu sin theta| at most: under 30 in all, 32 leaves headroom.  tests/test_ess_audit_cpu.py certifies the host's own
share: a float64 replay against a longdouble replay stays under a quarter of K.

oracle_trace(case) is samplers.ess_iter on the case's Philox chains; with a name of MUTANTS, the chain a kernel with that mistake
would produce, each of which the audit must reject on at least one case.  CASES is certified in tests/test_ess_audit_cpu.py on the
oracle alone -- in every fp64 chain a transition with nev = 1, one with nev >= 3 and both shrink sides, no undecidable comparison
-- so that tests/test_gpu_ess.py can hold the same conditions on the device's traces.
"""
import functools
import math
from dataclasses import dataclass, field

import numpy as np

from oracle import philox
from oracle import subspace_oracle as so
from subspaceinference_jl_amd import autoencoder as ae
from subspaceinference_jl_amd import samplers
from tests import advi_audit as aa
from tests import mala_audit as ma
from tests import rwmh_audit as ra
from tests.rwmh_audit import EPS, Z_ULPS, AuditFailure, _bits, _same_bits

LP_RTOL_F64, LP_RTOL_F32 = ra.LP_RTOL_F64, ra.LP_RTOL_F32
F32_UNDECIDABLE_CAP = ra.F32_UNDECIDABLE_CAP
ELLIPSE_ULPS = 32.0
P_NU, P_ANGLE = 9, 10
TWO_PI = samplers.ESS_TWO_PI


def uniform(seed, chain, step, block):
    """v_block = u53(x1, x0) of (chain, step, purpose 10, block)"""
    x = philox.philox4x32(philox._ctr(step, chain, P_ANGLE, block)[None, :], philox._key(seed)[None, :])
    return float(philox._u53(x[:, 1], x[:, 0])[0])


def nu_normals(seed, chain, step, m, purpose=P_NU):
    return aa.normals(seed, chain, step, purpose, 0, (m + 1) // 2)[:m]


def philox_draw(seed, chain, m):
    """the draw source of samplers.ess_iter on the Philox streams of chain `chain`: what si_sample_ess draws"""
    def draw(kind, t, j):
        if kind == samplers.ESS_DRAW_INITIAL:
            return philox.normals(seed, chain, 0, m)
        if kind == samplers.ESS_DRAW_NU:
            return nu_normals(seed, chain, t, m)
        if kind == samplers.ESS_DRAW_LEVEL:
            return philox.randexp(seed, chain, t)
        return uniform(seed, chain, t, j)
    return draw


@dataclass
class Report:
    kept: int = 0
    stuck: int = 0
    undecidable: int = 0            # transitions with an undecidable comparison
    comparisons: int = 0            # decidable comparisons replayed
    worst_z_ratio: float = 0.0
    worst_lp_rel: float = 0.0
    min_margin_over_tol: float = np.inf
    chain_nev1: list = field(default_factory=list)      # per chain: transitions with nev = 1
    chain_nev3: list = field(default_factory=list)      # ... with nev >= 3
    chain_lo: list = field(default_factory=list)        # ... shrinks that moved lo (theta < 0)
    chain_hi: list = field(default_factory=list)        # ... shrinks that moved hi
    chain_stuck: list = field(default_factory=list)
    evals: int = 0                                      # sum of |nev| without column 0
    rounds: int = 0                                     # sum over transitions of the largest |nev| among the chains

    @property
    def steps(self):
        return self.kept + self.stuck

    def line(self):
        def short(v):
            return v if len(v) <= 8 else sum(v)
        return ("kept %d, stuck %d, undecidable %d, comparisons %d, evals %d, rounds %d, nev=1 %s, nev>=3 %s, lo %s, hi %s, worst z ratio %.3f, "
                "worst lp rel %.2e, min |margin| / tol %.2e" % (self.kept, self.stuck, self.undecidable, self.comparisons, self.evals, self.rounds,
                                                                short(self.chain_nev1), short(self.chain_nev3), short(self.chain_lo),
                                                                short(self.chain_hi), self.worst_z_ratio, self.worst_lp_rel, self.min_margin_over_tol))


def ellipse_point(z, nu, theta, dtype=np.float64):
    """z cos theta + nu sin theta, every product and the sum rounded by itself in `dtype`; also the bound's scale"""
    if dtype is np.float64:
        cs, sn = math.cos(theta), math.sin(theta)
    else:
        cs, sn = np.cos(dtype(theta)), np.sin(dtype(theta))
    a, b = np.asarray(z, dtype=dtype) * cs, np.asarray(nu, dtype=dtype) * sn
    return a + b, np.abs(a) + np.abs(b)


def audit(Z, lp, nev, theta, density, sigma_z, max_evals, seed, chain_id0, lp_rtol=LP_RTOL_F64):
    """Z: M x itr x C, lp / nev / theta: itr x C.  density(z): the host fp64 log-density.  Raises AuditFailure naming chain, step and
    the first offending component; returns a Report."""
    Z, lp, theta = (np.asarray(a, dtype=np.float64) for a in (Z, lp, theta))
    nev = np.asarray(nev)
    if Z.ndim != 3 or lp.shape != Z.shape[1:] or nev.shape != lp.shape or theta.shape != lp.shape:
        raise AuditFailure("shapes: Z %s, lp %s, nev %s, theta %s" % (Z.shape, lp.shape, nev.shape, theta.shape))
    nm, itr, nch = Z.shape
    rep = Report()

    def fail(c, t, what):
        raise AuditFailure("chain %d (Philox chain %d), step %d: %s" % (c, chain_id0 + c, t, what))

    def check_lp(c, t, ref, what):
        rel = abs(lp[t, c] - ref) / abs(ref) if ref != 0.0 else abs(lp[t, c])
        if not rel <= lp_rtol:
            fail(c, t, "lp is %r, %s is %r: relative error %.3e > %g" % (lp[t, c], what, ref, rel, lp_rtol))
        rep.worst_lp_rel = max(rep.worst_lp_rel, float(rel))

    def check_z(c, t, zt, target, scale, ulps, what):
        err, bound = np.abs(zt - target), ulps * EPS * scale
        bad = np.flatnonzero(~(err <= bound))
        if bad.size:
            m = int(bad[0])
            fail(c, t, "component %d is %r, expected %s = %r: off by %.3g of the %g-unit bound (%d of %d components off)"
                 % (m, zt[m], what, target[m], err[m] / bound[m] if bound[m] > 0 else np.inf, ulps, bad.size, nm))
        rep.worst_z_ratio = max(rep.worst_z_ratio, float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0.0))))

    for c in range(nch):
        chain = chain_id0 + c
        z0 = sigma_z * philox.normals(seed, chain, 0, nm)
        check_z(c, 0, Z[:, 0, c], z0, np.abs(z0), Z_ULPS, "sigma_z n_0")
        check_lp(c, 0, density(Z[:, 0, c]), "the density at Z[:, 0]")
        if nev[0, c] != 1 or _bits(theta[0:1, c])[0] != 0:
            fail(c, 0, "column 0 has nev = %r and theta = %r, expected 1 and 0" % (nev[0, c], theta[0, c]))
        n1 = n3 = nlo = nhi = nstuck = 0
        for t in range(1, itr):
            zprev, lprev, zt = Z[:, t - 1, c], lp[t - 1, c], Z[:, t, c]
            k, th = int(nev[t, c]), float(theta[t, c])
            nu = sigma_z * nu_normals(seed, chain, t, nm)
            e_t = philox.randexp(seed, chain, t)
            logy = lprev - e_t
            if np.isnan(logy):
                fail(c, t, "the slice's level is NaN (lp[t-1] = %r)" % lprev)

            def tol(v):
                return lp_rtol * (abs(v) + abs(lprev)) + Z_ULPS * EPS * e_t
            if k < 0:
                if k != -max_evals or _bits(theta[t:t + 1, c])[0] != 0:
                    fail(c, t, "a stuck step has nev = %r and theta = %r, expected %d and 0" % (k, th, -max_evals))
                if not _same_bits(zt, zprev) or _bits(lp[t:t + 1, c])[0] != _bits(lp[t - 1:t, c])[0]:
                    fail(c, t, "a stuck step (nev = %d) whose column is not a bit copy of column t - 1" % k)
                nstuck += 1
            else:
                if not 1 <= k <= max_evals:
                    fail(c, t, "nev is %r, outside 1 .. max_evals = %d" % (k, max_evals))
                target, scale = ellipse_point(zprev, nu, th)
                check_z(c, t, zt, target, scale, ELLIPSE_ULPS, "z cos theta + nu sin theta at the trace's theta = %r" % th)
                ref = density(zt)
                check_lp(c, t, ref, "the density at Z[:, t]")
                if not lp[t, c] > logy - tol(lp[t, c]):
                    fail(c, t, "the kept point is not on the slice: lp[t] = %r, logy = lp[t-1] - e_t = %r - %r = %r" % (lp[t, c], lprev, e_t, logy))
                n1 += k == 1
                n3 += k >= 3
            # ---- the replay
            ang = TWO_PI * uniform(seed, chain, t, 0)
            lo, hi = ang - TWO_PI, ang
            last = (k if k > 0 else max_evals) - 1
            decided = True
            for j in range(last + 1):
                lpp = density(ellipse_point(zprev, nu, ang)[0])
                margin = lpp - logy
                if not np.isnan(margin) and abs(margin) <= tol(lpp):
                    rep.undecidable += 1
                    decided = False
                    break
                keep = bool(margin > 0.0)      # (a NaN is a decidable reject)
                rep.comparisons += 1
                if not np.isnan(margin):
                    rep.min_margin_over_tol = min(rep.min_margin_over_tol, abs(margin) / tol(lpp))
                want_keep = k > 0 and j == last
                if keep != want_keep:
                    fail(c, t, "evaluation %d of the bracket at theta = %r: the trace (nev = %d) %s, but lpp - logy = %r - %r = %r (tolerance %.3g) says %s"
                         % (j + 1, ang, k, "kept it" if want_keep else "went on", lpp, logy, margin, tol(lpp), "keep" if keep else "shrink"))
                if keep or j == last:
                    break
                if ang < 0.0:
                    lo = ang
                    nlo += 1
                else:
                    hi = ang
                    nhi += 1
                ang = lo + (hi - lo) * uniform(seed, chain, t, j + 1)
            if decided and k > 0 and _bits(np.array([ang]))[0] != _bits(theta[t:t + 1, c])[0]:
                fail(c, t, "theta is %r, the replay's angle after %d evaluations is %r (bracket [%r, %r])" % (th, k, ang, lo, hi))
        rep.kept += (itr - 1) - nstuck
        rep.stuck += nstuck
        rep.chain_nev1.append(int(n1))
        rep.chain_nev3.append(int(n3))
        rep.chain_lo.append(nlo)
        rep.chain_hi.append(nhi)
        rep.chain_stuck.append(nstuck)
    if itr > 1:
        a = np.abs(nev[1:, :].astype(np.int64))
        rep.evals, rep.rounds = int(a.sum()), int(a.max(axis=1).sum())
    return rep


# ----------------------------------------------------------------------------------------------- problems and cases
R, T, S, I = ra.R, ra.T, ra.S, ra.I
MODEL_A, MODEL_B = ra.MODEL_A, ra.MODEL_B
SMALL, RAGGED, F32_DENSE, SOFTPLUS = ma.SMALL, ma.RAGGED, ma.F32_DENSE, ma.SOFTPLUS


@dataclass(frozen=True)
class Case:
    name: str
    model: tuple            # (dims, acts, B) | ("conv", name) as rwmh_audit's | ("lik", name of a likelihood_cases.SAMPLER_PROBLEMS entry)
                            # | ("decoder", N of decoder_cases.MODELS) | ("node", name of a node_cases case)
    m: int
    sigma_z: float          # the prior's standard deviation on z
    nchains: int = 3
    itr: int = 30
    sigma_m: float = 0.8
    seed: int = 11
    chain_id0: int = 2
    prior: float = 0.0      # set_prior(sigma_p); 0 = off
    f32: bool = False       # compute_dtype = SI_F32
    per_chain: bool = True  # the conditions hold in EVERY chain; False: in the case as a whole (many short chains)
    max_evals: int = 128

    @property
    def lp_rtol(self):
        return LP_RTOL_F32 if self.f32 else LP_RTOL_F64

    @property
    def kind(self):
        return self.model[0] if self.model[0] in ("lik", "decoder", "node") else "chain"


DECODER_SEED = 43


def decoder_of(case):
    """the decoder_cases target model and the decoder (table, parameters) of a ("decoder", N) case"""
    from tests import decoder_cases as dc
    pb = dc.problem(case.model[1])
    return pb, dc.random_decoder((case.m, 4, pb.n), (dc.T, dc.I), seed=DECODER_SEED)


@functools.lru_cache(maxsize=None)
def density_of(case):
    """z -> the host fp64 log-density of the case, memoised by the bytes of z"""
    from tests import likelihood_cases as lc
    if case.kind == "lik":
        f = lc.sampler_problem(case.model[1])[0].density
    elif case.kind == "decoder":
        pb, (dtable, wdec) = decoder_of(case)

        def f(z):
            yhat = so.forward([list(r) for r in pb.table], ae.weights(pb.w_swa, dtable, wdec, z), pb.x)
            return so.mvnormal_logpdf_iso(pb.y.reshape(-1, order="F"), yhat.reshape(-1, order="F"), pb.sigma_m)[0]
    elif case.kind == "node":
        from tests import node_cases as nc
        ncase = nc.CASE_BY_NAME.get(case.model[1]) or getattr(nc, case.model[1])
        f = nc.density(ncase, nc.problem(ncase))
    else:
        f = ra._problem(case.model, case.m, case.sigma_m, case.prior).density
    return lc.cached(f)


MUTANTS = ("shrink_wrong_side", "first_bracket_pi", "nu_unscaled", "logy_plus_e", "same_v", "sin_cos_swapped", "lp_stale", "nu_purpose0",
           "normals_next_step", "normals_next_chain", "theta_not_recorded", "nev_off_by_one")


def _mutant_chain(density, m, itr, sigma_z, seed, chain, max_evals, mutant):
    """the statements of samplers.ess_iter on the Philox streams with one mistake (mutant None: none, bit for bit ess_iter's results)"""
    z = sigma_z * philox.normals(seed, chain, 0, m)
    lp = density(z)
    zs, lps = np.empty((m, itr), order="F"), np.empty(itr)
    nev, thetas = np.zeros(itr, dtype=np.int32), np.zeros(itr)
    zs[:, 0], lps[0], nev[0] = z, lp, 1
    for t in range(1, itr):
        if mutant == "nu_purpose0":
            n = philox.normals(seed, chain, t, m)
        elif mutant == "normals_next_step":
            n = nu_normals(seed, chain, t + 1, m)
        elif mutant == "normals_next_chain":
            n = nu_normals(seed, chain + 1, t, m)
        else:
            n = nu_normals(seed, chain, t, m)
        nu = n if mutant == "nu_unscaled" else sigma_z * n
        e = philox.randexp(seed, chain, t)
        logy = lp + e if mutant == "logy_plus_e" else lp - e
        theta = TWO_PI * uniform(seed, chain, t, 0)
        lo, hi = theta - (math.pi if mutant == "first_bracket_pi" else TWO_PI), theta
        k = 0
        while True:
            cs, sn = math.cos(theta), math.sin(theta)
            zp = z * sn + nu * cs if mutant == "sin_cos_swapped" else z * cs + nu * sn
            lpp = density(zp)
            k += 1
            if lpp > logy:
                z = zp
                if mutant != "lp_stale":
                    lp = lpp
                n_ev = k
                break
            if k == max_evals:
                n_ev, theta = -max_evals, 0.0
                break
            if (theta < 0.0) != (mutant == "shrink_wrong_side"):
                lo = theta
            else:
                hi = theta
            theta = lo + (hi - lo) * uniform(seed, chain, t, 1 if mutant == "same_v" else k)
        zs[:, t], lps[t] = z, lp
        nev[t], thetas[t] = (n_ev + 1 if mutant == "nev_off_by_one" and n_ev > 0 else n_ev), (0.0 if mutant == "theta_not_recorded" else theta)
    return zs, lps, nev, thetas


def oracle_trace(case, mutant=None, density=None):
    """samplers.ess_iter on the case's Philox chains: (Z M x itr x C, lp itr x C, nev itr x C int32, theta itr x C), the shapes of
    si_sample_ess.  mutant: one of MUTANTS -- the chain a kernel with that mistake would produce."""
    assert mutant is None or mutant in MUTANTS, mutant
    dens = density_of(case) if density is None else density
    Z = np.empty((case.m, case.itr, case.nchains), order="F")
    lps = np.empty((case.itr, case.nchains), order="F")
    nev = np.zeros((case.itr, case.nchains), dtype=np.int32, order="F")
    theta = np.zeros((case.itr, case.nchains), order="F")
    for c in range(case.nchains):
        chain = case.chain_id0 + c
        if mutant is None:
            stats = []
            Z[:, :, c], lps[:, c] = samplers.ess_iter(dens, case.m, case.itr, case.sigma_z, philox_draw(case.seed, chain, case.m), case.max_evals,
                                                      stats=stats)
            nev[:, c], theta[:, c] = [s[0] for s in stats], [s[1] for s in stats]
        else:
            Z[:, :, c], lps[:, c], nev[:, c], theta[:, c] = _mutant_chain(dens, case.m, case.itr, case.sigma_z, case.seed, chain,
                                                                          case.max_evals, mutant)
    return Z, lps, nev, theta


@functools.lru_cache(maxsize=None)
def cached_oracle_trace(case):
    out = oracle_trace(case)
    for a in out:
        a.setflags(write=False)
    return out


def audit_case(case, Z, lp, nev, theta, density=None):
    return audit(Z, lp, nev, theta, density_of(case) if density is None else density, case.sigma_z, case.max_evals, case.seed, case.chain_id0,
                 case.lp_rtol)


def check_caps(case, rep):
    """conditions on a case, not measurements: in every fp64 chain (per_chain = False: in the case as a whole) a transition with
    nev = 1, one with nev >= 3 and a shrink on either side; no undecidable comparison in fp64, at most 5 % of the transitions with
    SI_F32; max_evals < 3: a stuck step and a kept one in place of nev >= 3"""
    assert rep.steps == (case.itr - 1) * case.nchains
    cap = F32_UNDECIDABLE_CAP * rep.steps if case.f32 else 0
    assert rep.undecidable <= cap, "%d undecidable transitions of %d (cap %g)" % (rep.undecidable, rep.steps, cap)
    if case.itr == 1:
        return
    if case.max_evals < 3:
        assert rep.stuck >= 1 and rep.kept >= 1, "the case has %d stuck and %d kept steps" % (rep.stuck, rep.kept)
        return
    assert rep.stuck == 0, "%d stuck steps at max_evals = %d" % (rep.stuck, case.max_evals)
    rows = list(zip(rep.chain_nev1, rep.chain_nev3, rep.chain_lo, rep.chain_hi))
    if not case.per_chain:
        rows = [tuple(sum(v) for v in zip(*rows))]
    if case.f32:
        return
    for c, (n1, n3, nlo, nhi) in enumerate(rows):
        assert n1 >= 1 and n3 >= 1 and nlo >= 1 and nhi >= 1, (
            "chain %d has %d transitions with nev = 1, %d with nev >= 3, %d shrinks of lo and %d of hi: the case must reach all four"
            % (c, n1, n3, nlo, nhi))


# sigma_z (here the prior's standard deviation on z, not a step size) and the seeds: chosen on the CPU with the oracle alone so that
# every fp64 chain has a transition that keeps its first point, one that shrinks at least twice and shrinks on both sides.  The
# problems are mala_audit's; their P has |P z| ~ 0.1 |z| / sqrt(M / 4), so a prior of a few units lets the likelihood cut the
# ellipse where one of 0.2 (MALA's step) keeps nearly every first point.
CASES = [
    Case("small-M2", SMALL, 2, 3.0),
    Case("small-M1", SMALL, 1, 3.0),
    Case("ragged-M5", RAGGED, 5, 3.0),
    Case("A-M33", MODEL_A, 33, 3.0),
    Case("A-M33-prior", MODEL_A, 33, 3.0, prior=0.7),
    Case("A-M2-high-words", MODEL_A, 2, 3.0, seed=2 ** 40 + 7, chain_id0=2 ** 24 + 5),
    Case("B-M3", MODEL_B, 3, 0.5, nchains=2, itr=20),
    Case("A-M2-itr1", MODEL_A, 2, 3.0, itr=1),
    # 64 chains of 7 transitions: the conditions in the case as a whole, not in every chain
    Case("A-M33x64", MODEL_A, 33, 3.0, nchains=64, itr=8, seed=12, per_chain=False),
    # 257 Philox blocks: the 256-thread sweep runs twice
    Case("small-M513", SMALL, 513, 3.0, nchains=2, itr=20),
    Case("conv-f64", ("conv", "conv0"), 5, 3.0, nchains=2),
    Case("dense-f32", F32_DENSE, 4, 3.0, nchains=2, f32=True),
    Case("softplus", SOFTPLUS, 4, 3.0, nchains=2),
    Case("lik-cat3", ("lik", "cat3"), 3, 3.0, nchains=2),
    Case("decoder-N65", ("decoder", 65), 3, 3.0, nchains=2),
    Case("node-fixed-relu", ("node", "RWMH_FIXED"), 2, 3.0, nchains=2),
    # the cap: after two evaluations off the slice the state is kept
    Case("A-M5-cap2", MODEL_A, 5, 3.0, max_evals=2),
]
CASE_BY_NAME = {c.name: c for c in CASES}
