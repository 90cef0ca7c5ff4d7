"""Per-transition audit of a finished RWMH trace (reference src/space_inference.jl:111-116; the build's Philox stream,
oracle/philox.py) -- TEST INFRASTRUCTURE, no GPU needed.

A whole-chain comparison with the oracle holds only while no accept decision flips and lets one ulp of libm difference
compound over the chain; bit identity between the sampler forms shows that they agree, not that any of them is right.
The audit takes the trace's OWN previous state as given and checks every transition by itself:

  step 0   Z[:, 0] = sigma_z n_0 (z bound below), lp[0] = density(Z[:, 0]) within lp_rtol
  step t   exactly one of
    reject   Z[:, t] == Z[:, t-1] and lp[t] == lp[t-1], bit for bit
    accept   |Z[m, t] - (Z[m, t-1] + sigma_z n_t[m])| <= 16 2^-53 (|Z[m, t-1]| + sigma_z |n_t[m]|) for EVERY m, and
             lp[t] = density(Z[:, t]) within lp_rtol
  decision with zp = Z[:, t-1] + sigma_z n_t on the host: margin = density(zp) - lp[t-1] + e_t,
           tol = lp_rtol (|density(zp)| + |lp[t-1]|) + 16 2^-53 e_t; |margin| > tol => accepted exactly when margin > 0
           (|margin| <= tol: undecidable, counted, skipped for this check only)
  count    acc[c] (itr - 1) == number of accept-classified steps, exactly (itr == 1: acc == 0)
  weights  (optional) W[:, t] == W[:, t-1] on reject steps and W[:, t] == reconstruct(Z[:, t]) on every step, bit for bit

The 16 ulp of the z bound: host and device form t = 2 pi u2 and -2 log(u1) from identical bits; the OpenCL fp64 limits bound the
device's log (3 ulp), sin / cos (4 ulp) and sqrt (correctly rounded), the host libm adds at most 1 ulp each; the sqrt halves the
log's error; three roundings follow (r cos t, sigma_z n, the add): under 10 ulp in all, 16 leaves headroom.

The case list at the bottom names the problems, sizes and set_chain_loop modes at which the device samplers branch on M;
tests/test_rwmh_audit_cpu.py certifies every one of them on the oracle alone (both branches in every chain, no undecidable
step), so that tests/test_gpu_rwmh_audit.py, which runs the list on the device and audits the trace of each mode, can hold the caps
as conditions.
"""
import functools
from dataclasses import dataclass, field

import numpy as np

from oracle import philox
from oracle import subspace_oracle as so

Z_ULPS = 16.0
EPS = 2.0 ** -53
LP_RTOL_F64 = 1e-10    # the random-sweep log-density tolerance of tests/test_gpu_parity.py
LP_RTOL_F32 = 1e-5     # tests/test_gpu_f32.py
F32_UNDECIDABLE_CAP = 0.05


class AuditFailure(AssertionError):
    pass


@dataclass
class Report:
    accepts: int = 0
    rejects: int = 0
    undecidable: int = 0
    worst_z_ratio: float = 0.0
    worst_lp_rel: float = 0.0
    min_margin_over_tol: float = np.inf
    chain_accepts: list = field(default_factory=list)
    chain_rejects: list = field(default_factory=list)

    @property
    def steps(self):
        return self.accepts + self.rejects

    def line(self):
        return "accepts %d, rejects %d, undecidable %d, worst z ratio %.3f, worst lp rel %.2e, min |margin| / tol %.2e" % (
            self.accepts, self.rejects, self.undecidable, self.worst_z_ratio, self.worst_lp_rel, self.min_margin_over_tol)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _z_bound(zprev, step_noise):
    return Z_ULPS * EPS * (np.abs(zprev) + np.abs(step_noise))


def _explain(zt, zprev, m, sigma_z, seed, chain, t, nm):
    """what else the offending component is consistent with (a hint for the failure message only)"""
    def fits(noise):
        return abs(zt[m] - (zprev[m] + sigma_z * noise)) <= _z_bound(zprev[m], sigma_z * noise)
    hints = []
    if _bits(zt[m:m + 1])[0] == _bits(zprev[m:m + 1])[0]:
        hints.append("it did not move")
    n_t = philox.normals(seed, chain, t, nm)
    others = [j for j in range(nm) if j != m and fits(n_t[j])]
    if others:
        hints.append("it moved by the draw of component %d (Philox block %d, own block %d)" % (others[0], others[0] // 2, m // 2))
    for dt in (1, -1):
        if t + dt >= 0 and fits(philox.normals(seed, chain, t + dt, nm)[m]):
            hints.append("it moved by the draw of step %d" % (t + dt))
    for dc in (1, -1):
        if chain + dc >= 0 and fits(philox.normals(seed, chain + dc, t, nm)[m]):
            hints.append("it moved by the draw of Philox chain %d" % (chain + dc))
    return "; ".join(hints) if hints else "no neighbouring draw explains it"


def audit(Z, lp, acc, density, sigma_z, seed, chain_id0, lp_rtol, W=None, reconstruct=None):
    """Z: M x itr x C, lp: itr x C, acc: C.  density(z): the host fp64 log-density.  Raises AuditFailure naming chain, step and the
    first offending component; returns a Report."""
    Z = np.asarray(Z, dtype=np.float64)
    lp = np.asarray(lp, dtype=np.float64)
    acc = np.asarray(acc, dtype=np.float64)
    if Z.ndim != 3 or lp.shape != Z.shape[1:] or acc.shape != (Z.shape[2],):
        raise AuditFailure("shapes: Z %s, lp %s, acc %s" % (Z.shape, lp.shape, acc.shape))
    nm, itr, nch = Z.shape
    if W is not None and (reconstruct is None or W.shape[1:] != (itr, nch)):
        raise AuditFailure("W needs reconstruct and the shape N x itr x C, got %s" % (W.shape,))
    rep = Report()

    def fail(c, t, what):
        raise AuditFailure("chain %d (Philox chain %d), step %d: %s" % (c, chain_id0 + c, t, what))

    def check_z(c, t, zt, zprev, noise):
        target = zprev + noise
        err, bound = np.abs(zt - target), _z_bound(zprev, noise)
        bad = np.flatnonzero(~(err <= bound))
        if bad.size:
            m = int(bad[0])
            fail(c, t, "component %d is %r, expected %r + sigma_z * %r = %r: off by %.3g of the %g-ulp bound (%d of %d components off; %s)" % (
                m, zt[m], zprev[m], noise[m] / sigma_z, target[m], err[m] / bound[m] if bound[m] > 0 else np.inf, Z_ULPS, bad.size, nm,
                _explain(zt, zprev, m, sigma_z, seed, chain_id0 + c, t, nm)))
        ratio = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0.0)   # (bound == 0: err == 0 here, the exact case)
        rep.worst_z_ratio = max(rep.worst_z_ratio, float(np.max(ratio)))

    def check_lp(c, t, got, ref, what):
        rel = abs(got - ref) / abs(ref) if ref != 0.0 else abs(got)
        if not rel <= lp_rtol:
            fail(c, t, "lp is %r, %s is %r: relative error %.3e > %g" % (got, what, ref, rel, lp_rtol))
        rep.worst_lp_rel = max(rep.worst_lp_rel, float(rel))

    def check_w(c, t, rejected):
        if W is None:
            return
        if rejected and not _same_bits(W[:, t, c], W[:, t - 1, c]):
            r = int(np.flatnonzero(_bits(W[:, t, c]) != _bits(W[:, t - 1, c]))[0])
            fail(c, t, "a reject step, but weight %d changed from %r to %r" % (r, W[r, t - 1, c], W[r, t, c]))
        ref = np.asarray(reconstruct(Z[:, t, c])).reshape(-1)
        if not _same_bits(W[:, t, c], ref):
            r = int(np.flatnonzero(_bits(W[:, t, c]) != _bits(ref))[0])
            fail(c, t, "weight %d is %r, reconstruct(Z[:, t]) gives %r" % (r, W[r, t, c], ref[r]))

    for c in range(nch):
        chain = chain_id0 + c
        zero = np.zeros(nm)
        check_z(c, 0, Z[:, 0, c], zero, sigma_z * philox.normals(seed, chain, 0, nm))
        check_lp(c, 0, lp[0, c], density(Z[:, 0, c]), "density(Z[:, 0])")
        check_w(c, 0, False)
        n_acc = n_rej = 0
        for t in range(1, itr):
            zprev, zt = Z[:, t - 1, c], Z[:, t, c]
            noise = sigma_z * philox.normals(seed, chain, t, nm)
            zp = zprev + noise
            if _same_bits(zt, zprev):
                if _bits(lp[t:t + 1, c])[0] != _bits(lp[t - 1:t, c])[0]:
                    fail(c, t, "Z[:, t] is a bit copy of Z[:, t-1] (a reject) but lp changed from %r to %r" % (lp[t - 1, c], lp[t, c]))
                accepted = False
                n_rej += 1
            else:
                check_z(c, t, zt, zprev, noise)
                accepted = True
                n_acc += 1
            lpp = density(zp)
            if accepted:
                check_lp(c, t, lp[t, c], lpp if _same_bits(zt, zp) else density(zt), "density(Z[:, t])")
            e_t = philox.randexp(seed, chain, t)
            margin = lpp - lp[t - 1, c] + e_t
            tol = lp_rtol * (abs(lpp) + abs(lp[t - 1, c])) + Z_ULPS * EPS * e_t
            if abs(margin) > tol:
                rep.min_margin_over_tol = min(rep.min_margin_over_tol, abs(margin) / tol)
                if accepted != (margin > 0.0):
                    fail(c, t, "the trace %s, but density(zp) - lp[t-1] + e_t = %r - %r + %r = %r (tolerance %.3g) says %s" % (
                        "accepted" if accepted else "rejected", lpp, lp[t - 1, c], e_t, margin, tol, "accept" if margin > 0.0 else "reject"))
            elif not np.isnan(margin):
                rep.undecidable += 1
            else:
                fail(c, t, "the decision margin is NaN (density(zp) = %r, lp[t-1] = %r)" % (lpp, lp[t - 1, c]))
            check_w(c, t, not accepted)
        want = n_acc / (itr - 1) if itr > 1 else 0.0
        if acc[c] != want:
            raise AuditFailure("chain %d (Philox chain %d): acc is %r, the trace holds %d accepted of %d steps (%r)" % (
                c, chain, acc[c], n_acc, itr - 1, want))
        rep.accepts += n_acc
        rep.rejects += n_rej
        rep.chain_accepts.append(n_acc)
        rep.chain_rejects.append(n_rej)
    return rep


def check_caps(rep, f32=False):
    """conditions on a case, not measurements: both branches in every chain; no undecidable step in fp64, at most 5 % with SI_F32"""
    for c, (a, r) in enumerate(zip(rep.chain_accepts, rep.chain_rejects)):
        assert a >= 1 and r >= 1, "chain %d has %d accepts and %d rejects: the case must reach both branches in every chain" % (c, a, r)
    cap = F32_UNDECIDABLE_CAP * rep.steps if f32 else 0
    assert rep.undecidable <= cap, "%d undecidable steps of %d (cap %g)" % (rep.undecidable, rep.steps, cap)


# ----------------------------------------------------------------------------------------------- problems and cases
R, T, S, I = so.ACT_RELU, so.ACT_TANH, so.ACT_SIGMOID, so.ACT_IDENTITY

MODEL_A = ((16, 64, 2), (T, I), 200)                         # N = 1218: the one-workgroup loop's class
MODEL_B = ((2, 200, 50, 50, 50, 1), (R, R, R, R, I), 1000)   # docs/src/nn_example.md:112-118: the persistent grid loop's class
MODEL_C = ((6, 40, 24, 9), (R, R, S), 900)                   # a wide head with an activation of its own: no fused head
# (input (W, H, C), spec, B) -- the first case of tests/test_gpu_conv.py, kept here as data so that this module imports no GPU
# test module; tests/test_gpu_rwmh_audit.py asserts that the two are the same
CONV_MODELS = {
    "conv0": ((6, 6, 2), [("conv", (3, 3), 4, T, (1, 1), (1, 1)), ("maxpool", (2, 2)), ("conv", (2, 2), 3, S, (2, 1), (0, 1)),
                          ("flatten",), ("dense", 5, T), ("dense", 2, I)], 7),
}


@dataclass(frozen=True)
class Case:
    name: str
    model: tuple            # (dims, acts, B), or ("conv", name of a spec in CONV_MODELS)
    m: int
    modes: tuple            # set_chain_loop modes to run, in order
    nchains: int = 3
    itr: int = 60
    sigma_z: float = 0.05
    sigma_m: float = 0.8
    seed: int = 11
    chain_id0: int = 2
    prior: float = 0.0      # set_prior(sigma_p); 0 = off
    f32: bool = False       # compute_dtype = SI_F32
    how: str = "sample"     # "sample" | "weights" (sample_rwmh_weights) | "stepwise" (rwmh_begin / step_eval / step_accept / end)

    @property
    def lp_rtol(self):
        return LP_RTOL_F32 if self.f32 else LP_RTOL_F64


@dataclass(frozen=True)
class Problem:
    table: list
    n: int
    w: np.ndarray
    p: np.ndarray
    x: np.ndarray
    y: np.ndarray
    sigma_m: float
    prior: float

    def density(self, z):
        lp = so.logdensity(self.table, self.w, self.p, self.x, self.y, self.sigma_m, z)
        if self.prior > 0.0:
            lp += so.log_prior(self.w + self.p @ z, self.prior)
        return lp

    def reconstruct(self, z):
        return so.reconstruct(self.w, self.p, z)


@functools.lru_cache(maxsize=None)
def _problem(model, m, sigma_m, prior):
    if model[0] == "conv":
        whc, spec, b = CONV_MODELS[model[1]]
        rng = np.random.default_rng(100)
        table, n = so.conv_table(spec, whc)
        x = np.asfortranarray(rng.standard_normal((whc[0] * whc[1] * whc[2], b)))
        w = 0.3 * rng.standard_normal(n)
        y = np.asfortranarray(rng.standard_normal(so.forward(table, w, x).shape))
    else:
        dims, acts, b = model
        rng = np.random.default_rng(sum(dims) + b + m)
        table, n = so.layer_table(list(dims), list(acts))
        x, y = rng.standard_normal((dims[0], b)), rng.standard_normal((dims[-1], b))
        w = 0.3 * rng.standard_normal(n)
    p = np.asfortranarray(0.05 / np.sqrt(m / 4.0) * rng.standard_normal((n, m)))   # |P z| independent of M: acceptance stays near 1/2
    for a in (x, y, w, p):
        a.setflags(write=False)
    return Problem(table, n, w, p, x, y, sigma_m, prior)


def problem(case):
    return _problem(case.model, case.m, case.sigma_m, case.prior)


def oracle_trace(case, density=None):
    """so.rwmh on the case's Philox chains: (Z M x itr x C, lp itr x C, acc C), the shapes and the acc of si_sample_rwmh"""
    pb = problem(case)
    dens = pb.density if density is None else density
    z = np.empty((case.m, case.itr, case.nchains), order="F")
    lp = np.empty((case.itr, case.nchains), order="F")
    acc = np.empty(case.nchains)
    for c in range(case.nchains):
        z[:, :, c], lp[:, c], nacc = so.rwmh(dens, case.m, case.itr, case.sigma_z, case.seed, chain=case.chain_id0 + c)
        acc[c] = nacc / (case.itr - 1) if case.itr > 1 else 0.0
    return z, lp, acc


@functools.lru_cache(maxsize=None)
def cached_oracle_trace(case):
    out = oracle_trace(case)
    for a in out:
        a.setflags(write=False)
    return out


def audit_case(case, Z, lp, acc, W=None, reconstruct=None):
    pb = problem(case)
    return audit(Z, lp, acc, pb.density, case.sigma_z, case.seed, case.chain_id0, case.lp_rtol, W=W, reconstruct=reconstruct)


def _cases():
    out = []
    # A: launch-per-step kernels (mode 0), the fused tail (mode 2) and the one-workgroup loop (mode 1) from one Philox block to the
    # loop's limit of one z element per thread; odd M leave the last block half used
    for m in (1, 2, 33, 64, 65, 257, 1023, 1024):
        out.append(Case("A-M%d" % m, MODEL_A, m, (0, 2, 1), itr=40 if m >= 1023 else 60))
    out.append(Case("A'-M1025", MODEL_A, 1025, (1, 0), nchains=2, itr=40))
    for m in (31, 33, 65, 256):
        out.append(Case("B-M%d" % m, MODEL_B, m, (1,), nchains=2, itr=40))
    out.append(Case("B'-M127", MODEL_B, 127, (3,), nchains=2, itr=40))
    for m in (129, 257):
        out.append(Case("B'-M%d" % m, MODEL_B, m, (3, 1), nchains=2, itr=40))
    out.append(Case("C-M37", MODEL_C, 37, (1, 0), itr=40))
    out.append(Case("D-M33x64", MODEL_A, 33, (1, 0), nchains=64, itr=12, seed=12))
    out.append(Case("E-M33-prior", MODEL_A, 33, (1, 0), prior=0.7))
    out.append(Case("F-M65-stepwise", MODEL_A, 65, (1,), how="stepwise", itr=40))
    # (14 observations pin the posterior loosely: at sigma_z = 0.05 one of the chains never rejects in 40 steps, at 0.8 a fifth of the steps do)
    out.append(Case("G-conv-f64", ("conv", "conv0"), 5, (1,), nchains=2, itr=40, sigma_z=0.8))
    out.append(Case("G-conv-f32", ("conv", "conv0"), 5, (1,), nchains=2, itr=40, sigma_z=0.8, f32=True))
    out.append(Case("H-M33-weights", MODEL_A, 33, (1, 0), how="weights", itr=40))
    out.append(Case("I-M2-high-words", MODEL_A, 2, (1, 0), seed=2 ** 40 + 7, chain_id0=2 ** 24 + 5, itr=40))
    out.append(Case("I-M2-itr1", MODEL_A, 2, (1, 0), seed=2 ** 40 + 7, chain_id0=2 ** 24 + 5, itr=1))
    return out


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}
