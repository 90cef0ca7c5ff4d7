"""Per-transition audit of a finished NUTS trace (reference src/space_inference.jl:139-160; samplers.nuts_iter -- the leaf-by-leaf
restatement of samplers.nuts, the project's restatement of AdvancedHMC 0.2.27's NUTS [upstream, unverifiable offline] -- on the
build's Philox stream, oracle/philox.py) -- TEST INFRASTRUCTURE, no GPU needed.  The manner of tests/hmc_audit.py, whose functions
it reuses for everything the two samplers share: the audit takes the trace's OWN previous column and its OWN leaf log as given and
checks every leaf, every decision of the tree, the accepted state and every adaptor update by itself.

Streams of chain c (Philox chain chain_id0 + c): purposes 0, 5, 6 as hmc_audit; purpose 7, step t, block j: u53(x1, x0) < 0.5 is
the direction +1 of the doubling at depth j, u53(x3, x2) its progressive uniform; purpose 8, step t, block 16 leaf + level:
u53(x1, x0) is the uniform of the merge at `level` after leaf `leaf` (the running leaf count of the transition).  All EXACT on the host.

  column 0, the search, eps[t+1], Minv, freezing after n_adapts: hmc_audit's conditions, unchanged (its functions).  depth, nleaf
            and sel of column 0 are 0.
  leaf      every logged leaf (z1, r1, lp1, g1) is held to ONE leapfrog step of size v eps from the edge the replay extends -- the
            previous column (with r0 = n_t / sqrt(Minv) on the host) or an earlier logged leaf -- with v from the host's exact
            uniform:  rh = r + (v eps / 2) g,  |z1 - (z + v eps (Minv rh))| <= 24 2^-53 (|z| + |eps Minv r| + |eps Minv (eps / 2) g|)
            (hmc_audit's ZP_ULPS bound);  lp1, g1 within the stated tolerances of the oracle at the LOGGED z1 (an oracle value that
            is not finite asks for a logged one that is not finite);  |r1 - (rh + (v eps / 2) g1)| <= 24 2^-53 (|r| + |eps / 2 g| +
            |eps / 2 g1|) with the logged g1, which is tighter than the first-order effect of the gradient tolerance on the kick.
  decision  recomputed from the logged leaves alone, in this order: divergence (-dh > max_dh), every merge's pick and sub-tree
            U-turn, the progressive pick, the whole tree's U-turn, the depth limit.  Tolerances (derived, nothing from the device):
              dh        hmc_audit.dh_tolerance of the leaf against the previous column (lp / gradient tolerances + the sums' roundoff)
              logw      logaddexp moves by at most the larger error of its arguments: tol = max(tol_a, tol_b) + 8 2^-53 (1 + |logw|)
              pick      log u < logw_b - logw:  tol_b + tol + 8 2^-53 (|log u| + |logw_b| + |logw|)
              U-turn    rho . (Minv r) <= 0:  sum_m Minv_m (rho_tol_m |r_m| + |rho_m| r_tol_m) + (M + n + 8) 2^-53 sum_m Minv_m |rho|_m |r_m|
                        with r_tol = |eps / 2| (g_rtol |g1| + g_atol max|g1|) per leaf (18 2^-53 |r0| for r0), rho_tol its sum over
                        the n leaves of rho, |rho| the sum of the |r|
            a comparison inside its tolerance makes the transition UNDECIDABLE: counted, its decisions skipped from that point on.
            Otherwise depth[t], nleaf[t] and sel[t] must equal the replay's.
  state     Z[:, t], lp[t], G[:, t] are bit copies of the log entry of leaf sel[t] of the transition, or of column t - 1 when sel[t] = 0
  alpha[t]  within sum_leaves tol_leaf / n + (n + 4) 2^-53 of the replay's, tol_leaf = the spread of a(dh +- tol) with hmc_audit's
            16-unit allowance for the exponential

oracle_trace(case, mutant=...) is the Philox-driven host sampler in the device's output shapes; without a mutant its Z, lp, alpha
equal samplers.nuts_iter's on the Philox callback bit for bit (tests/test_nuts_audit_cpu.py).  MUTANTS names the wrong kernels it
can imitate.  `merge_ignores_stop` needs a note: a pick taken from a stopped sub-tree is never used (every stop ends the
transition before the progressive pick), so that half of the mistake cannot be seen in any output; the mutant therefore ignores
b.stop in BOTH statements of the merge -- the pick and the propagation of the stop -- which the leaf count shows.
"""
import functools
import math
import zlib
from dataclasses import dataclass, field

import numpy as np

from oracle import philox
from tests import hmc_audit as ha
from tests import mala_audit as ma
from tests import rwmh_audit as ra
from tests.rwmh_audit import EPS, Z_ULPS, AuditFailure, _bits, _same_bits

P_DOUBLING, P_MERGE = 7, 8
ZP_ULPS, EXP_ULPS = ha.ZP_ULPS, ha.EXP_ULPS
R0_ULPS = 18.0   # r0 = n / sqrt(Minv): rwmh_audit's 16 for the normals, the quotient, one of headroom


def uniforms(seed, chain, step, purpose, block):
    """(u53(x1, x0), u53(x3, x2)) of the Philox block"""
    x = philox.philox4x32(philox._ctr(step, chain, purpose, block)[None, :], philox._key(seed)[None, :])
    return float(philox._u53(x[:, 1], x[:, 0])[0]), float(philox._u53(x[:, 3], x[:, 2])[0])


def philox_draw(seed, chain, m):
    """the callback of samplers.nuts_iter on chain `chain`'s Philox streams: with it nuts_iter IS the device sampler's definition"""
    def draw(kind, t, depth, leaf, level):
        if kind == "initial":
            return philox.normals(seed, chain, 0, m)
        if kind == "search":
            return ha.momentum_normals(seed, chain, 0, m, ha.P_SEARCH)
        if kind == "momentum":
            return ha.momentum_normals(seed, chain, t + 1, m)
        if kind == "direction":
            return uniforms(seed, chain, t + 1, P_DOUBLING, depth)[0]
        if kind == "progressive":
            return uniforms(seed, chain, t + 1, P_DOUBLING, depth)[1]
        assert kind == "merge", kind
        return uniforms(seed, chain, t + 1, P_MERGE, 16 * leaf + level)[0]
    return draw


class Undecidable(Exception):
    pass


@dataclass
class Leaf:
    z: np.ndarray
    r: np.ndarray
    lp: float
    g: np.ndarray


MUTANTS = ("uturn_plain_z", "uturn_no_minv", "rho_not_accumulated", "merge_ignores_stop", "pick_logw_b_minus_a", "progressive_unbiased",
           "progressive_reuses_direction_u", "merge_block_leaf_only", "wrong_edge_minus", "stale_gradient_edge", "alpha_nominal_leaves",
           "divergent_eligible", "depth_limit_off_by_one", "h0_no_kinetic", "adaptor_fed_proposal", "tree_logw_not_updated",
           "no_second_kick")


def transition(z, lp, g, r0, eps, minv, next_leaf, uni, max_depth, max_dh, tols, ft=float, mutant=None, decisions=None):
    """One NUTS transition from (z, lp, g) with momentum r0: samplers.nuts_iter's statements in the number type `ft`, with the
    leaves supplied by next_leaf(edge: Leaf, v) -> Leaf (the oracle's leapfrog step, or the next entry of a trace's leaf log) and the
    uniforms by uni(kind, depth, leaf, level).  decisions: a list that receives (kind, diff, tol) of every comparison; when given, a
    comparison with |diff| <= tol raises Undecidable.  Returns a dict: ndoub, nleaf, sel, the candidate Leaf (None: the state is
    kept), alpha, alpha_tol, exits (names, for the coverage certificate), last_prop (the last doubling's proposal)."""
    m = z.size
    lp_rtol, g_rtol, g_atol = tols
    F = lambda a: np.asarray(a, dtype=ft)
    mi = F(minv)
    r0f = F(r0)
    k0 = 0.5 * np.sum(mi * r0f * r0f)
    h0 = ft(lp) - (ft(0.0) if mutant == "h0_no_kinetic" else k0)
    exits = set()

    def judge(kind, diff, tol):
        """records the comparison `diff < 0` (or <= 0); undecidable inside the tolerance"""
        if decisions is not None:
            decisions.append((kind, float(diff), float(tol)))
            if abs(float(diff)) <= tol:
                raise Undecidable(kind)

    def uturn(rho, rho_abs, rho_tol, nrho, rm, rm_tol, rp, rp_tol, kind, zspan=None):
        out = False
        for r_end, r_tol in ((rm, rm_tol), (rp, rp_tol)):
            rf = F(r_end)
            v_end = rf if mutant == "uturn_no_minv" else mi * rf
            lead = F(zspan) if zspan is not None else rho
            d = np.sum(lead * v_end)
            tol = float(np.sum(np.asarray(minv) * (rho_tol * np.abs(r_end) + np.abs(np.asarray(rho, dtype=np.float64)) * r_tol))
                        + (m + nrho + 8.0) * EPS * np.sum(np.asarray(minv) * rho_abs * np.abs(r_end)))
            if decisions is not None:
                decisions.append((kind, float(d), tol))
                if float(d) < -tol:
                    return True            # (decisively a U-turn at this end: the other end does not matter)
                if not float(d) > tol:
                    raise Undecidable(kind)
            elif d <= 0.0:
                out = True
        return out

    start = Leaf(np.asarray(z, dtype=np.float64), np.asarray(r0, dtype=np.float64), float(lp), np.asarray(g, dtype=np.float64))
    r0_tol = R0_ULPS * EPS * np.abs(start.r)
    ends = {-1: (start, r0_tol), 1: (start, r0_tol)}
    tree_rho, tree_rho_abs, tree_rho_tol, tree_n = r0f.copy(), np.abs(start.r), r0_tol.copy(), 1
    tree_logw, tree_logw_tol = ft(0.0), 0.0
    cand, sel = None, 0
    alpha_sum, alpha_tol_sum, n_alpha = ft(0.0), 0.0, 0
    nleaf = ndoub = 0
    last_prop = None
    limit = max_depth + 1 if mutant == "depth_limit_off_by_one" else max_depth
    for depth in range(limit):
        ndoub += 1
        v = 1 if uni("direction", depth, nleaf, 0) < 0.5 else -1
        ve = float(v) * eps
        side = 1 if (mutant == "wrong_edge_minus" and v < 0) else v
        edge, edge_tol = ends[side]
        if mutant == "stale_gradient_edge":
            edge = Leaf(edge.z, edge.r, edge.lp, start.g)
        stack = []
        stopped = False
        for k in range(1, 2 ** depth + 1):
            leaf = next_leaf(edge, v)
            nleaf += 1
            rl = F(leaf.r)
            k1 = 0.5 * np.sum(mi * rl * rl)
            h1 = ft(leaf.lp) - k1
            if not np.isfinite(h1):
                h1 = ft(-np.inf)
                exits.add("nonfinite")
            dh = h1 - h0
            if np.isfinite(float(dh)):
                dh_tol = ha.dh_tolerance(float(lp), leaf.lp, leaf.g, leaf.r, eps, np.asarray(minv), float(k0), float(k1), tols, m)
                a_leaf = np.exp(dh) if dh < 0 else ft(1.0)
                a_lo = ha.alpha_of(0.0, float(dh) - dh_tol) * (1.0 - EXP_ULPS * EPS)
                a_hi = min(1.0, ha.alpha_of(0.0, float(dh) + dh_tol) * (1.0 + EXP_ULPS * EPS))
                a_tol = max(a_hi - float(a_leaf), float(a_leaf) - a_lo, 0.0)
            else:
                dh_tol, a_leaf, a_tol = 0.0, (ft(0.0) if dh < 0 else ft(1.0)), 0.0
            gmax = float(np.max(np.abs(leaf.g))) if np.all(np.isfinite(leaf.g)) else 0.0
            r_tol = abs(0.5 * ve) * (g_rtol * np.abs(np.nan_to_num(leaf.g)) + g_atol * gmax)
            ent = dict(first=leaf, first_tol=r_tol, prop=leaf, sel=nleaf, logw=dh, logw_tol=dh_tol, rho=rl.copy(), rho_abs=np.abs(leaf.r),
                       rho_tol=r_tol.copy(), alpha=a_leaf, alpha_tol=a_tol, n=1, div=False)
            stack.append(ent)
            edge, edge_tol = leaf, r_tol
            judge("divergence", ft(max_dh) + dh, dh_tol)
            if (-dh) > max_dh:
                exits.add("divergence")
                ent["div"] = True
                if mutant != "merge_ignores_stop" or k % 2 == 1:
                    stopped = True
            level = 0
            while not stopped and (k >> level) & 1 == 0:
                level += 1
                b = stack.pop()
                a = stack.pop()
                logw = np.logaddexp(a["logw"], b["logw"])
                logw_tol = max(a["logw_tol"], b["logw_tol"]) + 8.0 * EPS * (1.0 + abs(float(logw)))
                out = dict(a)
                u = uni("merge", depth, nleaf, 1 if mutant == "merge_block_leaf_only" else level)
                rhs = b["logw"] - (a["logw"] if mutant == "pick_logw_b_minus_a" else logw)
                diff = np.log(ft(u)) - rhs
                judge("merge pick", diff, b["logw_tol"] + logw_tol + 8.0 * EPS * (abs(math.log(u)) + abs(float(b["logw"])) + abs(float(logw))))
                if diff < 0:
                    out.update(prop=b["prop"], sel=b["sel"])
                out["rho"] = a["rho"] + b["rho"]
                out["rho_abs"] = a["rho_abs"] + b["rho_abs"]
                out["rho_tol"] = a["rho_tol"] + b["rho_tol"]
                out["logw"], out["logw_tol"] = logw, logw_tol
                out["alpha"] = a["alpha"] + b["alpha"]
                out["alpha_tol"] = a["alpha_tol"] + b["alpha_tol"]
                out["n"] = a["n"] + b["n"]
                if level >= 3:
                    exits.add("merge level >= 3")
                first, last = out["first"], leaf
                (rm, rm_tol), (rp, rp_tol) = ((first.r, out["first_tol"]), (last.r, r_tol)) if v > 0 else ((last.r, r_tol), (first.r, out["first_tol"]))
                zspan = (last.z - first.z) * float(v) if mutant == "uturn_plain_z" else None
                stopped = uturn(out["rho"], out["rho_abs"], out["rho_tol"], out["n"], rm, rm_tol, rp, rp_tol, "sub-tree U-turn", zspan)
                if stopped:
                    exits.add("sub-tree U-turn")
                stack.append(out)
            if stopped:
                break
        sub = stack.pop()
        while stack:
            a = stack.pop()
            sub = dict(sub, alpha=a["alpha"] + sub["alpha"], alpha_tol=a["alpha_tol"] + sub["alpha_tol"], n=a["n"] + sub["n"])
        alpha_sum = alpha_sum + sub["alpha"]
        alpha_tol_sum += sub["alpha_tol"]
        n_alpha += 2 ** depth if mutant == "alpha_nominal_leaves" else sub["n"]
        last_prop = sub["prop"]
        if stopped and not (mutant == "divergent_eligible" and depth == 0 and sub.get("div")):
            break
        diff = np.log(ft(uni("direction" if mutant == "progressive_reuses_direction_u" else "progressive", depth, nleaf, 0))) - (
            sub["logw"] - (np.logaddexp(tree_logw, sub["logw"]) if mutant == "progressive_unbiased" else tree_logw))
        judge("progressive pick", diff, sub["logw_tol"] + tree_logw_tol + 8.0 * EPS * (abs(float(diff)) + 2.0 * abs(float(sub["logw"])) + 2.0 * abs(float(tree_logw))))
        if diff < 0:
            cand, sel = sub["prop"], sub["sel"]
        if stopped:
            break
        ends[side] = (edge, edge_tol)
        if mutant == "rho_not_accumulated":
            tree_rho, tree_rho_abs, tree_rho_tol, tree_n = sub["rho"], sub["rho_abs"], sub["rho_tol"], sub["n"]
        else:
            tree_rho, tree_rho_abs = tree_rho + sub["rho"], tree_rho_abs + sub["rho_abs"]
            tree_rho_tol, tree_n = tree_rho_tol + sub["rho_tol"], tree_n + sub["n"]
        if mutant != "tree_logw_not_updated":
            new_logw = np.logaddexp(tree_logw, sub["logw"])
            tree_logw_tol = max(tree_logw_tol, sub["logw_tol"]) + 8.0 * EPS * (1.0 + abs(float(new_logw)))
            tree_logw = new_logw
        zspan = (ends[1][0].z - ends[-1][0].z) if mutant == "uturn_plain_z" else None
        if uturn(tree_rho, tree_rho_abs, tree_rho_tol, tree_n, ends[-1][0].r, ends[-1][1], ends[1][0].r, ends[1][1], "tree U-turn", zspan):
            exits.add("tree U-turn")
            break
        if depth + 1 == limit:
            exits.add("depth limit")
    n = max(1, n_alpha)
    if sel == 0:
        exits.add("sel = 0")
    return dict(ndoub=ndoub, nleaf=nleaf, sel=sel, cand=cand, alpha=float(alpha_sum / n), alpha_tol=alpha_tol_sum / n + (nleaf + 4.0) * EPS,
                exits=exits, last_prop=last_prop)


# ----------------------------------------------------------------------------------------------- cases
problem, value_grad_of = ma.problem, ma.value_grad_of
SMALL, RAGGED, F32_DENSE, SOFTPLUS, MODEL_A = ma.SMALL, ma.RAGGED, ma.F32_DENSE, ma.SOFTPLUS, ma.MODEL_A
RELU = ((4, 12, 2), (ra.R, ra.I), 40)
SIGMOID = ((4, 12, 2), (ra.S, ra.I), 40)
RELU_DEEP = ((3, 8, 8, 8, 2), (ra.R, ra.R, ra.R, ra.I), 40)   # lp falls like |z|^8: an unstable trajectory overflows within a few leaves


@dataclass(frozen=True)
class Case:
    name: str
    model: tuple
    m: int
    sigma_z: float
    fused: bool             # the route si_sample_nuts must report
    nchains: int = 1
    itr: int = 12
    n_adapts: int = -1      # -1: the reference's round(itr / 2)
    delta: float = 0.8
    max_depth: int = 5
    max_dh: float = 1000.0
    sigma_m: float = 0.8
    seed: int = 11
    chain_id0: int = 2
    prior: float = 0.0
    f32: bool = False

    @property
    def tols(self):
        return (ma.LP_RTOL_F32, ma.G_RTOL_F32, ma.G_ATOL_F32) if self.f32 else (ma.LP_RTOL_F64, ma.G_RTOL_F64, ma.G_ATOL_F64)

    @property
    def adapts(self):
        return ha.n_adapts_of(self.itr, None if self.n_adapts < 0 else self.n_adapts)

    @property
    def leaf_cap(self):
        return self.itr * (2 ** self.max_depth - 1)   # every leaf of the longest possible run


@dataclass
class Trace:
    Z: np.ndarray        # M x (itr+1) x C
    lp: np.ndarray       # (itr+1) x C, like alpha, eps, depth, nleaf, sel
    alpha: np.ndarray
    eps: np.ndarray
    depth: np.ndarray
    nleaf: np.ndarray
    sel: np.ndarray
    G: np.ndarray
    Minv: np.ndarray
    leaf: np.ndarray     # (3M+1) x leaf_cap x C
    exits: list = field(default_factory=list)   # oracle only: per chain, per transition, the set of exits

    def arrays(self):
        return (self.Z, self.lp, self.alpha, self.eps, self.depth, self.nleaf, self.sel, self.G, self.Minv, self.leaf)


def perturbed(vg, tols, seed):
    """vg with every value moved to the edge of the stated tolerances, signs drawn from `seed` (deterministic in z)"""
    lp_rtol, g_rtol, g_atol = tols

    def f(z):
        lp, g = vg(z)
        rng = np.random.default_rng([seed, zlib.crc32(np.asarray(z).tobytes())])
        s = rng.choice([-1.0, 1.0], size=g.size + 1)
        if not np.isfinite(lp):
            return lp, g
        return lp * (1.0 + 0.9 * lp_rtol * s[0]), g + 0.9 * s[1:] * (g_rtol * np.abs(g) + g_atol * np.max(np.abs(g)))
    return f


def oracle_trace(case, value_grad=None, mutant=None):
    """samplers.nuts_iter on the case's Philox chains in si_sample_nuts's shapes, with the leaf log.  mutant: one of MUTANTS -- the
    trace a kernel with that mistake would produce."""
    assert mutant is None or mutant in MUTANTS, mutant
    vg = value_grad_of(problem(case)) if value_grad is None else value_grad
    m, itr, nc, cap = case.m, case.itr, case.nchains, case.leaf_cap
    Z, G, MI = (np.empty((m, itr + 1, nc), order="F") for _ in range(3))
    lps, al, ep = (np.empty((itr + 1, nc), order="F") for _ in range(3))
    dep, nlf, sl = (np.zeros((itr + 1, nc), dtype=np.int32, order="F") for _ in range(3))
    log = np.full((3 * m + 1, cap, nc), np.nan, order="F")
    all_exits = []
    for c in range(nc):
        chain = case.chain_id0 + c
        z = case.sigma_z * philox.normals(case.seed, chain, 0, m)
        lp, g = vg(z)
        eps0 = ha.search(vg, z, lp, g, ha.momentum_normals(case.seed, chain, 0, m, ha.P_SEARCH), case.tols)[0]
        ad = ha.Adaptor(m, case.adapts, eps0, case.delta, mutant="welford_proposed" if mutant == "adaptor_fed_proposal" else None)
        Z[:, 0, c], lps[0, c], G[:, 0, c], al[0, c], ep[0, c], MI[:, 0, c] = z, lp, g, 0.0, eps0, 1.0
        nlog = 0
        chain_exits = []
        for t in range(1, itr + 1):
            minv, eps = np.array(ad.minv, dtype=np.float64), float(ad.eps)
            r0 = ha.momentum_normals(case.seed, chain, t, m) / np.sqrt(minv)

            def next_leaf(edge, v):
                nonlocal nlog
                ve = float(v) * eps
                rh = edge.r + 0.5 * ve * edge.g
                z1 = edge.z + ve * (minv * rh)
                lp1, g1 = vg(z1)
                r1 = rh if mutant == "no_second_kick" else rh + 0.5 * ve * g1
                if nlog < cap:
                    log[:m, nlog, c], log[m:2 * m, nlog, c], log[2 * m, nlog, c], log[2 * m + 1:, nlog, c] = z1, r1, lp1, g1
                nlog += 1
                return Leaf(z1, r1, float(lp1), g1)

            def uni(kind, depth, leaf, level):
                if kind == "merge":
                    return uniforms(case.seed, chain, t, P_MERGE, 16 * leaf + level)[0]
                return uniforms(case.seed, chain, t, P_DOUBLING, depth)[0 if kind == "direction" else 1]
            out = transition(z, lp, g, r0, eps, minv, next_leaf, uni, case.max_depth, case.max_dh, case.tols, mutant=mutant)
            if out["cand"] is not None:
                z, lp, g = out["cand"].z, out["cand"].lp, out["cand"].g
            Z[:, t, c], lps[t, c], G[:, t, c], al[t, c], ep[t, c], MI[:, t, c] = z, lp, g, out["alpha"], eps, minv
            dep[t, c], nlf[t, c], sl[t, c] = out["ndoub"], out["nleaf"], out["sel"]
            chain_exits.append(out["exits"])
            ad.adapt(z, out["alpha"], out["last_prop"].z if out["last_prop"] is not None else z)
        all_exits.append(chain_exits)
    return Trace(Z, lps, al, ep, dep, nlf, sl, G, MI, log, all_exits)


@functools.lru_cache(maxsize=None)
def cached_oracle_trace(case):
    out = oracle_trace(case)
    for a in out.arrays():
        a.setflags(write=False)
    return out


# ----------------------------------------------------------------------------------------------- the audit
@dataclass
class Report:
    transitions: int = 0
    undecidable: int = 0             # transitions with a comparison inside its tolerance
    undecidable_search: int = 0
    leaves: int = 0
    kept: int = 0                    # transitions with sel = 0
    closes: int = 0
    worst_z_ratio: float = 0.0
    worst_r_ratio: float = 0.0
    worst_lp_rel: float = 0.0
    worst_g_ratio: float = 0.0
    worst_alpha_ratio: float = 0.0
    worst_logeps_ratio: float = 0.0
    worst_minv_ratio: float = 0.0
    decisions: list = field(default_factory=list)   # (chain, t, kind, diff, tol) of every comparison of the decidable replay
    chain_depths: list = field(default_factory=list)
    search_evals: list = field(default_factory=list)

    def line(self):
        return ("%d transitions, %d undecidable (+ %d searches), %d leaves, %d kept, %d closes; worst ratios: z %.3f, r %.3f, lp rel %.2e, g %.2e, "
                "alpha %.2e, log eps %.2e, Minv %.2e" % (self.transitions, self.undecidable, self.undecidable_search, self.leaves, self.kept,
                                                        self.closes, self.worst_z_ratio, self.worst_r_ratio, self.worst_lp_rel,
                                                        self.worst_g_ratio, self.worst_alpha_ratio, self.worst_logeps_ratio, self.worst_minv_ratio))


def audit(tr, value_grad, sigma_z, seed, chain_id0, n_adapts, delta, max_depth, max_dh, tols, ft=float, check_oracle=True):
    """tr: a Trace.  value_grad(z) -> (lp, g): the host fp64 oracle.  Raises AuditFailure naming chain, step and what is off;
    returns a Report.  ft = np.longdouble replays the decisions in extended precision (check_oracle=False skips the oracle)."""
    Z, lp, alpha, eps, G, Minv = (np.asarray(a, dtype=np.float64) for a in (tr.Z, tr.lp, tr.alpha, tr.eps, tr.G, tr.Minv))
    depth, nleaf, sel, log = np.asarray(tr.depth), np.asarray(tr.nleaf), np.asarray(tr.sel), np.asarray(tr.leaf, dtype=np.float64)
    nm, cols, nch = Z.shape
    if G.shape != Z.shape or Minv.shape != Z.shape or any(a.shape != Z.shape[1:] for a in (lp, alpha, eps, depth, nleaf, sel)) or \
            log.ndim != 3 or log.shape[0] != 3 * nm + 1 or log.shape[2] != nch:
        raise AuditFailure("shapes: Z %s, lp %s, depth %s, leaf log %s" % (Z.shape, lp.shape, depth.shape, log.shape))
    lp_rtol, g_rtol, g_atol = tols
    cap = log.shape[1]
    rep = Report()

    def ratio(err, bound):
        return float(np.max(np.divide(err, bound, out=np.where(err > 0.0, np.inf, 0.0), where=bound > 0.0))) if np.size(err) else 0.0

    for c in range(nch):
        chain = chain_id0 + c

        def fail(t, what):
            raise AuditFailure("chain %d (Philox chain %d), step %d: %s" % (c, chain, t, what))

        def check_vec(t, got, want, bound, what):
            err = np.abs(got - want)
            bad = np.flatnonzero(~(err <= bound))
            if bad.size:
                i = int(bad[0])
                fail(t, "%s: component %d is %r, expected %r: off by %.3g of its bound (%d of %d components off)" % (
                    what, i, got[i], want[i], err[i] / bound[i] if bound[i] > 0 else np.inf, bad.size, got.size))
            return ratio(err, bound)

        def check_lp_g(t, lpv, gv, zv, what):
            lp_ref, g_ref = value_grad(zv)
            if not np.isfinite(lp_ref):
                if np.isfinite(lpv):
                    fail(t, "%s: lp is %r, the oracle's value there is %r" % (what, lpv, lp_ref))
                return
            rel = abs(lpv - lp_ref) / abs(lp_ref) if lp_ref != 0.0 else abs(lpv)
            if not rel <= lp_rtol:
                fail(t, "%s: lp is %r, the oracle's value there is %r: relative error %.3e > %g" % (what, lpv, lp_ref, rel, lp_rtol))
            rep.worst_lp_rel = max(rep.worst_lp_rel, float(rel))
            rep.worst_g_ratio = max(rep.worst_g_ratio, check_vec(t, gv, g_ref, g_rtol * np.abs(g_ref) + g_atol * np.max(np.abs(g_ref)),
                                                                 "%s: gradient" % what))
        # column 0 and the search: hmc_audit's conditions
        n0 = sigma_z * philox.normals(seed, chain, 0, nm)
        rep.worst_z_ratio = max(rep.worst_z_ratio, check_vec(0, Z[:, 0, c], n0, Z_ULPS * EPS * np.abs(n0), "Z[:, 0] against sigma_z n_0"))
        if check_oracle:
            check_lp_g(0, lp[0, c], G[:, 0, c], Z[:, 0, c], "Z[:, 0]")
        if not np.all(Minv[:, 0, c] == 1.0) or alpha[0, c] != 0.0 or depth[0, c] != 0 or nleaf[0, c] != 0 or sel[0, c] != 0:
            fail(0, "column 0 must have Minv = 1, alpha = 0, depth = nleaf = sel = 0")
        if check_oracle:
            rho = ha.momentum_normals(seed, chain, 0, nm, ha.P_SEARCH)
            eps0, decidable, evals = ha.search(value_grad, Z[:, 0, c], lp[0, c], G[:, 0, c], rho, tols)
            rep.search_evals.append(evals)
            if not decidable:
                rep.undecidable_search += 1
            elif _bits(eps[0:1, c])[0] != _bits(np.array([eps0]))[0]:
                fail(0, "eps[0] is %r, the step-size search replayed from column 0 gives %r" % (eps[0, c], eps0))
        ad = ha.Adaptor(nm, n_adapts, eps[0, c], delta)
        win_first = None
        k_before = 0
        cursor = 0
        depths = []
        for t in range(1, cols):
            z, g, e, mi = Z[:, t - 1, c], G[:, t - 1, c], eps[t, c], Minv[:, t, c]
            if not (e > 0.0 and np.isfinite(e)):
                fail(t, "eps[t] is %r" % e)
            if not np.all((mi > 0.0) & np.isfinite(mi)):
                fail(t, "Minv[:, t] is not positive and finite")
            r0 = ha.momentum_normals(seed, chain, t, nm) / np.sqrt(mi)
            first = cursor
            n_t = int(nleaf[t, c])
            if not 1 <= n_t <= 2 ** max_depth - 1 or first + n_t > cap:
                fail(t, "nleaf[t] is %d (leaves so far %d, leaf log of %d)" % (n_t, first, cap))
            used = [0]

            def next_leaf(edge, v):
                i = first + used[0]
                if used[0] >= n_t:
                    fail(t, "the replay builds leaf %d of this transition, nleaf[t] is %d" % (used[0] + 1, n_t))
                rec = log[:, i, c]
                leaf = Leaf(rec[:nm], rec[nm:2 * nm], float(rec[2 * nm]), rec[2 * nm + 1:])
                used[0] += 1
                if not check_oracle:
                    return leaf
                ve = float(v) * e
                rh = edge.r + 0.5 * ve * edge.g
                what = "leaf %d (direction %+d)" % (used[0], v)
                rep.worst_z_ratio = max(rep.worst_z_ratio, check_vec(
                    t, leaf.z, edge.z + ve * (mi * rh), ZP_ULPS * EPS * (np.abs(edge.z) + np.abs(e * (mi * edge.r)) + np.abs(e * (mi * (0.5 * e * edge.g)))),
                    what + ": z against z + v eps (Minv (r + v eps / 2 g)) from the edge"))
                check_lp_g(t, leaf.lp, leaf.g, leaf.z, what)
                if np.all(np.isfinite(leaf.g)):
                    rep.worst_r_ratio = max(rep.worst_r_ratio, check_vec(
                        t, leaf.r, rh + 0.5 * ve * leaf.g, ZP_ULPS * EPS * (np.abs(edge.r) + np.abs(0.5 * e * edge.g) + np.abs(0.5 * e * leaf.g)),
                        what + ": r against the two half kicks"))
                return leaf

            def uni(kind, dpt, lf, level):
                if kind == "merge":
                    return uniforms(seed, chain, t, P_MERGE, 16 * lf + level)[0]
                return uniforms(seed, chain, t, P_DOUBLING, dpt)[0 if kind == "direction" else 1]
            dec = []
            rep.transitions += 1
            try:
                out = transition(z, lp[t - 1, c], g, r0, e, mi, next_leaf, uni, max_depth, max_dh, tols, ft=ft, decisions=dec)
            except Undecidable:
                out = None
                rep.undecidable += 1
            if out is not None:
                rep.decisions += [(c, t) + d for d in dec]
                if (depth[t, c], n_t, sel[t, c]) != (out["ndoub"], out["nleaf"], out["sel"]):
                    fail(t, "(depth, nleaf, sel) is (%d, %d, %d), the replay of the logged leaves gives (%d, %d, %d)" % (
                        depth[t, c], n_t, sel[t, c], out["ndoub"], out["nleaf"], out["sel"]))
                err = abs(alpha[t, c] - out["alpha"])
                if not err <= out["alpha_tol"]:
                    fail(t, "alpha[t] is %r, the replay gives %r (tolerance %.3g)" % (alpha[t, c], out["alpha"], out["alpha_tol"]))
                rep.worst_alpha_ratio = max(rep.worst_alpha_ratio, err / out["alpha_tol"])
            elif check_oracle:
                for _ in range(used[0], n_t):   # (the leaves the replay did not reach are still held to the oracle, not to an edge)
                    rec = log[:, first + used[0], c]
                    check_lp_g(t, float(rec[2 * nm]), rec[2 * nm + 1:], rec[:nm], "leaf %d" % (used[0] + 1))
                    used[0] += 1
            cursor = first + n_t
            rep.leaves += n_t
            depths.append(int(depth[t, c]))
            # the accepted state: a bit copy of the selected leaf's log entry, or of column t - 1
            s = int(sel[t, c])
            if not 0 <= s <= n_t:
                fail(t, "sel[t] is %d with nleaf[t] = %d" % (s, n_t))
            if s == 0:
                rep.kept += 1
                want = (z, lp[t - 1:t, c], g)
            else:
                rec = log[:, first + s - 1, c]
                want = (rec[:nm], rec[2 * nm:2 * nm + 1], rec[2 * nm + 1:])
            if not (_same_bits(Z[:, t, c], want[0]) and _same_bits(lp[t:t + 1, c], want[1]) and _same_bits(G[:, t, c], want[2])):
                fail(t, "column t is not a bit copy of %s" % ("column t - 1 (sel = 0)" if s == 0 else "the log entry of leaf %d" % s))
            # the adaptor's update after transition t, against column t + 1: hmc_audit's conditions
            if t <= n_adapts and ad.window_start <= t <= ad.window_end and win_first is None:
                win_first = t
            mu_used = float(ad.mu)
            ad.adapt(Z[:, t, c], alpha[t, c])
            if t + 1 >= cols:
                continue
            e1, mi1 = eps[t + 1, c], Minv[:, t + 1, c]
            if t > n_adapts:
                if _bits(eps[t + 1:t + 2, c])[0] != _bits(eps[t:t + 1, c])[0] or not _same_bits(mi1, mi):
                    fail(t, "adaptation ended after step %d, but eps or Minv changed from column %d to %d" % (n_adapts, t, t + 1))
                continue
            if not (e1 > 0.0 and np.isfinite(e1)):
                fail(t + 1, "eps[t] is %r" % e1)
            if t == n_adapts and ad.t > 0:
                bound = ha.logeps_bar_bound(ad.t, mu_used, ad.max_abs_log_eps) + 8.0 * EPS
                want_le = float(ad.log_eps_bar)
            else:
                k = ad.t if not ad.closed else k_before + 1
                bound = ha.logeps_bound(k, mu_used)
                want_le = math.log(float(ad.eps))
            err = abs(math.log(e1) - want_le)
            if not err <= bound:
                fail(t, "after this step's update eps is %r (column %d), the adaptor replayed from the trace's alpha gives %r: log eps off by "
                     "%.3g of its bound" % (e1, t + 1, math.exp(want_le), err / bound))
            rep.worst_logeps_ratio = max(rep.worst_logeps_ratio, err / bound)
            if ad.closed:
                rep.closes += 1
                want_minv, mbound = ha.window_minv(Z[:, win_first:t + 1, c])
                rep.worst_minv_ratio = max(rep.worst_minv_ratio, check_vec(t, mi1, want_minv.astype(np.float64), mbound,
                                                                           "Minv after the close of window %d .. %d" % (win_first, t)))
                win_first = None
                ad.minv = mi1.copy()
                ad.eps = e1
                ad.restart(e1)
            elif not _same_bits(mi1, mi):
                fail(t, "no window closed at this step, but Minv changed")
            k_before = ad.t
        rep.chain_depths.append(depths)
    return rep


def audit_case(case, tr, value_grad=None, ft=float, check_oracle=True):
    return audit(tr, value_grad_of(problem(case)) if value_grad is None else value_grad, case.sigma_z, case.seed, case.chain_id0,
                 case.adapts, case.delta, case.max_depth, case.max_dh, case.tols, ft=ft, check_oracle=check_oracle)


def check_caps(case, rep):
    """conditions on a case, not measurements: at most 1 transition in 50 undecidable in fp64 and never every transition; with
    SI_F32 rwmh_audit's F32_UNDECIDABLE_CAP of the transitions; the step-size search as hmc_audit caps it"""
    assert rep.transitions == case.itr * case.nchains
    frac = ra.F32_UNDECIDABLE_CAP if case.f32 else 1.0 / 50.0
    assert rep.undecidable <= frac * rep.transitions, "%d undecidable transitions of %d (cap %g)" % (rep.undecidable, rep.transitions, frac)
    assert rep.undecidable < rep.transitions
    cap = ra.F32_UNDECIDABLE_CAP * case.nchains if case.f32 else 0
    assert rep.undecidable_search <= cap, "%d undecidable searches of %d chains (cap %g)" % (rep.undecidable_search, case.nchains, cap)


EXITS = ("sub-tree U-turn", "tree U-turn", "divergence", "depth limit", "nonfinite", "sel = 0", "merge level >= 3", "a chain waits")


def coverage(case, tr):
    """the exits the oracle's trace of the case reaches (EXITS' names)"""
    got = set()
    for chain in tr.exits:
        for ex in chain:
            got |= ex
    if case.nchains > 1 and np.any(tr.nleaf[1:, :].max(axis=1) != tr.nleaf[1:, :].min(axis=1)):
        got.add("a chain waits")
    return got


# All small: at most 24 transitions of at most 2^max_depth - 1 <= 31 leaves.  sigma_z only places the initial point.  The fused
# class's four activations: identity (small-*), tanh (A-*), relu (relu-*), sigmoid (sigmoid-M3), all four in one chain (ragged-M5).
CASES = [
    Case("small-M2", SMALL, 2, 1.0, True, nchains=3),                                    # itr = 12, n_adapts = 6: no window
    Case("small-M1", SMALL, 1, 0.5, True),
    Case("ragged-M5", RAGGED, 5, 0.2, True),
    Case("relu-M3", RELU, 3, 0.5, True),
    Case("sigmoid-M3", SIGMOID, 3, 0.5, True),
    Case("A-M33", MODEL_A, 33, 0.2, True, nchains=3, max_depth=4),
    Case("A-M5x8", MODEL_A, 5, 0.2, True, nchains=8, itr=8),                             # eight chains whose tree sizes differ
    Case("A-M2-high-words", MODEL_A, 2, 0.2, True, itr=6, seed=2 ** 40 + 7, chain_id0=2 ** 24 + 5),
    Case("small-M513", SMALL, 513, 0.2, True, itr=4, max_depth=3),                       # 257 Philox blocks: the 256-thread sweep runs twice
    Case("small-M2-depth2", SMALL, 2, 1.0, True, nchains=3, max_depth=2),                # the depth limit
    Case("A-M2-steep", MODEL_A, 2, 5.0, True, nchains=3, itr=8, sigma_m=0.02),           # small sigma_m, large sigma_z: divergences at max_dh = 1000
    Case("small-M2-maxdh", SMALL, 2, 1.0, True, nchains=3, max_dh=0.3),                  # divergent leaves whose weight is not negligible
    Case("relu-deep-overflow", RELU_DEEP, 3, 3.0, True, nchains=3, itr=8, max_dh=1e300, seed=12),   # a leaf whose lp is not finite
    # (a window needs n_adapts >= 20: 24 transitions of at most 7 leaves; 15 % / 75 % / 10 %: the window is steps 4 .. 18, closed at 18)
    Case("small-M2-window", SMALL, 2, 1.0, True, itr=24, n_adapts=20, max_depth=3),
    Case("small-M2-frozen", SMALL, 2, 1.0, True, itr=8, n_adapts=0),                     # nothing adapts: eps and Minv frozen from column 0
    Case("small-M2-adapt-all", SMALL, 2, 1.0, True, itr=8, n_adapts=8),                  # the last column is the last update
    # the slow route.  With the prior on (sigma_p = 0.1) the leaves stay within |z| < 9.  Without it this chain's density is nearly
    # flat (seven observations behind saturating activations), the search returns a step of tens and the trees reach |z| of 20 .. 100,
    # where the device's Conv gradient -- si_logdensity_grad's, not this sampler's -- was measured at up to 6 times the stated
    # tolerance from the oracle at isolated points (lp agreeing to 1e-15; every leaf below |z| = 20 at 1e-7 of the tolerance): outside
    # the region the gradient tolerances were stated for, as hmc_audit notes of its own sigma_z.  (Probable cause, not established:
    # the restated MaxPool gradient goes to the first window element APPROXIMATELY equal to the maximum, and where the tanh layer in
    # front of it saturates many elements are within that margin of each other, so the choice turns on the last bits.)
    Case("conv-f64", ("conv", "conv0"), 5, 1.0, False, itr=8, max_depth=4, prior=0.1),
    # (SI_F32: every comparison carries the fp32 tolerances, about one transition in twenty is undecidable whatever the seed; shallow
    #  trees and 48 transitions, seed 15: none in the oracle's trace and at most one with the values moved to the tolerances' edge)
    Case("dense-f32", F32_DENSE, 4, 0.15, False, f32=True, nchains=3, itr=16, max_depth=2, seed=15),
]
CASE_BY_NAME = {c.name: c for c in CASES}
