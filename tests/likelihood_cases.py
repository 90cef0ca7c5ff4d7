"""The categorical and Bernoulli likelihoods of the density (si_infer_set_likelihood) -- the host definition and the shared case
list; TEST INFRASTRUCTURE, no GPU needed.

The definition: the weights W = W_swa + P z (or W_swa + decoder(z)), yhat = the oracle's forward pass (oracle/subspace_oracle.py),
then minus the cost's numerator as subspaceinference_jl_amd/costs.py forms it,

    categorical (1)   lp = -costs.numerator(LOGITCE,  yhat, Y) = sum_b sum_i Y_ib (yhat_ib - lse_b)
    bernoulli   (2)   lp = -costs.numerator(LOGITBCE, yhat, Y) = -sum((1 - Y) yhat + softplus(-yhat))

plus the oracle's log-prior when sigma_p > 0.  Its gradient is costs.dvalue (denominator 1, sign flipped) pulled back through the
oracle's reverse pass and P' (or the decoder's vjp).  tests/test_likelihood_cpu.py holds the definition to finite differences and
certifies the RWMH cases and the gradient samplers' cases below on it alone; tests/test_gpu_likelihood.py and
tests/test_gpu_likelihood_samplers.py hold the device to it.
"""
import functools
from dataclasses import dataclass

import numpy as np

from oracle import subspace_oracle as so
from subspaceinference_jl_amd import autoencoder as ae
from subspaceinference_jl_amd import costs
from tests import advi_audit as aa
from tests import cost_cases as cc
from tests import hmc_audit as ha
from tests import mala_audit as ma
from tests import nuts_audit as na
from tests import rwmh_audit as ra

GAUSSIAN, CATEGORICAL, BERNOULLI = 0, 1, 2
COST = {CATEGORICAL: costs.LOGITCE, BERNOULLI: costs.LOGITBCE}
I, R, T, S, SP = so.ACT_IDENTITY, so.ACT_RELU, so.ACT_TANH, so.ACT_SIGMOID, so.ACT_SOFTPLUS

# the Conv chain of tests/test_gpu_train_f32.py with a 3-class head: 3 x 3 x 4 relu on 6 x 6 x 1, flatten, Dense 3
CONV_INPUT, CONV_SPEC = (6, 6, 1), [("conv", (3, 3), 4, R, (1, 1), (1, 1)), ("flatten",), ("dense", 3, I)]


def nll_from_outputs(kind, yhat, y):
    return costs.numerator(COST[kind], yhat, y)


def value_w(table, w, x, y, kind, prior=0.0):
    """lp at the flat weight vector w"""
    lp = -nll_from_outputs(kind, so.forward(table, w, x), y)
    if prior > 0.0:
        lp += so.log_prior(w, prior)
    return lp


def value_and_grad_w(table, w, x, y, kind, prior=0.0):
    """(lp, d lp / d w): costs.dvalue with denominator 1, sign flipped, through the oracle's reverse pass"""
    hs = [x]
    for row in table:
        hs.append(so._layer_forward(row, w, hs[-1]))
    lp = -nll_from_outputs(kind, hs[-1], y)
    g = -costs.dvalue(COST[kind], hs[-1], y, denom=1.0)
    gw = np.zeros_like(w)
    for l in range(len(table) - 1, -1, -1):
        g = so._layer_backward(table[l], w, hs[l], hs[l + 1], g, gw)
    if prior > 0.0:
        lp += so.log_prior(w, prior)
        gw = gw - w / (prior * prior)
    return lp, gw


@dataclass(frozen=True)
class Problem:
    table: list
    n: int
    w: np.ndarray            # W_swa
    p: np.ndarray            # N x M
    x: np.ndarray
    y: np.ndarray
    kind: int
    prior: float = 0.0
    decoder: tuple = None    # (layer table, flat parameters): the weights are W_swa + decoder(z), P is ignored

    @property
    def m(self):
        return self.p.shape[1]

    def weights(self, z):
        if self.decoder is not None:
            return ae.weights(self.w, self.decoder[0], self.decoder[1], z)
        return so.reconstruct(self.w, self.p, z)

    def density(self, z):
        return value_w(self.table, self.weights(z), self.x, self.y, self.kind, self.prior)

    def density_grad(self, z):
        lp, gw = value_and_grad_w(self.table, self.weights(z), self.x, self.y, self.kind, self.prior)
        if self.decoder is not None:
            return lp, ae.decode_vjp(self.decoder[0], self.decoder[1], z, gw)
        return lp, self.p.T @ gw

    def with_(self, **kw):
        d = dict(table=self.table, n=self.n, w=self.w, p=self.p, x=self.x, y=self.y, kind=self.kind, prior=self.prior, decoder=self.decoder)
        d.update(kw)
        return Problem(**d)


def labels(kind, out, b, rng, soft=False):
    """one-hot columns (categorical) / 0-1 entries (Bernoulli); soft: positive weights whose columns do NOT sum to 1"""
    if soft:
        y = rng.uniform(0.0, 1.0, (out, b)) if kind == BERNOULLI else rng.uniform(0.05, 0.9, (out, b))
    elif kind == BERNOULLI:
        y = (rng.uniform(size=(out, b)) < 0.5).astype(np.float64)
    else:
        y = np.zeros((out, b))
        y[rng.integers(0, out, b), np.arange(b)] = 1.0
    return np.asfortranarray(y)


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def dense_problem(out, b, kind, m=3, soft=False, hidden=6, act=T, wscale=0.5, pscale=0.3, head_act=I):
    """Dense 4 -> hidden -> out with an identity head (head_act: another one, on the same draws), B observations"""
    rng = np.random.default_rng(1000 * out + 10 * b + kind + (500 if soft else 0))
    table, n = so.layer_table([4, hidden, out], [act, head_act])
    x = np.asfortranarray(rng.standard_normal((4, b)))
    y = labels(kind, out, b, rng, soft)
    w = wscale * rng.standard_normal(n)
    p = np.asfortranarray(pscale * rng.standard_normal((n, m)))
    _freeze(x, y, w, p)
    return Problem(table, n, w, p, x, y, kind)


@functools.lru_cache(maxsize=None)
def conv_problem(b=7, kind=CATEGORICAL, m=3, pscale=0.3):
    rng = np.random.default_rng(77 + b)
    table, n = so.conv_table(CONV_SPEC, CONV_INPUT)
    x = np.asfortranarray(rng.standard_normal((CONV_INPUT[0] * CONV_INPUT[1] * CONV_INPUT[2], b)))
    y = labels(kind, 3, b, rng)
    w = 0.3 * rng.standard_normal(n)
    p = np.asfortranarray(pscale * rng.standard_normal((n, m)))
    _freeze(x, y, w, p)
    return Problem(table, n, w, p, x, y, kind)


def points(pb, c=5, seed=3):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((pb.m, c)))


# ---- value cases: (kind, out) with B in BATCHES each.  out covers both sides of the fused narrow tail (out <= 4: the outputs in
# fw.yhat, slots out * B apart; above: the last activation buffer, slots act_elems apart), every seg = next_pow2(out) of the
# column reduction (1, 2, 4, 8, 16, 64 partly filled at 33, full at 64, striding at 65 and 130), and B gives ragged groups of
# 64 / seg columns per wave at every seg
BATCHES = (1, 7, 37)
CATEGORICAL_OUTS = (2, 3, 4, 5, 10, 33, 64, 65, 130)
BERNOULLI_OUTS = (1, 3, 10)
VALUE_CASES = [(CATEGORICAL, o) for o in CATEGORICAL_OUTS] + [(BERNOULLI, o) for o in BERNOULLI_OUTS]
F32_DIMS = (3, 10)          # SI_F32 at 4 -> 6 -> 3 and 4 -> 6 -> 10
NPOINTS = 5                 # C stacked points


# ---- RWMH cases.  sigma_z and seed are chosen so that on the definition alone every chain (Philox chains chain_id0 .. + 2) both
# accepts and rejects within itr steps and no step is undecidable at fp64 (tests/test_likelihood_cpu.py checks exactly that);
# nchains = 1 is Philox chain chain_id0 alone, the first of the three
@dataclass(frozen=True)
class RwmhCase:
    name: str
    model: tuple            # ("dense", out, B) | ("conv", B)
    sigma_z: float
    seed: int
    f32: bool = False
    itr: int = 60
    chain_id0: int = 2
    nchains: int = 3
    modes: tuple = (0, 1, 2)

    @property
    def lp_rtol(self):
        return ra.LP_RTOL_F32 if self.f32 else ra.LP_RTOL_F64


RWMH_CASES = [
    RwmhCase("dense3", ("dense", 3, 37), 0.5, 21),          # a narrow head: the one-workgroup loop's class if it were Gaussian
    RwmhCase("dense10", ("dense", 10, 37), 0.5, 22),
    RwmhCase("conv-f64", ("conv", 7), 0.8, 23),
    RwmhCase("dense3-f32", ("dense", 3, 37), 0.5, 24, f32=True),
]
RWMH_BY_NAME = {c.name: c for c in RWMH_CASES}


def rwmh_problem(case):
    if case.model[0] == "conv":
        return conv_problem(case.model[1])
    return dense_problem(case.model[1], case.model[2], CATEGORICAL)


# ---- the loop branches of the likelihood kernels and of the cost tail's logitcrossentropy kernel (csrc/kernels_lik.hip,
# kernels_cost.hip), by arithmetic on their launch geometry:
#   lik_elem_kernel / lik_logitce_kernel run on sse_blocks = min(ceil(out B / 256), 4 num_cu) workgroups of 256 threads.  Below the
#   cap a thread of lik_elem_kernel owns at most one element; above it, its grid-stride loop takes a second lap.
#   cost_logitce_kernel runs on min(ceil(groups / 4), COST_MAX_BLOCKS) workgroups of four waves, a wave owning one group of
#   64 / seg columns at a time (seg = next_pow2(out) up to 32, 64 above): more than 4 COST_MAX_BLOCKS groups make a second lap.
COST_MAX_BLOCKS, logitce_geometry = cc.COST_MAX_BLOCKS, cc.logitce_geometry
CAPPED_OUT = 10


def capped_batch(num_cu):
    """a B with CAPPED_OUT B > 256 * 4 num_cu, whatever the part: floor(1024 num_cu / 10) + 86.  26300 on 256 CUs, where
    lik_elem_kernel's second lap holds 856 of 263000 elements (ragged: most workgroups own none) and lik_logitce_kernel walks 6575
    groups on 4096 waves"""
    return (1024 * num_cu) // CAPPED_OUT + 86


# (out, B): seg 64, 1100 groups of one column on 1024 waves, a ragged second lap; seg 16, 1026 groups of four columns, the last
# group of the second lap holding three
COST_LAP_SHAPES = tuple(cc.LOGITCE_LAP_SHAPES)

# (kind, out, head): the last layer's activation enters the gradient through dact_full(yhat, act) in the cost tail; out <= 4 is
# the fused narrow tail, above it the generic one
HEAD_CASES = ((CATEGORICAL, 3, S), (CATEGORICAL, 5, T), (CATEGORICAL, 7, SP), (BERNOULLI, 2, R), (BERNOULLI, 3, T))
HEAD_B = 7


def head_problem(kind, out, head):
    return dense_problem(out, HEAD_B, kind, head_act=head)


# ---- the gradient samplers (si_sample_mala, si_sample_hmc, si_sample_nuts, si_fit_advi) under a likelihood.  The problems are the
# builders above; the sampler settings are the same for every problem (MALA's sigma_z aside: at 0.8 several problems never accept,
# cat65 never rejects at 0.3).  tests/test_likelihood_cpu.py certifies every (sampler, problem) pair on the definition alone, also
# with the definition moved to 0.9 of the stated tolerances; tests/test_gpu_likelihood_samplers.py holds the device's traces to the
# same audits under the same conditions.
SAMPLER_SEED, SAMPLER_CHAIN_ID0, SAMPLER_CHAINS = 31, 2, 2


@dataclass(frozen=True)
class SamplerProblem:
    name: str
    build: object           # () -> Problem
    mala_sigma: float
    f32: bool = False
    # ADVI's audit holds the ELBO relative to the ELBO itself, and the entropy cancels part of the mean lp: on cat65, ber1 and conv
    # an lp moved by 0.9 lp_rtol lands at 1.0 .. 1.3e-10 relative to the ELBO, so those three are not ADVI cases
    advi: bool = True


def _cat3_decoder():
    from tests import decoder_cases as dc
    pb = dense_problem(3, 37, CATEGORICAL)
    return pb.with_(decoder=dc.random_decoder((pb.m, 4, pb.n), (T, I), seed=43, dtype=np.float64))


SAMPLER_PROBLEMS = [
    SamplerProblem("cat3", lambda: dense_problem(3, 37, CATEGORICAL), 0.3),                    # the fused narrow tail
    SamplerProblem("cat3-f32", lambda: dense_problem(3, 37, CATEGORICAL), 0.3, f32=True),
    SamplerProblem("cat10", lambda: dense_problem(10, 37, CATEGORICAL), 0.3),                  # the generic tail, seg 16
    SamplerProblem("cat65", lambda: dense_problem(65, 7, CATEGORICAL), 0.5, advi=False),       # the lanes stride the column
    SamplerProblem("cat3-soft", lambda: dense_problem(3, 37, CATEGORICAL, soft=True), 0.3),
    SamplerProblem("ber1", lambda: dense_problem(1, 37, BERNOULLI), 0.5, advi=False),
    SamplerProblem("ber10", lambda: dense_problem(10, 37, BERNOULLI), 0.3),
    SamplerProblem("ber10-f32", lambda: dense_problem(10, 37, BERNOULLI), 0.3, f32=True),
    SamplerProblem("cat3-prior", lambda: dense_problem(3, 37, CATEGORICAL).with_(prior=0.7), 0.3),
    SamplerProblem("cat3-decoder", _cat3_decoder, 0.3),
    SamplerProblem("conv", lambda: conv_problem(7), 0.3, advi=False),
]
SAMPLER_BY_NAME = {sp.name: sp for sp in SAMPLER_PROBLEMS}
ADVI_PROBLEMS = [sp for sp in SAMPLER_PROBLEMS if sp.advi]


def cached(f):
    """f memoised by the bytes of z: the audits and the oracle traces ask for the same points many times"""
    memo = {}

    def g(z):
        k = np.ascontiguousarray(z, dtype=np.float64).tobytes()
        if k not in memo:
            memo[k] = f(z)
        return memo[k]
    return g


@functools.lru_cache(maxsize=None)
def sampler_problem(name):
    """(the Problem, its density_grad memoised) of a SamplerProblem's name"""
    pb = SAMPLER_BY_NAME[name].build()
    return pb, cached(pb.density_grad)


# the audit modules' own cases with model = None: their oracle_trace / audit_case never touch `model` when value_grad is given
def mala_case(sp):
    return ma.Case(sp.name, None, sampler_problem(sp.name)[0].m, sp.mala_sigma, False, nchains=SAMPLER_CHAINS, itr=40, seed=SAMPLER_SEED,
                   chain_id0=SAMPLER_CHAIN_ID0, f32=sp.f32)


def hmc_case(sp):
    return ha.Case(sp.name, None, sampler_problem(sp.name)[0].m, 0.5, False, nchains=SAMPLER_CHAINS, itr=40, delta=0.8, seed=SAMPLER_SEED,
                   chain_id0=SAMPLER_CHAIN_ID0, f32=sp.f32)


def nuts_case(sp):
    return na.Case(sp.name, None, sampler_problem(sp.name)[0].m, 0.5, False, nchains=SAMPLER_CHAINS, itr=10, max_depth=4, seed=SAMPLER_SEED,
                   chain_id0=SAMPLER_CHAIN_ID0, f32=sp.f32)


def advi_case(sp):
    return aa.Case(sp.name, None, sampler_problem(sp.name)[0].m, False, 6, s=3, w=4, nruns=SAMPLER_CHAINS, chain_id0=SAMPLER_CHAIN_ID0,
                   ndraws=3, sigma_z=0.3, seed=SAMPLER_SEED, f32=sp.f32)


def rwmh_oracle_trace(case, density):
    pb = rwmh_problem(case)
    z = np.empty((pb.m, case.itr, case.nchains), order="F")
    lp = np.empty((case.itr, case.nchains), order="F")
    acc = np.empty(case.nchains)
    for c in range(case.nchains):
        z[:, :, c], lp[:, c], nacc = so.rwmh(density, pb.m, case.itr, case.sigma_z, case.seed, chain=case.chain_id0 + c)
        acc[c] = nacc / (case.itr - 1)
    return z, lp, acc
