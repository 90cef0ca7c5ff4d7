"""SHA-256 of every output array of the four device samplers (si_sample_mala, si_sample_hmc, si_sample_nuts, si_fit_advi) on a
fixed list of the audits' cases: the smallest shapes that reach each path of their kernels -- M = 1 (half a Philox block), odd M, a
second lap of the thread-strided loops, several chains, the prior, window closes, divergent and non-finite leaves, the ring wrap,
the route that is not fused.  The optional outputs are asked for: G, Minv, depth / nleaf / sel, the leaf log, the theta trace, the
points, the ELBO.

Only the public Context API is used, so the same file runs against any build of the library:

    python tools/sampler_digests.py                         # the library of this tree
    python tools/sampler_digests.py --lib PATH --out FILE   # another build; the digests as JSON

tests/golden/device_sampler_digests.json is this tool's output on the MI355X; tests/test_gpu_sampler_bits.py compares the tree
under test with it.  The audits compare lp and g through tolerances in places; this comparison has none."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {
    "mala": ("small-M1", "ragged-M5", "A-M33-prior", "A-M33x64", "small-M513", "conv-f64"),
    "hmc": ("small-M1", "ragged-M5", "A-M33", "small-M513", "small-M2-adapt200", "conv-f64"),
    "nuts": ("small-M1", "ragged-M5", "A-M33", "small-M513", "small-M2-window", "small-M2-maxdh", "relu-deep-overflow", "conv-f64"),
    "advi": ("M1-S1", "M3-S10", "M33-W4-T11", "M300-S2", "M3-R3", "conv-f64"),
}
OUTPUTS = {
    "mala": ("Z", "lp", "accept_rate", "G"),
    "hmc": ("Z", "lp", "alpha", "eps", "G", "Minv"),
    "nuts": ("Z", "lp", "alpha", "eps", "depth", "nleaf", "sel", "G", "Minv", "leaf"),
    "advi": ("theta", "Z", "elbo", "theta_trace", "points"),
}


def _audit(sampler):
    from tests import advi_audit, hmc_audit, mala_audit, nuts_audit
    return {"mala": mala_audit, "hmc": hmc_audit, "nuts": nuts_audit, "advi": advi_audit}[sampler]


def run_case(si, ctx, sampler, name):
    """the outputs of one case, every optional one included, in OUTPUTS' order"""
    audit = _audit(sampler)
    case = audit.CASE_BY_NAME[name]
    pb = audit.problem(case)
    ctx.infer_setup(pb.table, pb.n, case.m, pb.w, pb.p, pb.x, pb.y, case.sigma_m, compute_dtype=si._capi.SI_F32 if case.f32 else si._capi.SI_F64)
    try:
        if case.prior > 0.0:
            ctx.set_prior(case.prior)
        if sampler == "advi":
            return ctx.fit_advi(case.t, case.sigma_z, case.seed, samples_per_step=case.s, eta=case.eta, tau=case.tau, window=case.w,
                                chain_id0=case.chain_id0, nruns=case.nruns, ndraws=case.ndraws, trace=True)
        args = dict(seed=case.seed, chain_id0=case.chain_id0, nchains=case.nchains, grad=True)
        if sampler == "mala":
            return ctx.sample_mala(case.itr, case.sigma_z, **args)
        args.update(n_adapts=None if case.n_adapts < 0 else case.n_adapts, delta=case.delta, metric=True)
        if sampler == "hmc":
            return ctx.sample_hmc(case.itr, case.sigma_z, **args)
        return ctx.sample_nuts(case.itr, case.sigma_z, max_depth=case.max_depth, max_dh=case.max_dh, leaf_cap=case.leaf_cap, **args)
    finally:
        ctx.set_prior(0.0)


def digests_of(sampler, out):
    assert len(out) == len(OUTPUTS[sampler]), (sampler, len(out))
    return {k: hashlib.sha256(np.asarray(a).tobytes(order="F")).hexdigest() for k, a in zip(OUTPUTS[sampler], out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libsubspace_hip.so")
    ap.add_argument("--out", default=None, help="write the digests here as JSON (default: standard output)")
    args = ap.parse_args()
    import subspaceinference_jl_amd as si
    if args.lib:
        si._capi.LIB_PATH = os.path.abspath(args.lib)
    result, slowest = {}, (0.0, "")
    with si.Context(0) as ctx:
        for sampler, names in CASES.items():
            for name in names:
                t0 = time.perf_counter()
                result["%s/%s" % (sampler, name)] = digests_of(sampler, run_case(si, ctx, sampler, name))
                slowest = max(slowest, (time.perf_counter() - t0, "%s/%s" % (sampler, name)))
    print("library: %s   %d cases, slowest %s: %.2f s" % (si._capi.LIB_PATH, len(result), slowest[1], slowest[0]), file=sys.stderr)
    text = json.dumps(result, indent=1, sort_keys=True) + "\n"
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
