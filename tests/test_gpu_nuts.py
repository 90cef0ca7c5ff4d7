"""si_sample_nuts: NUTS with its trajectory tree, step size, metric and adaptor state on the device (csrc/capi_nuts.hip,
kernels_nuts.hip).

Every case of tests/nuts_audit.py's list (certified on the oracle alone by tests/test_nuts_audit_cpu.py) runs on the device and its
trace is audited: every logged leaf is one leapfrog step from the edge the trace itself extended, with the value and gradient of the
fp64 oracle there; every decision of the tree -- divergence, merge picks, sub-tree and whole-tree U-turns, progressive picks, the
depth limit -- is the one the logged leaves give, outside its derived tolerance; the state is a bit copy of the selected leaf;
alpha, eps and Minv follow the replay and hmc_audit's adaptor conditions.

Then what the audit cannot see: the route, independence of a chain's bits from the call, the preamble shared with si_sample_hmc,
the leaf log against the public gradient, leaf_cap, the optional outputs, the refusals and state rules, and sub_inference's keyword."""
import ctypes

import numpy as np
import pytest

from tests import nuts_audit as na

pytestmark = pytest.mark.gpu


def _setup(si, ctx, case):
    pb = na.problem(case)
    ctx.infer_setup(pb.table, pb.n, case.m, pb.w, pb.p, pb.x, pb.y, case.sigma_m,
                    compute_dtype=si._capi.SI_F32 if case.f32 else si._capi.SI_F64)
    if case.prior > 0.0:
        ctx.set_prior(case.prior)
    return pb


def _run(ctx, case, **kw):
    args = dict(seed=case.seed, chain_id0=case.chain_id0, nchains=case.nchains, n_adapts=None if case.n_adapts < 0 else case.n_adapts,
                delta=case.delta, max_depth=case.max_depth, max_dh=case.max_dh, grad=True, metric=True, leaf_cap=case.leaf_cap)
    args.update(kw)
    return ctx.sample_nuts(case.itr, case.sigma_z, **args)


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _trace(out):
    z, lp, alpha, eps, depth, nleaf, sel, g, minv, leaf = out
    return na.Trace(z, lp, alpha, eps, depth, nleaf, sel, g, minv, leaf)


@pytest.mark.parametrize("case", na.CASES, ids=lambda c: c.name)
def test_every_transition_of_si_sample_nuts(si, gpu_ctx, case):
    try:
        _setup(si, gpu_ctx, case)
        tr = _trace(_run(gpu_ctx, case))
        fused, passes, search, rounds, leaves = gpu_ctx.nuts_kernel_info()
        cols = case.itr + 1
        assert tr.Z.shape == tr.G.shape == tr.Minv.shape == (case.m, cols, case.nchains)
        assert all(a.shape == (cols, case.nchains) for a in (tr.lp, tr.alpha, tr.eps, tr.depth, tr.nleaf, tr.sel))
        assert tr.leaf.shape == (3 * case.m + 1, case.leaf_cap, case.nchains)
        assert fused == int(case.fused) and passes == (1 if case.fused else case.nchains), (case.name, fused, passes)
        # the totals: every leaf counted, a round per leaf of the transition's largest tree
        assert leaves == int(tr.nleaf.sum()) and rounds == int(tr.nleaf[1:, :].max(axis=1).sum())
        assert 3 <= search <= 203
        rep = na.audit_case(case, tr)
        print("%s: fused %d, passes %d, search rounds %d, rounds %d, leaves %d: %s" % (case.name, fused, passes, search, rounds, leaves, rep.line()))
        na.check_caps(case, rep)
        if not case.f32:
            # the oracle's own kept / moved and depth counts in every chain, wherever the device's transitions were all decidable
            ref = na.cached_oracle_trace(case)
            if rep.undecidable == 0 and rep.undecidable_search == 0:
                for c in range(case.nchains):
                    assert int((tr.sel[1:, c] == 0).sum()) == int((ref.sel[1:, c] == 0).sum()), (case.name, c)
                    assert np.array_equal(np.bincount(tr.depth[1:, c], minlength=11), np.bincount(ref.depth[1:, c], minlength=11)), (case.name, c)
    finally:
        gpu_ctx.set_prior(0.0)


def test_a_chains_bits_do_not_depend_on_the_call(si, gpu_ctx):
    case = na.CASE_BY_NAME["A-M5x8"]
    _setup(si, gpu_ctx, case)
    eight = _run(gpu_ctx, case)
    assert _same(eight, _run(gpu_ctx, case))                     # a second identical call
    sizes = eight[5][1:, :].sum(axis=0)
    assert len(set(sizes.tolist())) >= 4, sizes                  # the chains' trees differ: most of them wait in most transitions
    for c in range(case.nchains):
        solo = _run(gpu_ctx, case, chain_id0=case.chain_id0 + c, nchains=1)
        assert gpu_ctx.nuts_kernel_info()[:2] == (1, 1)
        for a, b in zip(eight, solo):
            assert np.array_equal(a[..., c], b[..., 0], equal_nan=True), c


def test_the_preamble_is_si_sample_hmcs(si, gpu_ctx):
    case = na.CASE_BY_NAME["A-M33"]
    _setup(si, gpu_ctx, case)
    out = _run(gpu_ctx, case)
    zh, lph, _, epsh, gh, _ = gpu_ctx.sample_hmc(case.itr, case.sigma_z, seed=case.seed, chain_id0=case.chain_id0, nchains=case.nchains,
                                                 grad=True, metric=True)
    assert np.array_equal(out[0][:, 0, :], zh[:, 0, :]) and np.array_equal(out[1][0, :], lph[0, :])
    assert np.array_equal(out[7][:, 0, :], gh[:, 0, :]) and np.array_equal(out[3][0, :], epsh[0, :])
    assert gpu_ctx.nuts_kernel_info()[2] == gpu_ctx.hmc_kernel_info()[2]


@pytest.mark.parametrize("name", ["ragged-M5", "A-M33"])
def test_the_leaf_log_holds_the_public_gradients_bits(si, gpu_ctx, name):
    case = na.CASE_BY_NAME[name]
    _setup(si, gpu_ctx, case)
    out = _run(gpu_ctx, case)
    assert gpu_ctx.nuts_kernel_info()[0] == 1
    m = case.m
    for c in range(case.nchains):
        n = int(out[5][:, c].sum())
        log = out[9][:, :n, c]
        assert not np.isnan(log).any() and np.isnan(out[9][:, n:, c]).all()
        lpb, gb = gpu_ctx.logdensity_grad_batch(np.asfortranarray(log[:m, :]))
        assert gpu_ctx.grad_kernel_info() == 1
        assert np.array_equal(log[2 * m, :], lpb) and np.array_equal(log[2 * m + 1:, :], gb), (name, c)


def test_leaf_cap_smaller_than_the_run(si, gpu_ctx):
    case = na.CASE_BY_NAME["small-M2"]
    _setup(si, gpu_ctx, case)
    full = _run(gpu_ctx, case)
    n = full[5].sum(axis=0)
    cap = 7
    assert n.min() > cap
    short = _run(gpu_ctx, case, leaf_cap=cap)
    assert _same(full[:9], short[:9]) and np.array_equal(short[9], full[9][:, :cap, :])
    # nothing behind the cap: the raw call into a buffer with room to spare
    m, cols, nc = case.m, case.itr + 1, case.nchains
    z = np.empty((m, cols, nc), order="F")
    lp, alpha, eps = (np.empty((cols, nc), order="F") for _ in range(3))
    want = (3 * m + 1) * cap * nc
    buf = np.full(want + 64, 12345.678)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = gpu_ctx.lib.si_sample_nuts(gpu_ctx.h, case.itr, case.adapts, case.sigma_z, case.delta, case.max_depth, case.max_dh, case.seed,
                                    case.chain_id0, nc, p(z), p(lp), p(alpha), p(eps), None, None, None, None, None, p(buf), cap)
    assert rc == 0
    assert np.array_equal(buf[:want].reshape((3 * m + 1, cap, nc), order="F"), short[9]) and np.all(buf[want:] == 12345.678)
    assert np.array_equal(z, full[0]) and np.array_equal(lp, full[1]) and np.array_equal(alpha, full[2]) and np.array_equal(eps, full[3])


@pytest.mark.parametrize("name", ["ragged-M5", "conv-f64"])
def test_the_optional_outputs_are_optional(si, gpu_ctx, name):
    case = na.CASE_BY_NAME[name]
    try:
        _setup(si, gpu_ctx, case)
        full = _run(gpu_ctx, case)
        bare = _run(gpu_ctx, case, tree=False, grad=False, metric=False, leaf_cap=0)
        assert len(bare) == 4 and _same(full[:4], bare)
        assert _same(full[:7], _run(gpu_ctx, case, grad=False, metric=False, leaf_cap=0))
        assert _same(full[:4] + full[7:8], _run(gpu_ctx, case, tree=False, metric=False, leaf_cap=0))
        assert _same(full[:4] + full[8:9], _run(gpu_ctx, case, tree=False, grad=False, leaf_cap=0))
        assert _same(full[:4] + full[9:], _run(gpu_ctx, case, tree=False, grad=False, metric=False))
        assert gpu_ctx.nuts_kernel_info()[0] == int(case.fused)
    finally:
        gpu_ctx.set_prior(0.0)


def test_state_rules(si, gpu_ctx):
    caps = si._capi
    fresh = si.Context(0)
    try:
        fresh._m = 2
        with pytest.raises(si.SubspaceError) as e:
            fresh.sample_nuts(4, 0.1, seed=1)
        assert e.value.code == caps.SI_ERR_STATE and "si_infer_setup" in str(e.value)
        assert fresh.nuts_kernel_info() == (0, 0, 0, 0, 0)
    finally:
        fresh.close()
    case = na.CASE_BY_NAME["small-M2"]
    _setup(si, gpu_ctx, case)
    zpts = np.asfortranarray(np.random.default_rng(0).standard_normal((case.m, 3)))
    good_grad = gpu_ctx.logdensity_grad_batch(zpts)
    good_rwmh = gpu_ctx.sample_rwmh(8, 0.3, seed=4, nchains=2)
    good_mala = gpu_ctx.sample_mala(8, 1.0, seed=4, nchains=2, grad=True)
    good_hmc = gpu_ctx.sample_hmc(8, 1.0, seed=4, nchains=2, grad=True, metric=True)
    good_nuts = _run(gpu_ctx, case)

    def unchanged():
        assert _same(good_grad, gpu_ctx.logdensity_grad_batch(zpts))
        assert _same(good_rwmh, gpu_ctx.sample_rwmh(8, 0.3, seed=4, nchains=2))
        assert _same(good_mala, gpu_ctx.sample_mala(8, 1.0, seed=4, nchains=2, grad=True))
        assert _same(good_hmc, gpu_ctx.sample_hmc(8, 1.0, seed=4, nchains=2, grad=True, metric=True))
        assert _same(good_nuts, _run(gpu_ctx, case))

    nan = float("nan")
    for bad in (dict(itr=0), dict(nchains=0), dict(chain_id0=-1), dict(sigma_z=0.0), dict(sigma_z=-0.1), dict(sigma_z=nan),
                dict(n_adapts=-1), dict(n_adapts=5), dict(delta=0.0), dict(delta=1.0), dict(delta=nan),
                dict(max_depth=0), dict(max_depth=11), dict(max_dh=0.0), dict(max_dh=-1.0), dict(max_dh=nan)):
        kw = dict(itr=4, sigma_z=0.1, nchains=1, chain_id0=0, n_adapts=2, delta=0.8, max_depth=3, max_dh=1000.0)
        kw.update(bad)
        with pytest.raises(si.SubspaceError) as e:
            gpu_ctx.sample_nuts(kw.pop("itr"), kw.pop("sigma_z"), seed=1, **kw)
        assert e.value.code == caps.SI_ERR_INVALID, bad
        unchanged()
    # a leaf log without room: the raw call (the wrapper passes no buffer for leaf_cap = 0)
    z = np.empty((case.m, 5, 1), order="F")
    s = [np.empty((5, 1), order="F") for _ in range(3)]
    buf = np.full(16, 7.0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for cap in (0, -3):
        rc = gpu_ctx.lib.si_sample_nuts(gpu_ctx.h, 4, 2, 0.1, 0.8, 3, 1000.0, 1, 0, 1, p(z), p(s[0]), p(s[1]), p(s[2]), None, None, None,
                                        None, None, p(buf), cap)
        assert rc == caps.SI_ERR_INVALID and np.all(buf == 7.0)
    unchanged()
    gpu_ctx.rwmh_begin(4, 0.1, seed=1)
    try:
        with pytest.raises(si.SubspaceError) as e:
            gpu_ctx.sample_nuts(4, 0.1, seed=1)
        assert e.value.code == caps.SI_ERR_STATE and "step-wise RWMH session" in str(e.value)
    finally:
        gpu_ctx.rwmh_abort()
    unchanged()


def test_sub_inference_device_nuts(si, gpu_ctx):
    from subspaceinference_jl_amd import flux, samplers
    rng = np.random.default_rng(0)
    model = flux.Chain(flux.Dense(4, 8, "relu", rng=rng), flux.Dense(8, 1, rng=rng))
    x, y = rng.standard_normal((4, 50)), rng.standard_normal((1, 50))
    data = flux.DataLoader(x, y, batchsize=50)
    _, n = flux.layer_table(model)
    w_swa, p = 0.1 * rng.standard_normal(n), 0.05 * rng.standard_normal((n, 3))
    kw = dict(σ_z=0.3, itr=8, M=3, ctx=gpu_ctx, seed=5, alg=":nuts")
    z, lp = si.sub_inference(model, data, w_swa, p, chain_id=1, return_z=True, device_nuts=True, **kw)
    zd, lpd = gpu_ctx.sample_nuts(8, 0.3, seed=5, chain_id0=1, nchains=1)[:2]   # (sub_inference left its set-up in the ctx)
    assert gpu_ctx.nuts_kernel_info()[:2] == (1, 1)
    assert z.shape == (3, 8) and lp.shape == (8,)
    assert np.array_equal(z, zd[:, 1:, 0]) and np.array_equal(lp, lpd[1:, 0])
    z3, lp3 = si.sub_inference(model, data, w_swa, p, chain_id=1, nchains=3, return_z=True, device_nuts=True, **kw)
    assert z3.shape == (3, 8, 3) and lp3.shape == (8, 3) and np.array_equal(z3[:, :, 0], z) and np.array_equal(lp3[:, 0], lp)
    chn, lpw = si.sub_inference(model, data, w_swa, p, chain_id=1, device_nuts=True, **kw)
    assert len(chn) == 8 and np.array_equal(lpw, lp) and np.allclose(chn[5], w_swa + p @ z[:, 5], rtol=1e-13)
    chn3, _ = si.sub_inference(model, data, w_swa, p, chain_id=1, nchains=3, device_nuts=True, **kw)
    assert len(chn3) == 3 and len(chn3[2]) == 8 and np.allclose(chn3[2][7], w_swa + p @ z3[:, 7, 2], rtol=1e-13)
    for alg in (":mala", ":hmc", ":rwmh", ":advi"):
        with pytest.raises(si.SubspaceError):
            si.sub_inference(model, data, w_swa, p, itr=5, M=3, ctx=gpu_ctx, alg=alg, device_nuts=True)
    with pytest.raises(si.SubspaceError):
        si.sub_inference(model, data, w_swa, p, itr=5, M=3, ctx=gpu_ctx, alg=":nuts", nchains=2)
    # the default is the host loop on PCG64, unchanged: the direct samplers.nuts call with the same generator
    zh, lph = si.sub_inference(model, data, w_swa, p, chain_id=1, return_z=True, **kw)
    zh2, lph2 = si.sub_inference(model, data, w_swa, p, chain_id=1, return_z=True, device_nuts=False, **kw)
    zs, lps, _ = samplers.nuts(gpu_ctx.logdensity_grad, 3, 8, 0.3, np.random.default_rng([5, 1]))
    assert np.array_equal(zh, zs) and np.array_equal(lph, lps) and np.array_equal(zh2, zs) and np.array_equal(lph2, lps)
    assert not np.array_equal(zh, z)


def test_kernel_info_routes(si, gpu_ctx):
    for name, route in (("small-M2", 1), ("conv-f64", 0)):
        case = na.CASE_BY_NAME[name]
        try:
            _setup(si, gpu_ctx, case)
            out = _run(gpu_ctx, case, grad=False, metric=False, leaf_cap=0)
        finally:
            gpu_ctx.set_prior(0.0)
        fused, passes, search, rounds, leaves = gpu_ctx.nuts_kernel_info()
        assert fused == route and passes == (1 if route else case.nchains)
        assert leaves == int(out[5].sum()) and rounds == int(out[5][1:, :].max(axis=1).sum())
        assert rounds * case.nchains >= leaves
