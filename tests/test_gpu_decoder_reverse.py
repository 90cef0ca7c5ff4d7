"""The decoder's reverse kernels on the device (decoder_last_rev_partial_kernel, decoder_last_rev_final_kernel, decoder_head_rev_kernel
in csrc/kernels_decoder.hip) through si_decode_vjp, which runs the seam form_weights(keep_y) / pull_back_to_z and nothing else --
launch for launch what si_logdensity_grad runs around the model's sweep.  Exact results on the integer lattices of
tests/decoder_cases.py (REVERSE_LATTICE, FORWARD_BIG: every wave, a second pass of every thread-strided loop, a clipped and an empty
row block, one to three h0 rounds with and without a tail, head widths around 256 and at 1024, eight layers, the forward's
grid-stride loop on its second pass); tests/test_autoencoder_cpu.py proves on the CPU that the lists are exact and that they catch
ten faults restated in int64.  Then: the bits do not depend on what ran before, real-valued decoders with all eight activations,
the fixed-order claim for the gradient at every column, the second chunk of form_weights, and HMC, NUTS and ADVI with a decoder
audited against the definition."""
import time

import numpy as np
import pytest

from subspaceinference_jl_amd import autoencoder as ae
from subspaceinference_jl_amd import flux
from tests import advi_audit as aa
from tests import decoder_cases as dc
from tests import hmc_audit as ha
from tests import nuts_audit as nta
from tests.test_gpu_decoder import G_ATOL, G_RTOL, SAMPLER_M, _grad_close, _oracle, _sampler_problem

pytestmark = pytest.mark.gpu


def _setup(ctx, case_or_pb, m):
    pb = dc.case_problem(case_or_pb) if isinstance(case_or_pb, dc.LatticeCase) else case_or_pb
    ctx.infer_setup([list(r) for r in pb.table], pb.n, m, pb.w_swa, np.zeros((pb.n, m), order="F"), pb.x, pb.y, pb.sigma_m)
    return pb


# ---- 1. the pull-back, exact ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.REVERSE_LATTICE, ids=lambda c: c.name)
def test_the_pull_back_is_exact_on_the_lattice(si, gpu_ctx, case):
    _setup(gpu_ctx, case, case.m)
    wdec_i, z_i = dc.lattice_ints(case)
    gy_i = dc.lattice_cotangent(case)
    gy = gy_i.astype(np.float64)
    points = dc.reverse_points(case)
    ref = None
    for dtype, code in ((np.float32, si._capi.SI_F32), (np.float64, si._capi.SI_F64)):
        table, wdec, z = dc.lattice_decoder(case, dtype)
        if ref is None:
            ref = {c: dc.int_decode_vjp(table, wdec_i, z_i[:, c], gy_i).astype(np.float64) for c in points}
        gpu_ctx.set_decoder(table, wdec)
        assert gpu_ctx.decoder_info() == (case.depth, case.widths[-2], code)
        for c in points:
            g = gpu_ctx.decode_vjp(z[:, c], gy)
            assert np.array_equal(g, ref[c]), (case.name, dtype.__name__, c, np.flatnonzero(g != ref[c])[:8])
    gpu_ctx.set_decoder(None, None)


# ---- 2. the forward at the new shapes, exact --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.FORWARD_BIG, ids=lambda c: c.name)
def test_decode_and_reconstruct_are_exact_at_the_wide_shapes(si, gpu_ctx, case):
    k = dc.kernel_constants()
    if case.name == dc.GRID_CASE:
        import torch
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        if dc.forward_passes(case.n, k, cus) < 2:
            pytest.skip("%d CUs: the last layer forward's grid-stride loop runs a second pass from N = %d on, this case has N = %d"
                        % (cus, 2 * k.grid_per_cu * cus * k.threads + 1, case.n))
    pb = _setup(gpu_ctx, case, case.m)
    wdec_i, z_i = dc.lattice_ints(case)
    npts = max(dc.FORWARD_BIG_POINTS)
    table, _ = dc.decoder_table(case.widths, case.acts)
    y_ref = dc.int_decode(table, wdec_i, z_i[:, :npts])
    w_ref = (pb.w_swa.astype(np.int64)[:, None] + y_ref).astype(np.float64)
    y_ref = y_ref.astype(np.float64)
    for dtype in (np.float32, np.float64):
        _, wdec, z = dc.lattice_decoder(case, dtype)
        gpu_ctx.set_decoder(table, wdec)
        for c in dc.FORWARD_BIG_POINTS:
            assert np.array_equal(gpu_ctx.decode(z[:, :c]), y_ref[:, :c]), (case.name, dtype.__name__, c)
            assert np.array_equal(gpu_ctx.reconstruct(z[:, :c]), w_ref[:, :c]), (case.name, dtype.__name__, c)
    gpu_ctx.set_decoder(None, None)


# ---- 3. the bits do not depend on what ran before; the refusals -------------------------------------------------------------------------
def test_the_pull_back_does_not_depend_on_the_state(si, gpu_ctx):
    state = si._capi.SI_ERR_STATE
    case = dc.REVERSE_BY_NAME["W-257-255"]
    ptr = si._capi._ptr
    with si.Context(0) as fresh:
        a, b = np.zeros(case.m), np.zeros(case.n)
        assert fresh.lib.si_decode_vjp(fresh.h, ptr(a), ptr(b), ptr(a)) == state            # before a set-up
        assert fresh.lib.si_decode_vjp(fresh.h, ptr(a), None, ptr(a)) == si._capi.SI_ERR_INVALID
    _setup(gpu_ctx, case, case.m)
    table, wdec, z = dc.lattice_decoder(case, np.float64)
    wdec_i, z_i = dc.lattice_ints(case)
    gy_i = dc.lattice_cotangent(case)
    gy = gy_i.astype(np.float64)
    with pytest.raises(si.SubspaceError) as ei:
        gpu_ctx.decode_vjp(z[:, 0], gy)                                       # no decoder set
    assert ei.value.code == state
    gpu_ctx.set_decoder(table, wdec)
    ref = dc.int_decode_vjp(table, wdec_i, z_i[:, 0], gy_i).astype(np.float64)
    first = gpu_ctx.decode_vjp(z[:, 0], gy)                                  # `hid` holds one point
    assert np.array_equal(first, ref)
    assert gpu_ctx.decode(z).shape == (case.n, 9)                            # ... and is regrown to nine
    assert np.array_equal(gpu_ctx.decode_vjp(z[:, 0], gy), first)
    lp, g = gpu_ctx.logdensity_grad(z[:, 2])
    assert np.isfinite(lp) and np.all(np.isfinite(g))
    assert np.array_equal(gpu_ctx.decode_vjp(z[:, 0], gy), first)
    other = gpu_ctx.decode_vjp(z[:, 1], gy)
    assert np.array_equal(other, dc.int_decode_vjp(table, wdec_i, z_i[:, 1], gy_i).astype(np.float64)) and not np.array_equal(other, first)
    assert np.array_equal(gpu_ctx.decode_vjp(z[:, 0], gy), first)
    gpu_ctx.rwmh_begin(3, 0.1, 1)
    with pytest.raises(si.SubspaceError) as ei:
        gpu_ctx.decode_vjp(z[:, 0], gy)                                       # a step-wise session is open
    assert ei.value.code == state
    gpu_ctx.rwmh_abort()
    assert np.array_equal(gpu_ctx.decode_vjp(z[:, 0], gy), first)
    gpu_ctx.set_decoder(None, None)
    with pytest.raises(si.SubspaceError) as ei:
        gpu_ctx.decode_vjp(z[:, 0], gy)
    assert ei.value.code == state


# ---- 4. real-valued decoders, all eight activations -----------------------------------------------------------------------------------------
# G_RTOL / G_ATOL, not exactness: the last layer's block and tree order is not the definition's ascending order, and the device's
# tanh / exp are not NumPy's.
@pytest.mark.parametrize("shape", ["3-6-129", "300-9-69615"])
def test_real_decoders_against_the_definition(si, gpu_ctx, shape):
    if shape == "3-6-129":
        pb, widths = dc.problem(129), (3, 6, 129)
    else:
        pb, widths = dc.big_problem("N_2WAVE"), (300, 9, dc.big_n("N_2WAVE"))       # H = 9: three h0 rounds, rows on two waves
    _setup(gpu_ctx, pb, widths[0])
    rng = np.random.default_rng(len(shape))
    z, gy = rng.standard_normal(widths[0]), rng.standard_normal(pb.n)
    for act in range(8):
        for dtype in (np.float32, np.float64):
            table, wdec = dc.random_decoder(widths, (act, act), seed=300 + act, dtype=dtype)
            gpu_ctx.set_decoder(table, wdec)
            g = gpu_ctx.decode_vjp(z, gy)
            ref = ae.decode_vjp(table, wdec, z, gy)
            err = float(np.max(np.abs(g - ref) / (G_RTOL * np.abs(ref) + G_ATOL * np.max(np.abs(ref)))))
            print("%s, act %d, %s: worst error / bound %.3g" % (shape, act, dtype.__name__, err))
            assert np.max(np.abs(ref)) > 0.0 and _grad_close(g, ref), (shape, act, dtype.__name__, err)
    gpu_ctx.set_decoder(None, None)


# ---- 5. the fixed-order claim for the gradient ----------------------------------------------------------------------------------------------
def test_a_points_gradient_bits_depend_on_neither_column_nor_call_nor_context(si, gpu_ctx):
    n, m, act = 129, 2, flux.tanh                                              # test_oracle_parity_for_every_activation's problem
    pb = dc.problem(n)
    table, wdec = dc.random_decoder((m, 4, n), (act, act), seed=100 + act, dtype=np.float64)
    rng = np.random.default_rng(act)
    z = np.asfortranarray(rng.standard_normal((m, 5)))
    z[:, 3] = z[:, 1]
    gw = rng.standard_normal(n)
    _setup(gpu_ctx, pb, m)
    gpu_ctx.set_decoder(table, wdec)
    lpb, gb = gpu_ctx.logdensity_grad_batch(z)
    assert gpu_ctx.grad_kernel_info() == 0
    for c in range(5):
        lp1, g1 = gpu_ctx.logdensity_grad(z[:, c])
        assert lp1 == lpb[c] and np.array_equal(g1, gb[:, c]), c
    assert lpb[1] == lpb[3] and np.array_equal(gb[:, 1], gb[:, 3])
    ref = _oracle(pb, table, wdec, 0.0)(z[:, 4])
    assert abs(lpb[4] - ref[0]) <= 1e-11 * abs(ref[0]) and _grad_close(gb[:, 4], ref[1])
    v = [gpu_ctx.decode_vjp(z[:, 0], gw), gpu_ctx.decode_vjp(z[:, 0], gw)]
    with si.Context(0) as second:
        _setup(second, pb, m)
        second.set_decoder(table, wdec)
        v.append(second.decode_vjp(z[:, 0], gw))
        lp2, g2 = second.logdensity_grad(z[:, 4])
        assert lp2 == lpb[4] and np.array_equal(g2, gb[:, 4])
    assert np.array_equal(v[0], v[1]) and np.array_equal(v[0], v[2])
    assert _grad_close(v[0], ae.decode_vjp(table, wdec, z[:, 0], gw))
    gpu_ctx.set_decoder(None, None)


# ---- 6. the chunk boundary of form_weights -----------------------------------------------------------------------------------------------
def test_the_second_chunk_of_form_weights(si, gpu_ctx):
    k = dc.kernel_constants()
    itr, nchains = 8200, 2
    assert k.chunk < itr * nchains < 2 * k.chunk
    pb = dc.problem(7)
    _setup(gpu_ctx, pb, 2)
    table, wdec = dc.random_decoder((2, 3, 7), (flux.tanh, flux.identity), seed=11)
    gpu_ctx.set_decoder(table, wdec)
    t0 = time.perf_counter()
    zs, lp, acc, w = gpu_ctx.sample_rwmh_weights(itr, 0.5, seed=5, chain_id0=2, nchains=nchains)     # 16 400 points in one form_weights
    print("sample_rwmh_weights(%d, nchains=%d): %.2f s" % (itr, nchains, time.perf_counter() - t0))
    assert w.shape == (7, itr, nchains) and np.all(np.isfinite(lp))
    for c in range(nchains):
        assert np.array_equal(w[:, :, c], gpu_ctx.reconstruct(zs[:, :, c])), c                      # (groups of at most 64 points)
        assert np.allclose(w[:, :, c], ae.weights(pb.w_swa, table, wdec, zs[:, :, c]), rtol=1e-10, atol=1e-12)
    assert len({zs[:, t, 1].tobytes() for t in range(itr - 100, itr)}) > 2                          # (the chain still moves at the end)
    gpu_ctx.set_decoder(None, None)


# ---- 7. HMC, NUTS and ADVI with a decoder ---------------------------------------------------------------------------------------------------
# Chosen on the CPU from the definition's trace alone (hmc_audit / nuts_audit.oracle_trace driven by `_oracle`), among sigma_z in
# {0.5, 1.0} and seeds 1..8 at Philox chains 1 and 2: the reference's own audit has no undecidable search and no undecidable
# transition; both HMC chains accept and reject (7 or 8 accepts, 2 or 3 rejects of 10); both NUTS chains reach depth >= 2 (depths
# [2 1 1 1 2 1] and [3 1 3 2 3 3] at max_depth = 3, with sub-tree and tree U-turns and a divergence among the exits).
SAMPLER_SIGMA_Z, SAMPLER_SEED, SAMPLER_CHAIN0, SAMPLER_CHAINS = 0.5, 7, 1, 2
HMC_CASE = ha.Case("decoder", None, SAMPLER_M, SAMPLER_SIGMA_Z, False, nchains=SAMPLER_CHAINS, itr=10, seed=SAMPLER_SEED, chain_id0=SAMPLER_CHAIN0)
NUTS_CASE = nta.Case("decoder", None, SAMPLER_M, SAMPLER_SIGMA_Z, False, nchains=SAMPLER_CHAINS, itr=6, max_depth=3, seed=SAMPLER_SEED,
                     chain_id0=SAMPLER_CHAIN0)
ADVI_CASE = aa.Case("decoder", None, SAMPLER_M, False, 4, s=3, nruns=SAMPLER_CHAINS, chain_id0=SAMPLER_CHAIN0, seed=SAMPLER_SEED)


def _states_are_the_point_gradient(ctx, z, lp, g):
    """lp and G at column 0 and at every state a chain moved to are si_logdensity_grad's bits there"""
    for c in range(z.shape[2]):
        for t in [0] + [t for t in range(1, z.shape[1]) if not np.array_equal(z[:, t, c], z[:, t - 1, c])]:
            lp1, g1 = ctx.logdensity_grad(z[:, t, c])
            assert lp1 == lp[t, c] and np.array_equal(g1, g[:, t, c]), (c, t)


def test_hmc_with_a_decoder(si, gpu_ctx):
    case = HMC_CASE
    pb, table, wdec = _sampler_problem(gpu_ctx)
    vg = _oracle(pb, table, wdec, 0.0)
    z, lp, alpha, eps, g, minv = gpu_ctx.sample_hmc(case.itr, case.sigma_z, seed=case.seed, chain_id0=case.chain_id0, nchains=case.nchains,
                                                   grad=True, metric=True)
    fused, passes, rounds = gpu_ctx.hmc_kernel_info()
    assert (fused, passes) == (0, case.nchains)                              # StackedVgrad's column-by-column route
    rep = ha.audit_case(case, z, lp, alpha, eps, g, minv, value_grad=vg)
    print("hmc with a decoder: fused %d, passes %d, search rounds %d: %s" % (fused, passes, rounds, rep.line()))
    assert rep.undecidable == 0 and rep.steps == case.itr * case.nchains
    assert min(rep.chain_accepts) >= 1 and min(rep.chain_rejects) >= 1
    assert rounds == 1 + max(rep.search_evals)
    _states_are_the_point_gradient(gpu_ctx, z, lp, g)
    gpu_ctx.set_decoder(None, None)


def test_nuts_with_a_decoder(si, gpu_ctx):
    case = NUTS_CASE
    pb, table, wdec = _sampler_problem(gpu_ctx)
    vg = _oracle(pb, table, wdec, 0.0)
    out = gpu_ctx.sample_nuts(case.itr, case.sigma_z, seed=case.seed, chain_id0=case.chain_id0, nchains=case.nchains, max_depth=case.max_depth,
                              max_dh=case.max_dh, grad=True, metric=True, leaf_cap=case.leaf_cap)
    tr = nta.Trace(*out)
    fused, passes, search, rounds, leaves = gpu_ctx.nuts_kernel_info()
    assert (fused, passes) == (0, case.nchains)
    assert leaves == int(tr.nleaf.sum()) and rounds == int(tr.nleaf[1:, :].max(axis=1).sum())
    rep = nta.audit_case(case, tr, value_grad=vg)
    print("nuts with a decoder: fused %d, passes %d, search rounds %d, rounds %d, leaves %d: %s" % (fused, passes, search, rounds, leaves, rep.line()))
    assert rep.transitions == case.itr * case.nchains and rep.undecidable == 0 and rep.undecidable_search == 0
    assert all(max(d) >= 2 for d in rep.chain_depths), rep.chain_depths
    _states_are_the_point_gradient(gpu_ctx, tr.Z, tr.lp, tr.G)
    gpu_ctx.set_decoder(None, None)


def test_advi_with_a_decoder(si, gpu_ctx):
    case = ADVI_CASE
    pb, table, wdec = _sampler_problem(gpu_ctx)
    vg = _oracle(pb, table, wdec, 0.0)
    theta, z, elbo, trace, points = gpu_ctx.fit_advi(case.t, case.sigma_z, case.seed, samples_per_step=case.s, eta=case.eta, tau=case.tau,
                                                     window=case.w, chain_id0=case.chain_id0, nruns=case.nruns, ndraws=case.ndraws, trace=True)
    fused, passes = gpu_ctx.advi_kernel_info()
    assert (fused, passes) == (0, case.nruns * case.s)
    rep = aa.audit_case(case, trace, points, elbo, theta, z, value_grad=vg)
    print("advi with a decoder: fused %d, passes %d: %s" % (fused, passes, rep.line()))
    assert rep.steps == case.t * case.nruns
    # the mu half of every update and every ELBO estimate from si_logdensity_grad_batch at the trace's own points, to the bits
    m, ns, nt, nr = points.shape
    lpb, gb = gpu_ctx.logdensity_grad_batch(np.asfortranarray(points.reshape(m, -1, order="F")))
    lpb, gb = lpb.reshape(ns, nt, nr, order="F"), gb.reshape(m, ns, nt, nr, order="F")
    for r in range(nr):
        aa.mu_replay(trace[:, :, r], lambda t: (lpb[:, t, r], gb[:, :, t, r]), ns, case.w, case.eta, case.tau)
        for t in range(nt):
            assert elbo[t, r] == aa.elbo_of(lpb[:, t, r], aa.entropy(trace[m:, t, r])), (r, t)
    gpu_ctx.set_decoder(None, None)
