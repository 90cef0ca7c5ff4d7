"""The autoencoder trained on the device (si_ae_train_*; csrc/kernels_ae_train.hip, capi_ae_train.hip) against its definition,
subspaceinference_jl_amd/autoencoder.py: train_step.  Exact results on the integer lattice of tests/ae_train_cases.py; the
real-valued cases audited step by step, each device step against ONE definition step from the device's own read-back state; same
bits twice, from the host's X as from the construction's A in place, queued as synchronous; the refusals; its neighbours on the
context; and the API end to end."""
import numpy as np
import pytest

from subspaceinference_jl_amd import autoencoder as ae
from subspaceinference_jl_amd import flux
from subspaceinference_jl_amd._capi import SI_ERR_INVALID, SI_ERR_STATE, SI_F32, SubspaceError
from tests import ae_train_cases as ac

pytestmark = pytest.mark.gpu

GPU_TOL = 8 * ac.SPREAD_TOL


def _state(ctx):
    m, v, bp = ctx.ae_train_get_opt_state()
    return [ctx.ae_train_get_params(), m, v, list(bp)]


# ---- 1. exact on the lattice ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ac.LATTICE, ids=lambda c: c.name)
def test_one_step_is_exact_on_the_lattice(si, gpu_ctx, case):
    big = case.n > 10 ** 5                       # set up and stepped once
    ids = np.asarray(case.batch, dtype=np.int64)
    for dtype in (np.float32,) if big else (np.float32, np.float64):
        table, w, x = ac.lattice_problem(case, dtype)
        for name in ("descent",) if big else sorted(ac.OPTIMISERS):
            opt = ac.OPTIMISERS[name]
            penalty = name == "momentum"
            gpu_ctx.ae_train_setup(table, w, x, case.n, max(len(ids), 5), *opt, penalty=penalty)
            assert gpu_ctx.ae_train_info() == (True, case.n, case.k, w.size, True)
            if not big:
                assert gpu_ctx.ae_train_loss() == ae.train_loss(table, w, x, penalty)
            loss = gpu_ctx.ae_train_step(ids)
            zeros = np.zeros_like(w)
            loss_d, w_d, m_d, v_d, bp_d = ae.train_step(table, w, zeros, zeros, [opt[2], opt[3]], x[:, ids], opt, penalty)
            wg, mg, vg, bpg = _state(gpu_ctx)
            assert loss == loss_d, (name, dtype)
            assert np.array_equal(wg, w_d) and wg.dtype == dtype, (name, dtype, int(np.sum(wg != w_d)))
            if opt[0] >= 1:
                assert np.array_equal(mg, m_d), (name, dtype)
            if opt[0] == 2:
                assert np.array_equal(vg, v_d), (name, dtype)
            assert bpg == bp_d
    gpu_ctx.ae_train_free()
    assert gpu_ctx.ae_train_info()[0] is False


def _lattice_construction(ctx, x, storage):
    """an open construction whose deviation matrix is exactly x (integers): pushed at n = 1 each, w_k = 2 x_k + s_{k-1} gives
    s_k = s_{k-1} + x_k and the column w_k - s_k = x_k, every value a small integer"""
    n, k = x.shape
    ctx.construct_begin(n, k, 0)
    if storage == "f32":
        ctx.construct_set_storage(SI_F32)
    s = np.zeros(n)
    for j in range(k):
        ctx.construct_push((2.0 * x[:, j] + s).astype(np.float32), 1.0)
        s = s + x[:, j]
    assert np.array_equal(ctx.construct_get_A(0, k), x)


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("case", [c for c in ac.LATTICE if c.n < 10 ** 5][1::2], ids=lambda c: c.name)
def test_one_step_in_place_is_exact_on_the_lattice(si, gpu_ctx, case, storage):
    """both storages of A read in place (TA = double and TA = float), held to array_equal against the definition"""
    ids = np.asarray(case.batch, dtype=np.int64)
    opt = ac.OPTIMISERS["adam"]
    for dtype in (np.float32, np.float64):
        table, w, x = ac.lattice_problem(case, dtype)
        _lattice_construction(gpu_ctx, x, storage)
        gpu_ctx.ae_train_setup(table, w, None, case.n, max(len(ids), 5), *opt, penalty=True)
        assert gpu_ctx.ae_train_info() == (True, case.n, case.k, w.size, True)
        assert gpu_ctx.ae_train_loss() == ae.train_loss(table, w, x, True)
        loss = gpu_ctx.ae_train_step(ids)
        zeros = np.zeros_like(w)
        loss_d, w_d, m_d, v_d, bp_d = ae.train_step(table, w, zeros, zeros, [opt[2], opt[3]], x[:, ids], opt, True)
        wg, mg, vg, bpg = _state(gpu_ctx)
        assert loss == loss_d and bpg == bp_d
        assert np.array_equal(wg, w_d) and np.array_equal(mg, m_d) and np.array_equal(vg, v_d), (dtype, storage)
        gpu_ctx.ae_train_free()


# ---- 2. the audit, step by step ---------------------------------------------------------------------------------------------------------
def _within(got, ref, dtype):
    """8 x the measured summation-order spread, relative to the array's largest entry; one Float32 ulp of the stored value on top"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    tol = GPU_TOL * np.max(np.abs(ref)) if ref.size else 0.0
    if dtype == np.float32:
        tol = tol + np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    bad = np.abs(got - ref) > tol
    return not np.any(bad), float(np.max(np.abs(got - ref) / np.maximum(tol, 1e-300)))


@pytest.mark.parametrize("case", ac.REAL, ids=lambda c: c.name)
def test_every_step_is_one_definition_step(si, gpu_ctx, case):
    table, w, x, batches = ac.real_problem(case)
    opt = ac.OPTIMISERS[case.opt]
    gpu_ctx.ae_train_setup(table, w, x, ac.REAL_N, ac.REAL_BATCH, *opt, penalty=case.penalty)
    worst = 0.0
    for step, ids in enumerate(batches):
        w0, m0, v0, bp0 = _state(gpu_ctx)
        loss = gpu_ctx.ae_train_step(ids)
        loss_d, w_d, m_d, v_d, bp_d = ae.train_step(table, w0, m0, v0, bp0, x[:, ids], opt, case.penalty)
        wg, mg, vg, bpg = _state(gpu_ctx)
        assert abs(loss - loss_d) <= GPU_TOL * abs(loss_d), (step, loss, loss_d)
        for what, got, ref in (("w", wg, w_d), ("m", mg, m_d), ("v", vg, v_d)):
            ok, ratio = _within(got, ref, case.dtype)
            worst = max(worst, ratio)
            assert ok, (step, what, ratio)
        assert bpg == bp_d
    full = gpu_ctx.ae_train_loss()
    full_d = ae.train_loss(table, _state(gpu_ctx)[0], x, case.penalty)
    assert abs(full - full_d) <= GPU_TOL * abs(full_d)
    print("%s: worst gap / tolerance = %.3f" % (case.name, worst))
    gpu_ctx.ae_train_free()


# ---- 3. the same bits: twice, in place, queued ------------------------------------------------------------------------------------------
def _run(ctx, table, w, x, n, batches, opt, penalty, queued=False):
    ctx.ae_train_setup(table, w, x, n, ac.REAL_BATCH, *opt, penalty=penalty)
    losses = [ctx.ae_train_step(ids, want_loss=not queued) for ids in batches]
    out = list(_state(ctx)) + [ctx.ae_train_loss()] + ([] if queued else [losses])
    ctx.ae_train_free()
    return out


def _same(a, b):
    return all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(a, b))


def test_same_bits_twice_and_queued(si, gpu_ctx):
    case = ac.REAL[5]
    table, w, x, batches = ac.real_problem(case)
    opt = ac.OPTIMISERS[case.opt]
    first = _run(gpu_ctx, table, w, x, ac.REAL_N, batches, opt, case.penalty)
    assert _same(first, _run(gpu_ctx, table, w, x, ac.REAL_N, batches, opt, case.penalty))
    queued = _run(gpu_ctx, table, w, x, ac.REAL_N, batches, opt, case.penalty, queued=True)
    assert _same(first[:5], queued)


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_a_in_place_equals_x_from_the_host(si, gpu_ctx, storage):
    """X = NULL reads the open construction's deviation matrix where it lies; an fp32-stored one against its widened copy"""
    case = ac.REAL[4]
    table, w, x, batches = ac.real_problem(case)
    opt = ac.OPTIMISERS[case.opt]
    rng = np.random.default_rng(9)
    gpu_ctx.construct_begin(ac.REAL_N, ac.REAL_K, 0)
    if storage == "f32":
        gpu_ctx.construct_set_storage(SI_F32)
    for i in range(ac.REAL_K):
        gpu_ctx.construct_push(rng.standard_normal(ac.REAL_N).astype(np.float32), float(1 + i // 4))
    a = gpu_ctx.construct_get_A(0, ac.REAL_K)
    in_place = _run(gpu_ctx, table, w, None, ac.REAL_N, batches, opt, case.penalty)
    assert _same(in_place, _run(gpu_ctx, table, w, a, ac.REAL_N, batches, opt, case.penalty))
    assert np.array_equal(gpu_ctx.construct_get_A(0, ac.REAL_K), a)          # training reads A, it never writes it
    gpu_ctx.ae_train_setup(table, w, None, ac.REAL_N, ac.REAL_BATCH, *opt)
    gpu_ctx.construct_begin(ac.REAL_N, ac.REAL_K, 0)                         # a new construction drops the borrowed state
    assert gpu_ctx.ae_train_info()[0] is False
    with pytest.raises(SubspaceError) as e:
        gpu_ctx.ae_train_setup(table, w, None, ac.REAL_N, ac.REAL_BATCH, *opt)   # nothing pushed yet
    assert e.value.code == SI_ERR_STATE


# ---- 4. the refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(si, gpu_ctx):
    case = ac.LATTICE[3]
    table, w, x = ac.lattice_problem(case, np.float32)
    opt = ac.OPTIMISERS["adam"]

    def refused(needle, *args, **kw):
        with pytest.raises(SubspaceError) as e:
            gpu_ctx.ae_train_setup(*args, **kw)
        assert e.value.code == SI_ERR_INVALID and needle in str(e.value), str(e.value)
        assert gpu_ctx.ae_train_info()[0] is False

    conv = [("conv", (1, 1, 1, 1), (1, 1), (1, 1), (0, 0), (1, 1), 0, 0, 1)] + [list(r) for r in table[1:]]
    refused("non-Dense", conv, w, x, case.n, 5, *opt)
    refused("first layer's in", table, w, x[:-1], case.n - 1, 5, *opt)
    bad = [list(r) for r in table]
    bad[-1][1] -= 1
    refused("last layer's out", bad, w, x, case.n, 5, *opt)
    one, n1 = ac.table_of(ac.Case("one", 4, (), (), (0,), 1, (0,)))
    refused("E + D outside", one, np.zeros(n1, dtype=np.float32), np.zeros((4, 1)), 4, 5, *opt)
    deep = ac.Case("deep", 4, (2,) * 8, (2,) * 8, (0,) * 17, 1, (0,))
    t17, n17 = ac.table_of(deep)
    refused("E + D outside", t17, np.zeros(n17, dtype=np.float32), np.zeros((4, 1)), 4, 5, *opt)
    wide, nw = ac.table_of(ac.Case("wide", 4, (257,), (), (0, 0), 1, (0,)))
    refused("hidden width above 256", wide, np.zeros(nw, dtype=np.float32), np.zeros((4, 1)), 4, 5, *opt)
    refused("batch_max outside 1 .. 8", table, w, x, case.n, 9, *opt)
    refused("batch_max outside 1 .. 8", table, w, x, case.n, 0, *opt)
    refused("opt_kind", table, w, x, case.n, 5, 3, 0.1)
    gpu_ctx.ae_train_setup(table, w, x, case.n, 5, *opt)
    before = _state(gpu_ctx)
    for ids, needle in (([0] * 6, "nb > batch_max"), ([case.k], "outside 0 .. K-1"), ([-1], "outside 0 .. K-1"), ([], "at least one")):
        with pytest.raises(SubspaceError) as e:
            gpu_ctx.ae_train_step(np.asarray(ids, dtype=np.int64))
        assert e.value.code == SI_ERR_INVALID and needle in str(e.value)
    assert _same(before, _state(gpu_ctx))            # a refused step leaves the state alone
    gpu_ctx.ae_train_free()
    with pytest.raises(SubspaceError) as e:
        gpu_ctx.ae_train_step(np.zeros(1, dtype=np.int64))
    assert e.value.code == SI_ERR_STATE


# ---- 5. its neighbours on the context keep their bits -----------------------------------------------------------------------------------
def test_training_and_inference_set_ups_are_independent_of_it(si, gpu_ctx):
    from oracle import subspace_oracle as so
    rng = np.random.default_rng(2)
    tab, n = so.layer_table([10, 20, 2], [1, 0])
    xs, ys = rng.random((10, 40)), rng.random((2, 40))
    w0 = (0.3 * rng.standard_normal(n)).astype(np.float32)
    w_swa, p, z = 0.3 * rng.standard_normal(n), np.asfortranarray(0.05 * rng.standard_normal((n, 3))), rng.standard_normal((3, 2))
    case = ac.REAL[2]
    table, w, x, batches = ac.real_problem(case)
    opt = ac.OPTIMISERS[case.opt]
    alone = _run(gpu_ctx, table, w, x, ac.REAL_N, batches[:3], opt, case.penalty)

    def neighbours(with_ae):
        out = []
        gpu_ctx.train_setup(tab, n, w0, xs, ys, 8, 2, 0.01, 0.9, 0.999)
        gpu_ctx.infer_setup(tab, n, 3, w_swa, p, xs, ys, 1.0)
        out.append(gpu_ctx.train_step(np.arange(8)))
        if with_ae:
            gpu_ctx.ae_train_setup(table, w, x, ac.REAL_N, ac.REAL_BATCH, *opt, penalty=case.penalty)
            losses = [gpu_ctx.ae_train_step(ids) for ids in batches[:2]]
        out.append(gpu_ctx.train_step(np.arange(8, 16)))
        out.append(gpu_ctx.logdensity(z))
        if with_ae:
            losses.append(gpu_ctx.ae_train_step(batches[2]))
            out_ae = _state(gpu_ctx) + [gpu_ctx.ae_train_loss(), losses]
            gpu_ctx.ae_train_free()
            assert _same(alone, out_ae)
        out.append(gpu_ctx.train_get_weights())
        out.append(gpu_ctx.logdensity(z))
        return out
    assert _same(neighbours(False), neighbours(True))


# ---- 6. the API ---------------------------------------------------------------------------------------------------------------------------
def _toy(rng):
    x, y = rng.random((10, 100)), rng.random((2, 100))
    model = flux.Chain(flux.Dense(10, 20, rng=rng), flux.Dense(20, 20, rng=rng), flux.Dense(20, 2, rng=rng))
    n, m = 682, 3
    enc = flux.Chain(flux.Dense(n, 8, rng=rng), flux.Dense(8, m, rng=rng))
    dec = flux.Chain(flux.Dense(m, 8, flux.tanh, rng=rng), flux.Dense(8, n, rng=rng))
    return model, enc, dec, flux.DataLoader(x, y, shuffle=True, rng=rng), m


@pytest.mark.parametrize("mode", [True, "auto"])
def test_auto_encoder_subspace_on_the_device_matches_the_host_route(si, mode):
    """The README toy, T = 3: 300 columns, 60 ADAM steps on Float32 parameters.  The decoder (and the encoder) the device route
    returns is held to the audit tolerance of ONE step against the host route's after the whole pass: 8 SPREAD_TOL of the array's
    largest entry and one Float32 ulp of the stored value.  (On the CPU the definition's 60-step chain gives the host route's bits
    in all three summation orders: tests/test_ae_train_cpu.py.)"""
    def run(device_autoencoder):
        model, enc, dec, data, m = _toy(np.random.default_rng(0))
        w_swa, out = si.auto_encoder_subspace(model, flux.mse, data, flux.ADAM(0.1), enc, dec, T=3, M=m, seed=4, verbose=False,
                                              device_autoencoder=device_autoencoder)
        assert out is dec
        return w_swa, flux.params(enc) + flux.params(dec)
    swa_h, host = run(False)
    swa_d, dev = run(mode)
    assert np.array_equal(swa_h, swa_d)
    ratios = [_within(a, b, np.float32)[1] for a, b in zip(dev, host)]
    print("device against host route, worst gap / audit tolerance per array:", ["%.3f" % r for r in ratios])
    for a, b in zip(dev, host):
        assert a.dtype == b.dtype == np.float32
        assert _within(a, b, np.float32)[0]
    model, enc, dec, data, m = _toy(np.random.default_rng(0))
    assert any(not np.array_equal(a, b) for a, b in zip(flux.params(enc) + flux.params(dec), dev))      # it did train


def test_a_refused_set_up_raises_or_falls_back(si):
    def run(mode):
        rng = np.random.default_rng(0)
        model, _, _, data, m = _toy(rng)
        enc = flux.Chain(flux.Dense(682, 300, rng=rng), flux.Dense(300, m, rng=rng))      # a hidden width above 256
        dec = flux.Chain(flux.Dense(m, 8, flux.tanh, rng=rng), flux.Dense(8, 682, rng=rng))
        si.auto_encoder_subspace(model, flux.mse, data, flux.ADAM(0.1), enc, dec, T=1, M=m, seed=4, verbose=False, device_autoencoder=mode)
        return flux.params(enc) + flux.params(dec)
    with pytest.raises(SubspaceError, match="hidden width above 256"):
        run(True)
    assert all(np.array_equal(a, b) for a, b in zip(run("auto"), run(False)))


@pytest.mark.parametrize("alg", ["rwmh", "hmc"])
def test_autoencoder_inference_with_the_device_autoencoder(si, alg, capsys):
    def run():
        model, enc, dec, data, m = _toy(np.random.default_rng(0))
        return si.autoencoder_inference(model, flux.mse, data, flux.ADAM(0.1), enc, dec, itr=10, T=1, M=m, alg=alg, seed=4,
                                        verbose=alg == "rwmh", device_autoencoder=True)
    chn, lp = run()
    assert len(chn) == 10 and all(w.shape == (682,) and np.all(np.isfinite(w)) for w in chn) and np.all(np.isfinite(lp))
    if alg == "rwmh":                                     # verbose: si_ae_train_loss after every step
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("autoloss(re_weight) = ")]
        assert len(lines) == 20 and all(np.isfinite(float(ln.split("=")[1])) for ln in lines)
    chn2, lp2 = run()
    assert np.array_equal(lp2, lp) and all(np.array_equal(a, b) for a, b in zip(chn, chn2))
