"""The device training step with the costs of si_train_set_cost (csrc/kernels_cost.hip) against their definition, costs.py pushed
through the oracle's layers on the CPU (tests/cost_cases.py: reference).  The gradient is read back with train_grad +
train_grad_get."""
import numpy as np
import pytest

from oracle import subspace_oracle as so
from subspaceinference_jl_amd import costs
from tests import cost_cases as cc
from tests.test_gpu_conv import CASES as CONV_CASES

pytestmark = pytest.mark.gpu


def _dense_problem(dims, acts, btot, kind, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    table, n = so.layer_table(dims, acts)
    w0 = (0.3 * rng.standard_normal(n)).astype(np.float32)
    x = np.asfortranarray(rng.standard_normal((dims[0], btot)).astype(dtype))
    y = np.asfortranarray(cc.targets(kind, dims[-1], btot, rng).astype(dtype))
    return table, n, w0, x, y, rng


def _check_against_definition(ctx, table, w0, x, y, ids, cost, tag):
    """the bounds tests/test_gpu_parity.py holds the mse gradient to"""
    kind, param = cost
    num = ctx.train_grad(ids, ids.size)
    g = ctx.train_grad_get()
    num_ref, g_ref = cc.reference(table, w0.astype(np.float64), np.asarray(x[:, ids], dtype=np.float64),
                                  np.asarray(y[:, ids], dtype=np.float64), kind, param)
    den = costs.denominator(kind, y.shape[0], ids.size)
    print(tag, "loss", num / den, num_ref / den, "max |g - g_ref|", np.abs(g - g_ref).max(), "|g_ref|max", np.abs(g_ref).max())
    assert np.all(np.isfinite(g)) and np.isfinite(num), tag
    assert np.isclose(num / den, num_ref / den, rtol=1e-10), tag
    assert np.allclose(g, g_ref, rtol=1e-8, atol=1e-10 * max(1.0, np.abs(g_ref).max())), tag
    return num, g


# ---- 1. the fp64 Dense route -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", cc.HEADS)
@pytest.mark.parametrize("cost", cc.ALL_COSTS, ids=cc.cost_id)
def test_f64_dense_gradient(gpu_ctx, cost, out):
    """every cost x every head x batches of 1, 3, 5 and 257 observations, each a random subset of 300"""
    kind, param = cost
    dims = cc.head_dims(out)
    table, n, w0, x, y, rng = _dense_problem(dims, [cc.T, cc.I], cc.B_TOTAL, kind, 1000 * kind + out)
    gpu_ctx.train_setup(table, n, w0, x, y, max(cc.BATCHES), 0, 0.1)
    gpu_ctx.train_set_cost(kind, param)
    assert gpu_ctx.train_cost_info() == (kind, param)
    for nb in cc.BATCHES:
        ids = rng.permutation(cc.B_TOTAL)[:nb]
        _check_against_definition(gpu_ctx, table, w0, x, y, ids, cost, "%s out %d nb %d" % (costs.NAMES[kind], out, nb))


@pytest.mark.parametrize("cost", cc.NEW_COSTS, ids=cc.cost_id)
@pytest.mark.parametrize("out,act", [(3, cc.S), (5, cc.T), (2, cc.R), (7, so.ACT_SOFTPLUS)])
def test_last_layer_activation_applies(gpu_ctx, cost, out, act):
    """Delta_L = dL/dyhat .* act_L'(yhat), as for mse: fused heads (3, 2) and generic ones (5, 7)"""
    kind, param = cost
    table, n, w0, x, y, rng = _dense_problem([4, 6, out], [cc.R, act], 40, kind, 50 + 10 * kind + out)
    gpu_ctx.train_setup(table, n, w0, x, y, 40, 0, 0.1)
    gpu_ctx.train_set_cost(kind, param)
    _check_against_definition(gpu_ctx, table, w0, x, y, rng.permutation(40)[:33], cost, "act %d" % act)


# ---- 2. exact cases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out,nb", [(2, 8), (8, 16)])
@pytest.mark.parametrize("cost", [(costs.MAE, 0.0), (costs.HUBER, 1.0)], ids=cc.cost_id)
def test_mae_and_huber_exact_on_the_half_integer_lattice(gpu_ctx, cost, out, nb):
    """half-integer weights, biases and targets, even-integer inputs, identity / relu layers: every activation is an integer or a
    half-integer, every residual one of 0, +-0.5, +-1, +-1.5 (both Huber branches, the strict boundary |r| = 1 and sign(0)), and with
    out * nb a power of two every product and sum of the step is exact in fp64 whatever its order: the device's numbers ARE the
    definition's"""
    kind, param = cost
    rng = np.random.default_rng(7 * out + kind)
    dims, acts = [4, 6, out], [cc.R, cc.I]
    table, n = so.layer_table(dims, acts)
    w0 = (rng.integers(-2, 3, n) * 0.5).astype(np.float32)
    x = np.asfortranarray(2.0 * rng.integers(-1, 2, (4, nb)))
    yhat = so.forward(table, w0.astype(np.float64), x)
    r = rng.integers(-3, 4, (out, nb)) * 0.5
    r.reshape(-1)[:7] = [0.0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5]
    y = np.asfortranarray(yhat - r)
    assert np.array_equal(yhat - y, r)
    gpu_ctx.train_setup(table, n, w0, x, y, nb, 0, 0.1)
    gpu_ctx.train_set_cost(kind, param)
    num = gpu_ctx.train_grad(np.arange(nb), nb)
    g = gpu_ctx.train_grad_get()
    num_ref, g_ref = cc.reference(table, w0.astype(np.float64), x, y, kind, param)
    assert num == num_ref and np.array_equal(g, g_ref)


@pytest.mark.parametrize("out", [2, 4, 8, 64])
def test_logitcrossentropy_exact_bias_gradient(gpu_ctx, out):
    """last-layer weights zero, equal biases: every logit is the bias, exp(yhat - m) = 1, the sum is out and p = 1 / out exactly; with
    one-hot targets and nb a power of two the bias gradient of the last layer, rowsum((p - Y) / nb), is exact"""
    nb = 16
    rng = np.random.default_rng(out)
    dims = [4, 6, out]
    table, n = so.layer_table(dims, [cc.T, cc.I])
    w0 = (0.3 * rng.standard_normal(n)).astype(np.float32)
    _, _, _, w_off, b_off = table[-1]
    w0[w_off:b_off] = 0.0
    w0[b_off:b_off + out] = 0.5
    x = np.asfortranarray(rng.standard_normal((4, nb)))
    y = np.zeros((out, nb), order="F")
    y[rng.integers(0, out, nb), np.arange(nb)] = 1.0
    gpu_ctx.train_setup(table, n, w0, x, y, nb, 0, 0.1)
    gpu_ctx.train_set_cost(costs.LOGITCE)
    num = gpu_ctx.train_grad(np.arange(nb), nb)
    g = gpu_ctx.train_grad_get()
    db_ref = np.sum((1.0 / out - y) * (1.0 / nb), axis=1)
    assert np.array_equal(g[b_off:b_off + out], db_ref)
    g_ref = cc.reference(table, w0.astype(np.float64), x, y, costs.LOGITCE)[1]
    assert np.array_equal(g_ref[b_off:b_off + out], db_ref)
    assert np.allclose(g, g_ref, rtol=1e-8, atol=1e-10 * max(1.0, np.abs(g_ref).max()))
    assert np.isclose(num / nb, np.log(out), rtol=1e-14)


# ---- 3. stability ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", [3, 5, 70])
@pytest.mark.parametrize("cost", [(costs.LOGITCE, 0.0), (costs.LOGITBCE, 0.0)], ids=cc.cost_id)
def test_logits_of_800_stay_finite(gpu_ctx, cost, out):
    kind, param = cost
    table, n, w0, x, y, rng = _dense_problem([4, 6, out], [cc.T, cc.I], 21, kind, 300 + out + kind)
    b_off = table[-1][4]
    w0[b_off] = 800.0
    w0[b_off + 1] = -800.0
    w0[b_off + out - 1] = 800.0 if out > 3 else w0[b_off + out - 1]
    gpu_ctx.train_setup(table, n, w0, x, y, 21, 0, 0.1)
    gpu_ctx.train_set_cost(kind, param)
    _check_against_definition(gpu_ctx, table, w0, x, y, np.arange(21), cost, "big logits out %d" % out)


# ---- 4. the Conv route -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cost", [(costs.LOGITCE, 0.0), (costs.HUBER, 1.0)], ids=cc.cost_id)
@pytest.mark.parametrize("case", [0, 1, 4])
def test_conv_gradient_and_step(gpu_ctx, case, cost):
    """the bounds of tests/test_gpu_conv.py: test_conv_training_gradient_and_step"""
    kind, param = cost
    whc, spec, b = CONV_CASES[case]
    rng = np.random.default_rng(140 + case)
    table, n = so.conv_table(spec, whc)
    w0 = (0.3 * rng.standard_normal(n)).astype(np.float32)
    x = np.asfortranarray(rng.standard_normal((whc[0] * whc[1] * whc[2], b)))
    out = so.forward(table, w0.astype(np.float64), x[:, :1]).shape[0]
    y = cc.targets(kind, out, b, rng)
    gpu_ctx.train_setup(table, n, w0, x, y, b, 0, 0.05)      # Descent(0.05)
    gpu_ctx.train_set_cost(kind, param)
    idx = np.random.default_rng(1).permutation(b)[: max(2, b // 2)]
    num = gpu_ctx.train_grad(idx, idx.size)
    g = gpu_ctx.train_grad_get()
    w64 = w0.astype(np.float64)
    num_ref, g_ref = cc.reference(table, w64, np.asfortranarray(x[:, idx]), np.asfortranarray(y[:, idx]), kind, param)
    print("conv case", case, costs.NAMES[kind], num, num_ref, np.abs(g - g_ref).max(), np.abs(g_ref).max())
    assert np.isclose(num, num_ref, rtol=1e-11)
    assert np.allclose(g, g_ref, rtol=1e-8, atol=1e-10 * np.abs(g_ref).max())
    gpu_ctx.train_apply()
    w1 = gpu_ctx.train_get_weights()
    assert np.allclose(w1, (w64 - 0.05 * g_ref).astype(np.float32), rtol=1e-6, atol=1e-7)


# ---- 5. the fp32 Dense route -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cost", cc.NEW_COSTS, ids=cc.cost_id)
@pytest.mark.parametrize("dims,acts,b,bmax", [([7, 33, 18, 3], [2, 1, 3], 130, 100), ([12, 40, 24, 9], [1, 1, 0], 256, 256)])
def test_f32_dense_step(gpu_ctx, si, cost, dims, acts, b, bmax):
    """Float32 data: the fp32 pass with the cost's arithmetic in fp64, against the fp64 definition at the bounds of
    tests/test_gpu_train_f32.py: test_f32_gradient_on_other_shapes (one Descent step at eta = 1 IS the gradient, rounded twice)"""
    kind, param = cost
    table, n, w0, x, y, rng = _dense_problem(dims, acts, b, kind, sum(dims) + b + kind, dtype=np.float32)
    for ids in (np.arange(bmax), rng.permutation(b)[: max(1, bmax // 3)]):
        gpu_ctx.train_setup(table, n, w0, x, y, bmax, 0, 1.0)
        assert gpu_ctx.train_compute_dtype() == si._capi.SI_F32
        gpu_ctx.train_set_cost(kind, param)
        loss = gpu_ctx.train_step(ids)
        g_dev = w0.astype(np.float64) - gpu_ctx.train_get_weights().astype(np.float64)
        num, g64 = cc.reference(table, w0.astype(np.float64), x[:, ids].astype(np.float64), y[:, ids].astype(np.float64), kind, param)
        l64 = num / costs.denominator(kind, dims[-1], ids.size)
        scale = np.abs(g64).max()
        err, bound = np.abs(g_dev - g64).max(), 3e-6 * scale + 1.2e-7 * np.abs(w0).max()
        print(costs.NAMES[kind], dims, ids.size, "loss", loss, l64, "err", err, "bound", bound)
        assert np.isclose(loss, l64, rtol=2e-6), (loss, l64)
        assert err <= bound, (err, bound)


# ---- 5b. the second lap of cost_logitce_kernel ----------------------------------------------------------------------------------
@pytest.mark.parametrize("out,nb", cc.LOGITCE_LAP_SHAPES)
def test_f64_logitcrossentropy_beyond_one_lap(gpu_ctx, out, nb):
    """more column groups than the kernel's 1024 waves (cc.LOGITCE_LAP_SHAPES): `grp += nwaves` takes a ragged second lap in
    cost_logitce_kernel<double, double>; the bounds of test_f64_dense_gradient"""
    assert cc.logitce_geometry(out, nb)[1] > 4 * cc.COST_MAX_BLOCKS
    cost = (costs.LOGITCE, 0.0)
    btot = nb + 40
    table, n, w0, x, y, rng = _dense_problem(cc.head_dims(out), [cc.T, cc.I], btot, costs.LOGITCE, 7000 + out)
    gpu_ctx.train_setup(table, n, w0, x, y, nb, 0, 0.1)
    gpu_ctx.train_set_cost(*cost)
    _check_against_definition(gpu_ctx, table, w0, x, y, rng.permutation(btot)[:nb], cost, "logitce lap out %d nb %d" % (out, nb))


@pytest.mark.parametrize("out,nb", cc.LOGITCE_LAP_SHAPES)
def test_f32_logitcrossentropy_beyond_one_lap(gpu_ctx, si, out, nb):
    """the same shapes on the Float32 route, cost_logitce_kernel<float, float>; the bounds of test_f32_dense_step"""
    assert cc.logitce_geometry(out, nb)[1] > 4 * cc.COST_MAX_BLOCKS
    kind = costs.LOGITCE
    dims = cc.head_dims(out)
    btot = nb + 40
    table, n, w0, x, y, rng = _dense_problem(dims, [cc.T, cc.I], btot, kind, 7100 + out, dtype=np.float32)
    ids = rng.permutation(btot)[:nb]
    gpu_ctx.train_setup(table, n, w0, x, y, nb, 0, 1.0)
    assert gpu_ctx.train_compute_dtype() == si._capi.SI_F32
    gpu_ctx.train_set_cost(kind, 0.0)
    loss = gpu_ctx.train_step(ids)
    g_dev = w0.astype(np.float64) - gpu_ctx.train_get_weights().astype(np.float64)
    num, g64 = cc.reference(table, w0.astype(np.float64), x[:, ids].astype(np.float64), y[:, ids].astype(np.float64), kind)
    l64 = num / costs.denominator(kind, out, nb)
    err, bound = np.abs(g_dev - g64).max(), 3e-6 * np.abs(g64).max() + 1.2e-7 * np.abs(w0).max()
    print("logitce lap f32", dims, nb, "loss", loss, l64, "err", err, "bound", bound)
    assert np.isclose(loss, l64, rtol=2e-6), (loss, l64)
    assert err <= bound, (err, bound)


# ---- 6. determinism and the data-parallel scaling ----------------------------------------------------------------------------
@pytest.mark.parametrize("out", [3, 10])
@pytest.mark.parametrize("cost", cc.NEW_COSTS, ids=cc.cost_id)
def test_same_bits_and_shares_of_a_batch(gpu_ctx, cost, out):
    kind, param = cost
    nb = 64
    table, n, w0, x, y, rng = _dense_problem([4, 6, out], [cc.T, cc.I], 80, kind, 600 + kind + out)
    ids = rng.permutation(80)[:nb]

    def fresh():
        gpu_ctx.train_setup(table, n, w0, x, y, nb, 2, 0.01, 0.9, 0.999)
        gpu_ctx.train_set_cost(kind, param)

    fresh()
    num = gpu_ctx.train_grad(ids, nb)
    g = gpu_ctx.train_grad_get()
    num2 = gpu_ctx.train_grad(ids, nb)
    assert num2 == num and np.array_equal(gpu_ctx.train_grad_get(), g)          # fixed-order sums: same bits
    # two shares of the batch, each scaled by the WHOLE batch's denominator, add up to the whole-batch gradient
    na = gpu_ctx.train_grad(ids[:nb // 2], nb)
    ga = gpu_ctx.train_grad_get()
    nbb = gpu_ctx.train_grad(ids[nb // 2:], nb)
    gb = gpu_ctx.train_grad_get()
    print(costs.NAMES[kind], out, "shares: max rel err", np.max(np.abs(ga + gb - g) / np.maximum(np.abs(g), 1e-300)), num, na + nbb)
    assert np.isclose(na + nbb, num, rtol=1e-12)
    assert np.allclose(ga + gb, g, rtol=1e-12, atol=0.0)
    # grad + apply is the step, bit for bit
    gpu_ctx.train_grad(ids, nb)
    gpu_ctx.train_apply()
    w_ga = gpu_ctx.train_get_weights()
    fresh()
    loss = gpu_ctx.train_step(ids)
    assert np.array_equal(gpu_ctx.train_get_weights(), w_ga)
    assert loss == num / costs.denominator(kind, out, nb)


# ---- 7. state ----------------------------------------------------------------------------------------------------------------
def test_every_setup_starts_with_mse_and_mse_is_untouched(gpu_ctx):
    table, n, w0, x, y, rng = _dense_problem([5, 8, 3], [cc.T, cc.I], 48, costs.MSE, 71)
    batches = [rng.permutation(48)[:16] for _ in range(4)]

    def adam_run(detour):
        gpu_ctx.train_setup(table, n, w0, x, y, 16, 2, 0.01, 0.9, 0.999)
        assert gpu_ctx.train_cost_info() == (costs.MSE, 0.0)
        if detour:
            gpu_ctx.train_set_cost(costs.HUBER, 2.0)
            assert gpu_ctx.train_cost_info() == (costs.HUBER, 2.0)
            gpu_ctx.train_grad(batches[0], 16)
            gpu_ctx.train_grad_get()   # (a gradient of the other cost is formed and dropped: nothing is applied)
            gpu_ctx.train_setup(table, n, w0, x, y, 16, 2, 0.01, 0.9, 0.999)
            assert gpu_ctx.train_cost_info() == (costs.MSE, 0.0)   # a new set-up: mse again
            gpu_ctx.train_set_cost(costs.LOGITCE)
            gpu_ctx.train_set_cost(costs.MSE)                      # ... and set back by hand
        losses = [gpu_ctx.train_step(ids) for ids in batches]
        return losses, gpu_ctx.train_get_weights()

    l0, w_fresh = adam_run(False)
    l1, w_detour = adam_run(True)
    assert l0 == l1 and np.array_equal(w_fresh, w_detour)
    l_ref, _ = so.mse_value_and_grad(table, w0.astype(np.float64), x[:, batches[0]], y[:, batches[0]])
    assert np.isclose(l0[0], l_ref, rtol=1e-10)


def test_refusals_leave_the_context_usable(si, gpu_ctx):
    inval, state = si._capi.SI_ERR_INVALID, si._capi.SI_ERR_STATE
    table, n, w0, x, y, rng = _dense_problem([4, 6, 2], [cc.T, cc.I], 12, costs.MAE, 5)
    gpu_ctx.train_setup(table, n, w0, x, y, 12, 0, 0.1)
    for bad, param, what in [(5, 0.0, "unknown cost"), (-1, 0.0, "unknown cost"), (costs.HUBER, 0.0, "delta"),
                             (costs.HUBER, -1.0, "delta"), (costs.HUBER, float("nan"), "delta"), (costs.HUBER, float("inf"), "delta")]:
        with pytest.raises(si.SubspaceError, match=what) as e:
            gpu_ctx.train_set_cost(bad, param)
        assert e.value.code == inval
    assert gpu_ctx.train_cost_info() == (costs.MSE, 0.0)
    gpu_ctx.train_grad(np.arange(12), 12)
    with pytest.raises(si.SubspaceError, match="gradient is pending") as e:
        gpu_ctx.train_set_cost(costs.MAE)
    assert e.value.code == inval
    gpu_ctx.train_apply()
    gpu_ctx.train_set_cost(costs.MAE)
    _check_against_definition(gpu_ctx, table, gpu_ctx.train_get_weights(), x, y, np.arange(12), (costs.MAE, 0.0), "after refusals")
    # a NeuralODE set-up has its own loss
    gpu_ctx.train_setup_node([[2, 2, 0, 0, 4]], 6, np.zeros(6, np.float32), np.zeros((2, 3), order="F"), np.zeros((4, 3), order="F"),
                             np.array([0.5, 1.0]), 1, 0, 0.1, adaptive=False, dt=0.5, max_steps=100)
    with pytest.raises(si.SubspaceError, match="not available for NeuralODE training") as e:
        gpu_ctx.train_set_cost(costs.MAE)
    assert e.value.code == inval
    # without a training state
    with si.Context(0) as c2:
        with pytest.raises(si.SubspaceError) as e:
            c2.train_set_cost(costs.MAE)
        assert e.value.code == state
    gpu_ctx.train_setup(table, n, w0, x, y, 12, 0, 0.1)
    gpu_ctx.train_set_cost(costs.LOGITBCE)
    assert np.isfinite(gpu_ctx.train_step(np.arange(12)))


# ---- 8. the public interface -------------------------------------------------------------------------------------------------
def test_api_trains_a_classifier_on_the_device(si):
    """subspace_construction with flux.logitcrossentropy: the device step against the host step, matched the way
    tests/test_gpu_train_f32.py: test_api_picks_the_precision_from_the_data matches them"""
    from subspaceinference_jl_amd import flux
    rng = np.random.default_rng(2)
    x = rng.random((10, 96))
    y = np.eye(3)[:, rng.integers(0, 3, 96)]

    def run(device_training):
        r = np.random.default_rng(7)
        m = flux.Chain(flux.Dense(10, 20, flux.tanh, rng=r), flux.Dense(20, 20, flux.relu, rng=r), flux.Dense(20, 3, rng=r))
        data = flux.DataLoader(x, y, batchsize=32)
        return si.subspace_construction(m, flux.logitcrossentropy, data, flux.ADAM(0.01), T=4, c=1, M=3, verbose=False,
                                        device_training=device_training)

    w_host, p_host = run(False)
    w_dev, p_dev = run(True)
    print("api: max |w_dev - w_host|", np.abs(w_dev - w_host).max())
    assert np.allclose(w_dev, w_host, rtol=0, atol=5e-6)
    sign = np.sign(np.sum(p_dev * p_host, axis=0))
    assert np.allclose(p_dev * sign, p_host, rtol=0, atol=2e-4 * np.abs(p_host).max())


def test_api_trains_a_cnn_classifier(si):
    """a small CNN has no host gradient: it trains on the device alone (its first-step gradient is what test_conv_gradient_and_step
    checks)"""
    from subspaceinference_jl_amd import flux
    rng = np.random.default_rng(4)
    x4 = rng.random((8, 8, 1, 16))
    y = np.eye(3)[:, rng.integers(0, 3, 16)]
    r = np.random.default_rng(9)
    m = flux.Chain(flux.Conv((3, 3), 1, 4, flux.relu, rng=r), flux.MaxPool((2, 2)), flux.flatten, flux.Dense(36, 3, rng=r))
    w_before = flux.extract_params(flux.params(m)).copy()
    data = flux.DataLoader(x4, y, batchsize=8)
    w_swa, p = si.subspace_construction(m, flux.logitcrossentropy, data, flux.ADAM(0.01), T=3, c=1, M=2, verbose=False)
    assert np.all(np.isfinite(w_swa)) and np.all(np.isfinite(p)) and p.shape == (w_before.size, 2)
    assert not np.array_equal(flux.extract_params(flux.params(m)), w_before)
