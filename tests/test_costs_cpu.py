"""costs.py (the definition of the training step's costs) and their flux objects, on the CPU."""
import numpy as np
import pytest

from oracle import subspace_oracle as so
from subspaceinference_jl_amd import costs, flux
from tests import cost_cases as cc


@pytest.mark.parametrize("cost", cc.ALL_COSTS, ids=cc.cost_id)
def test_dvalue_is_the_derivative_of_value(cost):
    """central differences of costs.value in fp64: h = 1e-6 leaves a truncation + rounding error of about 1e-10 on values of
    order 1 / d; the data keep every residual 1e-3 away from the kinks (r = 0, |r| = delta)"""
    kind, param = cost
    rng = np.random.default_rng(10 + kind)
    out, nb = 5, 7
    y = cc.targets(kind, out, nb, rng)
    yhat = rng.standard_normal((out, nb))
    if kind in (costs.MAE, costs.HUBER):
        r = yhat - y
        near = (np.abs(r) < 1e-3) | (np.abs(np.abs(r) - 1.0) < 1e-3)
        yhat = yhat + 0.01 * near
    g = costs.dvalue(kind, yhat, y, param)
    h = 1e-6
    fd = np.zeros_like(yhat)
    for i in range(out):
        for b in range(nb):
            e = np.zeros_like(yhat)
            e[i, b] = h
            fd[i, b] = (costs.value(kind, yhat + e, y, param) - costs.value(kind, yhat - e, y, param)) / (2 * h)
    assert np.allclose(g, fd, rtol=1e-6, atol=1e-9)
    # a share of a larger batch: the derivative scales with the denominator handed in
    assert np.allclose(costs.dvalue(kind, yhat, y, param, denom=2 * costs.denominator(kind, out, nb)), 0.5 * g, rtol=1e-15)


def test_the_lap_shapes_pass_the_grid_of_the_logitcrossentropy_kernel():
    """arithmetic on cost_logitce_kernel's launch: min(ceil(groups / 4), SI_COST_MAX_BLOCKS) workgroups of four waves, so more than
    4 SI_COST_MAX_BLOCKS column groups send some waves on a second lap -- which cc.BATCHES never does"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    raw = open(os.path.join(root, "subspaceinference.jl_amd", "csrc", "si_internal.h")).read()
    assert int(re.search(r"constexpr\s+int\s+SI_COST_MAX_BLOCKS\s*=\s*(\d+)\s*;", raw).group(1)) == cc.COST_MAX_BLOCKS
    waves = 4 * cc.COST_MAX_BLOCKS
    assert max(cc.logitce_geometry(out, max(cc.BATCHES))[1] for out in cc.HEADS) <= waves
    assert [cc.logitce_geometry(o, nb) for o, nb in cc.LOGITCE_LAP_SHAPES] == [(64, 1100), (16, 1026)]
    assert all(waves < cc.logitce_geometry(o, nb)[1] < 2 * waves for o, nb in cc.LOGITCE_LAP_SHAPES)
    assert 4103 % 4 == 3                                        # the last group of (10, 4103) holds three columns


def test_denominator():
    assert costs.denominator(costs.LOGITCE, 10, 32) == 32.0
    for kind in (costs.MSE, costs.MAE, costs.HUBER, costs.LOGITBCE):
        assert costs.denominator(kind, 10, 32) == 320.0


@pytest.mark.parametrize("kind", [costs.LOGITCE, costs.LOGITBCE])
def test_logit_costs_are_stable_and_equal_the_naive_formulas(kind):
    rng = np.random.default_rng(3)
    out, nb = 6, 9
    y = cc.targets(kind, out, nb, rng)
    yhat = 3.0 * rng.standard_normal((out, nb))
    assert np.isclose(costs.value(kind, yhat, y), cc.naive_value(kind, yhat, y), rtol=1e-13)
    big = yhat.copy()
    big[0, :] = 800.0
    big[1, ::2] = -800.0
    v, g = costs.value(kind, big, y), costs.dvalue(kind, big, y)
    assert np.isfinite(v) and np.all(np.isfinite(g))
    if kind == costs.LOGITBCE:   # sigmoid(800) = 1, sigmoid(-800) = 0 to the last bit
        inv = 1.0 / (out * nb)
        assert np.array_equal(g[0], (1.0 - y[0]) * inv) and np.array_equal(g[1, ::2], (0.0 - y[1, ::2]) * inv)
    else:                        # the softmax is 1 on row 0
        assert np.allclose(g[0], (np.sum(y, axis=0) - y[0]) / nb, rtol=1e-15)


def test_logitcrossentropy_of_one_class_is_zero():
    y = np.array([[1.0, 0.3, 0.0]])
    yhat = np.array([[2.5, -800.0, 800.0]])
    assert costs.value(costs.LOGITCE, yhat, y) == 0.0
    assert np.array_equal(costs.dvalue(costs.LOGITCE, yhat, y), np.zeros((1, 3)))


def test_mae_and_huber_at_their_kinks():
    y = np.zeros((1, 4))
    yhat = np.array([[0.0, 1.0, -1.0, 0.5]])
    assert np.array_equal(costs.dvalue(costs.MAE, yhat, y), np.array([[0.0, 1.0, -1.0, 1.0]]) / 4)
    # |r| = delta takes the linear branch, delta (|r| - delta / 2) and delta sign(r) (the comparison is strict); one ulp below it
    # is quadratic, r^2 / 2 and r.  Huber's function is C1, so the two branches differ only in rounding there.
    d = 0.3
    below = np.nextafter(d, 0.0)
    yh = np.array([[d, -d, below, 3.0]])
    assert costs.numerator(costs.HUBER, yh[:, :1], y[:, :1], d) == d * (d - 0.5 * d)
    assert costs.numerator(costs.HUBER, yh[:, 2:3], y[:, 2:3], d) == 0.5 * below * below
    assert np.array_equal(costs.dvalue(costs.HUBER, yh, y, d), np.array([[d * 1.0, d * -1.0, below, d * 1.0]]) * (1.0 / 4))
    assert costs.numerator(costs.HUBER, np.array([[1.0]]), np.zeros((1, 1)), 1.0) == 0.5


@pytest.mark.parametrize("cost", cc.NEW_COSTS, ids=cc.cost_id)
@pytest.mark.parametrize("dims,acts", [([5, 7, 3], [cc.T, cc.I]), ([4, 6, 5, 2], [cc.R, cc.S, cc.T])])
def test_flux_value_and_grad_is_dvalue_through_the_oracle(cost, dims, acts):
    kind, param = cost
    rng = np.random.default_rng(sum(dims) + kind)
    layers = [flux.Dense(dims[i], dims[i + 1], acts[i], rng=rng) for i in range(len(acts))]
    for l in layers:
        l.b[...] = (0.1 * rng.standard_normal(l.b.shape)).astype(np.float32)
    model = flux.Chain(*layers)
    nb = 11
    x, y = rng.standard_normal((dims[0], nb)), cc.targets(kind, dims[-1], nb, rng)
    obj = {costs.MAE: flux.mae, costs.HUBER: flux.huber_loss, costs.LOGITCE: flux.logitcrossentropy,
           costs.LOGITBCE: flux.logitbinarycrossentropy}[kind]
    loss, gs = obj.value_and_grad(model, x, y)
    g = np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1, order="F") for a in gs])
    table, n = flux.layer_table(model)
    w64 = flux.extract_params(flux.params(model)).astype(np.float64)
    num, g_ref = cc.reference(table, w64, x, y, kind, param)
    assert np.isclose(loss, num / costs.denominator(kind, dims[-1], nb), rtol=1e-13)
    assert np.isclose(obj(model, x, y), loss, rtol=1e-13)
    assert np.allclose(g, g_ref, rtol=1e-11, atol=1e-13 * np.abs(g_ref).max())


def test_huber_takes_its_delta():
    h = flux.Huber(delta=2.0)
    assert flux.device_cost(h) == (costs.HUBER, 2.0)
    m = flux.Chain(flux.Dense(2, 1, rng=np.random.default_rng(0)))
    x, y = np.array([[1.0], [2.0]]), np.array([[30.0]])
    r = float(m(x)[0, 0] - 30.0)
    assert np.isclose(h(m, x, y), 2.0 * (abs(r) - 1.0), rtol=1e-14)
    with pytest.raises(flux.SubspaceError):
        flux.Huber(delta=0.0)


def test_flux_mse_is_still_the_oracle_s():
    rng = np.random.default_rng(5)
    model = flux.Chain(flux.Dense(6, 9, flux.tanh, rng=rng), flux.Dense(9, 2, rng=rng))
    x, y = rng.standard_normal((6, 13)), rng.standard_normal((2, 13))
    loss, gs = flux.mse.value_and_grad(model, x, y)
    table, _ = flux.layer_table(model)
    l_ref, g_ref = so.mse_value_and_grad(table, flux.extract_params(flux.params(model)).astype(np.float64), x, y)
    g = np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1, order="F") for a in gs])
    assert loss == l_ref and np.allclose(g, g_ref, rtol=1e-12, atol=1e-15)
    assert np.isclose(loss, costs.value(costs.MSE, model(x), y), rtol=1e-14)


def test_device_cost_maps_and_declines():
    assert flux.device_cost(flux.mse) == (costs.MSE, 0.0)
    assert flux.device_cost(flux.mae) == (costs.MAE, 0.0)
    assert flux.device_cost(flux.huber_loss) == (costs.HUBER, 1.0)
    assert flux.device_cost(flux.logitcrossentropy) == (costs.LOGITCE, 0.0)
    assert flux.device_cost(flux.logitbinarycrossentropy) == (costs.LOGITBCE, 0.0)
    assert flux.device_cost(flux.node_sse) is None
    assert flux.device_cost(lambda m, x, y: 0.0) is None

    class Mine:
        def value_and_grad(self, model, x, y):
            return 0.0, []
    assert flux.device_cost(Mine()) is None


def test_conv_chains_have_no_host_gradient():
    rng = np.random.default_rng(0)
    m = flux.Chain(flux.Conv((3, 3), 1, 2, flux.relu, rng=rng), flux.flatten, flux.Dense(72, 3, rng=rng))
    x, y = rng.random((8, 8, 1, 4)), np.eye(3)[:, [0, 1, 2, 0]]
    with pytest.raises(flux.SubspaceError, match="no AD on the Python host") as e:
        flux.logitcrossentropy.value_and_grad(m, x, y)
    with pytest.raises(flux.SubspaceError) as e0:
        flux.mse.value_and_grad(m, x, y)
    assert str(e.value) == str(e0.value)
    assert np.isfinite(flux.logitcrossentropy(m, x, y))
