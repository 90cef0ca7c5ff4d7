"""The definition of the autoencoder training step (subspaceinference_jl_amd/autoencoder.py: train_value_and_grad, train_step) on
the host: against central differences, against flux.gradient / flux.update, on the integer lattice recomputed in integers, the
summation-order spread behind SPREAD_TOL, a mutant catalogue that shows which case catches which mistake, and the API's host
route."""
import io
import contextlib

import numpy as np
import pytest

from subspaceinference_jl_amd import api, flux
from subspaceinference_jl_amd import autoencoder as ae
from subspaceinference_jl_amd._capi import SubspaceError
from tests import ae_train_cases as ac

U = 2.0 ** -53
ORDERS = ("ascending", "pairwise", "blocked")


def _chain(table, w):
    """a flux.Chain on copies of the flat parameters (Float64 arrays: flux.gradient then runs in fp64)"""
    layers = []
    for fin, fout, act, w_off, b_off in table:
        d = flux.Dense(fin, fout, act, rng=np.random.default_rng(0), dtype=w.dtype)
        d.W[...] = w[w_off:w_off + fin * fout].reshape((fout, fin), order="F")
        d.b[...] = w[b_off:b_off + fout]
        layers.append(d)
    return flux.Chain(*layers)


def test_the_definition_and_the_kernels_share_their_constants():
    assert (ae.AE_ROWS, ae.AE_GRID) == (ac.AE_ROWS, ac.AE_GRID) and ac.AE_ROWS % 64 == 0


@pytest.mark.parametrize("penalty", [False, True])
def test_gradient_against_central_differences(penalty):
    case = ac.RealCase("fd", flux.tanh, penalty, "adam", np.float64)
    table, w, x, batches = ac.real_problem(case)
    xb = x[:, batches[0]]
    loss, g = ae.train_value_and_grad(table, w, xb, penalty)
    rng = np.random.default_rng(1)
    for i in np.concatenate([rng.integers(0, w.size, 12), [t[4] for t in table], [t[3] for t in table]]):
        h = 1e-6
        wp, wm = w.copy(), w.copy()
        wp[i] += h
        wm[i] -= h
        fd = (ae.train_value_and_grad(table, wp, xb, penalty)[0] - ae.train_value_and_grad(table, wm, xb, penalty)[0]) / (2 * h)
        assert abs(fd - g[i]) <= 1e-7 * max(1.0, abs(g[i])) + 1e-9, (i, fd, g[i])


def _abs_gradient(table, w, xb):
    """the gradient's sums with every term replaced by its absolute value, unscaled: what a dot-product bound multiplies"""
    lay, outs = ae._train_forward(table, w, xb, "ascending")
    dt = np.abs(outs[-1] - outs[0]) * np.abs(ae.dact_from_output(outs[-1], lay[-1][2]))
    g = np.zeros(np.asarray(w).size)
    for l in range(len(lay) - 1, -1, -1):
        fin, fout, act, w_off, b_off = table[l]
        g[w_off:w_off + fin * fout] = (dt @ np.abs(outs[l]).T).reshape(-1, order="F")
        g[b_off:b_off + fout] = dt.sum(axis=1)
        if l > 0:
            dt = (np.abs(lay[l][0]).T @ dt) * np.abs(ae.dact_from_output(outs[l], lay[l - 1][2]))
    return g


@pytest.mark.parametrize("case", ac.REAL[:16:2], ids=lambda c: c.name)
def test_gradient_against_flux_within_the_dot_product_bound(case):
    """|g - g_flux| <= (L + 2) gamma_k s |G|, gamma_k = k u / (1 - k u) with k = N + the hidden widths + nb (the longest chain of
    additions behind an element) and |G| the gradient's sums over absolute terms: both gradients are the same sums of the same
    products, scaled before (flux) or after (here), so each differs from the exact one by at most that"""
    table, w, x, batches = ac.real_problem(case, np.float64)
    xb = x[:, batches[0]]
    loss, g = ae.train_value_and_grad(table, w, xb)
    loss_f, gs = flux.gradient(flux.mse, _chain(table, w), xb, xb)
    k = ac.REAL_N + sum(ac.REAL_ENC) + sum(ac.REAL_DEC) + xb.shape[1]
    gamma = k * U / (1 - k * U)
    s = 2.0 / xb.size
    bound = 2 * (len(table) + 2) * gamma * s * _abs_gradient(table, w, xb)
    assert np.all(np.abs(g - flux.extract_params(gs)) <= bound)
    assert abs(loss - loss_f) <= gamma * abs(loss_f)
    assert abs(ae.train_loss(table, w, xb) - loss_f) <= gamma * abs(loss_f)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", sorted(ac.OPTIMISERS))
def test_step_against_flux_update(name, dtype):
    """Descent and Momentum: the bits of flux.update.  ADAM: optimiser_update.h forms (1 - b2) * (g * g), flux.py ((1 - b2) * g) * g
    -- one rounding apart in v (one ulp of its element type), so the step (at most about eta) differs by that fraction of eta and w
    by two ulps of its own on top"""
    case = ac.RealCase("upd", flux.tanh, False, name, dtype)
    table, w, x, batches = ac.real_problem(case)
    opt = ac.OPTIMISERS[name]
    fopt = {"descent": flux.Descent(opt[1]), "momentum": flux.Momentum(opt[1], opt[2]), "adam": flux.ADAM(opt[1], (opt[2], opt[3]))}[name]
    model = _chain(table, w)
    m, v, bp = np.zeros_like(w), np.zeros_like(w), [opt[2], opt[3]]
    for ids in batches[:3]:
        xb = x[:, ids]
        _, g = ae.train_value_and_grad(table, w, xb)
        gs, off = [], 0
        for p in flux.params(model):
            gs.append(g[off:off + p.size].reshape(p.shape, order="F"))
            off += p.size
        flux.update(fopt, flux.params(model), gs)
        _, w, m, v, bp = ae.train_step(table, w, m, v, bp, xb, opt)
        wf = flux.extract_params(flux.params(model))
        if name == "adam":
            assert np.all(np.abs(w.astype(np.float64) - wf) <= 2 * np.spacing(np.abs(wf).astype(dtype)) + 2 * np.finfo(dtype).eps * opt[1])
            flux.load_flat(model, w)      # the next step starts from the same point
            for p, mm, vv in zip(flux.params(model), _split(m, model), _split(v, model)):
                fopt.state[id(p)][0][...] = mm
                fopt.state[id(p)][1][...] = vv
            assert fopt.state[id(flux.params(model)[0])][2] == bp
        else:
            assert np.array_equal(w, wf)


def _split(flat, model):
    out, off = [], 0
    for p in flux.params(model):
        out.append(flat[off:off + p.size].reshape(p.shape, order="F"))
        off += p.size
    return out


@pytest.mark.parametrize("case", ac.LATTICE, ids=lambda c: c.name)
def test_lattice_cases_are_exact_in_any_order(case):
    ssq, G, big = ac.lattice_integers(case)
    assert big < 2 ** 53
    nb = len(case.batch)
    for dtype in (np.float32, np.float64):
        table, w, x = ac.lattice_problem(case, dtype)
        ae.check_train_table(table, w, case.n)
        for order in ORDERS if case.n < 10 ** 5 else ("ascending", "blocked"):
            loss, g = ae.train_value_and_grad(table, w, x[:, list(case.batch)], order=order)
            assert loss == ssq / float(case.n * nb)
            assert np.array_equal(g, (2.0 / float(case.n * nb)) * G.astype(np.float64))
    assert np.any(G != 0), "a case whose gradient vanishes shows nothing"


def test_lattice_shapes_cover_the_kernels_branches():
    ns = {c.n for c in ac.LATTICE}
    assert {1, 2, 3, ac.AE_ROWS - 1, ac.AE_ROWS, ac.AE_ROWS + 1} <= ns and max(ns) > ac.AE_ROWS * ac.AE_GRID
    assert {1, 3, 4, 17} <= {c.enc[0] for c in ac.LATTICE} and {1, 3, 4, 17} <= {ac.widths(c)[-2] for c in ac.LATTICE}
    assert {1, 2, 3} <= {ac.depth(c)[0] for c in ac.LATTICE} and {1, 2, 3} <= {ac.depth(c)[1] for c in ac.LATTICE}
    assert {1, 2, 5, 8} <= {len(c.batch) for c in ac.LATTICE} and {1, 5, 7} <= {c.k for c in ac.LATTICE}


def _trajectory(case, dtype, order="ascending"):
    table, w, x, batches = ac.real_problem(case, dtype)
    opt = ac.OPTIMISERS[case.opt]
    m, v, bp = np.zeros_like(w), np.zeros_like(w), [opt[2], opt[3]]
    for ids in batches:
        yield table, w, m, v, bp, x[:, ids], opt
        _, w, m, v, bp = ae.train_step(table, w, m, v, bp, x[:, ids], opt, case.penalty, order)


def test_spread_tol_is_the_measured_spread():
    worst = 0.0
    for case in ac.REAL:
        for table, w, m, v, bp, xb, opt in _trajectory(case, np.float64):
            res = [ae.train_step(table, w, m, v, bp, xb, opt, case.penalty, o) for o in ORDERS]
            worst = max([worst] + [ac.rel_gap(res[0][k], r[k]) for r in res[1:] for k in range(4)])
    assert worst <= ac.SPREAD_TOL <= 1.1 * worst, worst


@pytest.mark.parametrize("case", [c for c in ac.REAL if c.act in (flux.relu, flux.leakyrelu)], ids=lambda c: c.name)
def test_no_pre_activation_near_a_kink(case):
    for table, w, m, v, bp, xb, opt in _trajectory(case, case.dtype):
        a = xb
        for W, b, act in ae._layers(table, w):
            u = W @ a + b[:, None]
            if act in (flux.relu, flux.leakyrelu):
                assert np.min(np.abs(u)) > 1e-6
            a = flux._act_fwd(u, act)


# ---- the mutant catalogue: a plain restatement of the step with one mistake switched on; each changes a named case ----------------
def _step(table, w, m, v, bp, xb, opt, penalty, mutant=None, batch_max=8):
    lay = list(ae._layers(table, w))
    rows = slice(0, ac.AE_ROWS) if mutant == "first-block-only" else slice(None)
    cols = slice(0, xb.shape[1] - 1) if mutant == "last-column-dropped" else slice(None)
    outs = [xb]
    for l, (W, b, act) in enumerate(lay):
        u = (W[:, rows] @ outs[-1][rows] if l == 0 else W @ outs[-1]) + b[:, None]
        outs.append(flux._act_fwd(u, act))
    r = outs[-1] - xb
    n, nb = xb.shape
    s = 2.0 / (n * (batch_max if mutant == "scale-batch-max" else nb))
    g = np.zeros(w.size)
    dt = r * ae.dact_from_output(outs[-1], lay[-1][2])
    w_new = None
    for l in range(len(lay) - 1, -1, -1):
        fin, fout, act, w_off, b_off = table[l]
        g[w_off:w_off + fin * fout] = (s * (dt[:, cols] @ outs[l][:, cols].T)).reshape(-1, order="F")
        g[b_off:b_off + fout] = 0.0 if mutant == "no-bias-gradient" else s * dt[:, cols].sum(axis=1)
        if penalty:
            g[w_off:w_off + fin * fout] += 2.0 * w[w_off:w_off + fin * fout]
            if mutant != "penalty-weights-only":
                g[b_off:b_off + fout] += 2.0 * w[b_off:b_off + fout]
        if l > 0:
            W = lay[l][0]
            if l == len(lay) - 1 and mutant == "post-update-pull-back":
                gl = np.zeros(w.size)
                gl[w_off:] = g[w_off:]
                w_new = ae.optimiser_update(w, m, v, gl, opt, bp)[0]
                W = w_new[w_off:w_off + fin * fout].astype(np.float64).reshape((fout, fin), order="F")
            dt = (W[rows].T @ dt[rows] if l == len(lay) - 1 else W.T @ dt) * ae.dact_from_output(outs[l], lay[l - 1][2])
    if mutant == "m-v-swapped":
        w2, v2, m2 = ae.optimiser_update(w, v, m, g, opt, bp)
    else:
        w2, m2, v2 = ae.optimiser_update(w, m, v, g, opt, bp)
    bp2 = list(bp) if mutant == "beta-powers-stuck" or opt[0] != 2 else [bp[0] * opt[2], bp[1] * opt[3]]
    return w2, m2, v2, bp2


MUTANTS = {   # mutant -> (the real-valued case that catches it, steps it takes)
    "post-update-pull-back": ("tanh", 1), "first-block-only": ("sigmoid", 1), "last-column-dropped": ("elu", 1),
    "no-bias-gradient": ("softplus", 1), "scale-batch-max": ("tanh-momentum", 1), "m-v-swapped": ("selu", 2),
    "beta-powers-stuck": ("identity", 2), "penalty-weights-only": ("relu-penalty", 1),
}


@pytest.mark.parametrize("mutant", [None] + sorted(MUTANTS))
def test_mutants_change_a_named_case(mutant):
    name, steps = MUTANTS.get(mutant, ("tanh-penalty", 2))
    case = next(c for c in ac.REAL if c.name == name)
    table, w, x, batches = ac.real_problem(case, np.float64)
    opt = ac.OPTIMISERS[case.opt]
    m, v, bp = np.zeros_like(w), np.zeros_like(w), [opt[2], opt[3]]
    wm, mm, vm, bpm = w, m, v, bp
    for ids in batches[:steps]:
        _, w, m, v, bp = ae.train_step(table, w, m, v, bp, x[:, ids], opt, case.penalty)
        wm, mm, vm, bpm = _step(table, wm, mm, vm, bpm, x[:, ids], opt, case.penalty, mutant)
    gap = max(ac.rel_gap(w, wm), ac.rel_gap(m, mm) if opt[0] else 0.0, ac.rel_gap(v, vm) if opt[0] == 2 else 0.0,
              abs(bp[0] - bpm[0]) / bp[0] if opt[0] == 2 else 0.0)
    if mutant is None:
        assert gap <= 1e-12      # the restatement itself is the definition up to rounding
    else:
        assert gap > 1e3 * 8 * ac.SPREAD_TOL, (mutant, gap)      # far outside what the GPU audit allows


# ---- the API ------------------------------------------------------------------------------------------------------------------------
class _HostCtx:
    """a stand-in for the device context: the SWA recursion of the reference in NumPy, enough for the host route"""

    def construct_begin(self, n, k, max_cols):
        self.swa, self.cols = np.zeros(n), []

    def construct_push(self, w, n):
        w = np.asarray(w, dtype=np.float64)
        self.swa = (n * self.swa + w) / (n + 1)
        self.cols.append(w - self.swa)

    def construct_get_A(self, k0, nk):
        return np.asfortranarray(np.stack(self.cols[k0:k0 + nk], axis=1))

    def construct_finish(self, m, want_swa=True, want_p=True):
        return self.swa.copy(), None

    def __getattr__(self, name):
        raise AssertionError("the host route must not call " + name)


def _toy(seed=0):
    rng = np.random.default_rng(seed)
    model = flux.Chain(flux.Dense(2, 3, flux.tanh, rng=rng), flux.Dense(3, 1, rng=rng))
    n = sum(p.size for p in flux.params(model))
    enc = flux.Chain(flux.Dense(n, 4, flux.tanh, rng=rng), flux.Dense(4, 2, rng=rng))
    dec = flux.Chain(flux.Dense(2, 4, flux.tanh, rng=rng), flux.Dense(4, n, rng=rng))
    x, y = rng.standard_normal((2, 12)), rng.standard_normal((1, 12))
    return model, enc, dec, flux.DataLoader(x, y, batchsize=4, rng=np.random.default_rng(seed))


def test_api_argument_errors():
    model, enc, dec, data = _toy()
    for bad in ("yes", 2, None):
        with pytest.raises(SubspaceError, match="device_autoencoder"):
            api.auto_encoder_subspace(model, flux.mse, data, flux.Descent(0.1), enc, dec, T=2, ctx=_HostCtx(), device_autoencoder=bad)
    table, n = ac.table_of(ac.LATTICE[3])
    with pytest.raises(SubspaceError):
        ae.check_train_table(table[:1], np.zeros(n), ac.LATTICE[3].n)
    with pytest.raises(SubspaceError, match="256"):
        ae.check_train_table(*(lambda t: (t[0], np.zeros(t[1])))(ac.table_of(ac.Case("wide", 4, (257,), (), (0, 0), 1, (0,)))))
    with pytest.raises(SubspaceError):
        ae._nsum(np.zeros(3), "random")


@pytest.mark.parametrize("penalty", [False, True])
def test_the_host_route_is_the_parents_loop_bit_for_bit(penalty):
    """device_autoencoder=False (the default): the arrays the loop of the parent commit leaves, restated here line by line"""
    model, enc, dec, data = _toy(3)
    ctx = _HostCtx()
    with contextlib.redirect_stdout(io.StringIO()):
        w_swa, out = api.auto_encoder_subspace(model, flux.mse, data, flux.Descent(0.1), enc, dec, T=3, ctx=ctx, verbose=True,
                                               device_training=False, seed=5, include_penalty=penalty)
    assert out is dec
    model2, enc2, dec2, _ = _toy(3)
    a = ctx.construct_get_A(0, len(ctx.cols))
    sae = flux.Chain(*enc2.layers, *dec2.layers)
    autops, aopt = flux.params(sae), flux.ADAM()
    for (xb,) in flux.DataLoader(a, batchsize=5, shuffle=True, rng=np.random.default_rng(5)):
        _, gs = flux.gradient(flux.mse, sae, xb, xb)
        if penalty:
            gs = [g + 2.0 * p.astype(np.float64) for g, p in zip(gs, autops)]
        flux.update(aopt, autops, gs)
    for p, q in zip(flux.params(enc) + flux.params(dec), autops):
        assert np.array_equal(p, q) and p.dtype == q.dtype
    assert np.array_equal(w_swa, ctx.swa)


def test_the_definitions_chain_gives_the_host_routes_arrays_on_the_readme_toy():
    """What the GPU test of the API rests on: on the README toy (T = 3: 300 columns, 60 ADAM steps, Float32 parameters) the
    definition's chain of train_step, in each of the three summation orders, ends within the audit tolerance of ONE step of the
    host route's arrays (8 SPREAD_TOL of the largest entry and one Float32 ulp) -- measured: the same bits"""
    def toy(rng):
        x, y = rng.random((10, 100)), rng.random((2, 100))
        model = flux.Chain(flux.Dense(10, 20, rng=rng), flux.Dense(20, 20, rng=rng), flux.Dense(20, 2, rng=rng))
        enc = flux.Chain(flux.Dense(682, 8, rng=rng), flux.Dense(8, 3, rng=rng))
        dec = flux.Chain(flux.Dense(3, 8, flux.tanh, rng=rng), flux.Dense(8, 682, rng=rng))
        return model, enc, dec, flux.DataLoader(x, y, shuffle=True, rng=rng)
    model, enc, dec, data = toy(np.random.default_rng(0))
    sae = flux.Chain(*enc.layers, *dec.layers)
    table, _ = flux.layer_table(sae)
    w0 = flux.extract_params(flux.params(sae)).copy()
    ctx = _HostCtx()
    api.auto_encoder_subspace(model, flux.mse, data, flux.ADAM(0.1), enc, dec, T=3, M=3, seed=4, verbose=False, ctx=ctx, device_training=False)
    host = flux.extract_params(flux.params(sae))
    a = ctx.construct_get_A(0, len(ctx.cols))
    opt = ac.OPTIMISERS["adam"]
    for order in ORDERS:
        w, m, v, bp = w0.copy(), np.zeros_like(w0), np.zeros_like(w0), [opt[2], opt[3]]
        loader = flux.DataLoader(np.zeros((1, a.shape[1])), batchsize=5, shuffle=True, rng=np.random.default_rng(4))
        for ids in loader.index_batches():
            _, w, m, v, bp = ae.train_step(table, w, m, v, bp, a[:, ids], opt, False, order)
        assert w.dtype == np.float32
        tol = 8 * ac.SPREAD_TOL * np.max(np.abs(host)) + np.spacing(np.abs(host)).astype(np.float64)
        assert np.all(np.abs(w.astype(np.float64) - host) <= tol), order
