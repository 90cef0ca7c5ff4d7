"""NeuralODE training on the device (si_train_setup_node, si_train_node_info; csrc/kernels_node_train.hip: node_train_tail_kernel
behind the forward with record and the reverse kernel of csrc/kernels_node.hip) against its definition -- node.train_value_and_grad
for a step's loss and gradient, tests/optimiser_audit.run_oracle for its update -- over the runs of tests/node_train_cases.py:
bit equality after every step where no transcendental function is involved; an audit from the device's own state where one is
(the gradient within the bound measured on the CPU, the update from the device's own gradient bit for bit, the loss within
VALUE_TOL); the equivalences grad + apply = step, queued = with loss_out, in place = through the index path, run = re-run; the API's
device step against its host step; the tutorial's call; a failed trajectory; the refusals."""
import numpy as np
import pytest

from subspaceinference_jl_amd import flux, node
from tests import node_cases as nc
from tests import node_grad_cases as gc
from tests import node_train_cases as tc
from tests import optimiser_audit as oa

pytestmark = pytest.mark.gpu

RUNS = [(n, p, k, pen) for n, p in tc.FIXED for k in tc.KINDS for pen in tc.PENALTIES]
AUDITS = [(n, p, k, pen) for n, p in tc.AUDITED for k in tc.KINDS for pen in tc.PENALTIES]


def _id(run):
    return "%s-%s-%s-%s" % (run[0], run[1], run[2], "pen" if run[3] else "nopen")


def _setup(ctx, name, pattern, kind, penalty, u0=None, y=None, batch_max=None, **over):
    case = tc.case_of(name)
    pb = gc.problem(case)
    hp = tuple(tc.HYPER[kind]) + (0.0, 0.0)
    kw = case.setup_kwargs()
    kw.update(over)
    ctx.train_setup_node([list(r) for r in pb.table], pb.n, tc.w0_of(name), pb.u0 if u0 is None else u0, pb.y if y is None else y, pb.ts,
                         tc.batch_size(case, pattern) if batch_max is None else batch_max, oa.KIND_ID[kind], hp[0], hp[1], hp[2], penalty, **kw)
    return case, pb


def _state(ctx):
    m, v, bp = ctx.train_get_opt_state()
    return ctx.train_get_weights(), m, v, bp


def _same_state(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and tuple(a[3]) == tuple(b[3])


@pytest.mark.parametrize("run", RUNS, ids=_id)
def test_fixed_step_runs_are_bit_equal_after_every_step(si, gpu_ctx, run):
    name, pattern, kind, penalty = run
    _setup(gpu_ctx, name, pattern, kind, penalty)
    assert gpu_ctx.train_compute_dtype() == si._capi.SI_F64 and gpu_ctx.train_node_info()[2:] == (-1, -1, 0)
    for k, s in enumerate(tc.trace(name, pattern, kind, penalty)):
        loss = gpu_ctx.train_step(s["ids"], want_loss=True)
        gw = gpu_ctx.train_grad_get()
        w, m, v, bp = _state(gpu_ctx)
        assert loss == s["loss"], (k, loss, s["loss"])
        oa.same_bits(gw, s["g"], "gw after step %d" % (k + 1))
        oa.same_bits(w, s["w"], "w after step %d" % (k + 1), g=s["g"])
        if kind != "descent":
            oa.same_bits(m, s["m"], "m after step %d" % (k + 1))
        if kind == "adam":
            oa.same_bits(v, s["v"], "v after step %d" % (k + 1))
            oa.same_powers(bp, s["bp"], "beta powers after step %d" % (k + 1))
    assert gpu_ctx.train_node_info()[2:] == (-1, -1, 0)


@pytest.mark.parametrize("run", AUDITS, ids=_id)
def test_transcendental_and_adaptive_runs_audited_from_the_devices_own_state(gpu_ctx, run):
    name, pattern, kind, penalty = run
    case, pb = _setup(gpu_ctx, name, pattern, kind, penalty)
    state = None
    for k, ids in enumerate(tc.batches(name, pattern)):
        w_k = gpu_ctx.train_get_weights()
        loss = gpu_ctx.train_step(ids, want_loss=True)
        gw = gpu_ctx.train_grad_get()
        w, m, v, bp = _state(gpu_ctx)
        loss_ref, g_ref = tc.value_and_grad(case, w_k.astype(np.float64), ids, penalty)
        print("%s step %d: spread gw %.3e (bound %.3e), loss %.3e (bound %.3e)" % (_id(run), k + 1, nc.spread(g_ref, gw), tc.GRAD_TOL[name],
                                                                                  nc.spread(loss_ref, loss), nc.VALUE_TOL))
        assert nc.spread(g_ref, gw) <= tc.GRAD_TOL[name]
        assert nc.spread(loss_ref, loss) <= nc.VALUE_TOL
        # the update from the device's own gradient: the optimiser oracle's bits
        want = oa.run_oracle(kind, tc.HYPER[kind], w_k, [gw], False, state)[-1]
        oa.same_bits(w, want[0], "w after step %d" % (k + 1), g=gw)
        if kind != "descent":
            oa.same_bits(m, want[1], "m after step %d" % (k + 1))
        if kind == "adam":
            oa.same_bits(v, want[2], "v after step %d" % (k + 1))
            oa.same_powers(bp, want[3], "beta powers after step %d" % (k + 1))
        state = (want[1], want[2], want[3])


def _run(ctx, name, pattern, kind, penalty, how, **kw):
    """the run's four steps -> (the state after every step, the gradient of every step, the losses asked for)"""
    _setup(ctx, name, pattern, kind, penalty, **kw)
    states, grads, losses = [], [], []
    for ids in tc.batches(name, pattern):
        if how == "grad+apply":
            losses.append(ctx.train_grad(ids, len(ids)))
            grads.append(ctx.train_grad_get())
            ctx.train_apply()
        else:
            losses.append(ctx.train_step(ids, want_loss=how == "loss"))
            grads.append(ctx.train_grad_get())
        states.append(_state(ctx))
    return states, grads, losses


@pytest.mark.parametrize("run", [("g-w64", "three", "adam", 100.0), ("g-d8", "shuffled", "momentum", None), ("g-ad-tanh-cube", "shuffled", "adam", 100.0),
                                 ("g-w15", "one", "descent", 100.0)], ids=_id)
def test_grad_apply_and_queued_steps_are_the_step(si, gpu_ctx, run):
    base = _run(gpu_ctx, *run, "loss")
    split = _run(gpu_ctx, *run, "grad+apply")
    assert all(_same_state(a, b) for a, b in zip(base[0], split[0]))
    assert all(np.array_equal(a, b) for a, b in zip(base[1], split[1])) and base[2] == split[2]
    # queued steps (no loss, nothing read between them) against steps with loss_out: the final state
    _setup(gpu_ctx, *run)
    for ids in tc.batches(run[0], run[1]):
        assert gpu_ctx.train_step(ids, want_loss=False) is None
    assert _same_state(_state(gpu_ctx), base[0][-1]) and np.array_equal(gpu_ctx.train_grad_get(), base[1][-1])
    # a re-run on a fresh context: the same bits
    with si.Context(0) as fresh:
        again = _run(fresh, *run, "loss")
    assert all(_same_state(a, b) for a, b in zip(base[0], again[0])) and base[2] == again[2]


@pytest.mark.parametrize("run", [("g-w64", "full", "adam", 100.0), ("g-tr-deep", "three", "momentum", 100.0)], ids=_id)
def test_a_batch_in_place_is_the_batch_through_the_index_path(gpu_ctx, run):
    """batch 0, 1, .., nb - 1 is used in place; the same columns in the same order out of the reversed data go through the
    pinned index buffer and gather_cols_kernel"""
    name, pattern = run[0], run[1]
    case = tc.case_of(name)
    pb = gc.problem(case)
    nb = tc.batch_size(case, pattern)
    out = []
    for rev in (False, True):
        u0, y = (np.asfortranarray(pb.u0[:, ::-1]), np.asfortranarray(pb.y[:, ::-1])) if rev else (pb.u0, pb.y)
        _setup(gpu_ctx, *run, u0=u0, y=y)
        ids = np.arange(nb) if not rev else case.f - 1 - np.arange(nb)
        losses = [gpu_ctx.train_step(ids, want_loss=True) for _ in range(3)]
        out.append((_state(gpu_ctx), gpu_ctx.train_grad_get(), losses))
    assert _same_state(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]


def _ode(case, dtype=np.float32, **kw):
    pb = gc.problem(case)
    dims = (case.d,) + tuple(case.hidden) + (case.d,)
    layers = [flux.Dense(a, b, act, dtype=dtype) for a, b, act in zip(dims[:-1], dims[1:], case.acts)]
    model = flux.NeuralODE(flux.Chain(*(([flux.cube] if case.pre_power == 3 else []) + layers)), (case.t0, case.t_last), pb.ts,
                           reltol=case.reltol, abstol=case.abstol, adaptive=case.adaptive, dt=case.dt, max_steps=case.max_steps, **kw)
    flux.load_flat(model, tc.w0_of(case.name).astype(dtype))
    return model, pb


def test_api_device_step_against_host_step(si, gpu_ctx):
    case = tc.case_of("g-3x5-cube")
    out = []
    for dev in (True, False):
        model, pb = _ode(case, sensealg="discrete_adjoint")
        opt = flux.ADAM(0.1)
        data = flux.DataLoader(pb.u0, pb.y)
        w_swa, p = si.subspace_construction(model, flux.node_sse, data, opt, T=2, M=2, ctx=gpu_ctx, verbose=False, device_training=dev)
        arrays = flux.params(model)
        out.append((w_swa, p, [a.copy() for a in arrays], [[np.copy(x) for x in opt.state[id(a)][:2]] + [list(opt.state[id(a)][2])] for a in arrays]))
    (ws_d, p_d, ar_d, st_d), (ws_h, p_h, ar_h, st_h) = out
    assert np.array_equal(ws_d, ws_h) and np.array_equal(p_d, p_h)
    assert all(np.array_equal(a, b) for a, b in zip(ar_d, ar_h))
    for a, b in zip(st_d, st_h):       # the optimiser as store_device_state leaves it: the host step's own state
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
        assert a[0].dtype == np.float32 and a[1].dtype == np.float32
    assert not np.array_equal(ar_d[0], _ode(case)[0].chain.layers[0].W)      # (it trained)


def _tutorial(seed=3, f=6, S=4, **kw):
    """the tutorial's model and data at a small size: x.^3 -> Dense(2, 15, tanh) -> Dense(15, 2), f trajectories, S save points"""
    rng = np.random.default_rng(seed)
    ts = np.linspace(0.0, 1.5, S)

    def make(r):
        return flux.NeuralODE(flux.Chain(flux.cube, flux.Dense(2, 15, "tanh", rng=np.random.default_rng(r)), flux.Dense(15, 2, rng=np.random.default_rng(r + 1))),
                              (0.0, 1.5), ts, reltol=1e-7, abstol=1e-9, max_steps=2000, **kw)
    u0 = np.asfortranarray(rng.uniform(-1.0, 1.0, (2, f)))
    y = np.asfortranarray(make(11)(u0) + 0.05 * rng.standard_normal((2 * S, f)))
    return (lambda: make(21)), flux.DataLoader(u0, y)


def test_the_tutorial_call(si, gpu_ctx):
    make, data = _tutorial(sensealg="discrete_adjoint")
    n = 2 * 15 + 15 + 15 * 2 + 2
    chn, lp, w_swa = si.subspace_inference(make(), flux.node_sse, data, flux.ADAM(0.1), σ_z=0.1, itr=20, T=1, M=3, alg="mh", ctx=gpu_ctx, verbose=False)
    assert len(chn) == 20 and all(c.shape == (n,) for c in chn) and lp.shape == (20,) and np.all(np.isfinite(lp))
    w_only, p_only = si.subspace_construction(make(), flux.node_sse, data, flux.ADAM(0.1), T=1, M=3, ctx=gpu_ctx, verbose=False)
    assert np.array_equal(w_swa, w_only) and p_only.shape == (n, 3)
    chn, lp, w_hmc = si.subspace_inference(make(), flux.node_sse, data, flux.ADAM(0.1), σ_z=0.1, itr=20, T=1, M=3, alg="hmc", ctx=gpu_ctx, verbose=False)
    assert len(chn) == 20 and np.all(np.isfinite(lp)) and np.array_equal(w_hmc, w_only)
    chn, lp, w_dm = si.subspace_inference(make(), flux.node_sse, data, flux.ADAM(0.1), σ_z=0.1, itr=20, T=1, M=3, alg="mh", method="diffusion",
                                          ctx=gpu_ctx, verbose=False)
    assert len(chn) == 20 and np.all(np.isfinite(lp)) and np.array_equal(w_dm, w_only)
    enc = flux.Chain(flux.Dense(n, 3, rng=np.random.default_rng(1)))
    dec = flux.Chain(flux.Dense(3, n, rng=np.random.default_rng(2)))
    chn, lp = si.autoencoder_inference(make(), flux.node_sse, data, flux.ADAM(0.1), enc, dec, σ_z=0.1, itr=6, T=1, M=3, ctx=gpu_ctx, verbose=False)
    assert len(chn) == 6 and all(c.shape == (n,) for c in chn) and np.all(np.isfinite(lp))


def test_a_failed_trajectory_does_not_reach_the_weights(si, gpu_ctx):
    """max_steps such that every trajectory of the first batch finishes and one of the second runs out of steps (status 1, a
    handled numerical status): the weights stay those after step 1, the next synchronising call names step 2, and a fresh set-up works"""
    name, kind = "g-ad-tanh-cube", "adam"
    case = tc.case_of(name)
    pb = gc.problem(case)
    sol = node.solve(pb.table, tc.w0_of(name).astype(np.float64), pb.u0, pb.ts, case.opts())
    need = sol.naccept + sol.nreject
    order = np.argsort(need, kind="stable")
    b1, b2 = order[:3].astype(np.int64), order[-3:].astype(np.int64)
    limit = int(need[b1].max())
    assert need[b2].max() > limit + 1      # (a condition on the case: its trajectories take different numbers of steps)
    _setup(gpu_ctx, name, "three", kind, 100.0, max_steps=limit)
    assert np.isfinite(gpu_ctx.train_step(b1, want_loss=True))
    after1 = _state(gpu_ctx)
    o = case.opts()
    o.max_steps = limit
    st = node.solve(pb.table, after1[0].astype(np.float64), pb.u0[:, b2], pb.ts, o).status
    assert st.any() and set(st.tolist()) <= {0, 1}
    first = int(np.flatnonzero(st)[0])
    assert gpu_ctx.train_step(b2, want_loss=False) is None        # queued: the failure is not known yet
    assert gpu_ctx.train_step(b1, want_loss=False) is None        # a later step of the set-up: a no-op too
    with pytest.raises(si.SubspaceError, match=r"step 2: trajectory %d of its batch ended with status 1" % first) as e:
        gpu_ctx.synchronize()
    assert e.value.code == si._capi.SI_ERR_INVALID
    assert gpu_ctx.train_node_info()[2:] == (2, first, 1)
    assert _same_state(_state(gpu_ctx), after1)                    # w, m, v and the beta powers as step 1 left them
    gpu_ctx.synchronize()                                           # (reported once)
    with pytest.raises(si.SubspaceError, match="an earlier NeuralODE training step failed"):
        gpu_ctx.train_step(b1, want_loss=True)
    assert _same_state(_state(gpu_ctx), after1)
    # the same through get_weights as the first synchronising call
    _setup(gpu_ctx, name, "three", kind, 100.0, max_steps=limit)
    gpu_ctx.train_step(b1, want_loss=False)
    gpu_ctx.train_step(b2, want_loss=False)
    with pytest.raises(si.SubspaceError, match="step 2: trajectory %d" % first):
        gpu_ctx.train_get_weights()
    assert np.array_equal(gpu_ctx.train_get_weights(), after1[0])
    # a fresh set-up on the same context works
    _setup(gpu_ctx, name, "three", kind, 100.0)
    assert gpu_ctx.train_node_info()[2:] == (-1, -1, 0)
    assert np.isfinite(gpu_ctx.train_step(b2, want_loss=True)) and gpu_ctx.train_node_info()[2:] == (-1, -1, 0)


def test_refusals(si, gpu_ctx):
    inval = si._capi.SI_ERR_INVALID
    wide = nc.CASE_BY_NAME["ex-d2-h65-p1"]
    pw = nc.problem(wide)
    with pytest.raises(si.SubspaceError, match="wider than 64") as e:
        gpu_ctx.train_setup_node([list(r) for r in pw.table], pw.n, pw.w_swa.astype(np.float32), pw.u0, pw.y, pw.ts, 1, 0, 0.1, **wide.setup_kwargs())
    assert e.value.code == inval
    # a record over the budget: batch_max = 100, d = 8, max_steps = 10^6 is 8 GB
    with pytest.raises(si.SubspaceError, match="lower max_steps or the batch size") as e:
        gpu_ctx.train_setup_node([[8, 8, 0, 0, 64]], 72, np.zeros(72, np.float32), np.zeros((8, 100), order="F"), np.zeros((16, 100), order="F"),
                                 np.array([0.5, 1.0]), 100, 0, 0.1, adaptive=False, dt=0.5, max_steps=1000000)
    assert e.value.code == inval
    with pytest.raises(si.SubspaceError, match="si_train_setup_node: the state dimension d must be 1 to 8"):
        gpu_ctx.train_setup_node([[9, 9, 0, 0, 81]], 90, np.zeros(90, np.float32), np.zeros((9, 2), order="F"), np.zeros((9, 2), order="F"),
                                 np.array([1.0]), 1, 0, 0.1, adaptive=False, dt=0.5)
    # the data-parallel entry points on a node set-up
    _setup(gpu_ctx, "g-w15", "one", "descent", 100.0)
    for call in (lambda: gpu_ctx.train_step_dp(np.arange(1), 1), lambda: gpu_ctx.train_allreduce_grad()):
        with pytest.raises(si.SubspaceError, match="not available for NeuralODE training") as e:
            call()
        assert e.value.code == inval
    with pytest.raises(si.SubspaceError, match="nb_total must equal nb"):
        gpu_ctx.train_grad(np.arange(1), 2)
    with pytest.raises(si.SubspaceError, match="bad batch"):
        gpu_ctx.train_step(np.arange(2), want_loss=False)        # batch_max = 1
    assert np.isfinite(gpu_ctx.train_step(np.arange(1), want_loss=True))
    # device_training=True with Float64 parameters
    case = tc.case_of("g-3x5-cube")
    model64, pb = _ode(case, dtype=np.float64, sensealg="discrete_adjoint")
    with pytest.raises(si.SubspaceError, match="Float32 parameters"):
        si.subspace_construction(model64, flux.node_sse, flux.DataLoader(pb.u0, pb.y), flux.ADAM(0.1), T=1, M=1, ctx=gpu_ctx, device_training=True)
    # ... and any other cost keeps the old text
    with pytest.raises(si.SubspaceError, match="training a NeuralODE through the solver is out of scope"):
        si.subspace_construction(model64, flux.mse, flux.DataLoader(pb.u0, pb.y), flux.ADAM(0.1), ctx=gpu_ctx)
    # a Chain set-up after a node set-up trains as before
    _setup(gpu_ctx, "g-w15", "one", "descent", 100.0)
    rng = np.random.default_rng(0)
    gpu_ctx.train_setup([(3, 2, flux.identity, 0, 6)], 8, rng.standard_normal(8).astype(np.float32), rng.standard_normal((3, 4)), rng.standard_normal((2, 4)), 4, 0, 0.1)
    assert gpu_ctx.train_node_info() == (False, 0, -1, -1, 0) and np.isfinite(gpu_ctx.train_step(np.arange(4), want_loss=True))
