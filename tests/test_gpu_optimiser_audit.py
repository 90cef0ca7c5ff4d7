"""The device optimiser, update by update and bit for bit (tests/optimiser_audit.py; its input set is certified on the host by
tests/test_optimiser_audit_cpu.py): optimiser_kernel / train_apply of csrc/capi_train.hip and the state around them (the beta
powers, m32 / v32, the g32 form, si_train_push, si_train_get_opt_state) against oracle.subspace_oracle.apply_update.

The gradient is INJECTED: si_train_grad(idx = empty, nb = 0, nb_total = 1) arms the pending gradient without a gradient kernel,
si_train_grad_set writes any fp64 words, si_train_apply runs the update, and si_train_get_weights / si_train_get_opt_state show
every bit it wrote.  The data are a dummy Dense table (identity, one observation, batch_max = 1); Float64 (X, Y) select the
Float64 form, Float32 (X, Y) the g32 form, where only Float32-representable gradients are injected (the kernel does not re-round
g, the oracle does).  Every step takes the device's own previous weights as given.

m, v and the beta powers pass fp64 multiply, add and conversions only: they are equal unconditionally.  ADAM's weight also
passes an fp64 division (IEEE on gfx950) and an fp64 square root, which nothing shows to be correctly rounded: a weight element
is accepted if it equals the oracle's with the root as NumPy computes it, or one fp64 ulp either way.  Each test prints how many
elements needed that; zero is the expectation.  On the first step of the dyadic set the root is exact by construction and no
nudge is accepted.

Printed count of bracketed elements on MI355X: NOT RECORDED YET -- no MI355X run of this file has completed; the file has only
been exercised against an oracle-backed stand-in for the context on the host.  Record the printed numbers here after the run.
"""
import os

import numpy as np
import pytest

from oracle import subspace_oracle as so
from tests import optimiser_audit as oa

pytestmark = pytest.mark.gpu

CASES = [(k, f) for k in oa.KINDS for f in (False, True)]
IDS = ["%s-%s" % (k, "g32" if f else "g64") for k, f in CASES]
# N = out (in + 1): one pass and one lane (2), one workgroup less one / exactly / plus one (255, 256, 257), the fixture's class
SMALL = [[1, 1], [16, 15], [15, 16], [256, 1], [10, 20, 20, 2]]
BIG = [1023, 1100]   # N = 1 126 400: three passes of the grid-stride loop on 256 CUs, the last one partial


def _table(dims):
    return so.layer_table(dims, [so.ACT_IDENTITY] * (len(dims) - 1))


def _setup(si, ctx, dims, w0, kind, hp, g32):
    from subspaceinference_jl_amd import _capi
    table, n = _table(dims)
    dt = np.float32 if g32 else np.float64
    x, y = np.zeros((dims[0], 1), dtype=dt, order="F"), np.zeros((dims[-1], 1), dtype=dt, order="F")
    p = tuple(hp) + (0.0,) * (3 - len(hp))
    ctx.train_setup(table, n, w0, x, y, 1, oa.KIND_ID[kind], p[0], p[1], p[2])
    assert ctx.train_compute_dtype() == (_capi.SI_F32 if g32 else _capi.SI_F64)
    return n


def _inject(ctx, g):
    ctx.train_grad(np.empty(0, dtype=np.int64), 1)    # arms the pending gradient (a zero share), no gradient kernel
    ctx.train_grad_set(g)
    ctx.train_apply()


def _eq(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _adam_brackets(w_prev, m, v, bp_prev, hp, g32):
    """ADAM's new weights from the stored (m, v) with the square root as computed, one fp64 ulp below, one above"""
    eta = np.float64(hp[0])
    root = np.sqrt(v.astype(np.float64) / (1.0 - bp_prev[1]))
    out = []
    for r in (root, np.nextafter(root, -np.inf), np.nextafter(root, np.inf)):
        step = m.astype(np.float64) / (1.0 - bp_prev[0]) / (r + so.FLUX_EPS) * eta
        out.append(w_prev - step.astype(np.float32) if g32 else (w_prev.astype(np.float64) - step).astype(np.float32))
    return out


class Follower:
    """the oracle beside one device context: after every apply, the device's (w, m, v, beta powers) against
    so.apply_update from the device's own previous weights"""

    def __init__(self, ctx, kind, hp, g32, w0, tag, exact_root_steps=0):
        self.ctx, self.kind, self.hp, self.g32, self.tag = ctx, kind, tuple(hp), g32, tag
        self.opt = oa.oracle_opt(kind, hp)
        self.w = np.array(w0, dtype=np.float32)
        self.state = so.optimiser_state(self.w.size, self.opt)
        self.t, self.nudged, self.exact_root_steps = 0, 0, exact_root_steps

    def check(self, g):
        """g: the gradient the device has just applied (fp64 words)"""
        g = np.asarray(g, dtype=np.float64)
        w_prev, bp_prev = self.w.copy(), self.state["bp"]
        if self.g32:
            assert np.array_equal(g.astype(np.float32).astype(np.float64), g, equal_nan=True), "a g32 gradient must be Float32-representable"
        with np.errstate(all="ignore"):
            so.apply_update(self.w, self.state, g.astype(np.float32) if self.g32 else g, self.opt)
        tag = "%s, step %d" % (self.tag, self.t)
        w_dev = self.ctx.train_get_weights()
        m_dev, v_dev, bp_dev = self.ctx.train_get_opt_state()
        extra = dict(g=g, w_prev=w_prev)
        oa.same_bits(m_dev, self.state["m"], tag + ", m", **extra)
        oa.same_bits(v_dev, self.state["v"], tag + ", v", **extra)
        if self.kind == "adam":
            oa.same_powers(bp_dev, self.state["bp"], tag + ", beta powers")
            with np.errstate(all="ignore"):
                mid, lo, hi = _adam_brackets(w_prev, self.state["m"], self.state["v"], bp_prev, self.hp, self.g32)
            oa.same_bits(mid, self.w, tag + ": the test's ADAM formula against the oracle's", **extra)
            central = _eq(w_dev, mid)
            if self.t >= self.exact_root_steps:
                ok = central | _eq(w_dev, lo) | _eq(w_dev, hi)
                self.nudged += int(np.count_nonzero(ok & ~central))
                if np.all(ok):
                    self.w[...] = w_dev     # the next step starts from the device's own weights
        oa.same_bits(w_dev, self.w, tag + ", w", m=self.state["m"], v=self.state["v"], **extra)
        self.t += 1
        return w_dev


def _run_injected(si, ctx, dims, kind, hpname, g32, special=False):
    hp = oa.HYPER[hpname][kind]
    n = _table(dims)[1]
    if special:
        w0, grads, _ = oa.inputs(kind, hpname, g32, n)
        ws, gs, labels = oa.special_arrays(kind, hpname, g32)
        assert len(labels) <= n
        w0[:len(labels)], grads[:, :len(labels)] = ws, gs
    else:
        w0, grads, _ = oa.inputs(kind, hpname, g32, n)
    assert _setup(si, ctx, dims, w0, kind, hp, g32) == n
    f = Follower(ctx, kind, hp, g32, w0, "%s %s %s N = %d" % (kind, hpname, "g32" if g32 else "g64", n),
                 exact_root_steps=1 if hpname == "dyadic" and not special else 0)
    for t in range(oa.STEPS):
        _inject(ctx, grads[t])
        f.check(grads[t])
    return f.nudged


@pytest.mark.parametrize("kind,g32", CASES, ids=IDS)
def test_every_injected_update_is_the_oracles(si, gpu_ctx, kind, g32):
    """three hyper-parameter sets x N = 2, 255, 256, 257, 682; six steps each, (w, m, v, beta powers) after every one"""
    nudged = 0
    for hpname in oa.HYPER:
        for dims in SMALL:
            nudged += _run_injected(si, gpu_ctx, dims, kind, hpname, g32)
    print("%s %s: %d weight elements needed the one-ulp square-root bracket" % (kind, "g32" if g32 else "g64", nudged))


@pytest.mark.parametrize("kind,g32", CASES, ids=IDS)
def test_three_passes_of_the_grid_stride_loop(si, gpu_ctx, kind, g32):
    """grid_for caps the grid at 8 num_cu workgroups of 256: N = 1 126 400 is more than two full passes of it"""
    import torch
    num_cu = torch.cuda.get_device_properties(gpu_ctx.device).multi_processor_count
    n = _table(BIG)[1]
    assert n == 1126400
    if not n > 2 * 8 * 256 * num_cu:
        pytest.skip("%d CUs: N = %d no longer reaches a third pass of the stride loop; the case needs a larger N" % (num_cu, n))
    nudged = _run_injected(si, gpu_ctx, BIG, kind, "flux", g32)
    print("%s %s, N = %d on %d CUs: %d weight elements needed the one-ulp square-root bracket" % (kind, "g32" if g32 else "g64", n, num_cu, nudged))


@pytest.mark.parametrize("kind,g32", CASES, ids=IDS)
def test_special_values(si, gpu_ctx, kind, g32):
    """+-0, +-inf, NaN, |g| = 1e200 (the Float32 stores overflow), 1e-310, Float32-subnormal m, v and w, a rounding tie: every row as
    the oracle has it, NaN for NaN.  A device that flushed Float32 subnormals would differ here (Julia does not flush)."""
    nudged = 0
    for hpname in oa.HYPER:
        nudged += _run_injected(si, gpu_ctx, [1, 16], kind, hpname, g32, special=True)
    print("%s %s, special values: %d weight elements needed the one-ulp square-root bracket" % (kind, "g32" if g32 else "g64", nudged))


TRAIN_DIMS, TRAIN_ACTS = [10, 20, 20, 2], [so.ACT_TANH, so.ACT_RELU, so.ACT_IDENTITY]
TRAIN_OPTS = {"descent": (0.1,), "momentum": (0.01, 0.9), "adam": (0.001, 0.9, 0.999)}   # tests/golden/make_golden.py


@pytest.mark.parametrize("kind,g32", CASES, ids=IDS)
def test_the_real_step_is_the_audited_update_of_its_own_gradient(si, gpu_ctx, kind, g32):
    """si_train_step == si_train_grad + si_train_apply bit for bit at every one of the fixture's 12 steps, and both are
    so.apply_update of the gradient the device itself computed: the gradient is then the only quantity of si_train_step that
    is not held to the bit (tests/test_gpu_lattice.py and the tolerance tests hold it)."""
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "toy_train_steps_f32.npz" if g32 else "toy_train_steps.npz"))
    batches = [row[row >= 0] for row in d["batches"]]
    hp = TRAIN_OPTS[kind]
    p = hp + (0.0,) * (3 - len(hp))
    table, n = so.layer_table(TRAIN_DIMS, TRAIN_ACTS)
    x, y = np.asfortranarray(d["X"]), np.asfortranarray(d["Y"])
    assert x.dtype == (np.float32 if g32 else np.float64)
    b = si.Context(0)
    try:
        for c in (gpu_ctx, b):
            c.train_setup(table, n, d["w0"], x, y, 25, oa.KIND_ID[kind], *p)
        f = Follower(b, kind, hp, g32, d["w0"], "real step, %s %s" % (kind, "g32" if g32 else "g64"))
        for ids in batches:
            gpu_ctx.train_step(ids, want_loss=False)
            b.train_grad(ids, ids.size)
            g = b.train_grad_get()
            b.train_apply()
            w_b = f.check(g)
            oa.same_bits(gpu_ctx.train_get_weights(), w_b, "si_train_step against si_train_grad + si_train_apply, step %d" % (f.t - 1), g=g)
        for got, want in zip(gpu_ctx.train_get_opt_state()[:2], b.train_get_opt_state()[:2]):
            oa.same_bits(got, want, "optimiser state of si_train_step against si_train_grad + si_train_apply")
        assert gpu_ctx.train_get_opt_state()[2] == b.train_get_opt_state()[2]
        print("real step, %s %s: %d weight elements needed the one-ulp square-root bracket" % (kind, "g32" if g32 else "g64", f.nudged))
    finally:
        b.close()


@pytest.mark.parametrize("kind", ["momentum", "adam"])
def test_a_zero_share_moves_the_weights_as_a_zero_gradient_does(si, gpu_ctx, kind):
    """si_train_grad(idx = empty, nb_total) + si_train_apply with a state that is not zero: the velocity / the moments still move
    the weights, exactly as the oracle's g = 0; on a fresh ADAM state the weights stay as they are, bit for bit"""
    dims = [16, 15]
    hp = oa.HYPER["flux"][kind]
    for g32 in (False, True):
        w0, grads, _ = oa.inputs(kind, "flux", g32, 255)
        _setup(si, gpu_ctx, dims, w0, kind, hp, g32)
        f = Follower(gpu_ctx, kind, hp, g32, w0, "zero share, %s %s" % (kind, "g32" if g32 else "g64"))
        zero = np.zeros(255)
        if kind == "adam":
            gpu_ctx.train_grad(np.empty(0, dtype=np.int64), 4)
            gpu_ctx.train_apply()
            oa.same_bits(f.check(zero), w0, "a zero gradient on the fresh ADAM state", w0=w0)
        for t in range(2):
            _inject(gpu_ctx, grads[t])
            f.check(grads[t])
        assert np.any(f.state["m"] != 0.0)
        before = f.w.copy()
        for nb_total in (1, 3):
            assert gpu_ctx.train_grad(np.empty(0, dtype=np.int64), nb_total) == 0.0
            assert not np.any(gpu_ctx.train_grad_get())
            gpu_ctx.train_apply()
            f.check(zero)
        assert np.any(f.w != before)
        print("zero share, %s %s: %d weight elements needed the one-ulp square-root bracket" % (kind, "g32" if g32 else "g64", f.nudged))


def test_state_life_cycle(si, gpu_ctx):
    """a second si_train_setup restores m = v = 0 and the beta powers to beta; 2000 applies give the running product beta beta ..
    beta (not beta ** t) bit for bit; si_train_apply without a pending gradient fails"""
    hp = oa.HYPER["flux"]["adam"]
    w0, grads, _ = oa.inputs("adam", "flux", False, 2)
    _setup(si, gpu_ctx, [1, 1], w0, "adam", hp, False)
    for t in range(3):
        _inject(gpu_ctx, grads[t])
    m, v, bp = gpu_ctx.train_get_opt_state()
    assert np.any(m != 0.0) and np.any(v != 0.0) and bp != (hp[1], hp[2])
    _setup(si, gpu_ctx, [1, 1], w0, "adam", hp, False)
    m, v, bp = gpu_ctx.train_get_opt_state()
    assert not np.any(m.view(np.uint32)) and not np.any(v.view(np.uint32)) and bp == (hp[1], hp[2])
    oa.same_bits(gpu_ctx.train_get_weights(), w0, "weights after the second set-up")
    with pytest.raises(si.SubspaceError, match="no gradient pending"):
        gpu_ctx.train_apply()
    want, differs = [hp[1], hp[2]], False
    for t in range(1, 2001):
        gpu_ctx.train_grad(np.empty(0, dtype=np.int64), 1)
        gpu_ctx.train_apply()
        want = [want[0] * hp[1], want[1] * hp[2]]
        differs = differs or want[0] != hp[1] ** (t + 1) or want[1] != hp[2] ** (t + 1)
        if t in (1, 2, 12, 500, 2000):
            oa.same_powers(gpu_ctx.train_get_opt_state()[2], want, "beta powers after %d applies" % t)
    assert differs          # (tests/test_optimiser_audit_cpu.py: the running product and pow part ways well before t = 2000)
    with pytest.raises(si.SubspaceError, match="no gradient pending"):
        gpu_ctx.train_apply()


@pytest.mark.parametrize("kind,g32", [("momentum", False), ("adam", True)], ids=["momentum-g64", "adam-g32"])
def test_train_push_averages_the_audited_weights(si, gpu_ctx, kind, g32):
    """si_construct_begin(N, 3), three si_train_push between injected steps: W_swa is the running mean of the audited Float32
    weights, by the oracle call tests/test_gpu_parity.py::test_swa_dev_push_bit_exact uses"""
    hp = oa.HYPER["flux"][kind]
    w0, grads, _ = oa.inputs(kind, "flux", g32, 255)
    gpu_ctx.construct_begin(255, 3)
    _setup(si, gpu_ctx, [16, 15], w0, kind, hp, g32)
    f = Follower(gpu_ctx, kind, hp, g32, w0, "push, %s" % kind)
    snaps, ns = [], [1.0, 1.0, 2.0]
    for t in range(oa.STEPS):
        _inject(gpu_ctx, grads[t])
        w = f.check(grads[t])
        if t in (0, 2, 5):
            gpu_ctx.train_push(ns[len(snaps)])
            snaps.append(w)
    w_ref, a_ref = so.construct_stream(snaps, ns)
    assert np.array_equal(gpu_ctx.construct_get_A(0, 3), a_ref)
    w_swa, _, _, k = gpu_ctx.construct_finish(1, want_p=False)
    assert k == 3
    oa.same_bits(w_swa, w_ref, "W_swa after three si_train_push")
    print("push, %s: %d weight elements needed the one-ulp square-root bracket" % (kind, f.nudged))


@pytest.mark.parametrize("optname", ["momentum", "adam"])
def test_the_host_optimiser_takes_over_the_devices_state(si, gpu_ctx, optname):
    """the small cases of tests/test_gpu_parity.py::test_optimiser_state_survives_device_training: after subspace_construction with
    device_training = True the host optimiser's per-array state and beta powers, flattened in extract_params order, are
    si_train_get_opt_state of the same context, bit for bit"""
    from subspaceinference_jl_amd import flux
    rng = np.random.default_rng(0)
    x, y = rng.random((6, 60)), rng.random((1, 60))
    wr = np.random.default_rng(3)
    mdl = flux.Chain(flux.Dense(6, 12, flux.tanh, rng=wr), flux.Dense(12, 1, rng=wr))
    opt = flux.Momentum(0.05, 0.9) if optname == "momentum" else flux.ADAM(0.01)
    si.subspace_construction(mdl, flux.mse, flux.DataLoader(x, y, batchsize=20), opt, T=3, c=1, M=2, ctx=gpu_ctx, verbose=False,
                             device_training=True)
    m_dev, v_dev, bp_dev = gpu_ctx.train_get_opt_state()
    ps = flux.params(mdl)
    assert np.any(m_dev != 0.0)
    oa.same_bits(flux.extract_params(ps), gpu_ctx.train_get_weights(), "the model's weights after device training")
    if optname == "momentum":
        host_m = [opt.v[id(a)] for a in ps]
    else:
        host_m, host_v = [opt.state[id(a)][0] for a in ps], [opt.state[id(a)][1] for a in ps]
        assert all(a.dtype == np.float32 and a.shape == p.shape for a, p in zip(host_v, ps))
        oa.same_bits(flux.extract_params(host_v), v_dev, "ADAM's second moment on the host")
        want = [opt.beta[0], opt.beta[1]]
        for _ in range(9):   # T = 3 epochs of 3 batches
            want = [want[0] * opt.beta[0], want[1] * opt.beta[1]]
        oa.same_powers(bp_dev, want, "the device's beta powers after 9 steps")
        for a in ps:
            oa.same_powers(opt.state[id(a)][2], bp_dev, "the host's beta powers")
    assert all(a.dtype == np.float32 and a.shape == p.shape for a, p in zip(host_m, ps))
    oa.same_bits(flux.extract_params(host_m), m_dev, "the velocity / first moment on the host")
