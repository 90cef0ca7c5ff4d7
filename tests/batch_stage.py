"""The batch stage of the device training step (train_batch in csrc/capi_train.hip), the same on every gradient route -- TEST
INFRASTRUCTURE for the routes' own files (tests/test_gpu_parity.py: Dense fp64, tests/test_gpu_train_f32.py: Dense fp32,
tests/test_gpu_conv.py: Conv; tests/test_gpu_node_train.py has the NeuralODE route's own form of it).

The batch 0, 1, .., nb - 1 is used in place.  The same columns in the same order out of the column-reversed data go through the
pinned index buffer and gather_cols_kernel into a buffer of their own; both are allocations of their own (256-byte aligned), so
every kernel behind the stage takes the same route and the step has the same bits."""
import numpy as np

ADAM = (2, 0.01, 0.9, 0.999)


def _record(ctx, table, n, w0, x, y, ids, **kw):
    """si_train_grad + si_train_apply, then one si_train_step, on a fresh set-up with batch_max = len(ids)"""
    ctx.train_setup(table, n, w0, x, y, len(ids), *ADAM, **kw)
    rec = {"sse": ctx.train_grad(ids, len(ids)), "gradient": ctx.train_grad_get()}
    ctx.train_apply()
    rec["w after grad + apply"] = ctx.train_get_weights()
    rec["loss of the next step"] = ctx.train_step(ids)
    rec["w after the step"] = ctx.train_get_weights()
    rec["m"], rec["v"], rec["beta powers"] = ctx.train_get_opt_state()
    return rec


def assert_in_place_is_the_index_path(ctx, table, n, w0, x, y, nb, **kw):
    btot = x.shape[1]
    assert nb < btot
    here = _record(ctx, table, n, w0, x, y, np.arange(nb), **kw)
    there = _record(ctx, table, n, w0, np.asfortranarray(x[:, ::-1]), np.asfortranarray(y[:, ::-1]), btot - 1 - np.arange(nb), **kw)
    for what in here:
        assert np.array_equal(here[what], there[what]), "%s: in place %r, through the index path %r" % (what, here[what], there[what])
    assert np.all(np.isfinite(here["gradient"])) and np.any(here["gradient"] != 0.0) and np.isfinite(here["loss of the next step"])
    assert not np.array_equal(here["w after the step"], np.asarray(w0, dtype=np.float32))     # (it trained)
