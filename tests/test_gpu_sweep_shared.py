"""si_logdensity_grad and the training step run ONE value-and-gradient pass: for the same chain, weights and data the two
gradients differ by the scale of Delta_L alone.

Inference is set up with W_swa = w, P = I (M = N), sigma_m = 1, no prior and no decoder, and evaluated at z = 0: K4 forms w + 0
exactly, Delta_L has scale 1, and P' g sums one non-zero per column, so the gradient returned is d lp / d w.  Training on the same
w and data with batch_max = B scales Delta_L by -2 / (out * B).  With out * B a power of two every intermediate of the two reverse
sweeps differs by that exact factor, so the gradients agree element for element under `==` -- as long as both entry points run the
same kernels in the same order on workspaces of the same shape."""
import numpy as np
import pytest

from oracle import subspace_oracle as so
from subspaceinference_jl_amd import _capi

pytestmark = pytest.mark.gpu

R, T, I, LR = so.ACT_RELU, so.ACT_TANH, so.ACT_IDENTITY, so.ACT_LEAKYRELU
B = 16
CONV = ("conv", (3, 3), 2, R)

CASES = {
    "dense_3_5_8_tanh": (so.layer_table([3, 5, 8], [T, I]), 3, _capi.SI_F64),          # out > SI_FUSE_MAX_OUT: no fused head
    "dense_3_8_1_relu_fused_head": (so.layer_table([3, 8, 1], [R, I]), 3, _capi.SI_F64),   # tail_bwd, part
    "dense_3_6_2_leakyrelu": (so.layer_table([3, 6, 2], [LR, I]), 3, _capi.SI_F64),    # narrow head, not fused (activation rule)
    "dense_3_8_1_relu_f32": (so.layer_table([3, 8, 1], [R, I]), 3, _capi.SI_F32),
    "conv_maxpool_fused_pidx": (so.conv_table([CONV, ("maxpool", (2, 2)), ("flatten",), ("dense", 2, I)], (6, 6, 1)), 36, _capi.SI_F64),
    "conv_kept_activation": (so.conv_table([CONV, ("flatten",), ("dense", 2, I)], (6, 6, 1)), 36, _capi.SI_F64),
}


@pytest.mark.parametrize("name", list(CASES))
def test_inference_and_training_gradients_differ_by_the_scale_alone(gpu_ctx, name):
    (table, n), in_dim, dtype = CASES[name]
    out = so.forward(table, np.zeros(n), np.zeros((in_dim, 1))).shape[0]
    assert (out * B) & (out * B - 1) == 0
    rng = np.random.default_rng(len(name))
    w = (0.5 * rng.standard_normal(n)).astype(np.float32)                  # Float32-representable: training holds Float32 parameters
    x = np.asfortranarray(rng.integers(-12, 13, (in_dim, B)) / 8.0)        # multiples of 1/8: the fp32 case sees the same operands
    y = np.asfortranarray(rng.integers(-12, 13, (out, B)) / 8.0)

    gpu_ctx.infer_setup(table, n, n, w.astype(np.float64), np.asfortranarray(np.eye(n)), x, y, 1.0, compute_dtype=dtype)
    _, g_inf = gpu_ctx.logdensity_grad(np.zeros(n))
    gpu_ctx.train_setup(table, n, w, x, y, B, 0, 0.1, compute_dtype=dtype)
    gpu_ctx.train_grad(np.arange(B), B)
    g_tr = gpu_ctx.train_grad_get()

    want = (-2.0 / (out * B)) * g_inf
    differ = np.flatnonzero(g_tr != want)
    print(name, "N", n, "max |g_inf|", np.abs(g_inf).max(), "min non-zero |g_tr|", np.abs(g_tr[g_tr != 0]).min(), "differing", differ,
          g_tr[differ], want[differ])
    assert np.all(np.isfinite(g_inf)) and np.abs(g_inf).max() > 0.0
    assert differ.size == 0
