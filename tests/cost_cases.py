"""Shared cases of the cost tests (tests/test_costs_cpu.py, tests/test_gpu_train_costs.py): the kinds, the shapes, the data each
kind is tried on, and the reference gradient -- costs.dvalue pushed through the oracle's _layer_forward / _layer_backward on the
CPU, never the device."""
import numpy as np

from oracle import subspace_oracle as so
from subspaceinference_jl_amd import costs

I, R, T, S = so.ACT_IDENTITY, so.ACT_RELU, so.ACT_TANH, so.ACT_SIGMOID

# (kind, param)
NEW_COSTS = [(costs.MAE, 0.0), (costs.HUBER, 1.0), (costs.LOGITCE, 0.0), (costs.LOGITBCE, 0.0)]
ALL_COSTS = [(costs.MSE, 0.0)] + NEW_COSTS

# heads of the fp64 Dense route: out <= 4 the fused head, 5 and above the generic one; 10 packs four columns into a wave of the
# logitcrossentropy kernel, 64 / 65 sit on both sides of one lane per class, 130 and 1000 stride the lanes over the column
HEADS = [1, 2, 3, 4, 5, 10, 64, 65, 130, 1000]
BATCHES = [1, 3, 5, 257]
B_TOTAL = 300

# (out, nb) of logitcrossentropy beyond one lap of cost_logitce_kernel: its grid is capped at SI_COST_MAX_BLOCKS = 256 workgroups of
# four waves, a wave owns one group of 64 / seg columns at a time (seg = next_pow2(out) up to 32, 64 above) and walks on with
# grp += 1024.  (33, 1100): seg 64, 1100 groups; (10, 4103): seg 16, 1026 groups, the last of three columns -- a ragged second lap
# in both.  BATCHES ends at 257 groups.
COST_MAX_BLOCKS = 256       # SI_COST_MAX_BLOCKS of csrc/si_internal.h (tests/test_costs_cpu.py reads it there)
LOGITCE_LAP_SHAPES = [(33, 1100), (10, 4103)]


def logitce_geometry(out, nb):
    """(seg, column groups) of cost_logitce_kernel -- and of lik_logitce_kernel -- at out classes and nb columns"""
    seg = 64
    if out <= 32:
        seg = 1
        while seg < out:
            seg *= 2
    return seg, -(-nb // (64 // seg))


def cost_id(c):
    return costs.NAMES[c[0]]


def head_dims(out):
    return [4, 6, out] if out <= 130 else [4, 8, out]


def targets(kind, out, b, rng):
    """targets of the kind a Flux user hands this cost: one-hot columns for logitcrossentropy (every third column soft and not
    normalised: sum_i Y_ib is kept, not assumed 1), 0 / 1 labels for logitbinarycrossentropy (every third column soft), reals
    otherwise"""
    if kind == costs.LOGITCE:
        y = np.zeros((out, b))
        y[rng.integers(0, out, b), np.arange(b)] = 1.0
        y[:, ::3] = rng.random((out, y[:, ::3].shape[1]))
        return np.asfortranarray(y)
    if kind == costs.LOGITBCE:
        y = (rng.random((out, b)) < 0.5).astype(np.float64)
        y[:, ::3] = rng.random((out, y[:, ::3].shape[1]))
        return np.asfortranarray(y)
    return np.asfortranarray(rng.standard_normal((out, b)))


def reference(table, w64, x, y, kind, param=0.0, denom=None):
    """(numerator, flat gradient) of the cost on the batch (x, y) for the weights w64: the definition through the oracle's layers"""
    hs = [x]
    for row in table:
        hs.append(so._layer_forward(row, w64, hs[-1]))
    num = costs.numerator(kind, hs[-1], y, param)
    g = costs.dvalue(kind, hs[-1], y, param, denom)
    gw = np.zeros_like(w64)
    for l in range(len(table) - 1, -1, -1):
        g = so._layer_backward(table[l], w64, hs[l], hs[l + 1], g, gw)
    return num, gw


def naive_value(kind, yhat, y, param=0.0):
    """the formulas as a textbook writes them (no stabilisation): what the stable forms must equal at moderate logits"""
    r = yhat - y
    if kind == costs.MSE:
        return np.mean(r * r)
    if kind == costs.MAE:
        return np.mean(np.abs(r))
    if kind == costs.HUBER:
        a = np.abs(r)
        return np.mean(np.where(a < param, 0.5 * a * a, param * (a - 0.5 * param)))
    if kind == costs.LOGITCE:
        p = np.exp(yhat) / np.sum(np.exp(yhat), axis=0, keepdims=True)
        return np.mean(-np.sum(y * np.log(p), axis=0))
    s = 1.0 / (1.0 + np.exp(-yhat))
    return np.mean(-y * np.log(s) - (1.0 - y) * np.log(1.0 - s))
