"""The costs of the training step, as NumPy: the definition csrc/kernels_cost.hip and the tests are held to.

Five costs of Flux 0.11.2 with their default `agg = mean` [upstream Flux 0.11.2 src/losses/functions.jl and NNlib's
logsoftmax / logσ, restated from memory, unverifiable offline].  yhat is the chain's output (out x nb), y the targets,
r = yhat - y, d = out * nb:

  MSE (0)       sum r^2 / d                                              2 r / d
  MAE (1)       sum |r| / d                                              sign(r) / d, sign(0) = 0
  HUBER (2)     sum h(r) / d, h = r^2 / 2 for |r| < delta (strict),      (r for |r| < delta, else delta sign(r)) / d
                delta (|r| - delta / 2) otherwise; param = delta
  LOGITCE (3)   (1 / nb) sum_b -sum_i y_ib (yhat_ib - lse_b),            (S_b p_ib - y_ib) / nb, p = softmax over i,
                lse_b = m_b + log sum_i exp(yhat_ib - m_b),              S_b = sum_i y_ib (kept: Zygote differentiates the
                m_b = max_i yhat_ib   (dims = 1)                          formula as written, it does not assume S_b = 1)
  LOGITBCE (4)  sum((1 - y) yhat + softplus(-yhat)) / d,                 (sigmoid(yhat) - y) / d, the sigmoid without
                softplus(-x) = max(-x, 0) + log1p(exp(-|x|))             overflow for either sign

`numerator` is the sum before the division (what si_train_grad returns for a share of a batch), `denominator` what it
is divided by, `value` the cost and `dvalue` its derivative with respect to yhat; `denom` overrides the denominator of the
derivative (a share of a larger batch: the data-parallel scaling).
"""
import numpy as np

MSE, MAE, HUBER, LOGITCE, LOGITBCE = 0, 1, 2, 3, 4
KINDS = (MSE, MAE, HUBER, LOGITCE, LOGITBCE)
NAMES = {MSE: "mse", MAE: "mae", HUBER: "huber_loss", LOGITCE: "logitcrossentropy", LOGITBCE: "logitbinarycrossentropy"}


def denominator(kind, out, nb):
    return float(nb) if kind == LOGITCE else float(out) * float(nb)


def _args(yhat, y):
    yhat, y = np.asarray(yhat, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if yhat.ndim != 2 or yhat.shape != y.shape:
        raise ValueError("DimensionMismatch: yhat and y are (out x nb) matrices of one shape")
    return yhat, y


def _softmax_parts(yhat):
    m = np.max(yhat, axis=0, keepdims=True)
    e = np.exp(yhat - m)
    se = np.sum(e, axis=0, keepdims=True)
    return m, e, se


def numerator(kind, yhat, y, param=0.0):
    yhat, y = _args(yhat, y)
    r = yhat - y
    if kind == MSE:
        return float(np.sum(r * r))
    if kind == MAE:
        return float(np.sum(np.abs(r)))
    if kind == HUBER:
        a = np.abs(r)
        return float(np.sum(np.where(a < param, 0.5 * r * r, param * (a - 0.5 * param))))
    if kind == LOGITCE:
        m, _, se = _softmax_parts(yhat)
        lse = m + np.log(se)
        return float(-np.sum(y * (yhat - lse)))
    if kind == LOGITBCE:
        return float(np.sum((1.0 - y) * yhat + np.maximum(-yhat, 0.0) + np.log1p(np.exp(-np.abs(yhat)))))
    raise ValueError("unknown cost %r" % (kind,))


def value(kind, yhat, y, param=0.0):
    yhat, y = _args(yhat, y)
    return numerator(kind, yhat, y, param) / denominator(kind, yhat.shape[0], yhat.shape[1])


def dvalue(kind, yhat, y, param=0.0, denom=None):
    yhat, y = _args(yhat, y)
    inv = 1.0 / (denominator(kind, yhat.shape[0], yhat.shape[1]) if denom is None else float(denom))
    r = yhat - y
    if kind == MSE:
        g = 2.0 * r
    elif kind == MAE:
        g = np.sign(r)
    elif kind == HUBER:
        g = np.where(np.abs(r) < param, r, param * np.sign(r))
    elif kind == LOGITCE:
        _, e, se = _softmax_parts(yhat)
        g = np.sum(y, axis=0, keepdims=True) * (e / se) - y
    elif kind == LOGITBCE:
        t = np.exp(-np.abs(yhat))
        g = np.where(yhat >= 0.0, 1.0 / (1.0 + t), t / (1.0 + t)) - y
    else:
        raise ValueError("unknown cost %r" % (kind,))
    return g * inv
