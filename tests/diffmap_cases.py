"""Inputs shared by test_diffmap_cpu.py and test_gpu_diffmap.py: the clustered deviation matrices of the case list and the
README toy trained for three epochs, each computed once per session."""
import functools

import numpy as np

# (N, K, clusters, generator seed).  The seeds were chosen on the CPU, from the dense spectrum alone, so that every case has
# spectrum_gap >= 1e-3 for M in MS and both kernel signs (test_diffmap_cpu.py asserts it): only there are the compared
# vectors well defined.
CASES = [(77, 5, 4, 3), (200, 7, 6, 0), (333, 12, 6, 0)]
MS = (2, 3, 5)
SIGNS = (-1, 1)


@functools.lru_cache(maxsize=None)
def clustered(n, k, nc, seed):
    """`nc` cluster centres, every weight a noisy copy of one of them, snapshot k scaled by 1 .. 2"""
    rng = np.random.default_rng(seed)
    cen = rng.random((nc, k))
    lab = rng.integers(0, nc, n)
    a = cen[lab] * np.linspace(1.0, 2.0, k) + 0.05 * rng.standard_normal((n, k))
    a = np.asfortranarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def trained_toy(seed=0):
    """The README toy (Dense 10-20-20-2, 100 observations, batchsize 10) trained for 3 epochs with ADAM on the host: the 30
    Float32 snapshots and their n = i / c, in push order (N = 682, K = 30)."""
    from subspaceinference_jl_amd import flux
    rng = np.random.default_rng(seed)
    x, y = rng.random((10, 100)), rng.random((2, 100))
    m = flux.Chain(flux.Dense(10, 20, flux.relu, rng=rng), flux.Dense(20, 20, flux.relu, rng=rng), flux.Dense(20, 2, rng=rng))
    data = flux.DataLoader(x, y, batchsize=10, shuffle=True, rng=rng)
    opt, ps = flux.ADAM(0.01), flux.params(m)
    snaps, ns = [], []
    for i in range(1, 4):
        for d in data:
            _, gs = flux.gradient(flux.mse, m, *d)
            flux.update(opt, ps, gs)
            snaps.append(flux.extract_params(ps).copy())
            ns.append(float(i))
    return tuple(snaps), tuple(ns), m, x, y


@functools.lru_cache(maxsize=None)
def toy_deviations(seed=0):
    """the toy's deviation matrix (N x 30) as the oracle's SWA recurrence forms it"""
    from oracle import subspace_oracle as so
    snaps, ns = trained_toy(seed)[:2]
    w_swa, a = so.construct_stream(list(snaps), list(ns))
    a = np.asfortranarray(a)
    a.setflags(write=False)
    return w_swa, a


def push_columns(ctx, a, storage=None):
    """a construction whose deviation columns are read back afterwards: the tests feed the restatement what the device holds"""
    n, k = a.shape
    ctx.construct_begin(n, k)
    if storage is not None:
        ctx.construct_set_storage(storage)
    # snapshots whose deviation columns are the columns of a (to rounding): with n = 1 the SWA update (s + w) / 2 gives
    # s_j = s_{j-1} + a_j and w_j - s_j = a_j for w_j = s_{j-1} + 2 a_j
    s = np.zeros(n)
    for j in range(k):
        ctx.construct_push(s + 2.0 * a[:, j], 1.0)
        s = s + a[:, j]
    return ctx.construct_get_A(0, k)
