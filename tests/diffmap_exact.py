"""An exact kernel-matrix family for method = :diffusion: deviation matrices on which every stage of steps 1-3 of
si_construct_finish_diffmap (csrc/kernels_diffmap.hip) is a short chain of correctly rounded operations, restated here operation
by operation in plain NumPy (a helper module for the tests, not a conftest; the diffusion twin of tests/lattice.py).

The inputs.  Every row of A (N x K) is an exact copy of one of a few centres with integer coordinates in 0 .. 8, pairwise
distinct; centre 0 is all zeros and centre 1 all eights, so every column holds both 0 and 8 and the rescaled Xr = (x - 0) * (1 / 8)
is an exact multiple of 1/8.  The SWA recurrence of tests/diffmap_cases.py::push_columns is exact on small integers and so is
fp32 storage: the device's A equals the lattice bit for bit.

The parameters.  kernel_sign = -1 and eps = 2^-16.  Two copies of one centre have d = 0 exactly (s_i, s_j and S_ij are exact sums
of a few multiples of 1/64) and exp(0) = 1; two different centres have d >= 1/64 (one coordinate apart by 1/8) or d >= 1 (not
rescaled), the argument of exp is <= -1024 and the entry is exactly 0: Kmat is the 0/1 membership matrix.  From there, in the
order the kernel file documents:
  p_i        the size of i's cluster: a sum of ones, exact in any order
  x_ij       Kmat_ij / w(p_i p_j), w = the product itself (alpha = 1) or pow(., 0) = 1 (alpha = 0)          [one division]
  part[c][i] the sum of x_ij over the 64 columns of chunk c in ascending j (dm_scale_rows_kernel)
  q_i        sqrt(sum_c part[c][i], c ascending)                                                            (dm_sum_parts_kernel)
  Kn_ij      x_ij / (q_i * q_j)                                                                             [one product, one division]
  u_1        q / sqrt(sum q_i^2): thread t of 256 sums q_i * q_i over i = t, t + 256, .. ascending, then the halving tree
             sh[t] += sh[t + s], s = 128 .. 1                                                               (dm_unit_kernel)
NumPy's elementwise +, *, / and sqrt on float64 are the IEEE operations, and the kernel file is compiled with -ffp-contract=off.

Two families of cluster sizes:
  "pow2"     every size a power of two (the binary digits of N, the largest split until there are three clusters): 1 / c^2, every
             sum and every square root's argument are exact, so the result does not depend on any order -- a wrong, missing or
             doubled partial still changes it.  The members are dealt over the index range with a stride coprime to N.
  "mod3", "mod5"   lab_i = (7 i + 3) mod nc: every cluster has members in every 64-block, the ragged last one included, and the
             sizes are general, so the documented order of the sums matters.
The operator is the projector blockdiag(J_c / c) (alpha = 1 and alpha = 0 alike, up to rounding): eigenvalue 1 once per cluster,
0 otherwise, every eigenvector constant on every cluster."""
import functools
import math

import numpy as np

EPS = 2.0 ** -16
SIGN = -1
DM_T = 64          # <- DM_T, kernels_diffmap.hip
UNIT_THREADS = 256  # <- dm_unit_kernel / dm_block_sum
FAMILIES = ("pow2", "mod3", "mod5")


def pow2_sizes(n):
    """the powers of two in n, the largest split in halves until there are three clusters (or all are 1)"""
    sizes = sorted((1 << b for b in range(n.bit_length()) if n >> b & 1), reverse=True)
    while len(sizes) < 3 and sizes[0] > 1:
        sizes = sorted(sizes[1:] + [sizes[0] // 2] * 2, reverse=True)
    return sizes


def labels(n, family):
    """the cluster of every weight (int array of n)"""
    if family == "pow2":
        sizes = pow2_sizes(n)
        stride = next(s for s in (7, 11, 13) if math.gcd(s, n) == 1)
        rank_cluster = np.repeat(np.arange(len(sizes)), sizes)
        lab = np.empty(n, dtype=np.int64)
        lab[(stride * np.arange(n) + 3) % n] = rank_cluster
        return lab
    nc = min(int(family[3:]), n)   # (N = 3: three clusters of one weight)
    return (7 * np.arange(n) + 3) % nc


def centres(nc, k):
    """nc pairwise distinct integer points of {0..8}^k, the first all zeros and the second all eights"""
    assert 2 <= nc <= 9
    c = np.zeros((nc, k))
    c[1] = 8.0
    for j in range(2, nc):
        c[j, 0] = j - 1
        c[j, 1:] = (3 * j + 5 * np.arange(1, k)) % 9
    return c


@functools.lru_cache(maxsize=None)
def lattice(n, k, family):
    """(A (n x k, Fortran order, read-only), labels)"""
    lab = labels(n, family)
    nc = int(lab.max()) + 1
    assert np.array_equal(np.unique(lab), np.arange(nc))
    a = np.asfortranarray(centres(nc, k)[lab])
    a.setflags(write=False)
    lab.setflags(write=False)
    return a, lab


def check_preconditions(a, lab):
    """what makes Kmat a 0/1 matrix; raises AssertionError"""
    assert np.exp(-1024.0) == 0.0 and np.exp(0.0) == 1.0
    assert np.array_equal(a, np.round(a)) and a.min() == 0.0 and a.max() == 8.0
    assert np.all(a.min(axis=0) == 0.0) and np.all(a.max(axis=0) == 8.0)        # range 8 in every column
    nc = int(lab.max()) + 1
    cen = np.array([a[np.argmax(lab == c)] for c in range(nc)])
    assert np.array_equal(a, cen[lab])                                          # rows are exact copies
    for i in range(nc):
        for j in range(i):
            assert np.any(cen[i] != cen[j])                                     # distinct centres
    for rescale in (False, True):
        x = a * 0.125 if rescale else a
        d = ((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)                  # exact: small multiples of 1/64
        diff = lab[:, None] != lab[None, :]
        assert np.all(d[~diff] == 0.0) and (not diff.any() or SIGN * d[diff].min() / EPS <= -1024.0)


def _sum_ascending(x):
    """sum over the columns of x in ascending order, one rounded addition each"""
    t = np.zeros(x.shape[0])
    for j in range(x.shape[1]):
        t = t + x[:, j]
    return t


def membership(lab):
    return (lab[:, None] == lab[None, :]).astype(np.float64)


def kernel(lab, alpha):
    """(Kn, q, u1) of the 0/1 kernel matrix of the labels, in the device's order of operations"""
    assert alpha in (0.0, 1.0)
    n = lab.size
    kmat = membership(lab)
    p = kmat.sum(axis=1)                                     # integers: exact in any order
    w = np.outer(p, p) if alpha == 1.0 else np.ones((n, n))  # pow(w, 0) = 1
    x = kmat / w
    nb = (n + DM_T - 1) // DM_T
    part = np.stack([_sum_ascending(x[:, DM_T * c:min(DM_T * (c + 1), n)]) for c in range(nb)], axis=1)
    q = np.sqrt(_sum_ascending(part))
    kn = x / (q[:, None] * q[None, :])
    return kn, q, unit(q)


@functools.lru_cache(maxsize=None)
def kernel_of(n, family, alpha):
    """kernel(labels(n, family), alpha), computed once per session and read-only"""
    out = kernel(labels(n, family), alpha)
    for x in out:
        x.setflags(write=False)
    return out


def unit(q):
    """u_1 = q / ||q|| in dm_unit_kernel's order"""
    sq = q * q
    sh = np.zeros(UNIT_THREADS)
    for i in range(q.size):          # thread i % 256, ascending i inside a thread
        sh[i % UNIT_THREADS] = sh[i % UNIT_THREADS] + sq[i]
    s = UNIT_THREADS // 2
    while s > 0:
        sh[:s] = sh[:s] + sh[s:2 * s]
        s //= 2
    return q / np.sqrt(sh[0])


def closed_form(lab):
    """the projector blockdiag(J_c / c) the operator is up to rounding"""
    kmat = membership(lab)
    return kmat / kmat.sum(axis=1)[:, None]


# ---------------------------------------------------------------------------------------------- the grid of the GPU test
NS = (3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 192, 193, 257)
KS = (1, 3, 4, 5, 8)
# (N, K, family, rescale, alpha, fp32 storage).  The full product pruned: every N meets every family and both values of each flag,
# K walks its list along the way (N = 3 with K = 8 is K > N), and N = 65 is the fp32-storage column with every K.
GRID = []
for _i, _n in enumerate(NS):
    for _j, _fam in enumerate(FAMILIES):
        _t = _i + _j
        GRID.append((_n, KS[_t % 5], _fam, bool(_t % 2), 1.0 if (_t // 2) % 2 == 0 else 0.0, False))
    GRID.append((_n, KS[(_i + 3) % 5], FAMILIES[_i % 3], bool((_i + 1) % 2), 0.0 if _i % 2 == 0 else 1.0, False))
GRID = [g for g in GRID if not (g[0] == 3 and g[1] == 8)] + [(3, 8, "mod3", True, 1.0, False), (3, 8, "pow2", False, 0.0, False)]
GRID += [(65, k, FAMILIES[i % 3], bool(i % 2), 1.0 if i % 3 else 0.0, True) for i, k in enumerate(KS)]
assert len(set(GRID)) == len(GRID)
