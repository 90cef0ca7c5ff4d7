"""tests/diffmap_exact.py certified without a GPU: the helper's preconditions hold on the whole grid of
tests/test_gpu_diffmap_exact.py, its operator agrees with the NumPy definition (diffmap.diffmap_kernel) on the same input to 4 ulp
with the same zero pattern, with the closed form blockdiag(J_c / c), and the power-of-two family is exact (no order can matter)."""
import numpy as np
import pytest

from tests import diffmap_exact as dx


@pytest.fixture(scope="module")
def dmp(si):
    from subspaceinference_jl_amd import diffmap
    return diffmap


def test_exp_underflows_and_the_grid_covers_what_it_says():
    assert np.exp(-1024.0) == 0.0 and np.exp(0.0) == 1.0
    assert {g[0] for g in dx.GRID} == set(dx.NS) and {g[1] for g in dx.GRID} == set(dx.KS)
    assert {g[2] for g in dx.GRID} == set(dx.FAMILIES)
    assert {g[3] for g in dx.GRID} == {False, True} and {g[4] for g in dx.GRID} == {0.0, 1.0}
    assert (3, 8) in {g[:2] for g in dx.GRID}                                    # K > N
    f32 = [g for g in dx.GRID if g[5]]
    assert {g[1] for g in f32} == set(dx.KS) and len({g[0] for g in f32}) == 1   # one fp32-storage column of the grid
    assert 50 <= len(dx.GRID) <= 70
    for n in dx.NS:   # every N meets both flags' values and both kinds of cluster sizes
        mine = [g for g in dx.GRID if g[0] == n]
        assert {g[3] for g in mine} == {False, True} and {g[4] for g in mine} == {0.0, 1.0} and {g[2] for g in mine} == set(dx.FAMILIES)


@pytest.mark.parametrize("n,k,family", sorted({g[:3] for g in dx.GRID}))
def test_preconditions(n, k, family):
    a, lab = dx.lattice(n, k, family)
    assert a.shape == (n, k) and a.flags.f_contiguous
    dx.check_preconditions(a, lab)
    sizes = np.bincount(lab)
    if family == "pow2":
        assert np.all(sizes & (sizes - 1) == 0) and sizes.sum() == n and (len(sizes) >= 3 or n < 3)
    else:
        assert np.array_equal(lab, (7 * np.arange(n) + 3) % len(sizes)) and len(sizes) == min(int(family[3:]), n)
        for b in range((n + 63) // 64):   # members in every 64-block, the ragged last one included (where it has nc rows)
            blk = lab[64 * b:64 * (b + 1)]
            assert len(set(blk)) == min(len(sizes), blk.size)
    assert np.array_equal(a, a.astype(np.float32))   # fp32 storage holds the lattice exactly


def _ulp_distance(x, y):
    return np.abs(x - y) / np.spacing(np.maximum(np.abs(x), np.abs(y)))


@pytest.mark.parametrize("n,k,family,rescale,alpha,f32", dx.GRID)
def test_helper_agrees_with_the_definition(dmp, n, k, family, rescale, alpha, f32):
    a, lab = dx.lattice(n, k, family)
    kn, q, u1 = dx.kernel(lab, alpha)
    kn_ref, q_ref = dmp.diffmap_kernel(a, dx.EPS, alpha, dx.SIGN, rescale)
    assert np.array_equal(kn == 0.0, kn_ref == 0.0) and np.array_equal(kn != 0.0, dx.membership(lab) == 1.0)
    nz = kn != 0.0
    assert _ulp_distance(kn[nz], kn_ref[nz]).max() <= 4.0
    assert _ulp_distance(q, q_ref).max() <= 4.0
    assert _ulp_distance(u1, q_ref / np.linalg.norm(q_ref)).max() <= 4.0
    assert np.array_equal(kn, kn.T)
    assert np.abs(kn - dx.closed_form(lab)).max() <= 4e-16
    # u_1's own norm sum (at most 2 + 8 + 1 additions deep), square root and division, then np.linalg.norm's sum of n squares
    assert abs(np.linalg.norm(u1) - 1.0) <= (n + 16) * 2.0 ** -53


@pytest.mark.parametrize("n", dx.NS)
@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_power_of_two_sizes_are_exact(n, alpha):
    """every summand is a power of two and every sum a sum of equal powers of two below 2^53: any order gives these bits"""
    lab = dx.labels(n, "pow2")
    kn, q, _ = dx.kernel(lab, alpha)
    sizes = np.bincount(lab)[lab].astype(np.float64)
    # the sums under the square root were exact: c copies of 1 / c^2 (alpha = 1) or of 1 (alpha = 0)
    assert np.array_equal(q, np.sqrt(1.0 / sizes if alpha == 1.0 else sizes))
    perm = np.random.default_rng(n).permutation(n)   # relabelled weights: the same entries at permuted places
    kn_p = dx.kernel(lab[perm], alpha)[0]
    assert np.array_equal(kn_p, kn[np.ix_(perm, perm)])


def test_general_sizes_depend_on_the_order():
    """the mod families are there because the order matters on them: summing a row's chunk partials in descending order changes
    bits somewhere on the grid (so a device that sums in another order than documented fails the bit comparison)"""
    changed = 0
    for n in (127, 129, 192, 193, 257):
        for fam in ("mod3", "mod5"):
            lab = dx.labels(n, fam)
            kmat = dx.membership(lab)
            p = kmat.sum(axis=1)
            x = kmat / np.outer(p, p)
            nb = (n + 63) // 64
            part = np.stack([dx._sum_ascending(x[:, 64 * c:min(64 * (c + 1), n)]) for c in range(nb)], axis=1)
            changed += int(np.any(dx._sum_ascending(part) != dx._sum_ascending(part[:, ::-1])))
    assert changed > 0
