"""Host side of the stacked gradient (no GPU): `samplers.mala_chains` is `samplers.mala` per chain, and the ctypes prototypes of
si_logdensity_grad_batch / si_grad_kernel_info are the header's."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _quadratic(m, seed):
    """a NumPy-only log-density with its gradient: lp(z) = -(z - mu)' A (z - mu) / 2 + sum(sin z)"""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((m, m))
    a = q @ q.T / m + np.eye(m)
    mu = rng.standard_normal(m)

    def one(z):
        d = z - mu
        return float(-0.5 * d @ a @ d + np.sin(z).sum()), -(a @ d) + np.cos(z)

    def batch(zz):
        calls.append(zz.shape[1])
        out = [one(np.array(zz[:, c])) for c in range(zz.shape[1])]
        return np.array([o[0] for o in out]), np.asfortranarray(np.stack([o[1] for o in out], axis=1))
    calls = []
    return one, batch, calls


def test_mala_chains_is_mala_per_chain():
    from subspaceinference_jl_amd import samplers
    m, itr, sigma_z, nc = 5, 60, 0.4, 4
    one, batch, calls = _quadratic(m, 1)
    zs, lps, acc = samplers.mala_chains(batch, m, itr, sigma_z, [np.random.default_rng([9, c]) for c in range(nc)])
    assert zs.shape == (m, itr, nc) and lps.shape == (itr, nc) and acc.shape == (nc,)
    assert calls == [nc] * itr          # one stacked gradient call per transition (and one for the initial states)
    for c in range(nc):
        z1, lp1, a1 = samplers.mala(one, m, itr, sigma_z, np.random.default_rng([9, c]))
        assert np.array_equal(zs[:, :, c], z1) and np.array_equal(lps[:, c], lp1) and acc[c] == a1
    assert 0.0 < acc.min() and len({tuple(zs[:, -1, c]) for c in range(nc)}) == nc   # chains moved, and differ


def test_mala_chains_single_chain_and_single_step():
    from subspaceinference_jl_amd import samplers
    one, batch, _ = _quadratic(3, 2)
    zs, lps, acc = samplers.mala_chains(batch, 3, 1, 0.3, [np.random.default_rng(4)])
    z1, lp1, a1 = samplers.mala(one, 3, 1, 0.3, np.random.default_rng(4))
    assert np.array_equal(zs[:, :, 0], z1) and np.array_equal(lps[:, 0], lp1) and acc[0] == a1 == 0.0


def test_prototypes_match_the_header():
    from subspaceinference_jl_amd import _capi
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "subspace_hip.h")).read(), flags=re.S)
    ctype = {"si_ctx*": ctypes.c_void_p, "double*": ctypes.c_void_p, "int32_t": ctypes.c_int32,
             "int32_t*": ctypes.POINTER(ctypes.c_int32)}
    want = {"si_logdensity_grad_batch": ["si_ctx*", "double*", "int32_t", "double*", "double*"],
            "si_grad_kernel_info": ["si_ctx*", "int32_t*"]}
    for name, cargs in want.items():
        m = re.search(r"\bint32_t\s+%s\s*\(([^;{]*?)\)\s*;" % name, text, flags=re.S)
        assert m, name + " is not declared in include/subspace_hip.h"
        args = []
        for a in m.group(1).split(","):
            a = re.sub(r"\s+", " ", re.sub(r"\bconst\b", " ", a)).strip()
            args.append(re.match(r"([A-Za-z_]\w*)", a.replace("*", " ").strip()).group(1) + "*" * a.count("*"))
        assert args == cargs, (name, args)
        res, sig = _capi.SIGNATURES[name]
        assert res is ctypes.c_int32 and sig == [ctype[a] for a in cargs], (name, sig)


def test_library_exports_the_new_entry_points():
    import subspaceinference_jl_amd as si
    lib = si.load()
    assert lib.si_version() == 500
    assert lib.si_logdensity_grad_batch.argtypes[2] is ctypes.c_int32 and lib.si_grad_kernel_info.restype is ctypes.c_int32
    fused = ctypes.c_int32(7)
    assert lib.si_grad_kernel_info(None, ctypes.byref(fused)) == si._capi.SI_ERR_INVALID   # (a NULL ctx is refused, not read)
    assert lib.si_logdensity_grad_batch(None, None, 1, None, None) == si._capi.SI_ERR_INVALID
