"""Every Gram and push kernel instantiation the shipped library can reach, bit for bit: the cases of tests/gram_routes.py (26
LDS-DMA Gram instantiations at four N classes each, 32 panel instantiations at three, the four reduce kernels, 16 push
instantiations; tests/test_gram_exact_cpu.py proves that the union of the cases' routes equals gram_routes.REACHABLE and that no
case is hollow).  Lattice snapshots with epoch counters n_j >= 1: A and G = A'A are integer matrices, every partial sum is below
2^53 in any order, so the kernel's G must EQUAL the exact one -- np.array_equal everywhere, no tolerance in this file.  The
cases run in ONE context in an order that alternates large and small N x K, so stale partial tiles, a stale G or stale padding
rows of the case before would show.  The CU count is the device's own.  profiles/gram_exact_kernel_names.txt is the kernel
trace of this file."""
import functools

import numpy as np
import pytest

from tests import gram_routes as gr
from tests import lattice as lat

pytestmark = pytest.mark.gpu

SI_F32, SI_F64 = gr.SI_F32, gr.SI_F64
HOST_PUSH_MAX_N = 4097   # the small N classes are pushed from the host, one snapshot at a time; the large ones in one device batch


@functools.lru_cache(maxsize=1)
def _num_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _ordered_gram_cases():
    return gr.gpu_order(gr.GRAM_CASES)     # (the order by size is the same on every device: N grows with the grid in every class)


@pytest.mark.parametrize("case", _ordered_gram_cases(), ids=lambda c: c.name)
def test_gram_exact(gpu_ctx, case):
    import torch
    num_cu = _num_cu()
    n, k = gr.gram_n(case, num_cu), case.k
    snaps, ns, a, g_ref = gr.gram_problem(n, k)
    # fp32 snapshots hold the same integers: alternate the snapshot type over the case list (by K)
    dtype = np.float32 if k % 2 else np.float64
    gpu_ctx.construct_begin(n, k)
    if case.storage == SI_F32:
        gpu_ctx.construct_set_storage(SI_F32)
    if n <= HOST_PUSH_MAX_N:
        for w, nn in zip(snaps, ns):
            gpu_ctx.construct_push(w.astype(dtype), nn)
    else:
        dev = torch.from_numpy(np.stack(snaps).astype(dtype)).cuda()
        gpu_ctx.construct_push_batch_dev(dev.data_ptr(), SI_F32 if dtype == np.float32 else SI_F64, n, ns)
        torch.cuda.synchronize()
    before = gpu_ctx.stats()["gram"]["launches"]
    gpu_ctx.construct_gram()
    g = gpu_ctx.construct_gram_get()
    # the case ran the route it is there for: one launch on the wave path, npan (npan + 1) / 2 on the panels
    assert gpu_ctx.stats()["gram"]["launches"] - before == gr.gram_launches(n, k, case.storage, num_cu)
    lat.assert_exact(g, g_ref, "G of %s (%d x %d, %s)" % (case.name, n, k, gr.gram_routes(n, k, case.storage, num_cu)[0]))
    assert np.array_equal(g, g.T)
    gpu_ctx.construct_gram()
    assert np.array_equal(gpu_ctx.construct_gram_get(), g), "a second Gram of the same A gives other bits"
    lat.assert_exact(gpu_ctx.construct_get_A(0, k), a, "A of %s" % case.name)


@pytest.mark.parametrize("case", gr.gpu_order(gr.PUSH_CASES), ids=lambda c: c.name)
def test_push_exact(gpu_ctx, case):
    """si_construct_push_dev / si_construct_push_batch_dev with the snapshot pointer, leading dimension and types set on purpose:
    A and W_swa equal the oracle's three rounded operations per push"""
    import torch
    num_cu = _num_cu()
    n = gr.push_n(case, num_cu)
    snaps, ns, w_ref, a_ref = gr.push_problem(case, num_cu)
    dtype = snaps[0].dtype
    dcode = SI_F32 if dtype == np.float32 else SI_F64
    # one flat device buffer: snapshot j starts `offset` elements past row j of a 256-byte aligned base.  Single pushes use rows
    # of pad_ld(N) elements, so every snapshot has the alignment of the offset alone
    ld = gr.pad_ld(n) if case.kind == "single" else n + case.ld_extra
    buf = np.full(case.count * ld + case.offset + 1, np.nan, dtype=dtype)
    for j, w in enumerate(snaps):
        buf[case.offset + j * ld: case.offset + j * ld + n] = w
    dev = torch.from_numpy(buf).cuda()
    assert dev.data_ptr() % 256 == 0
    esz = buf.itemsize
    ptr = lambda j: dev.data_ptr() + (case.offset + j * ld) * esz
    gpu_ctx.construct_begin(n, case.count)
    if case.storage == SI_F32:
        gpu_ctx.construct_set_storage(SI_F32)
    before = gpu_ctx.stats()["push"]["launches"]
    if case.kind == "single":
        for j, nn in enumerate(ns):
            gpu_ctx.construct_push_dev(ptr(j), dcode, nn)
        assert gpu_ctx.stats()["push"]["launches"] - before == case.count
    else:
        h = case.count // 2
        gpu_ctx.construct_push_batch_dev(ptr(0), dcode, ld, ns[:h])
        gpu_ctx.construct_push_batch_dev(ptr(h), dcode, ld, ns[h:])
        assert gpu_ctx.stats()["push"]["launches"] - before == 2
    torch.cuda.synchronize()
    assert np.array_equal(gpu_ctx.construct_get_A(0, case.count), a_ref), case.name
    w_swa, _, _, kk = gpu_ctx.construct_finish(1, want_p=False)
    assert kk == case.count and np.array_equal(w_swa, w_ref), case.name
