"""Context life cycle: create / use every family of entry points / destroy, many times -- the device memory the library
holds (incl. the buffers it caches between calls: staging of the output map, Gram partials, conv scratch) goes back."""
import numpy as np
import pytest

from oracle import subspace_oracle as so

pytestmark = pytest.mark.gpu


def test_no_device_memory_is_left_behind(si):
    import torch
    rng = np.random.default_rng(0)

    def free_mb():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0] / 2 ** 20

    spec = [("conv", (3, 3), 8, so.ACT_RELU, (1, 1), (1, 1)), ("maxpool", (2, 2)), ("flatten",), ("dense", 10, so.ACT_IDENTITY)]
    table, n = so.conv_table(spec, (8, 8, 3))
    w = 0.3 * rng.standard_normal(n)
    p = np.asfortranarray(0.1 * rng.standard_normal((n, 4)))
    x = np.asfortranarray(rng.standard_normal((8 * 8 * 3, 64)))
    y = np.asfortranarray(rng.standard_normal((10, 64)))
    dims = [(64, 300, 1, 0, 64 * 300), (300, 1, 0, 64 * 300 + 300, 64 * 300 + 300 + 300)]
    nd = 64 * 300 + 300 + 300 + 1
    wd = rng.standard_normal(nd)
    pd = np.asfortranarray(rng.standard_normal((nd, 5)))
    xd = np.asfortranarray(rng.standard_normal((64, 500)))
    yd = np.asfortranarray(rng.standard_normal((1, 500)))
    torch.zeros(1, device="cuda")
    base = None
    for it in range(24):
        ctx = si.Context(0)
        ctx.infer_setup(table, n, 4, w, p, x, y, 1.0)
        ctx.sample_rwmh(3, 0.1, seed=it)
        ctx.logdensity_grad(np.zeros(4))
        ctx.reconstruct(np.asfortranarray(rng.standard_normal((4, 70))))
        ctx.infer_setup(dims, nd, 5, wd, pd, xd, yd, 1.0)
        ctx.sample_rwmh(3, 0.1, seed=it, nchains=3)
        ctx.reconstruct(np.asfortranarray(rng.standard_normal((5, 9))))
        ctx.construct_begin(nd, 12)
        for k in range(12):
            ctx.construct_push(rng.standard_normal(nd).astype(np.float32), float(k))
        ctx.construct_finish(5)
        ctx.close()
        if it == 3:
            base = free_mb()
    assert abs(free_mb() - base) < 64.0


def test_every_family_of_buffers_many_times(si):
    """The families the test above never touches -- training state (Float64, Float32, set up again larger), inference set-ups
    that grow, shrink and change precision, the three sampler forms with the output map at 1 and 3 chains, the step-wise
    session (abandoned, then run to its end), batched device pushes and the refine route of the construction, a call that
    fails validation between working ones -- on a context that is built and closed 12 times.  Every call succeeds (the
    wrappers raise otherwise) or fails as stated; what the same seeds produce in round 0 they produce in round 11, bit for
    bit; the device memory goes back.
    si_sample_rwmh* picks its form by shape, and chain_kernel_info tells the specialised grid loop from the rest:
      small20  2-20-20-1 on 96 observations fits ONE workgroup's LDS: the one-workgroup loop, like 2-16-16-1 on 64;
      spec     2-40-40-1 on 1024 observations is past the one-workgroup loop's arithmetic limit (2 N B = 3.7e6 > 3e6), has a
               fused head and 1024 model outputs: the grid loop on the kernels compiled for its shapes at run time, with
               their own weight / output / permutation buffers, grown from 1 to 3 chains and rebuilt every round;
      grid     2-20-20-5 on 96 observations: a head of 5 is not fused, so the generic grid loop.
    One call on `spec` is long enough (1400 and then 2000 transitions of 3 chains: 134 and 192 KB of samples + lp) for its
    output to go through the pinned staging buffer, which grows between the two."""
    import torch
    from subspaceinference_jl_amd._capi import SI_ERR_INVALID, SI_F32, SI_F64, SubspaceError
    rng = np.random.default_rng(5)

    def free_mb():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0] / 2 ** 20

    def chain(dims, acts, b, m):
        table, n = so.layer_table(dims, acts)
        return dict(table=table, n=n, m=m, w=0.3 * rng.standard_normal(n), p=np.asfortranarray(0.05 * rng.standard_normal((n, m))),
                    x=np.asfortranarray(rng.standard_normal((dims[0], b))), y=np.asfortranarray(rng.standard_normal((dims[-1], b))))

    def setup(ctx, c, dtype=SI_F64):
        ctx.infer_setup(c["table"], c["n"], c["m"], c["w"], c["p"], c["x"], c["y"], 0.8, compute_dtype=dtype)

    small = chain([2, 16, 16, 1], [1, 1, 0], 64, 3)        # training chain; one-workgroup loop
    wide = chain([4, 24, 24, 2], [2, 1, 0], 128, 4)
    small20 = chain([2, 20, 20, 1], [1, 1, 0], 96, 3)      # one-workgroup loop as well
    spec = chain([2, 40, 40, 1], [1, 1, 0], 1024, 3)       # grid loop, kernels specialised to the chain's shapes
    grid = chain([2, 20, 20, 5], [1, 1, 0], 96, 3)         # head of 5: no fused head, so the grid loop
    w0 = (0.3 * rng.standard_normal(small["n"])).astype(np.float32)
    idx_a, idx_b, idx_c = np.arange(16), rng.permutation(64)[:16], rng.permutation(64)[:32]
    snaps = torch.tensor(rng.standard_normal((3, small["n"] + 5)), dtype=torch.float64, device="cuda")   # 3 columns, ld = n + 5
    basis, coef = rng.standard_normal((40, 3)), rng.standard_normal((3, 6))
    low_rank = [np.ascontiguousarray(basis @ coef[:, k]) for k in range(6)]   # 40 x 6 deviation matrix of rank 3

    def one_round():
        out = []
        ctx = si.Context(0)
        try:
            # training: Float64, then Float32, each set up again with a larger batch_max; pushes feed the construction
            ctx.construct_begin(small["n"], 8)
            for dt, want in ((np.float64, SI_F64), (np.float32, SI_F32)):
                x, y = small["x"].astype(dt), small["y"].astype(dt)
                ctx.train_setup(small["table"], small["n"], w0, x, y, 16, 2, 0.01, 0.9, 0.999)
                assert ctx.train_compute_dtype() == want
                out += [ctx.train_step(idx_a), ctx.train_step(idx_b)]
                ctx.train_push(1.0)
                ctx.train_setup(small["table"], small["n"], w0, x, y, 32, 2, 0.01, 0.9, 0.999)
                out += [ctx.train_step(idx_c), ctx.train_get_weights()]
            # construction: batched device pushes behind the two training pushes, then the finish
            ctx.construct_push_batch_dev(snaps.data_ptr(), SI_F64, small["n"] + 5, [2.0, 3.0, 4.0])
            out += list(ctx.construct_finish(2))
            # inference set-ups: Float32, then Float64 on other shapes (smaller, then larger); a prior on a 3-transition chain
            setup(ctx, wide, SI_F32)
            out += list(ctx.sample_rwmh(3, 0.1, seed=7, nchains=2))
            setup(ctx, small)
            ctx.set_prior(2.0)
            out += list(ctx.sample_rwmh(3, 0.1, seed=8))
            ctx.set_prior(0.0)
            # the three sampler forms with the output map, 1 and 3 chains
            forms = {}
            for name, c, mode in (("launch", small, 2), ("workgroup", small, 1), ("small20", small20, 1), ("spec", spec, 1),
                                  ("grid", grid, 1)):
                setup(ctx, c)
                ctx.set_chain_loop(mode)
                for nch in (1, 3):
                    z, lp, acc, w = ctx.sample_rwmh_weights(12, 0.1, seed=9, nchains=nch)
                    assert ctx.chain_kernel_info()[1] == (name == "spec"), (name, nch, ctx.chain_kernel_info())
                    # W = W_swa + P z: M = 3 products summed in fp64, whatever the column batching of the K4 launch
                    assert np.allclose(w[:, 5, nch - 1], ctx.reconstruct(z[:, 5, nch - 1])[:, 0], rtol=1e-12, atol=1e-12)
                    forms[name, nch] = (z, lp, acc, w)
                    out += [z, lp, acc, w]
                if name == "spec":   # long enough for the pinned staging of Z and lp, which then grows; same bits as per-step launches
                    long_a = ctx.sample_rwmh(1400, 0.05, seed=10, nchains=3)
                    assert ctx.chain_kernel_info()[1]
                    out += list(long_a) + list(ctx.sample_rwmh(2000, 0.05, seed=10, nchains=3))
                    ctx.set_chain_loop(2)
                    for a, b in zip(long_a, ctx.sample_rwmh(1400, 0.05, seed=10, nchains=3)):
                        assert np.array_equal(a, b)
                ctx.set_chain_loop(1)
            for nch in (1, 3):   # the forms are the same chain, bit for bit
                for a, b in zip(forms["launch", nch][:3], forms["workgroup", nch][:3]):
                    assert np.array_equal(a, b)
            # step-wise session: one abandoned, one run to its end (still on the last set-up)
            ctx.rwmh_begin(4, 0.1, seed=3, nchains=2)
            ctx.rwmh_step_accept(ctx.rwmh_step_eval())
            ctx.rwmh_abort()
            ctx.rwmh_begin(4, 0.1, seed=3, nchains=2)
            for _ in range(4):
                ctx.rwmh_step_accept(ctx.rwmh_step_eval())
            out += list(ctx.rwmh_end())
            # a call that fails validation in the middle, then a working call on the same context
            with pytest.raises(SubspaceError) as bad:
                ctx.infer_setup(grid["table"], grid["n"], 0, None, None, grid["x"], grid["y"], 0.8)
            assert bad.value.code == SI_ERR_INVALID
            out += list(ctx.sample_rwmh(3, 0.1, seed=4))
            # construction, refine route on a rank-deficient 40 x 6 deviation matrix
            ctx.construct_begin(40, 6)
            for k, wk in enumerate(low_rank):
                ctx.construct_push(wk, float(k))
            ctx.construct_gram()
            ctx.construct_refine()
            w_swa, p, s, k = ctx.construct_finish(3)
            assert k == 6 and np.all(np.isfinite(p)) and s[2] > 1e-6 * s[0]
            out += [w_swa, p, s]
        finally:
            ctx.close()
        return out

    torch.zeros(1, device="cuda")
    base = first = last = None
    for it in range(12):
        last = one_round()
        if it == 0:
            first = last
        if it == 3:
            base = free_mb()
    assert len(first) == len(last)
    for a, b in zip(first, last):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert abs(free_mb() - base) < 64.0
