"""The autoencoder route's definition (subspaceinference_jl_amd/autoencoder.py) and the argument errors of its API, on the CPU:
`decode` against a plain per-layer evaluation, the adjoint identity of its two Jacobian products under the fp64 dot-product bound,
`decode_jvp` against central differences, the lattice case list of tests/decoder_cases.py recomputed in int64, and the refusals of
auto_encoder_subspace / auto_inference that need no device.  For the reverse kernels' lists (REVERSE_LATTICE, FORWARD_BIG): every
case exact in int64 with an integer cotangent, what each case reaches computed from the kernels' own constants, and ten faults of
the kernels' decomposition restated in int64, each caught by a named case."""
import numpy as np
import pytest

from subspaceinference_jl_amd import autoencoder as ae
from subspaceinference_jl_amd import flux
from tests import decoder_cases as dc

EPS = 2.0 ** -53
ALL_ACTS = tuple(range(8))
SMOOTH = (flux.identity, flux.tanh, flux.sigmoid, flux.softplus)


def _plain(table, wdec, z):
    """W a + b per layer with NumPy's own matrix product"""
    a = np.asarray(z, dtype=np.float64)
    for fin, fout, act, w_off, b_off in table:
        w = np.asarray(wdec[w_off:w_off + fin * fout], dtype=np.float64).reshape((fout, fin), order="F")
        a = flux._act_fwd(w @ a + np.asarray(wdec[b_off:b_off + fout], dtype=np.float64), act)
    return a


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("act", ALL_ACTS)
def test_decode_is_the_per_layer_evaluation(act, dtype):
    table, wdec = dc.random_decoder((3, 6, 4, 11), (act, flux.tanh, act), seed=act, dtype=dtype)
    rng = np.random.default_rng(5)
    z = rng.standard_normal(3)
    y = ae.decode(table, wdec, z)
    # the sums differ in order only: n = 6 terms + the bias, values O(1)
    assert y.shape == (11,) and np.allclose(y, _plain(table, wdec, z), rtol=1e-13, atol=1e-14)
    zs = rng.standard_normal((3, 4))
    ys = ae.decode(table, wdec, zs)
    assert ys.shape == (11, 4)
    for c in range(4):
        assert np.array_equal(ys[:, c], ae.decode(table, wdec, zs[:, c]))          # a point's bits do not depend on its column
    w_swa = rng.standard_normal(11)
    assert np.array_equal(ae.weights(w_swa, table, wdec, zs), w_swa[:, None] + ys)


def _abs_jvp(table, wdec, z, adz):
    """the same product on absolute values: a bound on the sum of |terms| of every nested sum"""
    outs = ae._forward(table, wdec, z)
    t = np.abs(adz)
    for (w, _, act), a in zip(ae._layers(table, wdec), outs[1:]):
        t = np.abs(ae.dact_from_output(a, act)) * (np.abs(w) @ t)
    return t


@pytest.mark.parametrize("act", ALL_ACTS)
def test_adjoint_identity(act):
    widths = (5, 17, 9, 40)
    table, wdec = dc.random_decoder(widths, (act, flux.sigmoid, act), seed=20 + act)
    rng = np.random.default_rng(act)
    z, dz, gy = rng.standard_normal(5), rng.standard_normal(5), rng.standard_normal(40)
    lhs = float(gy @ ae.decode_jvp(table, wdec, z, dz))
    rhs = float(ae.decode_vjp(table, wdec, z, gy) @ dz)
    # both sides are the same multilinear form summed in two orders: the fp64 dot-product bound (n + 2) eps sum|terms| with n the
    # longest sum (the widest layer) and sum|terms| the form evaluated on absolute values
    n = max(widths)
    bound = (n + 2) * np.finfo(np.float64).eps * float(np.abs(gy) @ _abs_jvp(table, wdec, z, dz))
    print("adjoint identity, act %d: |lhs - rhs| = %.3e, bound %.3e" % (act, abs(lhs - rhs), bound))
    assert abs(lhs - rhs) <= bound


@pytest.mark.parametrize("act", SMOOTH)
def test_jvp_against_central_differences(act):
    table, wdec = dc.random_decoder((4, 7, 12), (act, act), seed=40 + act)
    rng = np.random.default_rng(act)
    z, dz = rng.standard_normal(4), rng.standard_normal(4)
    dz /= np.linalg.norm(dz)
    h = 1e-6
    fd = (ae.decode(table, wdec, z + h * dz) - ae.decode(table, wdec, z - h * dz)) / (2.0 * h)
    err = float(np.max(np.abs(fd - ae.decode_jvp(table, wdec, z, dz))))
    print("central differences, act %d: max error %.3e" % (act, err))
    assert err <= 1e-7      # truncation ~1e-12, rounding ~1e-10


@pytest.mark.parametrize("case", dc.LATTICE, ids=lambda c: c.name)
def test_lattice_cases_are_exact(case):
    """every sum of the case is an integer: `decode` in fp64 equals the int64 evaluation, in both storage types"""
    wdec_i, z_i = dc.lattice_ints(case)
    assert case.widths[-1] == case.n and set(case.acts) <= {dc.I, dc.R}
    for dtype in (np.float32, np.float64):
        table, wdec, z = dc.lattice_decoder(case, dtype)
        assert np.array_equal(wdec.astype(np.int64), wdec_i) and np.array_equal(z.astype(np.int64), z_i)
        ref = dc.int_decode(table, wdec_i, z_i)
        assert np.max(np.abs(ref)) < 2 ** 40
        y = ae.decode(table, wdec, z)
        assert np.array_equal(y, ref.astype(np.float64))
        pb = dc.problem(case.n, lattice=True)
        assert np.array_equal(ae.weights(pb.w_swa, table, wdec, z), (pb.w_swa.astype(np.int64)[:, None] + ref).astype(np.float64))
        for c in range(z.shape[1]):
            gy = np.arange(case.n, dtype=np.float64) % 5 - 2.0          # integer cotangent: the pull-back is exact too
            g = ae.decode_vjp(table, wdec, z[:, c], gy)
            assert np.array_equal(g, np.round(g))


def test_the_list_covers_what_the_issue_names():
    assert {c.depth for c in dc.LATTICE} == {1, 2, 3}
    assert {c.m for c in dc.LATTICE} == {1, 2, 5}
    assert {c.widths[-2] for c in dc.LATTICE if c.depth > 1} == {1, 3, 4, 17}
    assert {c.n for c in dc.LATTICE} == set(dc.MODELS) == {7, 65, 129, 682}
    assert all(dc.MODELS[n][2] <= 64 for n in dc.MODELS)
    for depth in (2, 3):
        assert {(c.widths[-2], c.m) for c in dc.LATTICE if c.depth == depth} == {(h, m) for h in (1, 3, 4, 17) for m in (1, 2, 5)}


# ---- the reverse kernels' case lists (tests/test_gpu_decoder_reverse.py) ------------------------------------------------------------
def _abs_bounds(table, wdec_i, z_i, gy_i):
    """bounds on every partial sum, in whatever order it is taken: the forward and the pull-back evaluated on absolute values"""
    layers = list(dc._int_layers(table, wdec_i))
    a, worst = np.abs(z_i), 0
    for w, b, _ in layers:
        a = np.abs(w) @ a + np.abs(b)[:, None]
        worst = max(worst, int(a.max()))
    fwd, g = worst, np.abs(gy_i)
    for w, _, _ in reversed(layers):
        g = np.abs(w).T @ g
        worst = max(worst, int(g.max()))
    return fwd, worst


@pytest.mark.parametrize("case", dc.REVERSE_LATTICE, ids=lambda c: c.name)
def test_reverse_cases_are_exact(case):
    """every sum of `decode` and of `decode_vjp` with the integer cotangent is an integer below 2^40 in any order: the definition in
    fp64 equals the int64 evaluation in both storage types, and so does the kernels' decomposition restated in int64 (emulate_*).
    On the N_STRIDE and N_GRID models the definition's row-by-row pull-back is left out (a Python loop over N): int64 alone."""
    k = dc.kernel_constants()
    wdec_i, z_i = dc.lattice_ints(case)
    gy_i = dc.lattice_cotangent(case)
    table, _ = dc.decoder_table(case.widths, case.acts)
    assert case.widths[-1] == case.n == dc.case_problem(case).n and set(case.acts) <= {dc.I, dc.R}
    assert np.abs(wdec_i).max() <= 2 and np.abs(z_i).max() <= 3 and np.abs(gy_i).max() <= 2
    points = dc.reverse_points(case)
    assert len(set(points)) == 3
    fwd_bound, bound = _abs_bounds(table, wdec_i, z_i, gy_i)            # (every column of Z; the pull-back's bound needs no mask)
    assert bound < 2 ** 40
    print("%s: forward sums <= %.3g, all sums <= %.3g" % (case.name, fwd_bound, bound))
    ref_y = dc.int_decode(table, wdec_i, z_i[:, :3])
    ref_g = {c: dc.int_decode_vjp(table, wdec_i, z_i[:, c], gy_i) for c in points}
    for c in points:
        assert np.array_equal(dc.emulate_vjp(table, wdec_i, z_i[:, c], gy_i, k), ref_g[c])
    assert np.array_equal(dc.emulate_decode(table, wdec_i, z_i[:, 0], k), ref_y[:, 0])
    w_swa = dc.case_problem(case).w_swa
    assert np.array_equal(w_swa, np.round(w_swa)) and np.abs(w_swa).max() <= 4
    for dtype in (np.float32, np.float64):
        _, wdec, z = dc.lattice_decoder(case, dtype)
        assert np.array_equal(wdec.astype(np.int64), wdec_i) and np.array_equal(z.astype(np.int64), z_i)
        assert np.array_equal(ae.decode(table, wdec, z[:, :3]), ref_y.astype(np.float64))
        if case.model in ("N_STRIDE", "N_GRID"):
            continue
        for c in points:
            assert np.array_equal(ae.decode_vjp(table, wdec, z[:, c], gy_i.astype(np.float64)), ref_g[c].astype(np.float64))


def test_reverse_points_differ_in_a_relu_mask():
    for case in dc.REVERSE_LATTICE:
        if dc.R not in case.acts:
            continue
        table, _ = dc.decoder_table(case.widths, case.acts)
        wdec_i, z_i = dc.lattice_ints(case)
        masks = [dc.relu_masks(table, wdec_i, z_i[:, c]) for c in dc.reverse_points(case)]
        if case in dc.LATTICE and np.array_equal(masks[0], masks[1]):      # (that list's seeds are fixed: D3-H1-M1-N682's one unit is off
            assert all(np.array_equal(dc.relu_masks(table, wdec_i, z_i[:, c]), masks[0]) for c in range(z_i.shape[1])), case.name
            continue                                                           # at all nine points)
        assert not np.array_equal(masks[0], masks[1]), case.name


def test_the_reverse_list_reaches_what_the_issue_names():
    """computed from N, H and the widths with the kernels' own constants, read out of the sources"""
    k = dc.kernel_constants()
    assert (k.blocks, k.threads, k.wave, k.ht, k.maxw, k.max_layers, k.grid_per_cu, k.chunk) == (1024, 256, 64, 4, 1024, 8, 8, 16384)
    assert [c.name for c in dc.REVERSE_LATTICE[:len(dc.LATTICE)]] == [c.name for c in dc.LATTICE]
    assert len({c.name for c in dc.REVERSE_LATTICE}) == len(dc.REVERSE_LATTICE)
    new = dc.REVERSE_LATTICE[len(dc.LATTICE):]
    rc = {c.name: dc.reach(c, k) for c in new}
    assert all(dc.reach(c, k)["per"] == 2 for c in dc.LATTICE)           # the premise: two lanes of wave 0 is all LATTICE reaches
    assert [dc.big_n(m) for m in ("N_2WAVE", "N_STRIDE", "N_GRID")] == [69615, 269636, 1098800]
    assert all(dc.BIG_MODELS[m][2] == 4 for m in dc.BIG_MODELS)
    # the last layer's reverse: rows on two waves, on all four, a second pass of r += 256, a clipped block and an empty one
    assert (rc["R-2WAVE-H5"]["per"], rc["R-2WAVE-H5"]["waves"], rc["R-2WAVE-H5"]["passes"]) == (68, 2, 1)
    for name in ("R-STRIDE-H9", "R-STRIDE-D1-M5"):
        r = rc[name]
        assert (r["per"], r["waves"], r["passes"]) == (264, k.threads // k.wave, 2) and r["clipped"] and r["empty"] >= 1
        assert r["blocks_with_rows"] > k.threads                           # the final kernel's own stride loop runs on non-zero partials
    assert rc["R-GRID-H2"]["passes"] > 2 and rc["R-GRID-H2"]["blocks_with_rows"] == k.blocks
    # h0 rounds 1, 2 and 3, each with and without a tail (3 without: the 64 rounds of H = 256), and a partial round alone
    on129 = {(rc["R-H%d-N129" % h]["rounds"], rc["R-H%d-N129" % h]["tail"]) for h in (1, 3, 4, 5, 8, 9)}
    assert on129 == {(1, 1), (1, 3), (1, 0), (2, 1), (2, 0), (3, 1)}
    assert (rc["R-STRIDE-H9"]["rounds"], rc["R-STRIDE-H9"]["tail"]) == (3, 1) and (rc["R-2WAVE-H5"]["rounds"], rc["R-2WAVE-H5"]["tail"]) == (2, 1)
    assert (rc["R-STRIDE-D1-M5"]["depth"], rc["R-STRIDE-D1-M5"]["m"], rc["R-STRIDE-D1-M5"]["rounds"]) == (1, 5, 2)
    assert rc["W-5-256"]["rounds"] >= 3 and rc["W-5-256"]["tail"] == 0
    # the head: widths below, at and above the thread count, at DEC_MAXW, M above the thread count, the deepest decoder
    heads = {w for c in dc.HEAD_CASES for w in c.widths[1:-1]}
    assert {k.threads - 1, k.threads, k.threads + 1, k.maxw} <= heads
    assert {c.m for c in dc.HEAD_CASES} >= {k.threads + 1, k.maxw} and max(c.depth for c in dc.HEAD_CASES) == k.max_layers
    both = [c for c in dc.HEAD_CASES if dc.R in c.acts[:-1] and c.acts[-1] == dc.R]
    assert 2 * len(both) >= len(dc.HEAD_CASES)
    # the forward: a second pass of the grid-stride loop on a 256-CU card; nothing below N_GRID has one
    assert dc.forward_passes(dc.big_n("N_GRID"), k, dc.MI355X_CUS) == 2
    assert all(dc.forward_passes(c.n, k, dc.MI355X_CUS) == 1 for c in dc.REVERSE_LATTICE if c.name != dc.GRID_CASE)
    assert [c.name for c in dc.FORWARD_BIG] == [c.name for c in dc.HEAD_CASES] + [dc.GRID_CASE] and dc.FORWARD_BIG_POINTS == (1, 3)


# every fault, restated in int64 (decoder_cases.emulate_vjp / emulate_decode), changes the result of the case named here -- on the
# reference alone: the lists would catch a device that has it.  No case needed another seed (LatticeCase.salt) for that.
MUTANT_CAUGHT_BY = {
    "lanes_from_64_dropped": "R-2WAVE-H5",
    "rows_from_r0_plus_256_dropped": "R-STRIDE-H9",
    "last_h0_round_dropped": "R-H8-N129",
    "tail_columns_dropped": "R-H5-N129",
    "stale_wave_sums": "R-STRIDE-H9",
    "head_outputs_from_256_dropped": "W-2-257",
    "head_inputs_from_256_dropped": "W-257-255",
    "block_partials_from_256_dropped": "R-2WAVE-H5",
    "pairs_beyond_the_grid_dropped": dc.GRID_CASE,
    "relu_mask_of_the_wrong_layer": "W-D8",
}


@pytest.mark.parametrize("mutant", dc.MUTANTS)
def test_the_lists_catch_every_mutant(mutant):
    assert set(MUTANT_CAUGHT_BY) == set(dc.MUTANTS)
    k = dc.kernel_constants()
    case = dc.REVERSE_BY_NAME[MUTANT_CAUGHT_BY[mutant]]
    table, _ = dc.decoder_table(case.widths, case.acts)
    wdec_i, z_i = dc.lattice_ints(case)
    gy_i = dc.lattice_cotangent(case)
    caught = []
    if mutant != "pairs_beyond_the_grid_dropped":
        assert case in dc.REVERSE_LATTICE
        caught += [c for c in dc.reverse_points(case)
                   if not np.array_equal(dc.emulate_vjp(table, wdec_i, z_i[:, c], gy_i, k, mutant), dc.int_decode_vjp(table, wdec_i, z_i[:, c], gy_i))]
        assert caught, "the pull-back of %s does not separate %s" % (case.name, mutant)
    if mutant in dc.FORWARD_MUTANTS:
        assert case in dc.FORWARD_BIG
        fwd = [c for c in range(max(dc.FORWARD_BIG_POINTS))
               if not np.array_equal(dc.emulate_decode(table, wdec_i, z_i[:, c], k, mutant), dc.int_decode(table, wdec_i, z_i[:, c]))]
        assert fwd, "the forward of %s does not separate %s" % (case.name, mutant)
    print("%s: caught by %s at points %s" % (mutant, case.name, caught))


def test_check_table_refusals():
    table, wdec = dc.random_decoder((3, 4, 9), (flux.tanh, flux.identity), seed=1)
    assert ae.check_table(table, wdec, 3, 9) == (3, 9)
    for bad_table, bad_w, m, n, what in (
            (table, wdec, 2, 9, "M = 2"),
            (table, wdec, 3, 8, "8 parameters"),
            ([table[0], (5,) + table[1][1:]], wdec, None, None, "do not chain"),
            ([table[0], table[1][:4] + (wdec.size - 1,)], wdec, None, None, "offset range"),
            ([table[0][:2] + (8,) + table[0][3:], table[1]], wdec, None, None, "unknown activation"),
            (table, wdec.astype(np.float16), None, None, "Float32 or Float64"),
            ([("flatten", 1, (1, 1))], wdec, None, None, "must be Dense")):
        with pytest.raises(ae.SubspaceError, match=what):
            ae.check_table(bad_table, bad_w, m, n)


def test_api_argument_errors(si):
    m = flux.Chain(flux.Dense(3, 2))                       # N = 8
    data = flux.DataLoader(np.zeros((3, 4)), np.zeros((2, 4)))
    dec = flux.Chain(flux.Dense(2, 4, flux.tanh), flux.Dense(4, 8))
    enc = flux.Chain(flux.Dense(8, 4, flux.tanh), flux.Dense(4, 2))
    w = np.zeros(8)
    with pytest.raises(si.SubspaceError, match="DimensionMismatch: the decoder takes 2 inputs but M = 3"):
        si.auto_inference(m, data, dec, w, M=3)
    with pytest.raises(si.SubspaceError, match="DimensionMismatch: the decoder returns 7 values"):
        si.auto_inference(m, data, flux.Chain(flux.Dense(2, 7)), w, M=2)
    with pytest.raises(si.SubspaceError, match="DimensionMismatch: W_swa"):
        si.auto_inference(m, data, dec, np.zeros(9), M=2)
    with pytest.raises(si.SubspaceError, match="Chain of Dense layers"):
        si.auto_inference(m, data, object(), w, M=2)
    with pytest.raises(si.SubspaceError, match="not avaliable"):
        si.auto_inference(object(), data, dec, w, M=2)                              # space_inference.jl:103 [sic]
    with pytest.raises(si.SubspaceError, match="bogus is not available"):
        si.auto_inference(m, data, dec, w, M=2, alg=":bogus")                       # space_inference.jl:316
    with pytest.raises(si.SubspaceError, match="Chain of Dense layers"):
        si.auto_encoder_subspace(m, flux.mse, data, flux.Descent(), object(), dec)
    with pytest.raises(si.SubspaceError, match="DimensionMismatch: the encoder takes 7 inputs"):
        si.auto_encoder_subspace(m, flux.mse, data, flux.Descent(), flux.Chain(flux.Dense(7, 2)), dec)
    with pytest.raises(si.SubspaceError, match="DimensionMismatch: the encoder returns 3 values but the decoder takes 2"):
        si.auto_encoder_subspace(m, flux.mse, data, flux.Descent(), flux.Chain(flux.Dense(8, 3)), dec)
    with pytest.raises(si.SubspaceError, match="BoundsError: no snapshot"):
        si.auto_encoder_subspace(m, flux.mse, data, flux.Descent(), enc, dec, T=1, c=2)
    # the reference's defaults (src/space_inference.jl:198-200,238-240; src/subspace_construction.jl:93)
    import inspect
    sig = inspect.signature(si.auto_inference).parameters
    assert [sig[k].default for k in ("σ_z", "σ_m", "σ_p", "itr", "M", "alg", "backend")] == [1.0, 1.0, 1.0, 100, 3, "hmc", "forwarddiff"]
    sig = inspect.signature(si.autoencoder_inference).parameters
    assert [sig[k].default for k in ("itr", "T", "c", "M", "print_freq", "alg")] == [1000, 25, 1, 20, 1, "hmc"]
    sig = inspect.signature(si.auto_encoder_subspace).parameters
    assert [sig[k].default for k in ("T", "c", "M", "print_freq", "include_penalty")] == [10, 1, 3, 1, False]


def test_binding_declares_the_decoder_entry_points(si):
    import ctypes
    lib = si.load()
    for name in ("si_infer_set_decoder", "si_infer_decoder_info", "si_decode"):
        assert name in si._capi.SIGNATURES and hasattr(lib, name)
    d = ctypes.c_int32(7)
    assert lib.si_infer_decoder_info(None, ctypes.byref(d), None, None) == si._capi.SI_ERR_INVALID   # (a NULL ctx is refused, not read)
    assert lib.si_decode(None, None, 1, None) == si._capi.SI_ERR_INVALID
    for f in (si.Context.set_decoder, si.Context.decoder_info, si.Context.decode):
        assert f.__doc__


def test_binding_declares_the_cotangent_entry_point(si):
    lib = si.load()
    assert "si_decode_vjp" in si._capi.SIGNATURES and hasattr(lib, "si_decode_vjp")
    assert lib.si_decode_vjp(None, None, None, None) == si._capi.SI_ERR_INVALID
    assert si.Context.decode_vjp.__doc__ and lib.si_version() == 500
