"""CPU side of tests/test_norm_edges_gpu.py: its case builders produce what they say (shapes past the grid caps, sums below 2^24,
which width takes which launch form), its float64 references agree with torch's own autograd, the one conditioning choice it makes
(x on a finer grid for one or two pixels per group) is measured with torch in float32, its checkers turn red on a planted error,
and the BatchNorm entry points refuse the same group counts."""
import ctypes

import pytest
import torch

import _norm_cases as E
from _bounds import tol
from _norm_cases import F32, BF16


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp(min=1e-30))


def test_shapes_pass_the_grid_caps_they_are_meant_to_pass():
    for dtype, C, G, npix in E.HOIST_LARGE:
        assert E.hoisted(dtype, C) and npix % G == 0
        gvec = npix // G * C // E.V[dtype]
        assert gvec > 2 * (E.HOIST_WG // G) * E.BLOCK                  # more than one trip of two pieces per thread
        assert E.hoist_trips(dtype, C, G, npix) == ((2 if G == 2 else 1), True)
        assert npix * C // E.V[dtype] == (2 if G == 2 else 1) * 1048768
    for dtype, C, G, npix in E.GENERIC_LARGE:
        assert not E.hoisted(dtype, C) and npix % G == 0 and C % E.V[dtype] == 0
        assert E.EW_WG * E.BLOCK < npix * C // E.V[dtype] < E.EW_WG * E.BLOCK + 64      # the second pass holds a few pieces
    dtype, C, G, npix = E.BWD_LARGE
    assert E.hoist_trips(dtype, C, G, npix) == (1, True) and npix // G * C // E.V[dtype] == 524384
    # small apply shapes: at <= 256 pieces the hoisted loop is skipped, above it entered
    for dtype in E.DTYPES:
        for C in (32, 64, 24, 48, 96):
            pieces = [P * E.pieces_per_pixel(dtype, C) for P in E.apply_pixel_counts(dtype, C)]
            assert min(pieces) == E.pieces_per_pixel(dtype, C)
            assert any(p <= 256 for p in pieces[1:]) and any(256 < p <= 512 for p in pieces) and any(p > 512 for p in pieces)
            if 256 % E.pieces_per_pixel(dtype, C) == 0:
                assert 256 in pieces
    # the backward's chunks: fewer pixels than chunks, chunk = 1 up to bpg pixels, 2 from bpg + 1
    for G in (1, 2, 4):
        bpg = E.BWD_CHUNKS // G
        assert E.bwd_pixel_counts(G) == [1, 2, bpg - 1, bpg, bpg + 1, 1200]
        assert -(-(bpg + 1) // bpg) == 2 and -(-1200 // bpg) == (2 if G == 1 else 3 if G == 2 else 5)
    # bn_finalize: tiles per group around its step 64 wpg and twice that, for every layout
    for G in (1, 2, 4):
        step = E.WAVE * (E.FIN_WAVES // G)
        for edge in (step, 2 * step):
            assert {edge - 1, edge, edge + 1} <= set(E.FIN_TILES)
    assert E.finalize_case(2, 1)["count"] == 1
    # LayerNorm: 49189 rows = three strides of the backward's grid plus a partial group; 1001 rows end inside a wavefront
    stride = E.LN_BWD_WG * E.LN_BWD_ROWS
    assert stride == 16384 and max(E.LN_ROWS) == 3 * stride + 37 and 37 % E.LN_BWD_ROWS != 0
    assert 1001 % E.LN_ROWS_PER_WAVE != 0 and 1000 % E.LN_ROWS_PER_WAVE == 0
    # reduce_partials: below, at and above its 8 phases and the unrolled loop's 32 rows
    assert {E.RED_PHASES - 1, E.RED_PHASES, E.RED_PHASES + 1, 31, 32, 33} <= set(E.RED_NT)


def test_integer_sums_stay_exact_in_float32():
    assert E.IMAX * 20001 == 160008 < E.EXACT_LIMIT
    assert E.IMAX * (max(E.COLSUM_P) + 1) < E.EXACT_LIMIT and E.IMAX * max(E.LN_ROWS) < E.EXACT_LIMIT
    assert E.IMAX * E.BWD_LARGE[3] < E.EXACT_LIMIT and E.IMAX * 4 * 1200 < E.EXACT_LIMIT
    with pytest.raises(AssertionError):
        E.ints((2, 2), E.gen(0), 1 << 21)
    x, before = E.colsum_case(BF16, 12, 255)
    assert bool((x == x.round()).all()) and float(x.abs().max()) == 8 and bool((E.rounded(x, BF16) == x).all())
    c = E.finalize_case(4, 300)
    s = c["partial"][:, E.FIN_INT].double()
    assert bool((s == s.round()).all()) and float(s.abs().sum(-1).max()) < E.EXACT_LIMIT
    assert bool(torch.isnan(c["partial"][:, E.FIN_C:]).all())
    c = E.bn_bwd_case(BF16, 32, 2, 511)
    assert bool((c["dout"] == c["dout"].round()).all()) and float((c["out"] == 0).double().mean()) > 0.4
    pre = c["x"].float() * c["ms"][:, None] + c["mh"][:, None]                # float32, as the kernel forms it
    assert bool((pre.double() == c["x"] * c["ms"].double()[:, None] + c["mh"].double()[:, None]).all())
    assert int((pre == 0).sum()) > 10 and 0.2 < float((pre > 0).double().mean()) < 0.8


def test_which_width_takes_which_form():
    assert [C for C in (24, 32, 48, 64, 96) if not E.hoisted(F32, C)] == [24, 48, 96]
    assert [C for C in (24, 32, 48, 64, 96) if not E.hoisted(BF16, C)] == [24, 48, 96]
    assert all(E.hoisted(BF16, C) for C in (8, 32, 512, 2048)) and all(E.hoisted(F32, C) for C in (4, 64, 1024))
    assert [C for C in E.COLSUM_C if E.colsum_vector_form(F32, C)] == [4, 8, 32, 64, 256]
    assert [C for C in E.COLSUM_C if E.colsum_vector_form(BF16, C)] == [8, 32, 64, 256]
    assert [C for C in E.COLSUM_C if 256 // C == 1] == [129, 200, 256]        # a single row phase in the scalar form
    assert [C for C in E.COLSUM_C if 256 % C] == [3, 12, 24, 48, 129, 200]    # idle lanes in the scalar form


def test_mask_bytes_are_packed_as_relu_mask_byte_states():
    y = torch.tensor([1.0, 0.0, -1.0, 2.0, 0.0, 0.0, 0.0, 3.0])
    assert E.pack_mask(y > 0, 4).tolist() == [0b1001, 0b1000] and E.pack_mask(y > 0, 8).tolist() == [0b10001001]


def test_written_out_references_agree_with_torch_autograd():
    c = E.bn_bwd_case(F32, 8, 2, 77)
    mean, invstd = E.bn_stats(c["x"])
    for mask in E.MASKS:
        dy = E.bn_bwd_dy(c, mask)
        dx, dg, db = E.bn_bwd_formula(c["x"], dy, mean, invstd, c["gamma"].double())
        adx, adg, adb = E.bn_autograd(c["x"], dy, c["gamma"])
        assert rel(dx, adx) < 1e-11 and rel(dg, adg) < 1e-11 and rel(db, adb) < 1e-11
    assert rel(c["mean"], mean) < 2.0 ** -23 and rel(c["invstd"], invstd) < 2.0 ** -23
    a = E.bn_apply_case(BF16, 24, 2, 43)       # its scale / shift are those of F.batch_norm in train mode, rounded to float32
    for k in range(2):
        y = torch.nn.functional.batch_norm(a["x"][k].t().reshape(1, 24, 43), None, None, a["gamma"].double(), a["beta"].double(), True)
        assert rel(E.bn_apply_ref(a, False, False)[k], y.reshape(24, 43).t()) < 1e-6
    assert bool((E.bn_apply_ref(a, True, True) == (E.bn_apply_ref(a, False, False) + a["res"]).clamp(min=0)).all())
    for dtype, rows in ((F32, 33), (BF16, 1001)):
        c = E.ln_case(dtype, rows)
        for eps in (1e-5, 1e-3):
            wy, st = E.ln_fwd_ref(c, eps)
            dx, dg, db = E.ln_bwd_formula(c["x"], c["dy"], st, c["gamma"].double())
            ay, adx, adg, adb = E.ln_autograd(c["x"], c["dy"], c["gamma"], c["beta"], float(torch.tensor(eps, dtype=F32)))
            assert rel(wy, ay) < 1e-11 and rel(dx, adx) < 1e-9 and rel(dg, adg) < 1e-11 and rel(db, adb) < 1e-12
        const, offset = E.ln_special_rows(rows)
        assert float(c["x"][const[0]].std()) == 0.0
        for r in offset:
            assert 50 < float(c["x"][r].mean() / c["x"][r].std()) < 200


def test_finalize_reference_is_torch_batchnorm_on_the_same_pixels():
    """float64 of the float32 partials against F.batch_norm on x itself, groups in order: the partials' rounding (2^-24 per tile) is all
    that separates them; on the constant channel 19 the unclamped variance is negative in every group, so the clamp decides invstd"""
    negative = 0
    for G, tpg in ((1, 65), (2, 129), (4, 300), (4, 63)):
        c = E.finalize_case(G, tpg)
        want = E.finalize_ref(c, 0.1, 1e-5)
        raw = E.finalize_ref(c, 0.1, 1e-5, clamp=False)
        negative += int((raw["var"][:, 19] < 0).all())
        assert rel(raw["invstd"][:, 19], want["invstd"][:, 19]) > 10 * tol(F32)      # a missing clamp would not pass the GPU test's bound
        rm, rv = c["rm"].double().clone(), c["rv"].double().clone()
        m = float(torch.tensor(0.1, dtype=F32))
        for k in range(G):
            torch.nn.functional.batch_norm(c["x"][k].t().reshape(1, E.FIN_C, -1), rm, rv, None, None, True, m, 1e-5)
        mean, invstd = E.bn_stats(c["x"], float(torch.tensor(1e-5, dtype=F32)))
        real = [k for k in range(E.FIN_C) if k not in E.FIN_CONST]
        assert rel(want["mean"], mean) < 1e-6 and rel(want["invstd"][:, real], invstd[:, real]) < 1e-5
        assert rel(want["rm"], rm) < 1e-6 and rel(want["rv"], rv) < 1e-5
        ratio = c["x"][..., E.FIN_OFFSET].mean(1) / c["x"][..., E.FIN_OFFSET].std(1)
        assert 6 < float(ratio.min()) and float(ratio.max()) < 11
    assert negative == 4
    one = E.finalize_ref(E.finalize_case(2, 1), 0.1, 1e-5)
    assert float(one["var"][:, E.FIN_INT].abs().max()) == 0.0                 # count = 1: var = 0, running_var takes it unscaled


def test_two_pixels_per_group_float32_distance_on_the_coarse_and_the_fine_grid():
    """Why bn_bwd_case puts x on a 256 times finer grid for P <= 2.  torch's float32 BatchNorm backward against its float64 one on two
    pixels per group: dx is (dy1 - dy2) / 2 x eps / (var + eps) x gamma invstd, a difference of O(1) terms that leaves 1e-5 of them at
    var ~ 5.  On the grid the other pixel counts use, float32 itself is 3.2e-3 of max |dx| away -- no float32 kernel meets 4 x 2e-5
    there; on the fine grid (var ~ eps) it is at 1.1e-7, far inside a quarter of that bound, which therefore holds for the kernel."""
    worst = {False: 0.0, True: 0.0}
    for C, G in ((4, 1), (4, 4), (64, 2), (1024, 4)):
        for small in (False, True):
            g = E.gen(9, C, G, small)
            x, _ = E.bn_x(F32, G, 2, C, g, small=small)
            dy = E.ints((G, 2, C), g, 2 * G)
            gamma, _ = E.bn_affine(C, g)
            d64 = E.bn_autograd(x, dy, gamma)[0]
            d32 = E.bn_autograd(x, dy, gamma, dtype=F32)[0]
            worst[small] = max(worst[small], rel(d32, d64))
    print("two pixels per group, float32 torch vs float64 torch, max |dx err| / max |dx|: coarse grid %.3e, fine grid %.3e" % (worst[False], worst[True]))
    assert worst[False] == pytest.approx(3.196e-3, rel=0.05) and worst[False] > 4 * tol(F32)
    assert 4 * worst[True] <= 4 * tol(F32)
    # the builder does use the fine grid there, and only there
    assert float(E.bn_bwd_case(F32, 4, 1, 2)["x"].abs().max()) < 0.02 < float(E.bn_bwd_case(F32, 4, 1, 3)["x"].abs().max())


def test_ordinary_cases_leave_the_stated_factors_in_reach():
    """float32 torch is within a quarter of the stated bound on the well-conditioned cases: BatchNorm dx (factor 4) at the chunk edge,
    LayerNorm y (1) and dx (3) on ordinary rows and on the constant / offset rows"""
    c = E.bn_bwd_case(F32, 64, 2, 513)
    d64 = E.bn_autograd(c["x"], c["dout"], c["gamma"])[0]
    d32 = E.bn_autograd(c["x"], c["dout"], c["gamma"], dtype=F32)[0]
    print("BatchNorm dx, float32 torch vs float64: %.3e of max" % rel(d32, d64))
    assert 4 * rel(d32, d64) <= 4 * tol(F32)
    c = E.ln_case(F32, 1001)
    keep = E.split_rows(1001, c["special"])
    a64 = E.ln_autograd(c["x"], c["dy"], c["gamma"], c["beta"], 1e-5)
    a32 = E.ln_autograd(c["x"], c["dy"], c["gamma"], c["beta"], 1e-5, dtype=F32)
    for idx, label in ((keep, "ordinary"), (~keep, "constant / offset")):
        dy_, dx_ = rel(a32[0][idx], a64[0][idx]), rel(a32[1][idx], a64[1][idx])
        print("LayerNorm %s rows, float32 torch vs float64: y %.3e, dx %.3e of max" % (label, dy_, dx_))
        assert 4 * dy_ <= tol(F32) and 4 * dx_ <= 3 * tol(F32)


def test_checkers_turn_red_on_a_planted_error():
    x, _ = E.colsum_case(F32, 24, 4097)
    want = x.sum(0)
    E.exact(want.float(), want, "column sum")
    with pytest.raises(AssertionError):
        E.exact((want - x[4096]).float(), want, "column sum with the last row dropped")
    with pytest.raises(AssertionError):
        E.exact((want + x[7]).float(), want, "column sum with a row counted twice")
    c = E.bn_bwd_case(F32, 64, 2, 513)
    dx = E.bn_bwd_ref(c, "out_relu")["dx"]
    E.bounded(dx.float(), dx, F32, "dx rounded to float32", factor=4)
    off = dx.clone()
    off[1, 400, 17] += 1e-3 * float(dx.abs().max())
    with pytest.raises(AssertionError):
        E.bounded(off.float(), dx, F32, "dx with one pixel off by 1e-3 of the maximum", factor=4)
    nan = dx.clone()
    nan[0, 0, 0] = float("nan")
    with pytest.raises(AssertionError):
        E.bounded(nan.float(), dx, F32, "dx with a NaN", factor=4)


NULL = None


def _entry_points(L, groups):
    """every BatchNorm entry point that takes a group count, called with `groups` and NO tensors: a refusal comes from the argument
    checks, before anything is launched"""
    mark = ctypes.c_char_p(b"\0" * 16)      # dh_*_bits test their mask pointer first
    return {
        "dh_bn_finalize": lambda: L.dh_bn_finalize(NULL, 4 * groups, 32, 24, groups, 8.0, NULL, NULL, NULL, NULL, 0.1, 1e-5, NULL, NULL, NULL,
                                                   NULL, NULL, NULL),
        "dh_bn_apply": lambda: L.dh_bn_apply(0, NULL, NULL, NULL, NULL, NULL, 4 * groups, 32, groups, 0, NULL),
        "dh_bn_apply_bits": lambda: L.dh_bn_apply_bits(0, NULL, NULL, NULL, NULL, NULL, 4 * groups, 32, groups, 1, mark, NULL),
        "dh_bn_bwd": lambda: L.dh_bn_bwd(0, NULL, NULL, NULL, NULL, NULL, NULL, 4 * groups, 32, groups, NULL, NULL, NULL, NULL, 0, NULL, NULL,
                                         NULL, NULL),
        "dh_bn_bwd_bits": lambda: L.dh_bn_bwd_bits(0, NULL, mark, NULL, NULL, NULL, NULL, 4 * groups, 32, groups, NULL, NULL, NULL, NULL, 0,
                                                   NULL, NULL),
        "dh_bn_bwd_from_partials": lambda: L.dh_bn_bwd_from_partials(0, NULL, NULL, NULL, 4 * groups, NULL, NULL, NULL, 4 * groups, 32, groups,
                                                                     NULL, NULL, NULL, 0, NULL, NULL),
    }


@pytest.mark.parametrize("groups", [3, 5, 8, 0])
def test_batchnorm_entry_points_agree_on_the_group_counts_they_take(groups):
    """1, 2 or 4 statistics groups everywhere: dh_bn_bwd used to take 3 (any count up to 4), which dh_bn_finalize refuses -- no statistics
    could exist for such a call -- and dh_bn_bwd_from_partials any count at all, past the four slots of bn_bwd_finalize_kernel"""
    from dahitra_amd import _lib
    L = _lib.lib()
    for name, call in _entry_points(L, groups).items():
        with pytest.raises(_lib.HipLibraryError, match=r"%s failed: bn_\w+: 1, 2 or 4 statistics groups, got %d" % (name, groups)):
            _lib.check(call(), name)
