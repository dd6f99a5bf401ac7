"""The numpy restatements of the xBD mask morphology (tests/_xbd_morph_cases.py) against scipy.ndimage on every case, shape and
window of the GPU test, the training masks against a literal transcription of xBD_code/train_unettransformer.py:262-273, mutation
checks that show those comparisons can fail, counts pinned so that no comparison passes on empty ground, and what the interface
refuses without a GPU."""
import ctypes

import numpy as np
import pytest
import torch
from scipy import ndimage

import _xbd_match_cases as M
import _xbd_morph_cases as C


def script_masks(msk_hw5):
    """lines 262-273 of the script on one bool [H, W, 5] array, dilation(., square(5)) as binary_dilation with a 5 x 5 square"""
    dilation = lambda a, s: ndimage.binary_dilation(a, structure=s)
    square = lambda k: np.ones((k, k), dtype=bool)
    msk = msk_hw5.copy()
    msk[..., 0] = False
    msk[..., 1] = dilation(msk[..., 1], square(5))
    msk[..., 2] = dilation(msk[..., 2], square(5))
    msk[..., 3] = dilation(msk[..., 3], square(5))
    msk[..., 4] = dilation(msk[..., 4], square(5))
    msk[..., 1][msk[..., 2:].max(axis=2)] = False
    msk[..., 3][msk[..., 2]] = False
    msk[..., 4][msk[..., 2]] = False
    msk[..., 4][msk[..., 3]] = False
    msk[..., 0][msk[..., 1:].max(axis=2)] = True
    msk = msk * 1
    return msk, msk.argmax(axis=2)


@pytest.mark.parametrize("N,H,W", C.SHAPES)
def test_the_window_restatements_equal_scipy(N, H, W):
    for name, a in C.map_cases(N, H, W).items():
        for k in C.KS:
            sq = np.ones((k, k), dtype=bool)
            dil, ero = C.win_or(a, k), C.erode(a, k)
            assert dil.dtype == ero.dtype == np.uint8 and dil.max(initial=0) <= 1
            for n in range(N):
                b = a[n] != 0
                assert np.array_equal(dil[n], ndimage.binary_dilation(b, structure=sq)), (name, k)
                assert np.array_equal(dil[n], ndimage.grey_dilation(b.astype(np.uint8), footprint=sq, mode='reflect')), (name, k)
                assert np.array_equal(ero[n], ndimage.binary_erosion(b, structure=sq, border_value=1)), (name, k)
                assert np.array_equal(C.opening(a, k)[n], ndimage.binary_dilation(ndimage.binary_erosion(b, structure=sq, border_value=1),
                                                                                 structure=sq)), (name, k)
                assert np.array_equal(C.closing(a, k)[n], ndimage.binary_erosion(ndimage.binary_dilation(b, structure=sq), structure=sq,
                                                                                 border_value=1)), (name, k)


def scipy_fill(a, background):
    st = ndimage.generate_binary_structure(2, 1 if background == 4 else 2)
    return np.stack([ndimage.binary_fill_holes(a[n] != 0, structure=st) for n in range(a.shape[0])]).astype(np.uint8)


@pytest.mark.parametrize("N,H,W", C.HOLE_SHAPES)
def test_the_hole_fill_restatement_equals_scipy(N, H, W):
    for name, a in C.hole_cases(N, H, W).items():
        for bg in (4, 8):
            assert np.array_equal(C.fill_holes(a, bg), scipy_fill(a, bg)), (name, bg)


@pytest.mark.parametrize("N,H,W", C.SHAPES)
def test_the_hole_fill_restatement_equals_scipy_on_the_map_cases(N, H, W):
    if H * W > 130 * 70:
        cases = {"checkerboard": C.map_cases(N, H, W)["checkerboard"]}          # the 50 % field of this shape is a hole case
    else:
        cases = C.map_cases(N, H, W)
    for name, a in cases.items():
        for bg in (4, 8):
            assert np.array_equal(C.fill_holes(a, bg), scipy_fill(a, bg)), (name, bg)


@pytest.mark.parametrize("N,H,W", C.SHAPES)
def test_the_training_masks_equal_the_script(N, H, W):
    for name, lbl in C.label_cases(N, H, W).items():
        msk = C.to_msk(lbl)
        assert not (msk[:, 0].astype(bool) & (lbl == 5)).any(), "label 5 sets no channel"
        got = C.msk_dilate(msk, 5)
        for n in range(N):
            want, lbl_msk = script_masks(np.moveaxis(msk[n], 0, 2).astype(bool))
            assert np.array_equal(np.moveaxis(got[n], 0, 2), want), name
            assert not lbl_msk.any(), "msk.argmax is 0 everywhere: the loader's shared zero tensor"
        for k in C.MSK_KS:
            out = C.msk_dilate(msk, k)
            assert not out.argmax(axis=1).any() and out.max(initial=0) <= 1
            assert np.array_equal(out[:, 0], np.maximum.reduce([out[:, c] for c in range(1, 5)]))
            assert (out[:, 1:].sum(axis=1) <= 1).all(), "the four damage channels are disjoint"
            sq = np.ones((k, k), dtype=bool)
            for n in range(N):
                d1, d2, d3, d4 = (ndimage.binary_dilation(lbl[n] == c, structure=sq) for c in range(1, 5))
                want = [d1 | d2 | d3 | d4, d1 & ~(d2 | d3 | d4), d2, d3 & ~d2, d4 & ~d2 & ~d3]
                assert np.array_equal(out[n], np.stack(want).astype(np.uint8)), (name, k)


def test_clean_footprint_restatement_is_open_close_fill():
    a = C.noise(1, 70, 130, 500)
    sq = np.ones((3, 3), dtype=bool)
    o = ndimage.binary_dilation(ndimage.binary_erosion(a[0] != 0, structure=sq, border_value=1), structure=sq)
    c = ndimage.binary_erosion(ndimage.binary_dilation(o, structure=sq), structure=sq, border_value=1)
    f = ndimage.binary_fill_holes(c)
    assert np.array_equal(C.clean_footprint(a, 3, 3, True)[0], f)
    assert np.array_equal(C.clean_footprint(a, 3, 0, False)[0], o)
    assert np.array_equal(C.clean_footprint(a)[0], a[0] != 0) and C.clean_footprint(a).dtype == np.uint8
    assert not np.array_equal(C.clean_footprint(a, 3, 3, True), C.closing(C.opening(C.fill_holes(a), 3), 3)), "the order matters"


def test_the_comparisons_catch_wrong_restatements():
    N, H, W = 1, 70, 130
    maps, holes, labels = C.map_cases(N, H, W), C.hole_cases(N, H, W), C.label_cases(N, H, W)
    # the window one column off centre: the single points tell
    assert not np.array_equal(C.win_or(maps["points"], 3, mutate="offcentre"), C.win_or(maps["points"], 3))
    assert np.array_equal(C.win_or(maps["ones"], 3, mutate="offcentre")[:, :, :-1], C.win_or(maps["ones"], 3)[:, :, :-1])
    # border_value = 0: the all-set image loses its rim; it does not under the convention of the kernel
    assert C.erode(maps["ones"], 5).all() and not C.erode(maps["ones"], 5, mutate="border0").all()
    assert not np.array_equal(C.erode(maps["pits"], 3, mutate="border0"), C.erode(maps["pits"], 3))
    # classes 3 and 4 swapped: the rectangles of that pair overlap
    msk = C.to_msk(labels["rects"])
    for k in C.MSK_KS:
        assert not np.array_equal(C.msk_dilate(msk, k, mutate="swap34"), C.msk_dilate(msk, k)), k
    # the left border ignored: the ring cut by column 0 fills
    assert not np.array_equal(C.fill_holes(holes["ring_left"], 4, mutate="noleft"), C.fill_holes(holes["ring_left"], 4))
    # the wrong background connectivity: the diagonal leak
    for bg in (4, 8):
        assert not np.array_equal(C.fill_holes(holes["ring_diag"], bg, mutate="conn"), C.fill_holes(holes["ring_diag"], bg)), bg
    assert set(C.MUTANTS) == {"offcentre", "border0", "swap34", "noleft", "conn"}


def filled(a, bg):
    return int(C.fill_holes(a, bg).sum()) - int((a != 0).sum())


def test_the_named_cases_are_not_empty_ground():
    N, H, W = 1, 70, 130
    holes = C.hole_cases(N, H, W)
    inside = (H - 8) * (W - 8)                                  # the pixels inside the ring at inset 3
    assert filled(holes["ring"], 4) == filled(holes["ring"], 8) == inside == 62 * 122
    inner = 2 * (H - 16) + 2 * (W - 16) - 4
    assert filled(holes["ring_in_ring"], 4) == filled(holes["ring_in_ring"], 8) == inside - inner
    assert filled(holes["ring_open"], 4) == filled(holes["ring_open"], 8) == 0
    assert filled(holes["ring_diag"], 4) == inside and filled(holes["ring_diag"], 8) == 0
    assert filled(holes["ring_left"], 4) == filled(holes["ring_left"], 8) == 0
    assert int((holes["ring_left"][:, 4:H - 4, 0] == 0).all()) == 1, "the cut ring's hole owns pixels of column 0"
    assert filled(holes["spiral_open"], 4) == filled(holes["spiral_open"], 8) == 0
    walls = int(holes["spiral_closed"].sum())
    assert filled(holes["spiral_closed"], 4) == filled(holes["spiral_closed"], 8) == (H - 4) * (W - 4) - walls
    assert (H - 4) * (W - 4) - walls == 4156, "the corridor and the core of the spiral"
    # the corridor is ONE component that runs round every ring: its 4-connected complement has the outside and nothing else
    lab, cnt = C.B.cc_label((holes["spiral_open"] == 0).astype(np.uint8), 4, False)
    assert cnt.tolist() == [1]
    # thousands of holes-to-be in the noisy complement: no table of a few thousand rows would do
    big = C.noise(1, 256, 256, 500)
    comps4 = ndimage.label(big[0] == 0)[1]
    assert comps4 > 4096 and filled(big, 4) > 1000 and filled(big, 8) > 100 and filled(big, 4) > filled(big, 8)
    # the dilation adds pixels and the priority rule takes pixels away
    maps = C.map_cases(N, H, W)
    assert int(C.win_or(maps["points"], 5).sum()) - 9 == 4 * 9 + 4 * 15 + 25 - 9
    assert int(C.erode(maps["pits"], 5).sum()) == H * W - (4 * 9 + 4 * 15 + 25)
    assert int(C.win_or(maps["noise0.5"], 3).sum()) > 5 * int((maps["noise0.5"] != 0).sum())
    for name, lbl in C.label_cases(N, H, W).items():
        msk = C.to_msk(lbl)
        for k in C.MSK_KS:
            out = C.msk_dilate(msk, k)
            plain = np.stack([C.win_or(msk[:, c], k) for c in range(1, 5)], axis=1)
            added = int(plain.sum()) - int(msk[:, 1:].sum())
            taken = int(plain.sum()) - int(out[:, 1:].sum())
            assert added > 0 and taken > 0, (name, k)
            if name == "rects":                                 # every priority pair loses pixels somewhere
                for hi, lo in C.PRIORITY_PAIRS:
                    assert (plain[:, lo - 1].astype(bool) & plain[:, hi - 1].astype(bool) & ~out[:, lo].astype(bool)).any(), (k, hi, lo)
    out = C.msk_dilate(C.to_msk(C.rects(N, H, W)), 5)
    plain = np.stack([C.win_or(C.to_msk(C.rects(N, H, W))[:, c], 5) for c in range(1, 5)], axis=1)
    # 48 rectangles of 9 pixels; their 7 x 7 dilations overlap, 2231 pixels over the four channels, of which the rule takes 467
    assert (int(C.to_msk(C.rects(N, H, W))[:, 1:].sum()), int(plain.sum()), int(out[:, 1:].sum())) == (432, 2231, 1764)


def test_the_cleaned_footprint_matches_two_buildings_and_the_raw_one_none():
    fp, gt = C.bridged_squares()
    clean = C.clean_footprint(fp, open=3, fill=True)
    assert np.array_equal(clean, (gt != 0).astype(np.uint8))
    assert M.building_match(clean * 2, gt)["loc"].tolist() == [2, 0, 0]
    assert M.building_match(fp * 2, gt)["loc"].tolist() == [0, 1, 2]
    assert M.building_match(C.clean_footprint(fp, fill=True) * 2, gt)["loc"].tolist() == [0, 1, 2], "the bridge still fuses them"
    assert M.building_match(C.clean_footprint(fp, open=3) * 2, gt)["loc"].tolist() == [2, 0, 0], "143 of 144 pixels: IoU above 1 / 2"


def test_the_binding_and_what_is_refused_without_a_gpu():
    from dahitra_amd import _lib, ops
    from dahitra_amd.models import xbd
    p = _lib.prototypes()
    i, vp, lg = ctypes.c_int, ctypes.c_void_p, ctypes.c_long
    assert p["dh_xbd_morph_u8"] == (i, [vp, i, i, i, i, i, vp, vp])
    assert p["dh_xbd_msk_dilate_u8"] == (i, [vp, i, i, i, i, vp, vp])
    assert p["dh_xbd_fill_holes_ws_bytes"] == (i, [i, i, i, vp])
    assert p["dh_xbd_fill_holes_u8"] == (i, [vp, i, i, i, i, vp, vp, lg, vp])
    lib = _lib.lib()
    assert (lib.dh_xbd_morph_tile_h(), lib.dh_xbd_morph_tile_w()) == ops.XBD_MORPH_TILE == (32, 64)
    # labels and count, the labelling's workspace, the key, the marks (H W + 1 bytes per image, padded to four)
    hw = 37 * 67
    assert ops.xbd_fill_holes_ws_bytes(2, 37, 67) == 4 * 2 * hw + 4 * 2 + ops.xbd_cc_ws_bytes(2, 37, 67) + (2 * hw + 3) // 4 * 4 \
        + (2 * (hw + 1) + 3) // 4 * 4
    for bad in ((0, 4, 4), (70000, 4, 4), (1, 0, 4), (1, 4, 0), (1, 65536, 65536)):
        with pytest.raises(ValueError, match="xbd_fill_holes_ws_bytes"):
            ops.xbd_fill_holes_ws_bytes(*bad)
    # the C entries refuse before they launch
    buf = (ctypes.c_ubyte * 64)()
    a, b = ctypes.addressof(buf), ctypes.addressof(buf) + 32
    for args, text in (((a, 1, 4, 4, 4, 0, b, None), "k=4"), ((a, 1, 4, 4, 33, 0, b, None), "k=33"), ((a, 1, 4, 4, -1, 0, b, None), "k=-1"),
                       ((a, 1, 4, 4, 3, 2, b, None), "op 2"), ((None, 1, 4, 4, 3, 0, b, None), "null"), ((a, 1, 4, 4, 3, 0, None, None), "null"),
                       ((a, 1, 4, 4, 3, 0, a, None), "overlaps"), ((a, 1, 4, 4, 3, 0, a + 15, None), "overlaps"), ((a, 0, 4, 4, 3, 0, b, None), "N=0")):
        assert lib.dh_xbd_morph_u8(*args) != 0 and lib.dh_last_error().decode().startswith("xbd_morph") and text in lib.dh_last_error().decode()
    for args, text in (((a, 1, 2, 2, 2, b, None), "k=2"), ((a, 1, 2, 2, 3, None, None), "null"), ((a, 1, 2, 2, 3, a + 19, None), "overlaps")):
        assert lib.dh_xbd_msk_dilate_u8(*args) != 0 and lib.dh_last_error().decode().startswith("xbd_msk_dilate") and text in lib.dh_last_error().decode()
    for args, text in (((a, 1, 2, 2, 6, b, b, 1 << 20, None), "connectivity 6"), ((a, 1, 2, 2, 4, b, None, 1 << 20, None), "null"),
                       ((a, 1, 2, 2, 4, b, b + 1, 1 << 20, None), "int32"), ((a, 1, 2, 2, 4, b, b, 8, None), "are needed"),
                       ((a, 1, 2, 2, 4, a, b, 1 << 20, None), "overlaps")):
        assert lib.dh_xbd_fill_holes_u8(*args) != 0 and lib.dh_last_error().decode().startswith("xbd_fill_holes") and text in lib.dh_last_error().decode()
    # the Python layer: ValueError before any launch
    m = torch.zeros(1, 8, 8, dtype=torch.uint8)
    msk = torch.zeros(1, 5, 8, 8, dtype=torch.uint8)
    for call in (lambda: ops.xbd_morph(m, "dilate", 3),                           # not on the device
                 lambda: ops.xbd_morph(m, "dilate", 4), lambda: ops.xbd_morph(m, "dilate", 33), lambda: ops.xbd_morph(m, "dilate", 0),
                 lambda: ops.xbd_morph(m, "dilate", -3), lambda: ops.xbd_morph(m, "dilate", True), lambda: ops.xbd_morph(m, "dilate", 3.0),
                 lambda: ops.xbd_morph(m, "open", 3), lambda: ops.xbd_morph(m, 0, 3), lambda: ops.xbd_morph(m[0], "erode", 3),
                 lambda: ops.xbd_morph(m.to(torch.int32), "erode", 3), lambda: ops.xbd_morph(m[:, :, ::2], "erode", 3),
                 lambda: ops.xbd_morph(m, "erode", 3, out=m), lambda: ops.xbd_morph(m, "erode", 3, out=m[:, :4]),
                 lambda: ops.xbd_morph(m[:, :0], "erode", 3)):
        with pytest.raises(ValueError, match="xbd_morph"):
            call()
    for call in (lambda: ops.xbd_msk_dilate(msk), lambda: ops.xbd_msk_dilate(msk, 4), lambda: ops.xbd_msk_dilate(msk, 33),
                 lambda: ops.xbd_msk_dilate(msk, True), lambda: ops.xbd_msk_dilate(msk, 5.0), lambda: ops.xbd_msk_dilate(msk[:, :4]),
                 lambda: ops.xbd_msk_dilate(m), lambda: ops.xbd_msk_dilate(msk.float()), lambda: ops.xbd_msk_dilate(msk, 5, out=msk),
                 lambda: ops.xbd_msk_dilate(msk, 5, out=m)):
        with pytest.raises(ValueError, match="xbd_msk_dilate"):
            call()
    for call in (lambda: ops.xbd_fill_holes(m), lambda: ops.xbd_fill_holes(m, 6), lambda: ops.xbd_fill_holes(m, True),
                 lambda: ops.xbd_fill_holes(m, 4.0), lambda: ops.xbd_fill_holes(m[0]), lambda: ops.xbd_fill_holes(m.to(torch.int32)),
                 lambda: ops.xbd_fill_holes(m, out=m), lambda: ops.xbd_fill_holes(m, out=m[:, :4]),
                 lambda: ops.xbd_fill_holes(m, ws=torch.zeros(8, dtype=torch.uint8)),
                 lambda: ops.xbd_fill_holes(m, ws=torch.zeros(1 << 12, dtype=torch.int32))):
        with pytest.raises(ValueError, match="xbd_fill_holes"):
            call()
    for fn in (lambda: xbd.dilate(m, 3), lambda: xbd.erode(m, 3), lambda: xbd.opening(m, 3), lambda: xbd.closing(m, 3),
               lambda: xbd.fill_holes(m), lambda: xbd.clean_footprint(m, open=3)):
        with pytest.raises(_lib.HipLibraryError, match="runs on MI355X only"):
            fn()


def test_make_batch_refuses_a_bad_dilate():
    from dahitra_amd.datasets.xbd_pipeline import GpuXbdPipeline
    pipe = GpuXbdPipeline.__new__(GpuXbdPipeline)              # host tensors: the checks come before anything touches the device
    pipe.pre = pipe.post = torch.zeros(2, 80, 96, 3, dtype=torch.uint8)
    pipe.pre_mask = pipe.post_label = torch.zeros(2, 80, 96, dtype=torch.uint8)
    pipe.files, pipe._zero_lbl, pipe._jitter_ws = ["a", "b"], None, None
    for bad in (dict(dilate=4), dict(dilate=5, train=False), dict(dilate=1), dict(dilate=33), dict(dilate=-5), dict(dilate=True),
                dict(dilate=5.0), dict(dilate="5")):
        with pytest.raises(ValueError, match="dilate"):
            pipe.make_batch([0, 1], 64, **bad)
    with pytest.raises(ValueError, match="dilate"):
        next(pipe.batches(2, 80, train=False, dilate=5))
