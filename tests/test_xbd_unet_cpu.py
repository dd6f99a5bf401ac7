"""The numpy restatement of cv2.warpAffine's fixed-point path (datasets/xbd_pipeline.warp_affine_u8, unet_reference_u8) held to
things that do not depend on it -- the identity, numpy's own reflect padding and rot90, a linear ramp in float64 -- and the
kernel's single gather (tests/_xbd_unet_cases.composed_u8) held to the restatement's explicit intermediate images; and
draw_unet_params against the script's draws, stream state for stream state.  No GPU.  An installed OpenCV is not compared: there
is none here, so the restatement -- written from imgwarp.cpp of OpenCV 4.x up to 4.10 -- is the contract."""
import importlib.util
import os
import random

import numpy as np
import pytest

import _xbd_unet_cases as C
from dahitra_amd.datasets import xbd_pipeline as X

REFERENCE = os.environ.get("DAHITRA_REFERENCE", "/root/reference")


def image(h, w, seed=3, c=None):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w) if c is None else (h, w, c)).astype(np.uint8)


@pytest.mark.parametrize("S", [1, 2, 5, 37, 256])
def test_angle_0_scale_1_is_the_identity(S):
    img = image(S, S, c=3)
    for centre in ((S // 2, S // 2), (S // 2 - 320, S // 2 + 320)):
        assert np.array_equal(X.warp_affine_u8(img, X.rotation_matrix(centre, 0, 1)), img), centre


@pytest.mark.parametrize("S", [2, 5, 37, 256])
def test_a_shift_is_the_slice_of_numpys_reflect_padding(S):
    img = image(S, S + 1)                                              # not square: x and y cannot be swapped unnoticed
    pad = np.pad(img, 330, mode='reflect')
    for sx, sy in C.shifts(S):
        want = pad[330 - sy:330 - sy + S, 330 - sx:330 - sx + S + 1]
        assert np.array_equal(X.warp_affine_u8(img, X.shift_matrix((sx, sy))), want), (sx, sy)


def test_a_shift_of_a_single_pixel_returns_the_pixel():
    img = np.array([[201]], dtype=np.uint8)
    for s in C.shifts(1):
        assert np.array_equal(X.warp_affine_u8(img, X.shift_matrix(s)), img)


def test_a_quarter_turn_about_an_integer_centre_is_rot90():
    img = image(37, 37, c=3)
    assert np.array_equal(X.warp_affine_u8(img, X.rotation_matrix((18, 18), 90, 1)), np.rot90(img, 1))


def test_a_ramp_stays_within_the_fixed_point_error_of_the_float64_affine_value():
    """I = 2 x + y + 20: bilinear interpolation of a linear image is exact, so what is left is the final rounding (0.5) and the
    coordinates' error -- 1/64 from the 1/32 grid plus 2 x 0.5/1024 from the two rounded tables, each -- times the slopes 2 and
    1.  (The largest difference over these cases is 0.5462.)"""
    S = 64
    y, x = np.mgrid[:S, :S].astype(np.float64)
    ramp = (2 * x + y + 20).astype(np.uint8)
    bound = 0.5 + (2 + 1) * (1 / 64 + 1 / 1024)
    worst = checked = 0
    for angle in (-10, -3, 1, 7, 10):
        for scale in (0.9, 1, 1.0999):
            M = X.rotation_matrix((S // 2, S // 2), angle, scale)
            A = np.linalg.inv(np.vstack([M, [0, 0, 1]]))
            sx, sy = A[0, 0] * x + A[0, 1] * y + A[0, 2], A[1, 0] * x + A[1, 1] * y + A[1, 2]
            inside = (sx >= 1) & (sx <= S - 3) & (sy >= 1) & (sy <= S - 3)          # every tap inside: no reflection
            got = X.warp_affine_u8(ramp, M).astype(np.float64)
            diff = np.abs(got - (2 * sx + sy + 20))[inside]
            assert inside.sum() > S * S // 2 and diff.max() <= bound, (angle, scale, diff.max(), bound)
            worst, checked = max(worst, diff.max()), checked + int(inside.sum())
    print("ramp: worst %.4f of %.4f over %d pixels" % (worst, bound, checked))
    assert worst > 0.5, "the cases reach the rounding"


@pytest.fixture(scope="module")
def src():
    return tuple(a[0] for a in C.sources(1, 40, 52))


def test_flips_and_quarter_turns_of_the_single_gather_are_numpys(src):
    pre, post, _, label = src
    S = 37
    for v in (0, 1):
        for k in range(4):
            img, msk = C.composed_u8(pre, post, label, C.row(3, 2, v, k), S)
            f = lambda a: np.rot90(a[2:2 + S, 3:3 + S][::-1] if v else a[2:2 + S, 3:3 + S], k)
            assert np.array_equal(img[:3], f(pre).transpose(2, 0, 1)) and np.array_equal(img[3:], f(post).transpose(2, 0, 1)), (v, k)
            assert all(np.array_equal(msk[c], f(label) == c) for c in (1, 2, 3, 4)), (v, k)
            assert np.array_equal(msk[0], (f(label) >= 1) & (f(label) <= 4))


@pytest.mark.parametrize("S,H,W", [(37, 40, 52), (1, 1, 1), (5, 9, 6)])
def test_the_single_gather_equals_the_chain_of_intermediate_images(S, H, W):
    """shift then rotate through an explicit S x S image whose border the second warp reflects, the four 0 / 255 class planes
    warped one by one and thresholded, shift_channels: unet_reference_u8 does each step on its own, composed_u8 does one gather"""
    pre, post, _, label = (a[0] for a in C.sources(1, H, W))
    ties = 0
    for r in C.param_rows(S, H, W):
        want = X.unet_reference_u8(pre, post, label, r, S)
        got = C.composed_u8(pre, post, label, r, S)
        assert np.array_equal(got[0], want[0]), ("img", r)
        assert np.array_equal(got[1], want[1]), ("msk", r)
        ties += int((want[1][1:].sum(axis=0) >= 2).sum())
    assert ties > 0 or S < 37, "two classes at weight 1/2 are both set somewhere"


@pytest.mark.reference
def test_shift_channels_is_the_references(src):
    path = os.path.join(REFERENCE, "xBD_code", "utils.py")
    if not os.path.exists(path):
        pytest.skip("the reference's xBD_code/utils.py is not on this machine")
    spec = importlib.util.spec_from_file_location("_reference_xbd_utils", path)
    utils = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(utils)
    pre, post, _, label = src
    S = 37
    edge = np.array([0, 3, 5, 250, 252, 255], dtype=np.uint8)
    pre, post = pre.copy(), post.copy()
    pre[:6, :6] = edge[:, None, None]
    post[:6, :6] = edge[None, :, None]                               # bytes that clip at either end
    for b, g, r in ((5, -5, 3), (-5, 5, -1), (0, 0, 0), (5, 5, 5), (-5, -5, -5)):
        for chan in (1, 2):
            img, _ = X.unet_reference_u8(pre, post, label, C.row(channels=(chan, b, g, r)), S)
            got = img.reshape(2, 3, S, S)
            for im, a in enumerate((pre, post)):
                bgr = np.ascontiguousarray(a[:S, :S, ::-1])               # the script reads its images with cv2: BGR
                want = utils.shift_channels(bgr, b, g, r) if im == chan - 1 else bgr
                assert np.array_equal(got[im].transpose(1, 2, 0), want[..., ::-1]), (b, g, r, chan, im)


SEED, SAMPLES = 1, 20000


def test_draw_unet_params_draws_what_the_script_draws():
    """the same rows, the same skipped operations and the same stream state after every one of 20 000 samples; the seed is one
    with which the script takes every branch that a seed can reach"""
    a, b = random.Random(SEED), random.Random(SEED)
    seen = set()
    for n in range(SAMPLES):
        crop = (256, 37)[n % 2]
        row, skipped = X.draw_unet_params(a, 1024, 1000, crop)
        want_row, want_skipped, took = C.script_draws(b, 1024, 1000, crop)
        assert row == want_row and skipped == want_skipped, (n, row, want_row, skipped, want_skipped)
        assert a.getstate() == b.getstate(), n
        assert set(skipped) <= set(X.UNET_SKIPPED)
        seen |= took
    assert seen == C.BRANCHES, (sorted(C.BRANCHES - seen), sorted(seen - C.BRANCHES))


class Scripted:
    """a stream that returns what it is told to"""

    def __init__(self, values):
        self.values = list(values)

    def random(self):
        return self.values.pop(0)

    def randint(self, lo, hi):
        v = self.values.pop(0)
        assert lo <= v <= hi
        return v

    def randrange(self, n):
        return self.randint(0, n - 1)


def test_angle_0_at_scale_1_skips_the_warp_but_not_its_draws():
    # x0, y0, flip, rot test, shift test, warp test, cx, cy, scale draw 0.5 -> 1.0, angle 10 - 10, then ten tests that fail
    values = [5, 6, 0.9, 0.0, 0.0, 0.7, -320, 320, 0.5, 10] + [0.0] * 10
    assert 0.9 + 0.5 * 0.2 == 1
    for draw in (X.draw_unet_params, lambda *a: C.script_draws(*a)[:2]):
        s = Scripted(values)
        row, skipped = draw(s, 300, 300, 256)
        assert row == C.row(5, 6, vflip=1) and skipped == [] and s.values == []
    s = Scripted(values[:9] + [11] + [0.0] * 10)
    assert X.draw_unet_params(s, 300, 300, 256)[0]["warp"] == (1, 1.0, (128 - 320, 128 + 320)) and s.values == []


def test_rows_and_tables_that_do_not_fit_are_refused():
    ok = C.row(3, 2, 1, 3, (320, -320), (10, 1.0999, (18 - 320, 18 + 320)), (2, 5, -5, 0))
    assert X.check_unet_rows([ok], 40, 52, 37) == [ok]
    tab = X.unet_warp_table([ok, C.row()], 37)
    assert tab.shape == (2, 4, 37) and tab.dtype == np.int32 and not tab[1].any() and tab[0].any()
    assert X.unet_warp_table([C.row(shift=(1, 2))], 37) is None
    p = X.unet_param_rows([ok])
    assert p.dtype == np.int32 and p.tolist() == [[3, 2, 1, 3, 320, -320, 1, 2, 0, -5, 5, 0]]      # b to plane 2
    for bad in (dict(x0=16), dict(y0=-1), dict(vflip=2), dict(rot=4), dict(rot=1.0), dict(shift=(1,)), dict(shift=(1.5, 0)),
                dict(shift=(1 << 21, 0)), dict(warp=(1, 1.0)), dict(warp=(1, float("nan"), (0, 0))), dict(warp=(1, 1.0, (0,))),
                dict(channels=(0, 1, 1, 1)), dict(channels=(1, 1, 1)), dict(channels=(1, 256, 0, 0)), dict(channels=(1, 0.5, 0, 0))):
        with pytest.raises(ValueError):
            X.check_unet_rows([dict(ok, **bad)], 40, 52, 37)
    with pytest.raises(ValueError):
        X.check_unet_rows([ok], 36, 52, 37)
    with pytest.raises(ValueError):
        X.check_unet_rows([[0] * 9], 40, 52, 37)
    with pytest.raises(ValueError):
        X.draw_unet_params(random.Random(0), 40, 52, 41)


def test_the_entry_refuses_before_any_launch_and_names_itself():
    from dahitra_amd import _lib, ops
    lib = _lib.lib()
    assert (lib.dh_xbd_augment_warp_tile_h(), lib.dh_xbd_augment_warp_tile_w()) == ops.XBD_WARP_TILE == (32, 32)
    assert ops.XBD_WARP_PARAM_WORDS == 12 == X.unet_param_rows([C.row()]).shape[1]
    for N, H, W, S in ((1, 40, 52, 37), (0, 40, 52, 37), (1, 40, 52, 0), (1, 40, 52, 41), (1, 52, 40, 41), (65536, 40, 52, 37)):
        assert lib.dh_xbd_augment_warp_u8(None, None, None, None, None, None, N, H, W, S, None, None, None) != 0
        assert lib.dh_last_error().decode().startswith("xbd_augment_warp"), lib.dh_last_error()


def test_a_tap_origin_outside_int16_is_refused():
    assert X.unet_warp_table([C.row(warp=(10, 0.9, (32000, 0)))], 37) is not None
    for warp in ((10, 0.9, (400000, 0)), (0, 1e-3, (200, 200)), (180, 1.0, (0, -20000))):
        with pytest.raises(ValueError, match="int16"):
            X.unet_warp_table([C.row(warp=warp)], 256)
    with pytest.raises(ValueError):
        X.warp_tables(np.array([[1e9, 0, 0], [0, 1e-9, 0]]), 37, 37)
    # a matrix that cannot be inverted: OpenCV's D = 0 maps everything to the origin
    assert np.array_equal(X.warp_affine_u8(image(5, 5), np.zeros((2, 3))), np.full((5, 5), image(5, 5)[0, 0]))
