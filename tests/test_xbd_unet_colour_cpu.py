"""The colour stage of xBD_code/train_unettransformer.py (lines 211-244) on the host: draw_unet_colour against draw_unet_params,
stream state for stream state; the restatements of saturation, brightness, contrast and gauss_noise against what the
reference's xBD_code/utils.py returned (tests/golden/xbd_unet_colour.npz, tools/make_unet_colour_golden.py), byte for byte; blur
against numpy's reflect padding; change_hsv against colorsys on a colour lattice.  No GPU.  No OpenCV is compared: there is
none here, so for cv2.blur and cv2.cvtColor the restatements are the contract."""
import colorsys
import os
import random

import numpy as np
import pytest

import _xbd_unet_colour_cases as K
from dahitra_amd.datasets import xbd_pipeline as X

SEED, SAMPLES = 1, 20000           # test_xbd_unet_cpu.py's: a seed with which the script takes every branch


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "xbd_unet_colour.npz"))


def rgb(bgr):
    return np.ascontiguousarray(bgr[..., ::-1])


def test_draw_unet_colour_consumes_draw_unet_params_stream():
    a, b = random.Random(SEED), random.Random(SEED)
    c = random.Random(SEED)
    np_rng = np.random.RandomState(3)
    seen, seen_noise = set(), 0
    for n in range(SAMPLES):
        crop = (256, 37)[n % 2]
        row, colour, skipped = X.draw_unet_colour(a, 1024, 1000, crop)
        want_row, want_skipped = X.draw_unet_params(b, 1024, 1000, crop)
        assert a.getstate() == b.getstate(), n
        assert row == want_row and set(colour) == {"hsv", "pre", "post"}
        names = X.unet_colour_names(colour)
        assert sorted(names + skipped) == sorted(want_skipped), (n, names, skipped, want_skipped)
        assert all(s.rsplit("_", 1)[0] in ("clahe", "elastic", "gauss_noise") for s in skipped)
        assert not any(name.startswith(("clahe", "elastic", "gauss_noise")) for name in names)
        X.check_unet_colour([colour], crop)
        for im in ("pre", "post"):
            if colour[im] is not None and colour[im][0] in ("saturation", "brightness", "contrast"):
                assert 0.9 <= colour[im][1] < 1.1
        if colour["hsv"] is not None:
            assert colour["hsv"][0] in (1, 2) and all(-5 <= v <= 5 for v in colour["hsv"][1:])
        seen |= set(names) | set(skipped)
        # with a numpy generator gauss_noise moves from skipped to colour, and nothing else changes
        row2, colour2, skipped2 = X.draw_unet_colour(c, 1024, 1000, crop, np_rng)
        assert c.getstate() == a.getstate() and row2 == row
        noisy = [s for s in skipped if s.startswith("gauss_noise")]
        assert sorted(skipped2 + noisy) == sorted(skipped) and sorted(X.unet_colour_names(colour2)) == sorted(names + noisy)
        for s in noisy:
            op, value = colour2[s.rsplit("_", 1)[1]]
            assert op == "gauss_noise" and value.shape == (crop, crop, 3) and value.dtype == np.uint8 and value.min() == 0
            seen_noise += 1
        X.check_unet_colour([colour2], crop)
    assert seen == set(X.UNET_SKIPPED), sorted(set(X.UNET_SKIPPED) - seen)
    assert seen_noise >= 2


def test_noise_is_drawn_pre_before_post_from_the_legacy_stream():
    np.random.seed(9)
    want = [X.draw_unet_noise(np.random, 5), X.draw_unet_noise(np.random, 5)]
    rs = np.random.RandomState(9)
    g = rs.normal(30, 30 ** 0.5, (5, 5, 3))
    assert np.array_equal(want[0], (g - g.min()).astype(np.uint8)), "RandomState(k) is np.random.seed(k)'s stream"
    # the draws themselves, through a scripted `random` stream that sends both images to gauss_noise
    values = iter([0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0] + [0.99, 0.0, 0.99] * 2 + [0.0, 0.0])

    class Scripted:
        def random(self):
            return next(values)

        def randint(self, lo, hi):
            return next(values)

        def randrange(self, n):
            return next(values)

    row, colour, skipped = X.draw_unet_colour(Scripted(), 9, 9, 5, np.random.RandomState(9))
    assert skipped == [] and colour["hsv"] is None and colour["pre"][0] == colour["post"][0] == "gauss_noise"
    assert np.array_equal(colour["pre"][1], want[0]) and np.array_equal(colour["post"][1], want[1])
    assert next(values, None) is None


def test_blends_and_noise_equal_the_references_bytes(golden):
    """saturation, brightness, contrast at five factors and gauss_noise after np.random.seed(k), on the fixture's images: exact.
    Contrast's mean is the one defined from the integer channel sums (contrast_mean); on these inputs it gives the bytes of the
    reference, which takes numpy's mean of the per-pixel greys."""
    factors = golden["factors"]
    assert factors[:3].tolist() == [0.9, 1.0, 1.0999] and len(factors) == 5 and all(0.9 <= f < 1.1 for f in factors)
    fns = (X.saturation_u8, X.brightness_u8, X.contrast_u8)
    for i in range(2):
        bgr = golden["bgr_%d" % i]
        assert bgr.shape in ((24, 20, 3), (33, 33, 3))
        for o, fn in enumerate(fns):
            for k, alpha in enumerate(factors):
                got = fn(rgb(bgr), float(alpha))
                assert got.dtype == np.uint8 and np.array_equal(got[..., ::-1], golden["blend_%d" % i][o, k]), (fn.__name__, i, alpha)
        for k, seed in enumerate(golden["noise_seeds"]):
            h, w = bgr.shape[:2]
            rs = np.random.RandomState(int(seed))
            if h == w:
                noise = X.draw_unet_noise(rs, h)
            else:
                g = rs.normal(30, 30 ** 0.5, (h, w, 3))
                noise = (g - g.min()).astype(np.uint8)
            assert np.array_equal(X.gauss_noise_u8(rgb(bgr), noise)[..., ::-1], golden["gauss_noise_%d" % i][k]), (i, seed)
        assert (golden["gauss_noise_%d" % i] == 255).any() and (golden["blend_%d" % i] == 255).any(), "the clip is reached"
    # the factor 1 returns the image, and brightness is the truncated product
    img = rgb(golden["bgr_1"])
    assert all(np.array_equal(fn(img, 1.0), img) for fn in fns)
    assert np.array_equal(X.brightness_u8(img, 0.9), (img * 0.9).astype(np.uint8))


def test_contrast_mean_is_the_grey_of_the_exact_sums():
    img = np.random.RandomState(2).randint(0, 256, size=(66, 66, 3)).astype(np.uint8)
    s = img.reshape(-1, 3).astype(np.int64).sum(axis=0)
    assert X.contrast_mean(img) == ((0.114 * int(s[2]) + 0.587 * int(s[1])) + 0.299 * int(s[0])) / (66 * 66)
    grey = (0.114 * img[..., 2].astype(np.float64) + 0.587 * img[..., 1]) + 0.299 * img[..., 0]
    assert abs(X.contrast_mean(img) - grey.mean()) < 1e-10


@pytest.mark.parametrize("h,w", [(2, 2), (2, 5), (33, 36), (66, 7)])
def test_blur_is_the_rounded_mean_under_numpys_reflect_padding(h, w):
    img = np.random.RandomState(h * 100 + w).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    img[0, 0], img[-1, -1] = 255, 0
    pad = np.pad(img.astype(np.int64), ((1, 1), (1, 1), (0, 0)), mode='reflect')
    total = np.zeros((h, w, 3), dtype=np.int64)
    for dy in range(3):
        for dx in range(3):
            total += pad[dy:dy + h, dx:dx + w]
    assert np.array_equal(X.blur_u8(img), np.rint(total / 9.).astype(np.uint8))
    assert np.array_equal(X.blur_u8(np.full((h, w, 3), 255, dtype=np.uint8)), np.full((h, w, 3), 255, dtype=np.uint8))


def test_blur_of_one_pixel_returns_it_and_every_rounding_of_a_ninth_agrees():
    one = np.array([[[7, 0, 255]]], dtype=np.uint8)
    assert np.array_equal(X.blur_u8(one), one)
    s = np.arange(9 * 255 + 1)
    want = (2 * s + 9) // 18
    assert np.array_equal(want, np.rint(s * (1 / 9)).astype(np.int64))
    assert np.array_equal(want, np.rint(s.astype(np.float32) * np.float32(1 / 9)).astype(np.int64))
    for k in (16, 23):
        assert np.array_equal(want, (s * round(2 ** k / 9) + 2 ** (k - 1)) >> k), k
    assert not (2 * s % 18 == 9).any(), "no tie"


def test_the_float_decode_inverts_the_normalisation_table():
    table = np.arange(256, dtype=np.float32) / np.float32(127) - np.float32(1)
    back = np.rint((table + np.float32(1)) * np.float32(127))
    assert back.dtype == np.float32 and np.array_equal(back, np.arange(256))


def test_hsv_of_the_lattice_is_within_one_of_colorsys():
    lat = K.lattice()
    orders = {tuple(np.argsort(c, kind="stable")) for c in lat if len(set(c.tolist())) == 3}
    assert len(orders) == 6 and (lat.max(axis=1) == 0).any() and len(lat) == 7 ** 3 + 256
    hsv = X.rgb_to_hsv_u8(lat[None])[0].astype(np.float64)
    assert hsv[:, 0].max() <= 179
    worst = [0.0, 0.0, 0.0]
    for (r, g, b), (H, S, V) in zip(lat.tolist(), hsv.tolist()):
        h, s, v = colorsys.rgb_to_hsv(r / 255, g / 255, b / 255)
        dh = abs(H - h * 180) % 180
        d = (min(dh, 180 - dh), abs(S - s * 255), abs(V - v * 255))
        assert max(d) <= 1, ((r, g, b), (H, S, V), (h * 180, s * 255, v * 255))
        worst = [max(a, b) for a, b in zip(worst, d)]
    print("hsv against colorsys: worst differences H %.3f S %.3f V %.3f" % tuple(worst))
    assert worst[2] == 0, "V is the maximum itself"
    # and the return: the round trip stays close, exactly so on the greys
    back = X.hsv_to_rgb_u8(X.rgb_to_hsv_u8(lat[None]))[0]
    assert np.abs(back.astype(int) - lat.astype(int)).max() <= 5
    grey = lat[:, 0] == lat[:, 1]
    grey &= lat[:, 1] == lat[:, 2]
    assert grey.sum() >= 256 and np.array_equal(back[grey], lat[grey])


def test_a_grey_pixel_stays_grey_and_takes_the_value_shift_exactly():
    grey = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)
    for h, s, v in ((0, 0, 0), (5, 0, 5), (-5, -5, -5), (3, -1, 200), (0, 0, -255), (255, -255, 255)):
        want = np.clip(grey.astype(int) + v, 0, 255).astype(np.uint8)
        assert np.array_equal(X.change_hsv_u8(grey, h, s, v), want), (h, s, v)
    # with a positive s a grey takes a colour (OpenCV does the same: its S becomes s), except black
    tinted = X.change_hsv_u8(grey, 0, 5, 0)
    assert np.array_equal(tinted[0, 0], [0, 0, 0]) and (tinted[0, 100:, 0] > tinted[0, 100:, 1]).all()


def test_a_hue_above_179_wraps_and_one_below_0_stays_0():
    hsv = np.zeros((1, 76, 3), dtype=np.uint8)
    hsv[0, :, 0], hsv[0, :, 1], hsv[0, :, 2] = np.arange(180, 256), 200, 220
    wrapped = hsv.copy()
    wrapped[0, :, 0] -= 180
    a, b = X.hsv_to_rgb_u8(hsv).astype(int), X.hsv_to_rgb_u8(wrapped).astype(int)
    assert np.abs(a - b).max() <= 1           # the fractions differ by float32 roundings of h: a byte moves only at a tie
    assert np.array_equal(a[0, 0], b[0, 0]) or np.abs(a[0, 0] - b[0, 0]).max() == 1
    # through change_hsv: a red of hue 178 shifted by 5 is the hue 3, not 183 clipped to 179
    red = X.hsv_to_rgb_u8(np.array([[[178, 255, 255]]], dtype=np.uint8))
    assert X.rgb_to_hsv_u8(red)[0, 0, 0] == 178
    got = X.rgb_to_hsv_u8(X.change_hsv_u8(red, 5, 0, 0))[0, 0]
    assert abs(int(got[0]) - 3) <= 1
    low = X.hsv_to_rgb_u8(np.array([[[2, 255, 255]]], dtype=np.uint8))
    assert np.array_equal(X.change_hsv_u8(low, -5, 0, 0), X.hsv_to_rgb_u8(np.array([[[0, 255, 255]]], dtype=np.uint8)))


def test_the_colour_reference_applies_change_hsv_then_the_block_operation():
    S = 9
    img6 = np.random.RandomState(4).randint(0, 256, size=(6, S, S)).astype(np.uint8)
    pre, post = (np.ascontiguousarray(img6[3 * i:3 * i + 3].transpose(1, 2, 0)) for i in (0, 1))
    colour = {"hsv": (2, 3, -4, 5), "pre": ("blur", None), "post": ("contrast", 1.05)}
    got = X.unet_colour_reference_u8(img6, colour)
    assert np.array_equal(got[:3].transpose(1, 2, 0), X.blur_u8(pre))
    assert np.array_equal(got[3:].transpose(1, 2, 0), X.contrast_u8(X.change_hsv_u8(post, 3, -4, 5), 1.05))
    for nothing in (None, {}, K.empty()):
        assert np.array_equal(X.unet_colour_reference_u8(img6, nothing), img6)
    jobs, noise = X.unet_colour_jobs([None, colour, K.empty()], S)
    assert noise is None and jobs.dtype == np.int32 and jobs.shape == (2, 12)
    bits = np.array([1.05]).view(np.int32).tolist()
    assert jobs.tolist() == [[1, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0], [1, 1, 1, 3, -4, 5, 5] + bits + [0, 0, 0]]
    assert X.unet_colour_jobs([None, {}], S) == (None, None)
    batch = K.colour_batch(S)
    jobs, noise = X.unet_colour_jobs(X.check_unet_colour(batch, S), S)
    assert noise.shape == (3, S, S, 3) and sorted(jobs[jobs[:, 6] == 1, 9].tolist()) == [0, 1, 2]
    assert len(jobs) == len({(j[0], j[1]) for j in jobs.tolist()}) and {j[6] for j in jobs.tolist()} == {0, 1, 2, 3, 4, 5}


def test_colour_entries_that_do_not_fit_are_refused():
    S = 5
    noise = np.zeros((S, S, 3), dtype=np.uint8)
    ok = {"hsv": (1, 5, -5, 255), "pre": ("gauss_noise", noise), "post": ("contrast", 1.01)}
    assert X.check_unet_colour([ok, None, {}, {"pre": ("blur", None)}], S)[0] is ok
    for bad in (dict(hsv=(0, 1, 1, 1)), dict(hsv=(1, 1, 1)), dict(hsv=(1, 256, 0, 0)), dict(hsv=(2, 0.5, 0, 0)), dict(hsv=(1, True, 0, 0)),
                dict(pre=("clahe", None)), dict(pre=("elastic", None)), dict(pre="blur"), dict(pre=("blur", 1.0)),
                dict(pre=("gauss_noise", None)), dict(pre=("gauss_noise", noise[:4])), dict(pre=("gauss_noise", noise.astype(np.int32))),
                dict(pre=("gauss_noise", noise.tolist())), dict(post=("contrast", float("nan"))), dict(post=("saturation", float("inf"))),
                dict(post=("brightness", None)), dict(post=("brightness", "1.0")), dict(other=None)):
        with pytest.raises(ValueError, match="colour"):
            X.check_unet_colour([None, dict(ok, **bad)], S)
    with pytest.raises(ValueError):
        X.check_unet_colour([[1, 2, 3]], S)
    with pytest.raises(ValueError):
        X.unet_colour_reference_u8(np.zeros((6, S, S), dtype=np.uint8), {"pre": ("gauss_noise", np.zeros((4, 4, 3), dtype=np.uint8))})


def test_the_entry_refuses_before_any_launch_and_names_itself():
    import ctypes
    from dahitra_amd import _lib, ops
    lib = _lib.lib()
    assert lib.dh_xbd_unet_colour_tile() == ops.XBD_COLOUR_TILE == 32
    assert ops.XBD_COLOUR_JOB_WORDS == 12
    i, vp = ctypes.c_int, ctypes.c_void_p
    assert _lib.prototypes()["dh_xbd_unet_colour_u8"] == (i, [vp, vp, vp, i, i, i, i, vp, ctypes.c_long, vp])
    # the workspace: the jobs' bytes, padded to four, and three sums per tile
    assert ops.xbd_unet_colour_ws_bytes(1, 1) == 4 + 12 and ops.xbd_unet_colour_ws_bytes(2, 33) == 6536 + 2 * 4 * 3 * 4
    assert ops.xbd_unet_colour_ws_bytes(32, 256) == 32 * 3 * 65536 + 32 * 64 * 3 * 4
    for J, S in ((0, 33), (1, 0), (1, 4097), (65536, 33)):
        with pytest.raises(ValueError, match="xbd_unet_colour_ws_bytes"):
            ops.xbd_unet_colour_ws_bytes(J, S)
    for N, S, J, K in ((1, 33, 1, 0), (0, 33, 1, 0), (1, 0, 1, 0), (1, 4097, 1, 0), (1, 33, 0, 0), (1, 33, 65536, 0), (1, 33, 1, -1),
                       (1, 33, 1, 1)):
        assert lib.dh_xbd_unet_colour_u8(None, None, None, N, S, J, K, None, 0, None) != 0
        assert lib.dh_last_error().decode().startswith("xbd_unet_colour"), lib.dh_last_error()
