"""Host side of the xBD device loader (datasets/xbd_pipeline.py), no GPU: the coefficient table of Pillow's two-pass BILINEAR
resize, applied by a small numpy evaluator, against Pillow itself byte for byte; draw_train_params against a literal restatement
of the reference's draw sequence (xBD_code/train.py:110-138); the checks on parameter rows."""
import random

import numpy as np
import pytest
from PIL import Image

# (h, w) -> S x S: identity, one pass only, both passes, a one-pixel-high source, a non-power-of-two output
SIZES = [(64, 64, 64), (50, 64, 64), (64, 37, 64), (45, 51, 64), (200, 173, 256), (63, 64, 64), (13, 64, 64), (1, 5, 64),
         (100, 90, 96)]


def one_pass(a, coef, axis):
    """Pillow's ImagingResampleHorizontal_8bpc / Vertical_8bpc with a (lo, k0, k1, k2) table: a uint8 -> uint8"""
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.empty((coef.shape[0],) + a.shape[1:], dtype=np.int64)
    for o, (lo, *k) in enumerate(coef.tolist()):
        acc = 1 << 21
        for t in range(3):
            if k[t]:                                   # a tap with coefficient 0 may lie outside the source
                acc = acc + a[lo + t] * k[t]
        out[o] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def two_pass(a, S):
    from dahitra_amd.datasets.xbd_pipeline import resize_coeffs
    h, w = a.shape[:2]
    return one_pass(one_pass(a, resize_coeffs(w, S), 1), resize_coeffs(h, S), 0)


def blocky(rng, h, w, values):
    """constant in 8 x 8 blocks: blends occur at the block borders"""
    small = rng.choice(np.asarray(values, dtype=np.uint8), size=(-(-h // 8), -(-w // 8)))
    return np.ascontiguousarray(np.kron(small, np.ones((8, 8), dtype=np.uint8))[:h, :w])


@pytest.mark.parametrize("h,w,S", SIZES)
def test_resize_coeffs_two_pass_equals_pillow_bilinear(h, w, S):
    rng = np.random.RandomState(h * 1000 + w)
    cases = {"rgb noise": rng.randint(0, 256, (h, w, 3)).astype(np.uint8),
             "labels": blocky(rng, h, w, [0, 1, 2, 3, 4]),
             "labels noise": rng.randint(0, 5, (h, w)).astype(np.uint8),
             "mask": blocky(rng, h, w, [0, 255]),
             "mask noise": (rng.randint(0, 2, (h, w)) * 255).astype(np.uint8)}
    for name, a in cases.items():
        want = np.asarray(Image.fromarray(a).resize((S, S), Image.BILINEAR))
        got = two_pass(a, S)
        assert got.shape == want.shape and np.array_equal(got, want), (name, int((got != want).sum()))


def test_resize_coeffs_table():
    from dahitra_amd.datasets.xbd_pipeline import resize_coeffs
    ident = resize_coeffs(64, 64)
    assert ident.dtype == np.int32 and ident.shape == (64, 4)
    assert np.array_equal(ident, np.stack([np.arange(64), np.full(64, 1 << 22), np.zeros(64), np.zeros(64)], 1))
    for n_in, n_out in [(1, 64), (5, 64), (37, 64), (824, 1024), (1023, 1024)]:
        c = resize_coeffs(n_in, n_out)
        assert (c[:, 0] >= 0).all() and (c[:, 0] < n_in).all() and (np.diff(c[:, 0]) >= 0).all() and (np.diff(c[:, 0]) <= 1).all()
        assert (c[:, 1:] >= 0).all() and (c[:, 1:] <= 1 << 22).all() and (np.abs(c[:, 1:].sum(1) - (1 << 22)) <= 2).all()
        for t in range(3):                            # a non-zero coefficient has its tap inside the source
            assert (c[:, 0][c[:, 1 + t] != 0] + t < n_in).all()
    for bad in [(200, 64), (0, 64), (2048, 1024)]:           # more than three taps, or no source
        with pytest.raises(ValueError):
            resize_coeffs(*bad)


def reference_draws(H, W, crop_size):
    """xBD_code/train.py:110-138, the calls on `random` only, in order; what each decides is returned"""
    x0 = random.randint(0, W - crop_size)
    y0 = random.randint(0, H - crop_size)
    got = dict(x0=x0, y0=y0, aug=False, hflip=False, vflip=False, resized=False, box=None, jitter=False)
    if random.random() > 0.7:
        got["aug"] = True
        if random.random() > 0.3:
            got["hflip"] = True
        if random.random() > 0.3:
            got["vflip"] = True
        if random.random() > 0.3:
            x = random.randint(0, 200)
            y = random.randint(0, 200)
            got["resized"] = True
            got["box"] = (x, y, crop_size - x, crop_size - y)          # TF.resized_crop's top, left, height, width
        if random.random() > 0.7:
            got["jitter"] = True
    return got


def test_draw_train_params_consumes_the_reference_draws():
    from dahitra_amd.datasets.xbd_pipeline import PARAM_FIELDS, draw_train_params
    H, W, crop = 1024, 1000, 608
    seen = set()
    for seed in range(50):
        random.seed(seed)
        want = [reference_draws(H, W, crop) for _ in range(3)]
        state = random.getstate()
        random.seed(seed)
        for w in want:
            row, jitter = draw_train_params(random, H, W, crop)
            r = dict(zip(PARAM_FIELDS, row))
            assert len(row) == 9 and all(type(v) is int for v in row)
            assert (r["x0"], r["y0"], r["hflip"], r["vflip"], r["resize"]) == (w["x0"], w["y0"], w["hflip"], w["vflip"], w["resized"])
            assert (r["top"], r["left"], r["height"], r["width"]) == (w["box"] if w["resized"] else (0, 0, crop, crop))
            assert jitter is w["jitter"]
            seen.add("none" if not w["aug"] else "resize" if w["resized"] else "no resize")
            seen.add("jitter" if w["jitter"] else "no jitter")
        assert random.getstate() == state, seed       # Python's generator stands where the reference leaves it
        # a random.Random instance draws the same sequence
        inst = random.Random(seed)
        random.seed(seed)
        assert draw_train_params(inst, H, W, crop) == draw_train_params(random, H, W, crop)
    assert seen == {"none", "resize", "no resize", "jitter", "no jitter"}


def test_parameter_rows_are_checked():
    from dahitra_amd.datasets.xbd_pipeline import check_params, coef_table, draw_train_params, resize_coeffs
    ok = [[5, 9, 1, 0, 1, 6, 11, 51, 45], [0, 0, 0, 0, 0, 0, 0, 64, 64]]
    p = check_params(ok, 80, 96, 64)
    assert p.shape == (2, 9)
    table = coef_table(p, 64)
    assert table.shape == (2, 2, 64, 4) and not table[1].any()
    assert np.array_equal(table[0, 0].numpy(), resize_coeffs(45, 64)) and np.array_equal(table[0, 1].numpy(), resize_coeffs(51, 64))
    assert coef_table(check_params(ok[1:], 80, 96, 64), 64) is None
    for bad in ([[33, 0, 0, 0, 0, 0, 0, 64, 64]],          # window leaves the image along x (96 - 64 = 32)
                [[0, 17, 0, 0, 0, 0, 0, 64, 64]],          # ... along y
                [[0, 0, 2, 0, 0, 0, 0, 64, 64]],           # a flag that is not 0 / 1
                [[0, 0, 0, 0, 1, 14, 0, 51, 64]],          # box leaves the crop: 14 + 51 > 64
                [[0, 0, 0, 0, 1, 0, 20, 64, 45]],          # ... along x
                [[0, 0, 0, 0, 1, 0, 0, 0, 64]],            # empty box
                [[0, 0, 0, 0, 1, -1, 0, 64, 64]]):
        with pytest.raises(ValueError):
            check_params(bad, 80, 96, 64)
    with pytest.raises(ValueError):
        check_params(ok, 60, 96, 64)                        # crop larger than the image
    with pytest.raises(ValueError):
        draw_train_params(random.Random(0), 60, 96, 64)
