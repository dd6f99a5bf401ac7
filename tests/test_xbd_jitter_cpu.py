"""Host side of the xBD loader's ColorJitter (datasets/xbd_pipeline.py), no GPU: draw_jitter_params against a literal restatement
of torchvision's draws, jitter_reference_u8 -- the project's statement of the arithmetic the kernel implements -- against PIL's
ImageEnhance chain byte for byte, the contrast mean of an intermediate image, a fused-multiply-add mutant that the GPU test's
own images tell from Pillow, and make_batch's rejections."""
import numpy as np
import pytest
import torch

import _xbd_jitter_cases as C


def reference_draws():
    """ColorJitter.get_params(brightness=[0.8, 1.2], contrast=[0.8, 1.2], saturation=[0.8, 1.2], hue=None) of torchvision
    >= 0.8, on torch's global generator"""
    fn_idx = torch.randperm(4)
    b = float(torch.empty(1).uniform_(0.8, 1.2))
    c = float(torch.empty(1).uniform_(0.8, 1.2))
    s = float(torch.empty(1).uniform_(0.8, 1.2))
    return fn_idx.tolist(), (b, c, s)


def test_draw_jitter_params_consumes_the_reference_draws():
    from dahitra_amd.datasets.xbd_pipeline import draw_jitter_params
    orders = set()
    for k in range(40):
        torch.manual_seed(k)
        want = [reference_draws() for _ in range(2)]                # pre, then post
        after = float(torch.rand(1))
        g = torch.Generator().manual_seed(k)
        got = [draw_jitter_params(g) for _ in range(2)]
        assert got == want, k
        assert float(torch.rand(1, generator=g)) == after          # the stream stands where the reference leaves it
        for order, factors in got:
            assert sorted(order) == [0, 1, 2, 3] and all(type(o) is int for o in order)
            assert all(type(f) is float and 0.8 <= f <= 1.2 and float(np.float32(f)) == f for f in factors)
            orders.add(tuple(order))
        # gen=None draws from the global generator
        torch.manual_seed(k)
        assert draw_jitter_params() == want[0] and draw_jitter_params(None) == want[1]
        assert float(torch.rand(1)) == after
    assert len(orders) > 12


def images():
    """odd sizes; noise, an image that clips at 255, one that reaches 0, and flat ones"""
    rng = np.random.RandomState(3)
    out = {"noise 37x53": rng.randint(0, 256, (37, 53, 3)).astype(np.uint8),
           "bright 19x7": rng.randint(180, 256, (19, 7, 3)).astype(np.uint8),
           "dark 5x61": rng.randint(0, 60, (5, 61, 3)).astype(np.uint8),
           "one pixel": np.asarray([[[255, 0, 128]]], dtype=np.uint8),
           "extremes 3x3": rng.choice(np.asarray([0, 255], dtype=np.uint8), size=(3, 3, 3))}
    out["dark 5x61"][rng.rand(5, 61, 3) < 0.2] = 0
    return out


FACTOR_SETS = [(0.8, 0.8, 0.8), (1.0, 1.0, 1.0), (1.2, 1.2, 1.2), (1.2, C.PINNED[0], C.PINNED[1]), (0.8, C.PINNED[1], C.PINNED[0]),
               (C.PINNED[0], 1.2, 0.8), (C.PINNED[1], 0.8, 1.2)]


@pytest.mark.parametrize("order", C.PERMS, ids=lambda o: "".join(map(str, o)))
def test_reference_equals_the_imageenhance_chain(order):
    from dahitra_amd.datasets.xbd_pipeline import jitter_reference_u8
    rng = np.random.RandomState(sum(o * 4 ** i for i, o in enumerate(order)))
    sets = FACTOR_SETS + [tuple(float(np.float32(f)) for f in rng.uniform(0.8, 1.2, 3)) for _ in range(6)]
    clipped = {0: False, 255: False}
    for name, img in images().items():
        for factors in sets:
            want = C.pil_jitter(img, order, factors)
            got = jitter_reference_u8(img, order, factors)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (name, order, factors, int((got != want).sum()))
            for v in clipped:
                clipped[v] |= bool(((want == v) & (img != v)).any())
    assert clipped == {0: True, 255: True}


def test_single_operations_and_bad_arguments():
    from dahitra_amd.datasets.xbd_pipeline import jitter_reference_u8
    img = images()["noise 37x53"]
    for op in (0, 1, 2):
        for f in (0.8, 1.0, 1.2) + C.PINNED:
            assert np.array_equal(jitter_reference_u8(img, [op], (f, f, f)), C.pil_jitter(img, [op], (f, f, f)))
    assert np.array_equal(jitter_reference_u8(img, [3], (2.0, 2.0, 2.0)), img)          # hue: nothing
    assert np.array_equal(jitter_reference_u8(img, [0, 1, 2], (1.0, 1.0, 1.0)), img)
    with pytest.raises(ValueError):
        jitter_reference_u8(img, [4], (1.0, 1.0, 1.0))
    with pytest.raises(ValueError):
        jitter_reference_u8(img[..., 0], [0], (1.0, 1.0, 1.0))


def test_contrast_takes_the_mean_of_the_image_as_it_stands():
    """brightness 1.2 clips the bright image: the mean of L after it is not 1.2 x the mean before it, and contrast after
    brightness uses the former"""
    from dahitra_amd.datasets.xbd_pipeline import _luma, jitter_reference_u8
    img = images()["bright 19x7"]
    factors = (1.2, 0.8, 1.0)
    mean = lambda a: (2 * int(_luma(a).sum()) + a.shape[0] * a.shape[1]) // (2 * a.shape[0] * a.shape[1])
    lit = jitter_reference_u8(img, [0], factors)
    assert np.array_equal(lit, C.pil_jitter(img, [0], factors)) and (lit == 255).any()
    before, after = mean(img), mean(lit)
    assert after != before and after < int(1.2 * before)                        # 255 cut it short
    want = C.pil_jitter(img, [0, 1], factors)
    assert np.array_equal(jitter_reference_u8(img, [0, 1], factors), want)
    # contrast around the mean of the ORIGINAL image gives other bytes: Pillow does use the intermediate image's
    d = np.full_like(lit, before)
    from dahitra_amd.datasets.xbd_pipeline import _blend_u8
    assert not np.array_equal(_blend_u8(d, lit, 0.8), want)
    assert np.array_equal(_blend_u8(np.full_like(lit, after), lit, 0.8), want)
    # and the order matters
    assert not np.array_equal(C.pil_jitter(img, [1, 0], factors), want)


def fused_blend_u8(d, i, factor):
    """the mutant: fma(alpha, i - d, d), one rounding (the float64 product and sum are exact)"""
    alpha = np.float64(np.float32(factor))
    d = np.broadcast_to(d, i.shape).astype(np.float64)
    t = (d + alpha * (i.astype(np.float64) - d)).astype(np.float32)
    if not 0 <= alpha <= 1:
        t = np.clip(t, np.float32(0), np.float32(255))
    return t.astype(np.int32).astype(np.uint8)


@pytest.mark.parametrize("S", [64, 70])
def test_a_contracted_blend_shows_on_the_gpu_tests_images(S, monkeypatch):
    """the fused form differs from Pillow on the images, rows and pinned factors that tests/test_xbd_jitter_gpu.py uses: a
    kernel whose blend the compiler contracted fails there"""
    from dahitra_amd.datasets import xbd_pipeline
    src, rows, cases = C.sources(), C.rows_for(S), C.jitter_cases()
    windows = [C.host_windows(src, i, row, S)[:2] for i, row in zip(C.IDX, rows)]
    for win, case in zip(windows, cases):                                       # the unfused statement is Pillow's, here too
        for img, (order, factors) in zip(win, case):
            assert np.array_equal(xbd_pipeline.jitter_reference_u8(img, order, factors), C.pil_jitter(img, order, factors))
    monkeypatch.setattr(xbd_pipeline, "_blend_u8", fused_blend_u8)
    differing = 0
    for win, case in zip(windows, cases):
        for img, (order, factors) in zip(win, case):
            bad = int((xbd_pipeline.jitter_reference_u8(img, order, factors) != C.pil_jitter(img, order, factors)).sum())
            differing += bad > 0
    print("images on which the fused blend differs from Pillow: %d of %d" % (differing, 2 * len(cases)))
    assert differing >= 1


def cpu_pipe():
    """a pipeline object over host tensors: make_batch's checks on `jitter` come before anything touches the device"""
    from dahitra_amd.datasets.xbd_pipeline import GpuXbdPipeline
    pipe = GpuXbdPipeline.__new__(GpuXbdPipeline)
    pipe.pre = pipe.post = torch.zeros(2, 80, 96, 3, dtype=torch.uint8)
    pipe.pre_mask = pipe.post_label = torch.zeros(2, 80, 96, dtype=torch.uint8)
    pipe.files, pipe._zero_lbl, pipe._jitter_ws = ["a", "b"], None, None
    return pipe


def test_make_batch_rejects_bad_jitter():
    from dahitra_amd.datasets.xbd_pipeline import JITTER_WORDS, jitter_table
    pipe = cpu_pipe()
    ok = ([0, 3, 2, 1], (1.0, 0.9, 1.1))
    for bad in (dict(jitter=[(ok, ok), None], train=False),                      # validation batches are not jittered
                dict(jitter=[(ok, ok)]),                                         # one entry for two samples
                dict(jitter=[(ok, ok), None, None]),
                dict(jitter=[(ok, ([0, 1, 2, 2], ok[1])), None]),                # no permutation
                dict(jitter=[(ok, ([0, 1, 2], ok[1])), None]),
                dict(jitter=[None, (([0, 1, 2, 4], ok[1]), ok)]),
                dict(jitter=[None, (ok, (ok[0], (1.0, float("nan"), 1.0)))]),    # a factor that is not finite
                dict(jitter=[None, (ok, (ok[0], (float("inf"), 1.0, 1.0)))]),
                dict(jitter=[None, (ok, (ok[0], (1e39, 1.0, 1.0)))]),            # ... as a float32
                dict(jitter=[None, (ok, (ok[0], (1.0, 1.0)))]),
                dict(jitter=[None, (ok,)])):
        with pytest.raises(ValueError):
            pipe.make_batch([0, 1], 64, **bad)
    table = jitter_table([None, (ok, ([3, 2, 0, 1], (0.8, C.PINNED[0], 1.2)))])
    assert table.dtype == np.int32 and table.shape == (2, 2, JITTER_WORDS) and not table[0].any()
    assert table[1, 0].tolist()[:4] == [1, 0, 2, 1] and table[1, 1].tolist()[:4] == [1, 2, 0, 1] and table[1, 1, 7] == 0
    assert table[1, 1, 4:7].view(np.float32).tolist() == [float(np.float32(0.8)), float(np.float32(C.PINNED[0])), float(np.float32(1.2))]
    assert table[1, 1, 5] == 1064503735
    assert jitter_table([None, None]) is None
