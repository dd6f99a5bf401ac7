"""The device loader's Gaussian blur, host side (no GPU): gpu_pipeline.box_blur_weights against Pillow's
ImageFilter.GaussianBlur through a numpy model of the six 3-tap passes the kernel runs (three along the rows, three along the
columns, uint8 after every pass, the edge pixel replicated in every pass), against the reference-written fixtures of
tests/golden/data_pipeline.npz, and the order of the loader's random draws."""
import hashlib
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image, ImageFilter

from dahitra_amd.datasets.gpu_pipeline import GpuPairLoader, GpuPairPipeline, blur_table, box_blur_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def model_blur(img, ww, fw):
    """HxWxC uint8 -> the six passes in unsigned 32-bit arithmetic"""
    x = img.astype(np.uint32)
    for axis in (1, 0):
        for _ in range(3):
            n = x.shape[axis]
            p = np.concatenate([x.take([0], axis), x, x.take([n - 1], axis)], axis)        # replicate THIS pass's edge
            x = (x * np.uint32(ww) + (p.take(range(0, n), axis) + p.take(range(2, n + 2), axis)) * np.uint32(fw)
                 + np.uint32(1 << 23)) >> np.uint32(24)
    return x.astype(np.uint8)


def pil_blur(img, r):
    return np.asarray(Image.fromarray(img).filter(ImageFilter.GaussianBlur(r)))


def sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def replay_draws(i):
    """the draws CDDataAugmentation.transform makes for training item i of the fixture: hflip, vflip, the `> 0` draw, radius"""
    random.seed(100 + i)
    hf, vf = random.random() > 0.5, random.random() > 0.5
    assert random.random() > 0
    return hf, vf, random.random()


def test_model_with_box_blur_weights_equals_pillow():
    random.seed(7)
    rng = np.random.RandomState(7)
    radii = [0.0] + [random.random() for _ in range(200)]
    for r in radii:
        ww, fw = box_blur_weights(r)
        assert 0 < ww <= 1 << 24 and fw >= 0 and ww + 2 * fw <= 1 << 24
        for shape in ((17, 23, 3), (1, 9, 3)):
            img = rng.randint(0, 256, shape).astype(np.uint8)
            assert np.array_equal(model_blur(img, ww, fw), pil_blur(img, r)), (r, shape)
    assert box_blur_weights(0.0) == (1 << 24, 0)
    img = rng.randint(0, 256, (17, 23, 3)).astype(np.uint8)
    assert np.array_equal(model_blur(img, 1 << 24, 0), img) and np.array_equal(pil_blur(img, 0.0), img)


def test_extreme_radii_equal_pillow():
    """the radii at the ends of the float32 derivation, and the part of [1, sqrt(2)) the reference never draws"""
    rng = np.random.RandomState(3)
    for r in (0, 1e-9, 0.999999, 0.5, 1e-3, 0.25, 1.0 - 2.0 ** -24, 1.0, 1.2, 1.4142):
        ww, fw = box_blur_weights(r)
        for shape in ((17, 23, 3), (1, 9, 3), (5, 1, 3)):
            img = rng.randint(0, 256, shape).astype(np.uint8)
            assert np.array_equal(model_blur(img, ww, fw), pil_blur(img, r)), (r, shape)
            hard = (rng.randint(0, 2, shape) * 255).astype(np.uint8)
            assert np.array_equal(model_blur(hard, ww, fw), pil_blur(hard, r)), (r, shape)
    assert box_blur_weights(0.25) == (16427691, 174762)          # (a float64 derivation gives 16427690)


def test_fixture_replay_equals_reference_hashes():
    gold = np.load(os.path.join(G, "data_pipeline.npz"))
    names = gold["names"].tolist()
    want_w = [(13993602, 1391807), (12002798, 2387209), (13938140, 1419538), (13756994, 1510111)]
    for i in range(4):
        hf, vf, r = replay_draws(i)
        assert box_blur_weights(r) == want_w[i]
        for sub in ("A", "B"):
            img = np.asarray(Image.open(os.path.join(G, "levir", "train", sub, names[i])).convert("RGB"))
            img = img[:, ::-1] if hf else img
            img = img[::-1] if vf else img
            out = model_blur(img, *box_blur_weights(r)).transpose(2, 0, 1)
            assert sha(out) == str(gold["train_%d_%s" % (i, sub)])
            if i == 1:
                assert np.array_equal(out, gold["train_1_%s_u8" % sub])


def test_bad_radii_raise():
    for r in (1.5, -0.1, float("nan"), float("inf"), 2.0 ** 0.5 + 1e-3):
        with pytest.raises(ValueError):
            box_blur_weights(r)
    with pytest.raises(ValueError):
        blur_table([0.3, 1.5])
    t = blur_table([0.0, 0.25])
    assert t.dtype == torch.int32 and t.tolist() == [[1 << 24, 0], [16427691, 174762]]


class _StubPipe(GpuPairPipeline):
    """records what the loaders hand to make_batch; no device"""

    def __init__(self, n):
        self.n, self.calls = n, []

    def __len__(self):
        return self.n

    def make_batch(self, indices, img_size, flips=None, patch=None, blur=None):
        self.calls.append((list(indices), None if flips is None else torch.as_tensor(flips).tolist(), blur))
        return len(self.calls)


# permutation and flips of one epoch over 7 pairs at batch 3 from torch.Generator().manual_seed(11), recorded with the loader as it
# was before it knew about the blur
PARENT_EPOCH = [([4, 0, 2], [[1, 0], [1, 1], [0, 1]]), ([6, 3, 1], [[0, 0], [1, 1], [0, 1]]), ([5], [[1, 1]])]
PARENT_EPOCH_2 = [([5, 0, 1], [[0, 0], [0, 1], [1, 0]]), ([4, 3, 6], [[0, 0], [1, 0], [1, 0]]), ([2], [[0, 0]])]


def test_draw_order_without_blur_is_unchanged_and_radii_follow_the_flips():
    for run in ("loader", "batches"):
        p = _StubPipe(7)
        g = torch.Generator().manual_seed(11)
        if run == "loader":
            ld = GpuPairLoader(p, 3, 256, True, g)
            list(ld)
            list(ld)
            assert [c[:2] for c in p.calls[3:]] == PARENT_EPOCH_2
        else:
            list(p.batches(3, 256, train=True, generator=g))
        assert [c[:2] for c in p.calls[:3]] == PARENT_EPOCH and all(c[2] is None for c in p.calls)
    # blur on: the first batch's permutation and flips are the same draws, its radii are the next ones
    g = torch.Generator().manual_seed(11)
    torch.randperm(7, generator=g)
    torch.rand(3, 2, generator=g)
    want_radii = torch.rand(3, generator=g).tolist()
    for run in ("loader", "batches"):
        p = _StubPipe(7)
        g = torch.Generator().manual_seed(11)
        list(GpuPairLoader(p, 3, 256, True, g, blur=True) if run == "loader" else
             p.batches(3, 256, train=True, generator=g, blur=True))
        assert p.calls[0][:2] == PARENT_EPOCH[0] and p.calls[0][2] == want_radii
        assert [c[0] for c in p.calls] == [c[0] for c in PARENT_EPOCH]                # same permutation
        assert all(len(c[2]) == len(c[0]) and all(0.0 <= r < 1.0 for r in c[2]) for c in p.calls)
    # evaluation never blurs, and draws nothing
    for run in ("loader", "batches"):
        p = _StubPipe(7)
        list(GpuPairLoader(p, 3, 256, False, blur=True) if run == "loader" else p.batches(3, 256, train=False, blur=True))
        assert p.calls == [([0, 1, 2], None, None), ([3, 4, 5], None, None), ([6], None, None)]
