"""The device loader's Gaussian blur on the MI355X (dh_augment_pairs_blur_u8, csrc/augment_blur.hip): byte for byte the
reference's training augmentation (fixtures written by the reference's code, tests/golden/data_pipeline.npz) and Pillow's
ImageFilter.GaussianBlur on the cropped, flipped window -- crop windows inside a larger source, windows that are no multiple of
the tile, a one-pixel-high window -- and the loader surface.  Every comparison is exact: the blur is integer arithmetic and the
normalisation is the unblurred kernel's expression."""
import hashlib
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image, ImageFilter

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def u8(t):
    """normalised float tensor -> the uint8 image it came from, as oracle/make_data_golden.py"""
    return (t.cpu() * 0.5 + 0.5).mul(255).round().clamp(0, 255).to(torch.uint8).numpy()


def sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def pil_blur(img, r):
    return np.asarray(Image.fromarray(np.ascontiguousarray(img)).filter(ImageFilter.GaussianBlur(r)))


def normalise(img_hwc):
    """uint8 HWC -> float32 CHW, the kernels' expression in float32 numpy"""
    x = img_hwc.transpose(2, 0, 1).astype(np.float32)
    return (x / np.float32(255) - np.float32(0.5)) / np.float32(0.5)


def test_reference_fixture_training_batch():
    from dahitra_amd.datasets.gpu_pipeline import GpuPairPipeline, box_blur_weights
    gold = np.load(os.path.join(G, "data_pipeline.npz"))
    names = gold["names"].tolist()
    pipe = GpuPairPipeline.from_dataset_root(os.path.join(G, "levir"), "train", device="cuda:0", names=names)
    flips, radii = [], []
    for i in range(4):
        random.seed(100 + i)                         # CDDataAugmentation.transform's draws: hflip, vflip, `> 0`, radius
        flips.append([int(random.random() > 0.5), int(random.random() > 0.5)])
        assert random.random() > 0
        radii.append(random.random())
    assert [box_blur_weights(r) for r in radii] == [(13993602, 1391807), (12002798, 2387209), (13938140, 1419538),
                                                    (13756994, 1510111)]
    batch = pipe.make_batch([0, 1, 2, 3], 256, flips, blur=radii)
    a, b, lab = u8(batch["A"]), u8(batch["B"]), batch["L"].cpu().numpy()
    for i in range(4):
        assert sha(a[i]) == str(gold["train_%d_A" % i]) and sha(b[i]) == str(gold["train_%d_B" % i])
        assert sha(lab[i]) == str(gold["train_%d_L" % i])
    assert np.array_equal(a[1], gold["train_1_A_u8"]) and np.array_equal(b[1], gold["train_1_B_u8"])
    assert np.array_equal(lab[1], gold["train_1_L_u8"])
    assert batch["name"] == names
    # the float values themselves are exactly (u8 / 255 - 0.5) / 0.5
    assert np.array_equal(batch["A"][1].cpu().numpy(), normalise(gold["train_1_A_u8"].transpose(1, 2, 0)))


def test_window_border_is_not_the_source_border():
    """crops of the 1024 x 1024 tile (32 x 32 blocks of constant colour): a halo read from outside the window changes bytes"""
    from dahitra_amd.datasets.gpu_pipeline import GpuPairPipeline
    root = os.path.join(G, "levir1024")
    pipe = GpuPairPipeline.from_dataset_root(root, "test", device="cuda:0")
    src = {s: np.asarray(Image.open(os.path.join(root, "test", s, "tile_0.png")).convert("RGB")) for s in ("A", "B")}
    lab = np.array(Image.open(os.path.join(root, "test", "label", "tile_0.png")), dtype=np.uint8) // 255
    for patch in (None, 0, 5, 15):
        x0, y0 = (256 * (patch // 4), 256 * (patch % 4)) if patch else (256, 256)
        got = pipe.make_batch([0], 256, patch=patch, blur=[0.9])
        for s in ("A", "B"):
            crop = src[s][y0:y0 + 256, x0:x0 + 256]
            want = pil_blur(crop, 0.9)
            assert not np.array_equal(want, crop)
            assert np.array_equal(got[s][0].cpu().numpy(), normalise(want)), (patch, s)
        assert np.array_equal(got["L"][0, 0].cpu().numpy(), lab[y0:y0 + 256, x0:x0 + 256])


@pytest.mark.parametrize("S,H,W,h,w,x0,y0", [(3, 50, 70, 37, 45, 5, 9),           # odd sizes inside one tile
                                             (3, 90, 170, 70, 150, 11, 13),       # several tiles both ways, ragged last tiles
                                             (3, 50, 70, 1, 5, 5, 9),             # one row
                                             (3, 40, 90, 33, 68, 2, 3)])          # w % 4 == 0 (wide stores), one pixel past a tile
def test_c_abi_on_noise_equals_pillow_on_the_cropped_flipped_window(S, H, W, h, w, x0, y0):
    from dahitra_amd import ops
    from dahitra_amd.datasets.gpu_pipeline import blur_table
    rng = np.random.RandomState(H * 1000 + w)
    a = rng.randint(0, 256, (S, H, W, 3)).astype(np.uint8)
    b = rng.randint(0, 256, (S, H, W, 3)).astype(np.uint8)
    lab = rng.randint(0, 2, (S, H, W)).astype(np.uint8)
    idx = [2, 0, 1, 0]
    flips = [[0, 0], [1, 0], [0, 1], [1, 1]]
    radii = [0.0, 0.31, 0.77, 0.999]
    N = 4
    dev = "cuda:0"
    ta, tb, tl = (torch.from_numpy(x).to(dev) for x in (a, b, lab))
    tidx = torch.tensor(idx, dtype=torch.int32, device=dev)
    params = torch.tensor([[x0, y0, hf, vf] for hf, vf in flips], dtype=torch.int32, device=dev)
    table = blur_table(radii).to(dev)

    def run(name, *extra):
        oa = torch.full((N, 3, h, w), float("nan"), dtype=torch.float32, device=dev)
        ob = torch.full_like(oa, float("nan"))
        ol = torch.full((N, 1, h, w), 255, dtype=torch.uint8, device=dev)
        ops._call(name, ops.P(ta), ops.P(tb), ops.P(tl), ops.P(tidx), ops.P(params), *extra, N, H, W, h, w,
                  ops.P(oa), ops.P(ob), ops.P(ol), ops.S())
        torch.cuda.synchronize()
        return oa.cpu().numpy(), ob.cpu().numpy(), ol.cpu().numpy()

    oa, ob, ol = run("dh_augment_pairs_blur_u8", ops.P(table))
    pa, pb, pl = run("dh_augment_pairs_u8")
    for n in range(N):
        hf, vf = flips[n]

        def window(x):
            x = x[idx[n], y0:y0 + h, x0:x0 + w]
            x = x[:, ::-1] if hf else x
            return x[::-1] if vf else x

        for got, src in ((oa, a), (ob, b)):
            want = normalise(pil_blur(window(src), radii[n]))
            assert np.array_equal(got[n], want), (n, np.argwhere(got[n] != want)[:4])
        assert np.array_equal(ol[n, 0], window(lab))
    # radius 0 is the unblurred kernel bit for bit; the labels always are
    assert np.array_equal(oa[0].view(np.uint32), pa[0].view(np.uint32))
    assert np.array_equal(ob[0].view(np.uint32), pb[0].view(np.uint32))
    assert np.array_equal(ol, pl)


@pytest.mark.parametrize("h,w", [(16, 16), (24, 40)])
@pytest.mark.parametrize("blur", [False, True])
def test_wrapper_gives_the_raw_entrys_bytes(blur, h, w):
    """ops.augment_pairs against dh_augment_pairs_u8 / dh_augment_pairs_blur_u8 on the same arguments, into fresh outputs and into
    sentinel-filled ones: a 16 x 16 window of 24 x 40 sources and the whole image; a repeated index, every flip"""
    from dahitra_amd import ops
    from dahitra_amd.datasets.gpu_pipeline import blur_table
    rng = np.random.RandomState(31)
    dev = "cuda:0"
    ta, tb = (torch.from_numpy(rng.randint(0, 256, (3, 24, 40, 3)).astype(np.uint8)).to(dev) for _ in range(2))
    tl = torch.from_numpy(rng.randint(0, 2, (3, 24, 40)).astype(np.uint8)).to(dev)
    tidx = torch.tensor([2, 0, 2], dtype=torch.int32, device=dev)
    x0, y0 = (40 - w, 24 - h)
    params = torch.tensor([[x0, y0, 1, 0], [x0 // 2, y0 // 2, 0, 1], [0, 0, 1, 1]], dtype=torch.int32, device=dev)
    table = blur_table([0.31, 0.0, 0.999]).to(dev) if blur else None

    def sentinels():
        return (torch.full((3, 3, h, w), float("nan"), dtype=torch.float32, device=dev),
                torch.full((3, 3, h, w), float("nan"), dtype=torch.float32, device=dev),
                torch.full((3, 1, h, w), 255, dtype=torch.uint8, device=dev))

    want = sentinels()
    ops._call(*(("dh_augment_pairs_blur_u8",) if blur else ("dh_augment_pairs_u8",)), ops.P(ta), ops.P(tb), ops.P(tl), ops.P(tidx),
              ops.P(params), *((ops.P(table),) if blur else ()), 3, 24, 40, h, w, *(ops.P(t) for t in want), ops.S())
    torch.cuda.synchronize()
    assert not torch.isnan(want[0]).any() and not torch.isnan(want[1]).any() and int(want[2].max()) <= 1
    given = sentinels()
    for got in (ops.augment_pairs(ta, tb, tl, tidx, params, h, w, table),
                ops.augment_pairs(ta, tb, tl, tidx, params, h, w, table, out_a=given[0], out_b=given[1], out_l=given[2])):
        torch.cuda.synchronize()
        assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
        assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)) and torch.equal(got[2], want[2])
    assert all(g is o for g, o in zip(got, given))
    # without the label stack, as the header allows: the images alone
    got = ops.augment_pairs(ta, tb, None, tidx, params, h, w, table)
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and got[2] is None
    with pytest.raises(ValueError, match="out_l"):
        ops.augment_pairs(ta, tb, None, tidx, params, h, w, table, out_l=given[2])


def test_loader_surface():
    from dahitra_amd.datasets.gpu_pipeline import GpuPairLoader, GpuPairPipeline
    pipe = GpuPairPipeline.from_dataset_root(os.path.join(G, "levir"), "train", device="cuda:0")

    def epoch(train, blur, seed=5):
        return list(GpuPairLoader(pipe, 3, 256, train=train, generator=torch.Generator().manual_seed(seed), blur=blur))

    one, two, plain = epoch(True, True), epoch(True, True), epoch(True, False)
    assert [b["A"].shape[0] for b in one] == [3, 1]
    for x, y, p in zip(one, two, plain):
        assert x["name"] == y["name"] == p["name"]
        assert torch.equal(x["A"], y["A"]) and torch.equal(x["B"], y["B"]) and torch.equal(x["L"], y["L"])
    # the first batch draws the same permutation and flips as the unblurred loader's (the radii are drawn after them; later batches
    # then see a generator that has advanced by those radii): same labels, other images
    assert torch.equal(one[0]["L"], plain[0]["L"])
    assert not torch.equal(one[0]["A"], plain[0]["A"]) and not torch.equal(one[0]["B"], plain[0]["B"])
    whole = [list(GpuPairLoader(pipe, 4, 256, train=True, generator=torch.Generator().manual_seed(5), blur=bl)) for bl in (True, False)]
    assert len(whole[0]) == len(whole[1]) == 1 and whole[0][0]["name"] == whole[1][0]["name"]
    assert torch.equal(whole[0][0]["L"], whole[1][0]["L"]) and not torch.equal(whole[0][0]["A"], whole[1][0]["A"])
    for x, p in zip(epoch(False, True), epoch(False, False)):
        assert torch.equal(x["A"], p["A"]) and torch.equal(x["B"], p["B"]) and torch.equal(x["L"], p["L"])
    # blur=None is the unblurred entry point, called as before
    from dahitra_amd import ops
    flips = [[1, 0], [0, 1], [1, 1], [0, 0]]
    got = pipe.make_batch([3, 2, 1, 0], 256, flips, blur=None)
    idx = torch.tensor([3, 2, 1, 0], dtype=torch.int32, device="cuda:0")
    params = torch.tensor([[0, 0] + f for f in flips], dtype=torch.int32, device="cuda:0")
    oa = torch.empty(4, 3, 256, 256, dtype=torch.float32, device="cuda:0")
    ob, ol = torch.empty_like(oa), torch.empty(4, 1, 256, 256, dtype=torch.uint8, device="cuda:0")
    ops._call("dh_augment_pairs_u8", ops.P(pipe.a), ops.P(pipe.b), ops.P(pipe.l), ops.P(idx), ops.P(params), 4, 256, 256, 256,
              256, ops.P(oa), ops.P(ob), ops.P(ol), ops.S())
    assert torch.equal(got["A"], oa) and torch.equal(got["B"], ob) and torch.equal(got["L"], ol)
    with pytest.raises(ValueError):
        pipe.make_batch([0, 1], 256, blur=[0.5])
    with pytest.raises(ValueError):
        pipe.make_batch([0], 256, blur=[1.5])
