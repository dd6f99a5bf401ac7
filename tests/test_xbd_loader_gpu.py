"""The xBD device loader on the MI355X (dh_xbd_augment_u8, csrc/augment_xbd.hip; datasets/xbd_pipeline.py): byte for byte what
TrainData / ValData.__getitem__ (xBD_code/train.py:99-183, 194-244) compute with Pillow -- crop, flips, TF.resized_crop =
crop(box).resize(BILINEAR) on images, label and pre mask, the mask channels, preprocess_inputs -- restated here on the host.
Every comparison is exact: the resize is integer arithmetic and the normalisation is two float32 roundings."""
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def blocky(rng, n, h, w, values):
    """constant in 8 x 8 blocks, so that the resize blends at block borders"""
    small = rng.choice(np.asarray(values, dtype=np.uint8), size=(n, -(-h // 8), -(-w // 8)))
    return np.ascontiguousarray(np.kron(small, np.ones((1, 8, 8), dtype=np.uint8))[:, :h, :w])


def sources(n, H, W, seed):
    """pre, post (noise), pre mask (0 / 255), post label (0 .. 4)"""
    rng = np.random.RandomState(seed)
    pre = rng.randint(0, 256, (n, H, W, 3)).astype(np.uint8)
    post = rng.randint(0, 256, (n, H, W, 3)).astype(np.uint8)
    return pre, post, blocky(rng, n, H, W, [0, 255]), blocky(rng, n, H, W, [0, 1, 2, 3, 4])


def preprocess_inputs(x):
    """xBD_code/utils.py:112-116"""
    x = np.asarray(x, dtype='float32')
    x /= 127
    x -= 1
    return x


def host_sample(src, i, row, S, train):
    """one sample as the reference builds it: (img [6, S, S] float32, msk [5, S, S] uint8, lbl_msk [S, S])"""
    x0, y0, hf, vf, rs, top, left, bh, bw = row

    def window(a):
        a = a[i, y0:y0 + S, x0:x0 + S]
        a = a[:, ::-1] if hf else a
        a = a[::-1] if vf else a
        a = np.ascontiguousarray(a)
        if rs:
            a = np.asarray(Image.fromarray(a).crop((left, top, left + bw, top + bh)).resize((S, S), Image.BILINEAR))
        return a

    img1, img2, msk0, lbl_msk1 = (window(a) for a in src)
    chan = [msk0] + [np.where(lbl_msk1 == k, 255, 0).astype(np.uint8) for k in (1, 2, 3, 4)]
    msk = np.stack(chan, axis=2) > 127
    if train:                                              # train.py:162-174
        msk[..., 0] = False
        msk[..., 0][msk[..., 1:].max(axis=2)] = True
        lbl = (msk * 1).argmax(axis=2)
        assert not lbl.any()
    else:                                                  # train.py:233-235
        lbl = (msk * 1)[..., 1:].argmax(axis=2)
    img = preprocess_inputs(np.concatenate([img1, img2], axis=2)).transpose(2, 0, 1)
    return img, (msk * 1).transpose(2, 0, 1).astype(np.uint8), lbl.astype(np.uint8)


def call_abi(src, idx, rows, S, train):
    """dh_xbd_augment_u8 on outputs pre-filled with NaN / 255: an element the kernel does not write shows"""
    from dahitra_amd import ops
    from dahitra_amd.datasets.xbd_pipeline import check_params, coef_table
    n, (_, H, W, _) = len(idx), src[0].shape
    pre, post, pmask, label = (torch.from_numpy(a).to(DEV) for a in src)
    p = check_params(rows, H, W, S)
    coef = coef_table(p, S)
    coef = coef.to(DEV) if coef is not None else None
    tidx, p = torch.tensor(idx, dtype=torch.int32, device=DEV), p.to(DEV)
    img = torch.full((n, 6, S, S), float("nan"), dtype=torch.float32, device=DEV)
    msk = torch.full((n, 5, S, S), 255, dtype=torch.uint8, device=DEV)
    lbl = torch.full((n, S, S), 255, dtype=torch.uint8, device=DEV)
    ops._call("dh_xbd_augment_u8", ops.P(pre), ops.P(post), ops.P(None if train else pmask), ops.P(label), ops.P(tidx), ops.P(p),
              ops.P(coef), n, H, W, S, 0 if train else 1, ops.P(img), ops.P(msk), ops.P(None if train else lbl), ops.S())
    torch.cuda.synchronize()
    return img.cpu().numpy(), msk.cpu().numpy(), lbl.cpu().numpy()


def compare(src, idx, rows, S, train):
    img, msk, lbl = call_abi(src, idx, rows, S, train)
    for n, (i, row) in enumerate(zip(idx, rows)):
        wimg, wmsk, wlbl = host_sample(src, i, row, S, train)
        bad = np.argwhere(img[n].view(np.uint32) != wimg.view(np.uint32))
        assert bad.size == 0, ("img", n, row, len(bad), bad[:4].tolist())
        bad = np.argwhere(msk[n] != wmsk)
        assert bad.size == 0, ("msk", n, row, len(bad), bad[:4].tolist())
        if train:
            assert (lbl[n] == 255).all()                   # train mode leaves out_lbl alone
        else:
            assert np.array_equal(lbl[n], wlbl), ("lbl", n, row)
    return img, msk, lbl


# x0, y0, hflip, vflip, resize, top, left, height, width at S = 64 inside 80 x 96 sources
ROWS_64 = [[5, 9, 0, 0, 0, 0, 0, 64, 64],              # no augmentation at crop origin (5, 9)
           [32, 16, 1, 0, 0, 0, 0, 64, 64],            # flips only, the window in the source's last rows and columns
           [0, 0, 0, 1, 1, 0, 13, 64, 51],             # box (top 0, left 13): horizontal pass only
           [7, 3, 0, 0, 1, 9, 0, 55, 64],              # box (top 9, left 0): vertical pass only
           [11, 2, 1, 1, 1, 13, 7, 51, 57],            # box (13, 7) with both flips, as the reference draws it (crop - x, crop - y)
           [20, 16, 1, 0, 1, 6, 11, 51, 45]]           # a box of height 51 and width 45 at (6, 11), not reaching the crop's end


def test_c_abi_train_equals_pillow_on_the_cropped_flipped_window():
    src = sources(3, 80, 96, seed=1)
    img, msk, _ = compare(src, [2, 0, 1, 0, 2, 1], ROWS_64, 64, train=True)
    assert set(np.unique(msk)) == {0, 1}
    # the resize does blend: a resized sample differs from the crop it came from, an identity box does not
    plain = call_abi(src, [2, 0, 1, 0, 2, 1], [r[:4] + [0, 0, 0, 64, 64] for r in ROWS_64], 64, train=True)
    assert np.array_equal(img[:2].view(np.uint32), plain[0][:2].view(np.uint32))
    for n in (2, 3, 4, 5):
        assert not np.array_equal(img[n], plain[0][n]) and not np.array_equal(msk[n], plain[1][n])
    ident = call_abi(src, [2, 0, 1, 0, 2, 1], [r[:4] + [1, 0, 0, 64, 64] for r in ROWS_64], 64, train=True)
    assert np.array_equal(ident[0].view(np.uint32), plain[0].view(np.uint32)) and np.array_equal(ident[1], plain[1])


def test_c_abi_flip_combinations_without_a_box():
    src = sources(3, 80, 96, seed=2)
    compare(src, [0, 1, 2, 1], [[3, 1, hf, vf, 0, 0, 0, 64, 64] for hf, vf in ((0, 0), (1, 0), (0, 1), (1, 1))], 64, train=True)


def test_c_abi_several_tiles_and_a_ragged_last_tile():
    """S = 160 is 2.5 tiles wide and 5 tiles high"""
    src = sources(2, 200, 230, seed=3)
    compare(src, [1, 0, 1], [[70, 40, 0, 1, 1, 37, 31, 123, 129],
                             [17, 33, 1, 0, 0, 0, 0, 160, 160],
                             [0, 0, 1, 1, 1, 159, 159, 1, 1]],          # a one-pixel box: every output is that pixel
            160, train=True)


def test_c_abi_odd_size_takes_the_narrow_stores():
    """S = 61: neither a multiple of 4 (float4 stores) nor of 16 (mask stores), last tile column 61 % 4 = 1 wide"""
    src = sources(2, 80, 96, seed=4)
    compare(src, [1, 0], [[35, 19, 1, 0, 1, 5, 3, 50, 58], [2, 1, 0, 1, 0, 0, 0, 61, 61]], 61, train=True)
    compare(src, [0, 1], [[35, 19, 0, 0, 1, 0, 0, 61, 47], [2, 1, 0, 1, 0, 0, 0, 61, 61]], 61, train=False)


def test_c_abi_val_mode_whole_image():
    src = sources(3, 64, 64, seed=5)
    rows = [[0, 0, 0, 0, 0, 0, 0, 64, 64]] * 3
    img, msk, lbl = compare(src, [0, 1, 2], rows, 64, train=False)
    pmask, label = src[2], src[3]
    assert np.array_equal(msk[:, 0], (pmask > 127).astype(np.uint8))          # msk[0] comes from the pre mask
    for k in (1, 2, 3, 4):
        assert np.array_equal(msk[:, k], (label == k).astype(np.uint8))
    assert np.array_equal(lbl, np.where(label >= 1, label - 1, 0))             # lbl - 1 on the buildings, 0 elsewhere
    assert lbl.max() == 3 and not np.array_equal(msk[:, 0], msk[:, 1:].max(1))
    # the kernel's val mode resizes the pre mask like the label, though ValData never asks for it
    compare(src, [2, 0], [[0, 0, 1, 0, 1, 6, 11, 51, 45], [0, 0, 0, 0, 0, 0, 0, 64, 64]], 64, train=False)


def test_c_abi_refuses_bad_arguments():
    from dahitra_amd import _lib, ops
    z = torch.zeros(64, dtype=torch.uint8, device=DEV)
    f = torch.zeros(64, dtype=torch.float32, device=DEV)
    i = torch.zeros(16, dtype=torch.int32, device=DEV)

    def call(N=1, H=8, W=8, S=2, mode=0, pmask=None, lbl=None, pre=z):
        ops._call("dh_xbd_augment_u8", ops.P(pre), ops.P(z), ops.P(pmask), ops.P(z), ops.P(i), ops.P(i), ops.P(None), N, H, W,
                  S, mode, ops.P(f), ops.P(z), ops.P(lbl), ops.S())

    for bad in (dict(S=9), dict(N=0), dict(mode=2), dict(mode=1), dict(mode=1, pmask=z), dict(pre=None)):
        with pytest.raises(_lib.HipLibraryError):
            call(**bad)


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("S", [32, 37])
def test_wrapper_gives_the_raw_entrys_bytes(S, train):
    """ops.xbd_augment against dh_xbd_augment_u8 on the same arguments, into fresh outputs and into sentinel-filled ones.  40 x 48
    sources; S = 32 takes the vector stores, S = 37 the scalar ones; a repeated index, a sample with both flips, one with the box"""
    from dahitra_amd import ops
    from dahitra_amd.datasets.xbd_pipeline import check_params, coef_table
    src = sources(3, 40, 48, seed=11)
    idx = [2, 0, 2]
    rows = [[48 - S, 40 - S, 0, 0, 0, 0, 0, S, S], [2, 1, 1, 1, 0, 0, 0, S, S], [0, 3, 0, 1, 1, 4, 6, S - 7, S - 10]]
    want = compare(src, idx, rows, S, train)                                  # the raw entry, and equal to Pillow
    pre, post, pmask, label = (torch.from_numpy(a).to(DEV) for a in src)
    p = check_params(rows, 40, 48, S)
    coef, tidx, p = coef_table(p, S).to(DEV), torch.tensor(idx, dtype=torch.int32, device=DEV), p.to(DEV)

    def same_bytes(got):
        torch.cuda.synchronize()
        assert np.array_equal(got[0].cpu().numpy().view(np.int32), want[0].view(np.int32))
        assert np.array_equal(got[1].cpu().numpy(), want[1])

    fresh = ops.xbd_augment(pre, post, pmask, label, tidx, p, coef, S, train)
    same_bytes(fresh)
    assert fresh[2] is None if train else np.array_equal(fresh[2].cpu().numpy(), want[2])
    out = (torch.full((3, 6, S, S), float("nan"), dtype=torch.float32, device=DEV),
           torch.full((3, 5, S, S), 255, dtype=torch.uint8, device=DEV), torch.full((3, S, S), 255, dtype=torch.uint8, device=DEV))
    given = ops.xbd_augment(pre, post, pmask, label, tidx, p, coef, S, train, out_img=out[0], out_msk=out[1], out_lbl=out[2])
    assert all(g is o for g, o in zip(given, out))
    same_bytes(given)
    assert np.array_equal(out[2].cpu().numpy(), want[2])                       # train mode: still the sentinel, as the raw call's
    assert bool((out[2] == 255).all()) == train


EPOCH_SEED = 0          # an epoch of three samples with a resized and an unresized one (asserted where it is used)


def make_pipe(src):
    from dahitra_amd.datasets.xbd_pipeline import GpuXbdPipeline
    return GpuXbdPipeline(*(torch.from_numpy(a).to(DEV) for a in src), files=["s%d" % i for i in range(len(src[0]))])


def test_loader_surface():
    from dahitra_amd import datasets
    from dahitra_amd.datasets.xbd_pipeline import GpuXbdPipeline
    assert datasets.GpuXbdPipeline is GpuXbdPipeline and callable(datasets.resize_coeffs) and callable(datasets.draw_train_params)
    src = sources(3, 80, 96, seed=1)
    pipe = make_pipe(src)
    assert len(pipe) == 3
    idx = [2, 0, 1, 0, 2, 1]
    got = pipe.make_batch(idx, 64, ROWS_64)
    img, msk, _ = call_abi(src, idx, ROWS_64, 64, train=True)
    assert got["img"].dtype == torch.float32 and got["msk"].dtype == torch.uint8 and got["lbl_msk"].dtype == torch.uint8
    assert np.array_equal(got["img"].cpu().numpy().view(np.uint32), img.view(np.uint32))
    assert np.array_equal(got["msk"].cpu().numpy(), msk)
    assert got["lbl_msk"].shape == (6, 64, 64) and not got["lbl_msk"].any()
    assert got["fn"] == ["s2", "s0", "s1", "s0", "s2", "s1"]
    # no params: the crop at the origin, unaugmented; val mode fills lbl_msk
    plain = pipe.make_batch([1], 64)
    want = host_sample(src, 1, [0, 0, 0, 0, 0, 0, 0, 64, 64], 64, True)
    assert np.array_equal(plain["img"][0].cpu().numpy(), want[0]) and np.array_equal(plain["msk"][0].cpu().numpy(), want[1])
    val = pipe.make_batch([1], 64, train=False)
    want = host_sample(src, 1, [0, 0, 0, 0, 0, 0, 0, 64, 64], 64, False)
    assert np.array_equal(val["msk"][0].cpu().numpy(), want[1]) and np.array_equal(val["lbl_msk"][0].cpu().numpy(), want[2])

    # a validation epoch: the samples in order, whole (square) images, ValData's masks
    vsrc = sources(3, 64, 64, seed=5)
    vals = list(make_pipe(vsrc).batches(2, 64, train=False))
    assert [b["fn"] for b in vals] == [["s0", "s1"], ["s2"]] and vals[1]["lbl_msk"].shape == (1, 64, 64)
    want = host_sample(vsrc, 2, [0, 0, 0, 0, 0, 0, 0, 64, 64], 64, False)
    assert np.array_equal(vals[1]["img"][0].cpu().numpy(), want[0]) and np.array_equal(vals[1]["msk"][0].cpu().numpy(), want[1])
    assert np.array_equal(vals[1]["lbl_msk"][0].cpu().numpy(), want[2])
    with pytest.raises(ValueError):
        next(pipe.batches(2, 64, train=False))                               # 64 is not the 80 x 96 image
    # the zero lbl_msk of training batches of one shape is one shared tensor
    assert pipe.make_batch([0], 64)["lbl_msk"] is plain["lbl_msk"]

    with pytest.raises(ValueError):
        pipe.make_batch([0], 64, [[0, 0, 0, 0, 1, 14, 0, 51, 64]])          # the box leaves the crop
    with pytest.raises(ValueError):
        pipe.make_batch([0], 64, [[33, 0, 0, 0, 0, 0, 0, 64, 64]])          # the window leaves the image
    with pytest.raises(ValueError):
        pipe.make_batch([0], 96)                                             # a crop larger than the 80-row image
    with pytest.raises(ValueError):
        pipe.make_batch([0, 1], 64, ROWS_64[:1])
    with pytest.raises(ValueError):
        pipe.make_batch([3], 64)
    with pytest.raises(ValueError):
        next(pipe.batches(2, 64, train=True))


def test_epochs_draw_the_reference_parameters_and_repeat_under_a_seed():
    """crop 208 > 200: the reference's randint(0, 200) box always leaves something of the crop"""
    from dahitra_amd.datasets.xbd_pipeline import draw_train_params
    src = sources(3, 240, 232, seed=8)
    pipe = make_pipe(src)

    def epoch(seed):
        return list(pipe.batches(2, 208, train=True, rng=random.Random(seed)))

    one, two, other = epoch(EPOCH_SEED), epoch(EPOCH_SEED), epoch(EPOCH_SEED + 1)
    assert [b["img"].shape[0] for b in one] == [2, 1] and sorted(sum((b["fn"] for b in one), [])) == ["s0", "s1", "s2"]
    for x, y in zip(one, two):
        assert x["fn"] == y["fn"] and torch.equal(x["img"], y["img"]) and torch.equal(x["msk"], y["msk"])
        assert torch.equal(x["lbl_msk"], y["lbl_msk"])
    assert any(not torch.equal(x["img"], y["img"]) for x, y in zip(one, other))
    # the epoch is: shuffle, then draw_train_params per sample in batch order
    rng = random.Random(EPOCH_SEED)
    order = [0, 1, 2]
    rng.shuffle(order)
    rows = [draw_train_params(rng, 240, 232, 208)[0] for _ in order]
    assert any(r[4] for r in rows) and not all(r[4] for r in rows)
    for b, ind, rws in zip(one, (order[:2], order[2:]), (rows[:2], rows[2:])):
        want = pipe.make_batch(ind, 208, rws)
        assert b["fn"] == want["fn"] and torch.equal(b["img"], want["img"]) and torch.equal(b["msk"], want["msk"])
        for n, (i, row) in enumerate(zip(ind, rws)):
            wimg, wmsk, _ = host_sample(src, i, row, 208, True)
            assert np.array_equal(b["img"][n].cpu().numpy().view(np.uint32), wimg.view(np.uint32))
            assert np.array_equal(b["msk"][n].cpu().numpy(), wmsk)


def test_from_image_dir_follows_the_reference_naming(tmp_path):
    from dahitra_amd.datasets.xbd_pipeline import GpuXbdPipeline
    src = sources(2, 40, 48, seed=6)
    images, masks = tmp_path / "images", tmp_path / "masks"
    images.mkdir(), masks.mkdir()
    for i, name in enumerate(["b-flood_00000001", "a-fire_00000007"]):
        Image.fromarray(src[0][i]).save(str(images / (name + "_pre_disaster.png")))
        Image.fromarray(src[1][i]).save(str(images / (name + "_post_disaster.png")))
        Image.fromarray(src[2][i]).save(str(masks / (name + "_pre_disaster.png")))
        Image.fromarray(src[3][i]).save(str(masks / (name + "_post_disaster.png")))
    pipe = GpuXbdPipeline.from_image_dir(str(images), DEV)
    assert [os.path.basename(f) for f in pipe.files] == ["a-fire_00000007_pre_disaster.png", "b-flood_00000001_pre_disaster.png"]
    for got, want in zip((pipe.pre, pipe.post, pipe.pre_mask, pipe.post_label), src):
        assert np.array_equal(got.cpu().numpy(), want[::-1])
    one = GpuXbdPipeline.from_image_dir(str(images), DEV, files=[str(images / "b-flood_00000001_pre_disaster.png")])
    assert len(one) == 1 and np.array_equal(one.post_label[0].cpu().numpy(), src[3][0])
    with pytest.raises(ValueError):
        GpuXbdPipeline.from_image_dir(str(masks / "nothing"), DEV)


def test_end_to_end_one_eager_xbd_step_from_the_loader():
    import cdnet_ref as O
    from dahitra_amd.models import xbd
    name, S = "xbd_unet_transformer_nodecpos", 128
    src = sources(2, 150, 140, seed=9)
    rows = [[12, 22, 1, 0, 1, 23, 40, S - 23, S - 40], [0, 5, 0, 1, 0, 0, 0, S, S]]
    batch = make_pipe(src).make_batch([1, 0], S, rows, train=True)
    for n, (i, row) in enumerate(zip([1, 0], rows)):
        wimg, wmsk, _ = host_sample(src, i, row, S, True)
        assert np.array_equal(batch["img"][n].cpu().numpy().view(np.uint32), wimg.view(np.uint32))
        assert np.array_equal(batch["msk"][n].cpu().numpy(), wmsk)
    net = xbd.BASE_Transformer_UNet(input_nc=3, output_nc=5, token_len=4, resnet_stages_num=4, with_pos='learned',
                                    with_decoder_pos=None, enc_depth=1, dec_depth=8).cuda()
    net.load_state_dict(O.deterministic_state(name))
    net.train()
    opt = xbd.AdamW(net.parameters(), lr=1e-4, weight_decay=1e-6)
    before = [p.detach().clone() for p in net.parameters()]
    net.zero_grad()
    loss = xbd.xbd_loss(net(batch["img"]), batch["msk"])
    loss.backward()
    norm = float(xbd.clip_grad_norm_(net.parameters(), 0.999))
    opt.step()
    loss = float(loss.detach())
    assert np.isfinite(loss) and loss > 0 and np.isfinite(norm) and norm > 0
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, net.parameters()))
    assert all(bool(torch.isfinite(p).all()) for p in net.parameters())
