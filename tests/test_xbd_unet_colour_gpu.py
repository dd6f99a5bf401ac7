"""The colour stage of xBD_code/train_unettransformer.py on the MI355X (dh_xbd_unet_colour_u8, csrc/augment_xbd_colour.hip;
GpuXbdPipeline.make_unet_batch(colour=) / unet_batches(colour=True)) against datasets/xbd_pipeline.unet_colour_reference_u8, the
numpy restatement that tests/test_xbd_unet_colour_cpu.py holds to the reference's bytes, to numpy and to colorsys.  Every
comparison is exact: uint32 views of the float32 images.  The warp launch's outputs are pre-filled with 0xAA, as in
test_xbd_unet_gpu.py.  The kernels' tile is 32 x 32 and a lane takes four pixels: S = 1 is the smallest, 2 is the reflect-101
edge case (both neighbours of a pixel are the other one), 33 lies one pixel past a tile and is odd (element-wise loads and
stores), 36 is past a tile on the 4-wide path, 66 is several tiles for contrast's sums; 256 is the script's crop.  A build that
contracts the blends or the HSV return into fused multiply-adds fails these comparisons."""
import collections
import functools
import random

import numpy as np
import pytest
import torch

import _xbd_unet_cases as C
import _xbd_unet_colour_cases as K

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL = 0xAA
SHAPES = [(1, 1, 1), (2, 3, 4), (33, 40, 35), (36, 40, 52), (66, 70, 75)]           # S, H, W


def filled(n, S):
    img = torch.full((n, 6, S, 4 * S), FILL, dtype=torch.uint8, device=DEV).view(torch.float32)
    return img, torch.full((n, 5, S, S), FILL, dtype=torch.uint8, device=DEV)


@functools.lru_cache(maxsize=None)
def case(S, H, W):
    """sources, rows (geometry and shift_channels under the colour stage), colour dicts and both restatements' batches, computed
    once and shared"""
    from dahitra_amd.datasets.xbd_pipeline import unet_colour_reference_u8, unet_reference_u8
    src = C.sources(2, H, W)
    colour = K.colour_batch(S)
    geometry = C.param_rows(S, H, W)
    rows = [geometry[(7 * n + 3) % len(geometry)] if n % 3 else C.row(W - S, H - S, channels=(1 + n % 2, 5, -5, 5))
            for n in range(len(colour))]
    idx = [(3 * n + 1) % 2 for n in range(len(rows))]
    warp = [unet_reference_u8(src[0][i], src[1][i], src[3][i], r, S) for i, r in zip(idx, rows)]
    plain = np.stack([C.normalise(w[0]) for w in warp])
    want = np.stack([C.normalise(unet_colour_reference_u8(w[0], c)) for w, c in zip(warp, colour)])
    msk = np.stack([w[1] for w in warp])
    for a in src + (plain, want, msk):
        a.setflags(write=False)
    return src, rows, idx, colour, plain, want, msk


@functools.lru_cache(maxsize=None)
def pipe(S, H, W):
    from dahitra_amd.datasets import GpuXbdPipeline
    return GpuXbdPipeline(*(torch.from_numpy(np.array(a)).to(DEV) for a in case(S, H, W)[0]))


def assert_equal(got, want, what, notes):
    for n in range(len(want)):
        bad = np.argwhere(got[n].view(np.uint32) != want[n].view(np.uint32))
        assert bad.size == 0, (what, n, notes[n], len(bad), bad[:4].tolist(),
                               [(float(got[n][tuple(b)]), float(want[n][tuple(b)])) for b in bad[:4]])


def names(colour):
    from dahitra_amd.datasets.xbd_pipeline import unet_colour_names
    return [unet_colour_names(c) for c in colour]


def warp_batch(p, S, H, W):
    from dahitra_amd import ops
    from dahitra_amd.datasets.xbd_pipeline import unet_param_rows, unet_warp_table
    src, rows, idx = case(S, H, W)[:3]
    img, msk = filled(len(rows), S)
    tab = unet_warp_table(rows, S)
    ops.xbd_augment_warp(p.pre, p.post, p.post_label, torch.tensor(idx, dtype=torch.int32, device=DEV),
                         torch.from_numpy(unet_param_rows(rows)).to(DEV), torch.from_numpy(tab).to(DEV) if tab is not None else None,
                         S, out_img=img, out_msk=msk)
    return img, msk


def test_the_tile_is_the_one_the_shapes_were_chosen_for():
    from dahitra_amd import _lib, ops
    assert _lib.lib().dh_xbd_unet_colour_tile() == ops.XBD_COLOUR_TILE == 32
    assert {1, 2, 33, 36, 66} == {s[0] for s in SHAPES} and 33 == 32 + 1 and 36 == 32 + 4 and 66 == 2 * 32 + 2


@pytest.mark.parametrize("S,H,W", SHAPES)
def test_c_abi_equals_the_restatement(S, H, W):
    """every operation alone, change_hsv followed by each block operation and both images of one sample in ONE call whose job
    rows are not in sample order; samples without a job keep the warp launch's bits"""
    from dahitra_amd import ops
    from dahitra_amd.datasets.xbd_pipeline import check_unet_colour, unet_colour_jobs
    src, rows, idx, colour, plain, want, want_msk = case(S, H, W)
    p = pipe(S, H, W)
    img, msk = warp_batch(p, S, H, W)
    before = img.clone()
    assert_equal(before.cpu().numpy(), plain, "warp", rows)
    jobs, noise = unet_colour_jobs(check_unet_colour(colour, S), S)
    order = [(5 * j + 2) % len(jobs) for j in range(len(jobs))]               # len(jobs) = 18: a permutation
    assert sorted(order) == list(range(len(jobs))) and order != sorted(order)
    assert {(j[0], j[1]) for j in jobs.tolist() if j[0] == len(colour) - 3} == {(len(colour) - 3, 0), (len(colour) - 3, 1)}
    ws = torch.full((ops.xbd_unet_colour_ws_bytes(len(jobs), S) + 8,), FILL, dtype=torch.uint8, device=DEV)
    out = ops.xbd_unet_colour(img, torch.from_numpy(jobs[order]).to(DEV), torch.from_numpy(noise).to(DEV), ws=ws)
    assert out is img
    assert_equal(img.cpu().numpy(), want, "img", names(colour))
    assert bool((ws[-8:] == FILL).all()), "nothing is written past the workspace's size"
    assert np.array_equal(msk.cpu().numpy(), want_msk)
    untouched = [n for n, c in enumerate(colour) if not names([c])[0]]
    assert len(untouched) == 2
    assert torch.equal(img[untouched].view(torch.int32), before[untouched].view(torch.int32))
    if S >= 33:
        changed = [n for n in range(len(colour)) if n not in untouched]
        assert all(not torch.equal(img[n].view(torch.int32), before[n].view(torch.int32)) for n in changed)
    # a fresh workspace and the jobs in sample order give the same bits
    img2, _ = warp_batch(p, S, H, W)
    ops.xbd_unet_colour(img2, torch.from_numpy(jobs).to(DEV), torch.from_numpy(noise).to(DEV))
    assert torch.equal(img2.view(torch.int32), img.view(torch.int32))


def test_the_hsv_lattice_as_an_image():
    """greys, V == 0, all six channel orders, two-channel ties, 0 and 255 under shifts that clip at either end and wrap the hue"""
    from dahitra_amd.datasets import GpuXbdPipeline
    from dahitra_amd.datasets.xbd_pipeline import change_hsv_u8
    S = 33
    lat = K.lattice_image(S)
    assert S * S >= len(K.lattice())
    pre, post = lat, np.ascontiguousarray(lat[::-1, ::-1])
    zeros = np.zeros((1, S, S), dtype=np.uint8)
    p = GpuXbdPipeline(*(torch.from_numpy(a).to(DEV) for a in (pre[None], post[None], zeros, zeros)))
    colour = [{"hsv": (1 + n % 2,) + shift, "pre": None, "post": None} for n, shift in enumerate(K.HSV_SHIFTS)]
    batch = p.make_unet_batch([0] * len(colour), S, [C.row()] * len(colour), dilate=0, colour=colour)
    want = []
    for c in colour:
        im, shift = c["hsv"][0], c["hsv"][1:]
        a, b = (change_hsv_u8(pre, *shift), post) if im == 1 else (pre, change_hsv_u8(post, *shift))
        want.append(C.normalise(np.concatenate([a, b], axis=2).transpose(2, 0, 1)))
    assert_equal(batch['img'].cpu().numpy(), np.stack(want), "lattice", K.HSV_SHIFTS)


@pytest.mark.parametrize("S,H,W", [(33, 40, 35), (36, 40, 52)])
def test_no_colour_is_the_batch_as_before(S, H, W):
    src, rows, idx, colour, plain, want, want_msk = case(S, H, W)
    p = pipe(S, H, W)
    old = p.make_unet_batch(idx, S, rows, 5)
    assert_equal(old['img'].cpu().numpy(), plain, "img", rows)
    p._colour_ws = None
    for nothing in (None, [None] * len(rows), [K.empty() for _ in rows], [{}] * len(rows)):
        new = p.make_unet_batch(idx, S, rows, 5, colour=nothing)
        assert torch.equal(new['img'].view(torch.int32), old['img'].view(torch.int32)) and torch.equal(new['msk'], old['msk'])
        assert new['lbl_msk'] is old['lbl_msk'] and new['fn'] == old['fn']
    assert p._colour_ws is None, "no job, no workspace and no launch"
    # and with the colour dicts: the restatement, the masks as before
    new = p.make_unet_batch(idx, S, rows, 5, colour)
    assert_equal(new['img'].cpu().numpy(), want, "img", names(colour))
    assert torch.equal(new['msk'], old['msk'])


EPOCHS = ((7090, 3, None, {'change_hsv_pre': 1, 'contrast_post': 1, 'change_hsv_post': 1}, {'elastic_pre': 1}),
          (6783, 8, None, {'change_hsv_pre': 1, 'blur_pre': 1}, {'elastic_post': 1}),
          (1324, 5, 4, {'gauss_noise_post': 1, 'change_hsv_post': 1}, {'elastic_post': 1}))        # seeds found on the CPU: 8 samples of 40 x 52, crop 36


@pytest.mark.parametrize("seed,bs,np_seed,applied,skipped", EPOCHS)
def test_an_epoch_reproduces_make_unet_batch_of_the_same_draws(seed, bs, np_seed, applied, skipped):
    from dahitra_amd.datasets import GpuXbdPipeline
    from dahitra_amd.datasets.xbd_pipeline import draw_unet_colour, draw_unet_params
    S, H, W, n = 36, 40, 52, 8
    p = GpuXbdPipeline(*(torch.from_numpy(np.array(a)).to(DEV) for a in C.sources(n, H, W, seed=11)))
    np_rng = lambda: None if np_seed is None else np.random.RandomState(np_seed)
    got = list(p.unet_batches(bs, S, random.Random(seed), dilate=0, colour=True, np_rng=np_rng()))
    assert dict(p.unet_applied) == applied and dict(p.unet_skipped) == skipped
    rng, gen, plain_rng = random.Random(seed), np_rng(), random.Random(seed)
    order = list(range(n))
    rng.shuffle(order)
    plain_rng.shuffle(list(range(n)))
    drawn, differ = collections.Counter(), 0
    for s, b in zip(range(0, n, bs), got):
        ind = order[s:s + bs]
        draws = [draw_unet_colour(rng, H, W, S, gen) for _ in ind]
        for _ in ind:
            drawn.update(draw_unet_params(plain_rng, H, W, S)[1])
        want = p.make_unet_batch(ind, S, [d[0] for d in draws], 0, [d[1] for d in draws])
        assert b['fn'] == want['fn'] and torch.equal(b['msk'], want['msk'])
        assert torch.equal(b['img'].view(torch.int32), want['img'].view(torch.int32))
        without = p.make_unet_batch(ind, S, [d[0] for d in draws], 0)
        differ += int(not torch.equal(b['img'].view(torch.int32), without['img'].view(torch.int32)))
    assert len(got) == -(-n // bs) and differ >= 1
    # what was applied and what was skipped add up to what the sample drew
    assert p.unet_applied + p.unet_skipped == drawn and rng.getstate() == plain_rng.getstate()
    # without colour=True the epoch is the one before: nothing applied, everything drawn reported as skipped
    list(p.unet_batches(bs, S, random.Random(seed), dilate=0))
    assert p.unet_skipped == drawn and not p.unet_applied


def test_refused_calls_leave_the_batch_untouched():
    from dahitra_amd import _lib, ops
    S, H, W = 33, 40, 35
    p = pipe(S, H, W)
    img, _ = warp_batch(p, S, H, W)
    N = img.shape[0]
    keep = img.clone()
    jobs = torch.tensor([[0, 0, 1, 5, 5, 5, 1, 0, 0, 0, 0, 0]], dtype=torch.int32, device=DEV)
    noise = torch.full((1, S, S, 3), 9, dtype=torch.uint8, device=DEV)
    need = ops.xbd_unet_colour_ws_bytes(1, S)
    ws = torch.zeros(need + 4, dtype=torch.uint8, device=DEV)
    good = [ops.P(img), ops.P(jobs), ops.P(noise), N, S, 1, 1, ops.P(ws), need]
    for at, value in ((0, ops.P(None)), (1, ops.P(None)), (2, ops.P(None)), (7, ops.P(None)), (3, 0), (3, -1), (4, 0), (4, 4097),
                      (5, 0), (5, 65536), (6, 0), (6, -1), (8, need - 1), (7, ops._vp(ws.data_ptr() + 1))):
        args = list(good)
        args[at] = value
        with pytest.raises(_lib.HipLibraryError, match="xbd_unet_colour"):
            ops._call("dh_xbd_unet_colour_u8", *args, ops.S())
    torch.cuda.synchronize()
    assert torch.equal(img.view(torch.int32), keep.view(torch.int32)) and not ws.any()
    # the wrappers refuse before any launch
    for call in (lambda: ops.xbd_unet_colour(img[:, :5], jobs, noise), lambda: ops.xbd_unet_colour(img, jobs[:, :10].contiguous(), noise),
                 lambda: ops.xbd_unet_colour(img, jobs.cpu(), noise), lambda: ops.xbd_unet_colour(img, jobs, noise[:, :32]),
                 lambda: ops.xbd_unet_colour(img, jobs, noise, ws=ws[:need - 4]), lambda: ops.xbd_unet_colour(img, jobs[:0], noise),
                 lambda: ops.xbd_unet_colour(img.double(), jobs, noise)):
        with pytest.raises(ValueError, match="xbd_unet_colour"):
            call()
    rows, idx = case(S, H, W)[1:3]
    for bad in ([None], [{"pre": ("clahe", None)}] * N, [{"hsv": (1, 300, 0, 0)}] + [None] * (N - 1),
                [{"post": ("gauss_noise", np.zeros((S, S + 1, 3), dtype=np.uint8))}] * N):
        with pytest.raises(ValueError, match="colour"):
            p.make_unet_batch(idx, S, rows, 0, bad)
    torch.cuda.synchronize()
    assert torch.equal(img.view(torch.int32), keep.view(torch.int32))
    # rows that point outside: the sample and the noise plane are clamped, the image is one bit, an unknown op is none
    wild = torch.tensor([[N + 7, 2, 0, 0, 0, 0, 9, 0, 0, 0, 0, 0], [-3, 3, 0, 0, 0, 0, 1, 0, 0, 99, 0, 0]], dtype=torch.int32, device=DEV)
    ops.xbd_unet_colour(img, wild, noise)
    torch.cuda.synchronize()
    got, was = img.cpu().numpy(), keep.cpu().numpy()
    assert np.array_equal(got[1:].view(np.uint32), was[1:].view(np.uint32)), "the last sample's pre image went through unchanged"
    assert np.array_equal(got[0, :3].view(np.uint32), was[0, :3].view(np.uint32))
    byte = lambda a: np.rint((a + np.float32(1)) * np.float32(127)).astype(np.int64)
    assert np.array_equal(byte(got[0, 3:]), np.minimum(byte(was[0, 3:]) + 9, 255))


def test_one_batch_of_the_scripts_crop():
    from dahitra_amd.datasets.xbd_pipeline import draw_unet_noise, unet_colour_reference_u8, unet_reference_u8
    S, H, W = 256, 300, 308
    src = C.sources(2, H, W)
    from dahitra_amd.datasets import GpuXbdPipeline
    p = GpuXbdPipeline(*(torch.from_numpy(a).to(DEV) for a in src))
    geometry = C.param_rows(S, H, W)
    rows = [geometry[-1], C.row(W - S, H - S), geometry[-3]]
    noise = draw_unet_noise(np.random.RandomState(1), S)
    colour = [{"hsv": (1, 5, -4, 3), "pre": ("contrast", K.FACTORS[3]), "post": ("blur", None)}, None,
              {"hsv": (2, -5, 5, -5), "pre": ("gauss_noise", noise), "post": ("saturation", K.FACTORS[2])}]
    idx = [1, 0, 1]
    batch = p.make_unet_batch(idx, S, rows, 5, colour)
    warp = [unet_reference_u8(src[0][i], src[1][i], src[3][i], r, S) for i, r in zip(idx, rows)]
    want = np.stack([C.normalise(unet_colour_reference_u8(w[0], c)) for w, c in zip(warp, colour)])
    assert_equal(batch['img'].cpu().numpy(), want, "img", names(colour))
    plain = p.make_unet_batch(idx, S, rows, 5)
    assert torch.equal(batch['msk'], plain['msk']) and torch.equal(batch['img'][1].view(torch.int32), plain['img'][1].view(torch.int32))
    assert not torch.equal(batch['img'][0].view(torch.int32), plain['img'][0].view(torch.int32))
