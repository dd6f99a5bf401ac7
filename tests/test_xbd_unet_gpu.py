"""The loader of xBD_code/train_unettransformer.py on the MI355X (dh_xbd_augment_warp_u8, csrc/augment_xbd_warp.hip;
GpuXbdPipeline.make_unet_batch / unet_batches) against datasets/xbd_pipeline.unet_reference_u8, the numpy restatement that
tests/test_xbd_unet_cpu.py holds to numpy and to float64.  Everything is integer up to the 256-entry normalisation table, so
every comparison is exact: bytes of the masks, uint32 views of the float32 images.  The outputs are pre-filled with 0xAA so that
an element the kernel does not write shows.  The kernel's tile is 32 x 32: S = 33 lies one pixel past a tile in both directions
and S = 66 two pixels past two; 37 is odd (scalar stores), 1 is the smallest, 256 is the script's crop."""
import functools
import random

import numpy as np
import pytest
import torch

import _xbd_unet_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL = 0xAA
SHAPES = [(37, 40, 52), (1, 1, 1), (33, 40, 35), (66, 70, 75), (256, 300, 308)]           # S, H, W


def filled(n, S):
    img = torch.full((n, 6, S, 4 * S), FILL, dtype=torch.uint8, device=DEV).view(torch.float32)
    return img, torch.full((n, 5, S, S), FILL, dtype=torch.uint8, device=DEV)


@functools.lru_cache(maxsize=None)
def case(S, H, W):
    """sources (two of them), rows, the source of every row (not sorted) and the restatement's batch, computed once and shared"""
    from dahitra_amd.datasets.xbd_pipeline import unet_reference_u8
    src = C.sources(2, H, W)
    rows = C.param_rows(S, H, W)
    idx = [(3 * n + 1) % 2 for n in range(len(rows))]
    want = [unet_reference_u8(src[0][i], src[1][i], src[3][i], r, S) for i, r in zip(idx, rows)]
    img = np.stack([C.normalise(w[0]) for w in want])
    msk = np.stack([w[1] for w in want])
    for a in src + (img, msk):
        a.setflags(write=False)
    return src, rows, idx, img, msk


@functools.lru_cache(maxsize=None)
def pipe(S, H, W):
    from dahitra_amd.datasets import GpuXbdPipeline
    return GpuXbdPipeline(*(torch.from_numpy(np.array(a)).to(DEV) for a in case(S, H, W)[0]))


def assert_equal(got, want, what, rows):
    for n in range(len(rows)):
        g, w = got[n], want[n]
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (what, n, rows[n], len(bad), bad[:4].tolist())


def test_the_tile_is_the_one_the_shapes_were_chosen_for():
    from dahitra_amd import _lib, ops
    assert (_lib.lib().dh_xbd_augment_warp_tile_h(), _lib.lib().dh_xbd_augment_warp_tile_w()) == ops.XBD_WARP_TILE == (32, 32)
    assert {33, 66, 37, 1, 256} == {s[0] for s in SHAPES} and 33 == 32 + 1 and 66 == 2 * 32 + 2


@pytest.mark.parametrize("S,H,W", SHAPES)
def test_c_abi_equals_the_restatement(S, H, W):
    """every operation alone and all composed, in one launch whose samples take their sources in an order that is not sorted"""
    from dahitra_amd import ops
    from dahitra_amd.datasets.xbd_pipeline import check_unet_rows, unet_param_rows, unet_warp_table
    src, rows, idx, want_img, want_msk = case(S, H, W)
    p = pipe(S, H, W)
    n = len(rows)
    check_unet_rows(rows, H, W, S)
    img, msk = filled(n, S)
    tab = torch.from_numpy(unet_warp_table(rows, S)).to(DEV)
    out = ops.xbd_augment_warp(p.pre, p.post, p.post_label, torch.tensor(idx, dtype=torch.int32, device=DEV),
                               torch.from_numpy(unet_param_rows(rows)).to(DEV), tab, S, out_img=img, out_msk=msk)
    assert out[0] is img and out[1] is msk
    assert_equal(msk.cpu().numpy(), want_msk, "msk", rows)
    assert_equal(img.cpu().numpy(), want_img, "img", rows)
    if S >= 33:
        assert (want_msk[:, 1:].sum(axis=1) >= 2).any(), "two classes at weight 1/2 are both set somewhere"
    # without tables no sample warps: the rows without a warp give the same bytes, and nothing is read through the NULL pointer
    plain = [n for n, r in enumerate(rows) if r["warp"] is None]
    img2, msk2 = filled(len(plain), S)
    ops.xbd_augment_warp(p.pre, p.post, p.post_label, torch.tensor([idx[n] for n in plain], dtype=torch.int32, device=DEV),
                         torch.from_numpy(unet_param_rows([rows[n] for n in plain])).to(DEV), None, S, out_img=img2, out_msk=msk2)
    assert torch.equal(msk2, msk[plain]) and torch.equal(img2.view(torch.int32), img[plain].view(torch.int32))


@pytest.mark.parametrize("S,H,W", [(37, 40, 52), (256, 300, 308)])
def test_a_mixed_batch_and_its_plain_sample_and_the_dilation(S, H, W):
    from dahitra_amd import ops
    src, rows, idx, want_img, want_msk = case(S, H, W)
    p = pipe(S, H, W)
    nothing = C.row(W - S, H - S)
    first = lambda f: next(n for n, r in enumerate(rows) if f(r))
    pick = [first(lambda r: r["shift"] is not None and r["warp"] is not None and r["channels"] is not None),
            first(lambda r: r["shift"] not in (None, (0, 0)) and r["warp"] is None),
            first(lambda r: r == nothing),
            first(lambda r: r["warp"] is not None and r["shift"] is None)]
    ind = [idx[n] for n in pick]
    assert ind != sorted(ind) and pick != sorted(pick)
    batch = p.make_unet_batch(ind, S, [rows[n] for n in pick], dilate=0)
    assert batch['img'].dtype == torch.float32 and batch['msk'].dtype == torch.uint8 and batch['fn'] == [p.files[i] for i in ind]
    assert_equal(batch['msk'].cpu().numpy(), want_msk[pick], "msk", [rows[n] for n in pick])
    assert_equal(batch['img'].cpu().numpy(), want_img[pick], "img", [rows[n] for n in pick])
    assert batch['lbl_msk'].shape == (4, S, S) and not batch['lbl_msk'].any()
    # dilate=5 (the default) is xbd_msk_dilate of the undilated batch; lbl_msk is the one shared zero tensor of that shape
    dil = p.make_unet_batch(ind, S, [rows[n] for n in pick])
    assert torch.equal(dil['msk'], ops.xbd_msk_dilate(batch['msk'], 5)) and not torch.equal(dil['msk'], batch['msk'])
    assert torch.equal(dil['img'].view(torch.int32), batch['img'].view(torch.int32)) and dil['lbl_msk'] is batch['lbl_msk']
    # the sample without an operation is train.py's loader, byte for byte
    old = p.make_batch([ind[2]], S, [[W - S, H - S, 0, 0, 0, 0, 0, S, S]])
    assert torch.equal(old['msk'][0], batch['msk'][2]) and torch.equal(old['img'][0].view(torch.int32), batch['img'][2].view(torch.int32))


def test_an_epoch_reproduces_make_unet_batch_of_the_same_rows():
    from dahitra_amd.datasets.xbd_pipeline import draw_unet_params
    S, H, W = 37, 40, 52
    p = pipe(S, H, W)
    got = list(p.unet_batches(1, S, random.Random(5), dilate=0)) + list(p.unet_batches(2, S, random.Random(6)))
    assert [b['img'].shape[0] for b in got] == [1, 1, 2]
    for seed, bs, dilate, batches in ((5, 1, 0, got[:2]), (6, 2, 5, got[2:])):
        rng = random.Random(seed)
        order = [0, 1]
        rng.shuffle(order)
        for s, b in zip(range(0, 2, bs), batches):
            ind = order[s:s + bs]
            rows = [draw_unet_params(rng, H, W, S)[0] for _ in ind]
            want = p.make_unet_batch(ind, S, rows, dilate)
            assert b['fn'] == want['fn'] and torch.equal(b['msk'], want['msk'])
            assert torch.equal(b['img'].view(torch.int32), want['img'].view(torch.int32))
    with pytest.raises(ValueError):
        next(p.unet_batches(1, S, None))


def test_refused_calls_leave_the_outputs_untouched():
    from dahitra_amd import _lib, ops
    from dahitra_amd.datasets.xbd_pipeline import unet_param_rows
    S, H, W = 37, 40, 52
    p = pipe(S, H, W)
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    par = torch.from_numpy(unet_param_rows([C.row()])).to(DEV)
    img, msk = filled(1, S)
    keep = (img.clone(), msk.clone())
    good = [ops.P(p.pre), ops.P(p.post), ops.P(p.post_label), ops.P(idx), ops.P(par), ops.P(None), 1, H, W, S, ops.P(img), ops.P(msk)]
    for at, value in ((0, ops.P(None)), (1, ops.P(None)), (2, ops.P(None)), (3, ops.P(None)), (4, ops.P(None)), (10, ops.P(None)),
                      (11, ops.P(None)), (9, 0), (9, -1), (9, H + 1), (9, W + 1), (6, 0), (6, -3), (6, 65536)):
        args = list(good)
        args[at] = value
        with pytest.raises(_lib.HipLibraryError, match="xbd_augment_warp"):
            ops._call("dh_xbd_augment_warp_u8", *args, ops.S())
    torch.cuda.synchronize()
    assert torch.equal(img.view(torch.int32), keep[0].view(torch.int32)) and torch.equal(msk, keep[1])
    # the wrappers refuse before any launch
    for bad in (dict(crop=H + 1), dict(rows=[C.row(x0=W)]), dict(rows=[C.row(), C.row()]), dict(indices=[2]), dict(dilate=4),
                dict(rows=[C.row(warp=(10, 0.9, (400000, 0)))])):
        kw = dict(dict(indices=[0], crop=S, rows=[C.row()], dilate=5), **bad)
        with pytest.raises(ValueError):
            p.make_unet_batch(kw["indices"], kw["crop"], kw["rows"], kw["dilate"])
    with pytest.raises(ValueError):
        ops.xbd_augment_warp(p.pre, p.post, p.post_label, idx, par[:, :9].contiguous(), None, S)
    with pytest.raises(ValueError):
        ops.xbd_augment_warp(p.pre, p.post, p.post_label, idx.cpu(), par, None, S)
    ops._call("dh_xbd_augment_warp_u8", *good, ops.S())
    torch.cuda.synchronize()
    assert not torch.equal(msk, keep[1])
