"""The xBD damage map and visual grid on the MI355X: dh_xbd_damage_map_u8 / dh_xbd_vis_grid_u8 (csrc/xbd_visual.hip) against the
numpy restatement of xBD_code/visualize_results.py:204-220 (tests/_xbd_visual_cases.py), then models/xbd.damage_map / visual_grid /
visualize_dir on the model.  Everything is integer: every comparison is on bytes."""
import os

import numpy as np
import pytest
import torch

import _xbd_visual_cases as V
import cdnet_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAME = "xbd_unet_transformer_nodecpos"
SENTINEL = 0xA5
# (1, 37, 41): odd, not square, W % 4 != 0, less than one workgroup; (2, 40, 40): two images on the vector path, dword stores;
# (1, 1024, 1024): the reference's tile, 16-byte stores, one run per thread; (1, 1040, 2048): 133120 runs of 16 pixels are more than
# the 512 x 256 threads of the largest launch: the grid-stride loop runs
SHAPES = [(1, 37, 41), (2, 40, 40), (1, 1024, 1024), (1, 1040, 2048)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def case(N, H, W):
    return (V.masks(N, H, W, seed=V.seed_of(N, H, W)),) + V.pictures(N, H, W, seed=V.seed_of(N, H, W))


def offset_view(a, offset=1, whole=False):
    """a device copy of the uint8 array `a` that starts `offset` bytes into a larger buffer filled with the sentinel (whole: and
    that buffer)"""
    buf = torch.full((a.size + 32,), SENTINEL, dtype=torch.uint8, device=DEV)
    view = buf[offset:offset + a.size].view(a.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return (view, buf) if whole else view


@pytest.mark.parametrize("N,H,W", SHAPES)
def test_both_kernels_are_byte_equal_to_the_restatement(N, H, W):
    from dahitra_amd import ops
    msk, pre, post, gt = case(N, H, W)
    dmsk, dpre, dpost, dgt = (dev(a) for a in (msk, pre, post, gt))
    for loc in V.LOCS:
        want = V.damage_map(msk, loc)
        out = torch.full((N, H, W), SENTINEL, dtype=torch.uint8, device=DEV)            # every byte of a given buffer is written
        got = ops.xbd_damage_map(dmsk, loc, out=out)
        assert got is out and np.array_equal(got.cpu().numpy(), want), loc
        fresh = ops.xbd_damage_map(dmsk, loc)
        assert fresh.shape == (N, H, W) and fresh.dtype == torch.uint8 and torch.equal(fresh, out), loc
        want = V.vis_grid(pre, post, gt, msk, loc)
        out = torch.full((N, H, 4 * W, 3), SENTINEL, dtype=torch.uint8, device=DEV)
        got = ops.xbd_vis_grid(dpre, dpost, dgt, dmsk, loc, out=out)
        assert got is out and np.array_equal(got.cpu().numpy(), want), loc
        fresh = ops.xbd_vis_grid(dpre, dpost, dgt, dmsk, loc)
        assert fresh.shape == (N, H, 4 * W, 3) and fresh.dtype == torch.uint8 and torch.equal(fresh, out), loc
    assert sorted(np.unique(V.damage_map(msk, V.SCRIPT_THR)).tolist()) == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("N,H,W", [(2, 40, 40), (1, 8, 32)])
def test_unaligned_pointers_give_the_aligned_result(N, H, W):
    """views that start 1 byte into their buffers take the pixel-by-pixel path; an output 4 bytes in keeps the vector loads and
    stores dwords ((1, 8, 32): W % 16 == 0, whose aligned call stores 16-byte vectors)"""
    from dahitra_amd import ops
    msk, pre, post, gt = case(N, H, W)
    loc = V.SCRIPT_THR
    aligned = [dev(a) for a in (pre, post, gt, msk)]
    assert all(t.data_ptr() % 16 == 0 for t in aligned)
    want_map, want_grid = V.damage_map(msk, loc), V.vis_grid(pre, post, gt, msk, loc)
    assert np.array_equal(ops.xbd_damage_map(aligned[3], loc).cpu().numpy(), want_map)
    assert np.array_equal(ops.xbd_vis_grid(*aligned, loc).cpu().numpy(), want_grid)
    shifted = [offset_view(a) for a in (pre, post, gt, msk)]
    assert all(t.data_ptr() % 16 == 1 for t in shifted)
    assert np.array_equal(ops.xbd_damage_map(shifted[3], loc).cpu().numpy(), want_map)
    for which in ((3,), (0,), (2,), (1,), (0, 1, 2, 3)):                                   # msk, pre, gt, post alone; all
        args = [shifted[i] if i in which else aligned[i] for i in range(4)]
        assert np.array_equal(ops.xbd_vis_grid(*args, loc).cpu().numpy(), want_grid), which
    for offset in (1, 4):                                                                   # the outputs
        for args in (aligned, shifted):
            out = offset_view(np.full(want_map.shape, SENTINEL, dtype=np.uint8), offset)
            ops.xbd_damage_map(args[3], loc, out=out)
            assert np.array_equal(out.cpu().numpy(), want_map), offset
            out, whole = offset_view(np.full(want_grid.shape, SENTINEL, dtype=np.uint8), offset, whole=True)
            ops.xbd_vis_grid(*args, loc, out=out)
            assert np.array_equal(out.cpu().numpy(), want_grid), offset
            rest = torch.cat([whole[:offset], whole[offset + want_grid.size:]])
            assert bool((rest == SENTINEL).all()), "nothing outside the output is written"


def test_a_label_outside_the_table_is_magenta_through_ops_and_a_keyerror_at_the_model_level():
    from dahitra_amd import ops
    from dahitra_amd.models import xbd
    for N, H, W in ((1, 37, 41), (2, 40, 40), (1, 16, 32)):                                # scalar, dword and 16-byte stores
        msk, pre, post, gt = case(N, H, W)
        gt = gt.copy()
        gt[0, 3, 5], gt[N - 1, H - 1, W - 1] = 5, 255
        got = ops.xbd_vis_grid(dev(pre), dev(post), dev(gt), dev(msk)).cpu().numpy()
        assert np.array_equal(got, V.vis_grid(pre, post, gt, msk))
        assert tuple(got[0, 3, 2 * W + 5]) == tuple(got[N - 1, H - 1, 3 * W - 1]) == V.MAGENTA == (255, 0, 255)
        assert int((got[:, :, 2 * W:3 * W] == V.MAGENTA).all(-1).sum()) == 2
        for bad in (5, 255):
            with pytest.raises(KeyError):
                xbd.visual_grid(torch.nn.Identity(), dev(pre), dev(post), dev(np.minimum(gt, bad)))


def test_refused_arguments_return_failure_and_write_nothing():
    from dahitra_amd import _lib, ops
    L = _lib.lib()
    P, S = ops.P, ops.S
    img = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=DEV)
    gt = torch.zeros(1, 8, 8, dtype=torch.uint8, device=DEV)
    msk = torch.zeros(1, 8, 8, 5, dtype=torch.uint8, device=DEV)
    out = torch.full((1, 8, 8), SENTINEL, dtype=torch.uint8, device=DEV)
    grid = torch.full((1, 8, 32, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    good = dict(pre=P(img), post=P(img), gt=P(gt), msk=P(msk), N=1, H=8, W=8, use=1, b0=97, b1=34, b2=36, grid=P(grid))
    order = ("pre", "post", "gt", "msk", "N", "H", "W", "use", "b0", "b1", "b2", "grid")
    for change in (dict(H=1 << 14, W=1 << 14),                  # 12 W H = 3 * 2^30: the grid of one image exceeds the limit
                   dict(b0=300), dict(b1=257), dict(b2=-1), dict(use=0, b0=300), dict(N=0), dict(N=-1), dict(H=0), dict(W=0),
                   dict(H=1 << 16, W=1 << 15), dict(pre=P(None)), dict(post=P(None)), dict(gt=P(None)), dict(msk=P(None)),
                   dict(grid=P(None))):
        args = dict(good, **change)
        assert L.dh_xbd_vis_grid_u8(*[args[k] for k in order], S()) != 0, change
        assert L.dh_last_error().decode().startswith("xbd_vis_grid"), (change, L.dh_last_error())
    good = dict(msk=P(msk), N=1, H=8, W=8, use=1, b0=97, b1=34, b2=36, out=P(out))
    order = ("msk", "N", "H", "W", "use", "b0", "b1", "b2", "out")
    for change in (dict(b0=300), dict(b1=257), dict(b2=-1), dict(N=0), dict(H=0), dict(W=0), dict(H=1 << 16, W=1 << 15),
                   dict(msk=P(None)), dict(out=P(None))):
        args = dict(good, **change)
        assert L.dh_xbd_damage_map_u8(*[args[k] for k in order], S()) != 0, change
        assert L.dh_last_error().decode().startswith("xbd_damage_map"), (change, L.dh_last_error())
    # what ops refuses before any launch, on device tensors: a CPU tensor among them, strides, a wrong `out`
    for kw in (dict(pre_u8=img.cpu()), dict(gt_u8=gt.cpu()), dict(out=grid.cpu()), dict(out=grid[:, :, :, :2]),
               dict(post_u8=torch.zeros(1, 8, 16, 3, dtype=torch.uint8, device=DEV)[:, :, ::2]),
               dict(out=torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=DEV)), dict(loc=float("nan"))):
        with pytest.raises(ValueError):
            ops.xbd_vis_grid(**dict(dict(pre_u8=img, post_u8=img, gt_u8=gt, msk_u8=msk, out=grid), **kw))
    for kw in (dict(msk_u8=msk.cpu()), dict(out=out.cpu()), dict(out=grid), dict(loc=(0.1, 0.2))):
        with pytest.raises(ValueError):
            ops.xbd_damage_map(**dict(dict(msk_u8=msk, out=out), **kw))
    with pytest.raises((_lib.HipLibraryError, ValueError)):
        ops.xbd_damage_map(msk[:0])
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((grid == SENTINEL).all())
    # the good calls do write: four equal bytes are class 1, and with m0 = 0 below every bound the rule drops it
    ops.xbd_damage_map(msk, out=out)
    ops.xbd_vis_grid(img, img, gt, msk, V.SCRIPT_THR, out=grid)
    assert bool((out == 1).all()) and bool((grid == 0).all())


# ---- model level -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_case():
    """the net of test_xbd_tta_gpu.py (fp32 compute, deterministic weights) and one 64 x 64 pair with labels"""
    from dahitra_amd.models import xbd
    net = xbd.BASE_Transformer_UNet(input_nc=3, output_nc=5, token_len=4, resnet_stages_num=4, with_pos='learned',
                                    with_decoder_pos=None, enc_depth=1, dec_depth=8).cuda()
    net.load_state_dict(O.deterministic_state(NAME))
    net.eval()
    pre, post, gt = V.pictures(1, 64, 64, seed=64)
    return {"net": net, "np": (pre, post, gt), "dev": tuple(dev(a) for a in (pre, post, gt))}


def test_visual_grid_is_the_restatement_of_the_models_own_prediction(model_case):
    from dahitra_amd.models import xbd
    net = model_case["net"]
    pre, post, gt = model_case["np"]
    dpre, dpost, dgt = model_case["dev"]
    msk = xbd.predict_tta(net, dpre, dpost).clone()
    assert torch.equal(msk, xbd.predict_tta(net, dpre, dpost, graph=False))
    m = msk.cpu().numpy()
    assert m.shape == (1, 64, 64, 5) and len(np.unique(m)) > 8, "a degenerate net cannot pass"
    for loc in V.LOCS:
        want = V.vis_grid(pre, post, gt, m, loc)
        for graph in (True, False):
            got = xbd.visual_grid(net, dpre, dpost, dgt, loc=loc, graph=graph)
            assert got.shape == (1, 64, 256, 3) and got.dtype == torch.uint8 and got.is_cuda
            assert np.array_equal(got.cpu().numpy(), want), (loc, graph)
        assert np.array_equal(xbd.damage_map(msk, loc).cpu().numpy(), V.damage_map(m, loc)), loc
    # the other channel order feeds the net another image and reaches the picture
    rgb = xbd.visual_grid(net, dpre, dpost, dgt, order="rgb").cpu().numpy()
    assert np.array_equal(rgb, V.vis_grid(pre, post, gt, xbd.predict_tta(net, dpre, dpost, order="rgb").cpu().numpy()))
    # the recorded prediction step is the one predict_tta made, and still returns the same bytes
    assert len(net._xbd_predict_steps) == 2
    assert torch.equal(xbd.predict_tta(net, dpre, dpost), msk)


def test_visualize_dir_writes_the_scripts_pictures(model_case, tmp_path):
    """Two synthetic pairs, 96 x 80 and 64 x 64, with crop=64: the crop cuts the first on both axes and leaves the second whole.
    (A 48 x 48 crop of 64 x 64 tiles cannot be predicted: the net's decoder attention batches its images in rows of 16, and the
    3 x 3 map of a 48 x 48 tile at 1/16 scale has 9 rows per image -- ops.linear asserts.  64 is the smallest tile the net takes.)"""
    from PIL import Image
    from dahitra_amd.models import xbd
    net = model_case["net"]
    images, masks, out = tmp_path / "images", tmp_path / "masks", tmp_path / "outputs"
    images.mkdir()
    masks.mkdir()
    pairs = {}
    for i, (H, W) in enumerate(((96, 80), (64, 64))):
        pre, post, gt = V.pictures(1, H, W, seed=70 + i)
        f = "area_%08d_pre_disaster.png" % i
        Image.fromarray(pre[0]).save(str(images / f))
        Image.fromarray(post[0]).save(str(images / f.replace("_pre_", "_post_")))
        Image.fromarray(gt[0]).save(str(masks / f.replace("_pre_", "_post_")))
        pairs[f] = (pre[:, :64, :64], post[:, :64, :64], gt[:, :64, :64])
    names = sorted(pairs)
    written = xbd.visualize_dir(net, str(images), str(masks), str(out), crop=64, loc=V.SCRIPT_THR)
    assert written == names
    assert sorted(os.listdir(str(out))) == ["TUNet_area_%08d_visdisaster.png" % i for i in range(2)]
    for f in names:
        pre, post, gt = pairs[f]
        msk = xbd.predict_tta(net, dev(pre), dev(post)).cpu().numpy()
        img = Image.open(str(out / xbd.visual_name(f)))
        assert img.mode == "RGB" and img.size == (4 * 64, 64)
        assert np.array_equal(np.asarray(img), V.vis_grid(pre, post, gt, msk, V.SCRIPT_THR)[0]), f
        assert len(np.unique(np.asarray(img)[:, 3 * 64:].reshape(-1, 3), axis=0)) > 1, "more than one class is painted"
    # `files` narrows the list, crop=None takes the whole tile, model_str names the file, the one-element list is the script's `models`
    other = tmp_path / "other"
    assert xbd.visualize_dir([net], str(images), str(masks), str(other), model_str="m", crop=None, files=[names[1]]) == [names[1]]
    assert os.listdir(str(other)) == ["m_area_00000001_visdisaster.png"]
    got = np.asarray(Image.open(str(other / "m_area_00000001_visdisaster.png")))
    pre, post, gt = pairs[names[1]]
    assert np.array_equal(got, V.vis_grid(pre, post, gt, xbd.predict_tta(net, dev(pre), dev(post)).cpu().numpy())[0])
    # a crop the net cannot take is refused before anything is predicted
    with pytest.raises(ValueError, match="multiples of 64"):
        xbd.visualize_dir(net, str(images), str(masks), str(other), crop=48, files=[names[1]])
    assert os.listdir(str(other)) == ["m_area_00000001_visdisaster.png"]
    # shapes that differ after the crop: the 96 x 80 pair with a 64 x 64 mask, uncropped
    Image.fromarray(pairs[names[0]][2][0]).save(str(masks / names[0].replace("_pre_", "_post_")))
    with pytest.raises(ValueError, match="differ"):
        xbd.visualize_dir(net, str(images), str(masks), str(other), crop=None, files=[names[0]])
