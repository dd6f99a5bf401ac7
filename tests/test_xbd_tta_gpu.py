"""The xBD prediction on the MI355X: dh_xbd_tta_pack_u8 / dh_xbd_tta_merge_u8 (csrc/xbd_predict.hip) against the numpy
restatement of the reference's predictor (tests/_xbd_tta_cases.py, xBD_code/predict_test_cls.py:62-94), then
models/xbd.predict_tta / predict_dir and graph.GraphedXbdPredictStep on the model.  The pack comparison is on float32 bits.  The
merge comparison is exact where the logits are built so that no last bit of an expf can decide a byte, and against the float64
value with a derived band elsewhere."""
import os

import numpy as np
import pytest
import torch

import _xbd_tta_cases as T
import cdnet_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAME = "xbd_unet_transformer_nodecpos"
SENTINEL = 0xA5
# (1, 37, 41): odd, not square, W % 4 != 0, less than one workgroup; (2, 40, 40): two images on the vector path;
# (1, 1024, 1024): the reference's size, and the grid-stride loop runs
SHAPES = [(1, 37, 41), (2, 40, 40), (1, 1024, 1024)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("N,H,W", SHAPES)
def test_pack_is_bit_equal_to_the_restatement_for_both_orders(N, H, W):
    from dahitra_amd import ops
    pre, post = T.sources(N, H, W, seed=N * 1000 + W)
    dpre, dpost = dev(pre), dev(post)
    for order in ("bgr", "rgb"):
        want = T.pack(pre, post, order)
        got = ops.xbd_tta_pack(dpre, dpost, order)
        assert got.shape == (4 * N, 6, H, W) and got.dtype == torch.float32
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), order
        out = torch.full((4 * N, 6, H, W), float("nan"), device=DEV)         # every element of a given buffer is written
        assert ops.xbd_tta_pack(dpre, dpost, order, out=out) is out
        assert np.array_equal(bits(out.cpu().numpy()), bits(want)), order
    assert np.array_equal(bits(ops.xbd_tta_pack(dpre, dpost).cpu().numpy()), bits(T.pack(pre, post, "bgr"))), "'bgr' is the default"


@pytest.mark.parametrize("N,H,W", SHAPES)
def test_merge_is_exact_on_three_level_logits(N, H, W):
    from dahitra_amd import ops
    logits = T.three_level(N, H, W, seed=N * 100 + H)
    want = T.check_three_level(logits)
    out = torch.full((N, H, W, 5), SENTINEL, dtype=torch.uint8, device=DEV)
    got = ops.xbd_tta_merge(dev(logits), out=out)
    assert got is out and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(ops.xbd_tta_merge(dev(logits)).cpu().numpy(), want)


@pytest.mark.parametrize("H,W", [(37, 41), (40, 40), (1024, 1024)])
def test_merge_undoes_every_flip_and_writes_channels_last(H, W):
    """logits[k] = flip_k(L): the output is the quantisation of sigmoid(L) alone; a wrong un-flip mixes levels (bytes other than
    0 / 127 / 255 appear), a channel-first layout puts them elsewhere"""
    from dahitra_amd import ops
    logits, L = T.equivariant(H, W, seed=H + W)
    want = T.check_three_level(logits)
    single = np.trunc(T.sigmoid32(L) * np.float32(255)).astype(np.uint8).transpose(1, 2, 0)
    assert np.array_equal(want[0], single) and set(np.unique(single).tolist()) == {0, 127, 255}
    got = ops.xbd_tta_merge(dev(logits)).cpu().numpy()
    assert got.shape == (1, H, W, 5) and np.array_equal(got[0], single)


@pytest.mark.parametrize("N,H,W", [(1, 37, 41), (2, 40, 40), (1, 128, 1024)])
def test_merge_on_random_logits_agrees_with_the_float64_restatement(N, H, W):
    from dahitra_amd import ops
    logits = T.random_logits(N, H, W, seed=N * 10 + H)
    got = ops.xbd_tta_merge(dev(logits)).cpu().numpy()
    share = T.check_against_merge64(got, T.merge64(logits))
    same = float((got == T.merge(logits)).mean())
    print("undecided bytes: %.3f %%; equal to the float32 restatement: %.4f %%" % (100 * share, 100 * same))
    assert len(np.unique(got)) > 8


def offset_view(a, dtype):
    """a device copy of `a` that starts one element into a larger buffer"""
    buf = torch.zeros(a.size + 1, dtype=dtype, device=DEV)[1:].view(a.shape)
    buf.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return buf


def test_unaligned_base_pointers_take_the_scalar_path():
    """views that start 1 float / 1 byte into their buffers: no plane is aligned to its vector, although W % 4 == 0"""
    from dahitra_amd import ops
    N, H, W = 2, 40, 40
    for logits in (T.three_level(N, H, W, seed=11), T.random_logits(N, H, W, seed=12)):
        aligned = ops.xbd_tta_merge(dev(logits))
        if set(np.unique(logits).tolist()) <= set(T.LEVELS):
            assert np.array_equal(aligned.cpu().numpy(), T.check_three_level(logits))
        dl = offset_view(logits, torch.float32)
        out = torch.full((N * H * W * 5 + 1,), SENTINEL, dtype=torch.uint8, device=DEV)
        ov = out[1:].view(N, H, W, 5)
        assert dl.data_ptr() % 16 == 4 and ov.data_ptr() % 4 == 1
        assert torch.equal(ops.xbd_tta_merge(dl), aligned)              # unaligned logits, aligned output
        ops.xbd_tta_merge(dev(logits), out=ov)                          # aligned logits, unaligned output
        assert torch.equal(ov, aligned) and int(out[0]) == SENTINEL
        ops.xbd_tta_merge(dl, out=ov.fill_(SENTINEL))                   # both
        assert torch.equal(ov, aligned) and int(out[0]) == SENTINEL
    # the pack: sources one byte in, the output one float in
    pre, post = T.sources(N, H, W, seed=13)
    want = T.pack(pre, post, "bgr")
    dpre, dpost = offset_view(pre, torch.uint8), offset_view(post, torch.uint8)
    assert dpre.data_ptr() % 4 == 1
    assert np.array_equal(bits(ops.xbd_tta_pack(dpre, dpost).cpu().numpy()), bits(want))
    buf = torch.full((want.size + 1,), float("nan"), device=DEV)
    inp = buf[1:].view(want.shape)
    assert inp.data_ptr() % 16 == 4
    ops.xbd_tta_pack(dev(pre), dev(post), out=inp)
    assert np.array_equal(bits(inp.cpu().numpy()), bits(want)) and bool(torch.isnan(buf[0]))


def test_refused_arguments_raise_and_write_nothing():
    from dahitra_amd import _lib, ops
    L = _lib.lib()
    P, S = ops.P, ops.S
    pre = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=DEV)
    inp = torch.full((4, 6, 8, 8), -7.0, device=DEV)
    logits = torch.zeros(4, 5, 8, 8, device=DEV)
    out = torch.full((1, 8, 8, 5), SENTINEL, dtype=torch.uint8, device=DEV)
    good = dict(pre=P(pre), post=P(pre), N=1, H=8, W=8, bgr=1, inp=P(inp))
    order = ("pre", "post", "N", "H", "W", "bgr", "inp")
    for change in (dict(N=0), dict(N=-1), dict(N=16384), dict(H=0), dict(W=0), dict(H=1 << 16, W=1 << 15), dict(pre=P(None)),
                   dict(post=P(None)), dict(inp=P(None))):
        args = dict(good, **change)
        assert L.dh_xbd_tta_pack_u8(*[args[k] for k in order], S()) != 0, change
        assert L.dh_last_error().decode().startswith("xbd_tta_pack"), (change, L.dh_last_error())
    good = dict(logits=P(logits), N=1, H=8, W=8, out=P(out))
    order = ("logits", "N", "H", "W", "out")
    for change in (dict(N=0), dict(N=-1), dict(N=16384), dict(H=0), dict(W=0), dict(H=1 << 16, W=1 << 15), dict(logits=P(None)),
                   dict(out=P(None))):
        args = dict(good, **change)
        assert L.dh_xbd_tta_merge_u8(*[args[k] for k in order], S()) != 0, change
        assert L.dh_last_error().decode().startswith("xbd_tta_merge"), (change, L.dh_last_error())
    # through ops: 4 N = 65536 and N = 0 reach the library and are refused there
    big = torch.zeros(16384, 1, 1, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.HipLibraryError):
        ops.xbd_tta_pack(big, big)
    with pytest.raises(_lib.HipLibraryError):
        ops.xbd_tta_merge(torch.zeros(65536, 5, 1, 1, device=DEV))
    with pytest.raises((_lib.HipLibraryError, ValueError)):
        ops.xbd_tta_pack(pre[:0], pre[:0])
    with pytest.raises((_lib.HipLibraryError, ValueError)):
        ops.xbd_tta_merge(logits[:0])
    # ... and what ops itself refuses before any launch
    for bad in (torch.zeros(4, 7, 8, 8, device=DEV),                        # 7 channels
                torch.zeros(6, 5, 8, 8, device=DEV),                        # not four flips per image
                torch.zeros(4, 5, 8, 8),                                    # CPU
                torch.zeros(4, 5, 8, 8, device=DEV, dtype=torch.float16),
                torch.zeros(5, 8, 8, device=DEV),
                torch.zeros(4, 5, 8, 16, device=DEV)[..., ::2]):            # not contiguous
        with pytest.raises(ValueError):
            ops.xbd_tta_merge(bad, out=out)
    with pytest.raises(ValueError):
        ops.xbd_tta_merge(logits, out=out.cpu())
    with pytest.raises(ValueError):
        ops.xbd_tta_merge(logits, out=torch.zeros(1, 5, 8, 8, dtype=torch.uint8, device=DEV))
    for a, b, kw in ((pre, pre, dict(order="grb")), (pre.cpu(), pre.cpu(), {}), (pre, pre.cpu(), {}), (pre[0], pre[0], {}),
                     (pre.float(), pre.float(), {}), (pre, pre[:, :4], {}), (pre.permute(0, 2, 1, 3)[:, :, ::2], ) * 2 + ({},),
                     (pre, pre, dict(out=torch.zeros(4, 6, 8, 4, device=DEV)))):
        with pytest.raises(ValueError):
            ops.xbd_tta_pack(a, b, **dict(dict(out=inp), **kw))
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((inp == -7.0).all())
    # the good calls do write
    ops.xbd_tta_pack(pre, pre, out=inp)
    ops.xbd_tta_merge(logits, out=out)
    assert bool((inp == -1.0).all()) and bool((out == 127).all())          # byte 0 -> -1; sigmoid(0) = 0.5 -> trunc(127.5)


# ---- model level -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_case():
    """the net (fp32 compute, deterministic weights), two pairs of random 256 x 256 sources, and per pair the eager prediction
    with the net's own eager logits on ops.xbd_tta_pack's output (computed once)"""
    from dahitra_amd import ops
    from dahitra_amd.models import xbd
    net = xbd.BASE_Transformer_UNet(input_nc=3, output_nc=5, token_len=4, resnet_stages_num=4, with_pos='learned',
                                    with_decoder_pos=None, enc_depth=1, dec_depth=8).cuda()
    net.load_state_dict(O.deterministic_state(NAME))
    net.eval()
    pairs, eager, logits = [], [], []
    for seed in (31, 32):
        pre, post = (dev(a) for a in T.sources(1, 256, 256, seed=seed))
        pairs.append((pre, post))
        eager.append(xbd.predict_tta(net, pre, post, graph=False).clone())
        with torch.no_grad():
            logits.append(net(ops.xbd_tta_pack(pre, post)).float().cpu().numpy())
    return {"net": net, "pairs": pairs, "eager": eager, "logits": logits}


def test_eager_predict_is_the_restatement_on_the_nets_own_logits(model_case):
    from dahitra_amd.models import xbd
    for (pre, post), got, logits in zip(model_case["pairs"], model_case["eager"], model_case["logits"]):
        assert logits.shape == (4, 5, 256, 256) and logits.dtype == np.float32
        got = got.cpu().numpy()
        assert got.shape == (1, 256, 256, 5) and got.dtype == np.uint8
        share = T.check_against_merge64(got, T.merge64(logits))
        want = T.merge(logits)
        print("undecided bytes: %.3f %%; differ from the float32 restatement: %d of %d; distinct bytes: %d"
              % (100 * share, int((got != want).sum()), got.size, len(np.unique(got))))
        assert len(np.unique(got)) > 8, "a degenerate net cannot pass"
    assert not torch.equal(model_case["eager"][0], model_case["eager"][1])
    # the two orders feed the net different images
    pre, post = model_case["pairs"][0]
    assert not torch.equal(xbd.predict_tta(model_case["net"], pre, post, order="rgb", graph=False), model_case["eager"][0])


def test_graphed_predict_replays_bit_equal_to_the_eager_path_and_checks_its_inputs(model_case):
    from dahitra_amd.graph import GraphedXbdPredictStep
    from dahitra_amd.models import xbd
    net, pairs, eager = model_case["net"], model_case["pairs"], model_case["eager"]
    got = xbd.predict_tta(net, *pairs[0])
    assert got.shape == (1, 256, 256, 5) and got.dtype == torch.uint8 and torch.equal(got, eager[0])
    steps = net._xbd_predict_steps
    assert len(steps) == 1
    step = next(iter(steps.values()))
    assert isinstance(step, GraphedXbdPredictStep) and got is step.out
    again = xbd.predict_tta(net, *pairs[1])                      # a second replay, other sources
    assert again is step.out and torch.equal(again, eager[1]) and len(steps) == 1
    assert torch.equal(step.step(*pairs[0]), eager[0])
    # a pair of another shape is refused, nothing is broadcast
    pre, post = pairs[0]
    for bad in ((pre[:, :128], post[:, :128]), (pre, post[:, :, :128]), (pre.expand(2, -1, -1, -1), post.expand(2, -1, -1, -1)),
                (pre.float(), post.float()), (pre, None)):
        with pytest.raises(ValueError):
            step.step(*bad)
    assert torch.equal(step.out, eager[0])
    # a net in training mode
    net.train()
    with pytest.raises(RuntimeError, match="eval-mode forward"):
        step.step(pre, post)
    net.eval()
    # the arena is rebuilt (a parameter replaced): predict_tta records a new step and does not replay the stale one
    p = next(net.parameters())
    p.data = p.data.clone()
    fresh = xbd.predict_tta(net.train(False), *pairs[1])
    new = next(iter(steps.values()))
    assert len(steps) == 1 and new is not step and new._generation == net._arena.generation != step._generation
    assert fresh is new.out and torch.equal(fresh, eager[1])
    with pytest.raises(RuntimeError, match="rebuilt"):
        step.step(pre, post)


def test_predict_dir_writes_the_scripts_files(model_case, tmp_path):
    from PIL import Image
    from dahitra_amd.models import xbd
    net = model_case["net"]
    src, dst = tmp_path / "images", tmp_path / "pred" / "cls_"
    src.mkdir()
    names = []
    for i, size in enumerate((256, 256, 256)):
        pre, post = T.sources(1, size, size, seed=40 + i)
        if i == 2:
            post = post[:, :128, :128]                         # a pair whose shapes differ: skipped
        f = "area_%08d_pre_disaster.png" % i
        Image.fromarray(pre[0]).save(str(src / f))
        Image.fromarray(np.ascontiguousarray(post[0])).save(str(src / f.replace("_pre_", "_post_")))
        names.append((f, pre, post))
    written = xbd.predict_dir(net, str(src), str(dst))
    assert written == [names[0][0], names[1][0]]
    assert sorted(os.listdir(str(dst))) == sorted(n for f in written for n in xbd.predict_names(f))
    for f, pre, post in names[:2]:
        want = xbd.predict_tta(net, dev(pre), dev(post))[0].cpu().numpy()
        full, part1, part2 = xbd.predict_names(f)
        assert full == f.replace(".png", "_full.png.png.npy")
        msk = np.load(str(dst / full))
        assert msk.shape == (256, 256, 5) and msk.dtype == np.uint8 and np.array_equal(msk, want)
        # what cv2.imread(..., IMREAD_UNCHANGED) returns is the stored RGB image with its channels reversed
        for name, part in ((part1, msk[..., :3]), (part2, msk[..., 2:])):
            img = Image.open(str(dst / name))
            assert img.mode == "RGB" and np.array_equal(np.asarray(img)[..., ::-1], part), name
    assert len(np.unique(msk)) > 8
