"""The xBD prediction for several snapshots and 4 or 8 views on the MI355X: dh_xbd_tta_pack_views_u8 / dh_xbd_tta_merge_multi_u8
(csrc/xbd_ensemble.hip) against the numpy restatement (tests/_xbd_ensemble_cases.py) and against the 4-flip kernels, then
models/xbd.predict_ensemble / predict_dir_ensemble / load_snapshot and graph.GraphedXbdEnsembleStep on the model.  The pack
comparison is on float32 bits.  The merge comparison is exact where the logits are built so that no rounding can decide a byte,
and against the float64 value with the band of _xbd_tta_cases elsewhere."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _xbd_ensemble_cases as E
import _xbd_tta_cases as T
import cdnet_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAME = "xbd_unet_transformer_nodecpos"
SENTINEL = 0xA5
SHAPES = [(N, S) for S in E.SIZES for N in E.BATCHES]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("N,S", SHAPES)
def test_pack_is_bit_equal_to_the_restatement_for_both_view_counts_and_orders(N, S):
    from dahitra_amd import ops
    pre, post = T.sources(N, S, S, seed=N * 1000 + S)
    dpre, dpost = dev(pre), dev(post)
    for V in (4, 8):
        for order in ("bgr", "rgb"):
            want = E.pack_views(pre, post, order, V)
            out = torch.full((V * N, 6, S, S), float("nan"), device=DEV)         # every element of a given buffer is written
            assert ops.xbd_tta_pack_views(dpre, dpost, order, V, out=out) is out
            assert np.array_equal(bits(out.cpu().numpy()), bits(want)), (V, order)
            got = ops.xbd_tta_pack_views(dpre, dpost, order, views=V)
            assert got.shape == (V * N, 6, S, S) and got.dtype == torch.float32 and torch.equal(got, out)
            if V == 4:
                assert torch.equal(got, ops.xbd_tta_pack(dpre, dpost, order))
    assert torch.equal(ops.xbd_tta_pack_views(dpre, dpost), ops.xbd_tta_pack(dpre, dpost)), "'bgr' and views=4 are the defaults"


def test_pack_of_an_image_that_is_not_square():
    """views=4 only: a partial tile on either side, both paths"""
    from dahitra_amd import ops
    for N, H, W in ((1, 37, 41), (2, 33, 68), (1, 70, 36)):
        pre, post = T.sources(N, H, W, seed=H + W)
        got = ops.xbd_tta_pack_views(dev(pre), dev(post), "rgb", 4)
        assert np.array_equal(bits(got.cpu().numpy()), bits(T.pack(pre, post, "rgb")))


def offset_view(a, dtype):
    """a device copy of `a` that starts one element into a larger buffer"""
    buf = torch.zeros(a.size + 1, dtype=dtype, device=DEV)[1:].view(a.shape)
    buf.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return buf


def test_unaligned_base_pointers_take_the_scalar_path():
    """a destination that starts 4 bytes into its buffer, sources one byte in, logits one float in, an output one byte in: no
    vector is aligned although S % 4 == 0, and the bytes are the same"""
    from dahitra_amd import ops
    N, S = 2, 36
    pre, post = T.sources(N, S, S, seed=13)
    for V in (4, 8):
        want = E.pack_views(pre, post, "bgr", V)
        buf = torch.full((want.size + 1,), float("nan"), device=DEV)
        inp = buf[1:].view(want.shape)
        assert inp.data_ptr() % 16 == 4
        ops.xbd_tta_pack_views(dev(pre), dev(post), views=V, out=inp)
        assert np.array_equal(bits(inp.cpu().numpy()), bits(want)) and bool(torch.isnan(buf[0]))
        dpre, dpost = offset_view(pre, torch.uint8), offset_view(post, torch.uint8)
        assert dpre.data_ptr() % 4 == 1
        assert np.array_equal(bits(ops.xbd_tta_pack_views(dpre, dpost, views=V).cpu().numpy()), bits(want))
        logits = E.random_multi(2, V, N, S, seed=14 + V)
        aligned = ops.xbd_tta_merge_multi([dev(l) for l in logits], V)
        T.check_against_merge64(aligned.cpu().numpy(), E.merge_multi64(logits, V))
        shifted = [dev(logits[0]), offset_view(logits[1], torch.float32)]      # one misaligned entry turns the vector loads off
        assert shifted[1].data_ptr() % 16 == 4
        assert torch.equal(ops.xbd_tta_merge_multi(shifted, V), aligned)
        out = torch.full((N * S * S * 5 + 1,), SENTINEL, dtype=torch.uint8, device=DEV)
        ov = out[1:].view(N, S, S, 5)
        ops.xbd_tta_merge_multi([dev(l) for l in logits], V, out=ov)
        assert torch.equal(ov, aligned) and int(out[0]) == SENTINEL
        ops.xbd_tta_merge_multi(shifted, V, out=ov.fill_(SENTINEL))
        assert torch.equal(ov, aligned) and int(out[0]) == SENTINEL


@pytest.mark.parametrize("N,S", [(2, 4), (1, 33), (2, 36), (1, 68), (1, 256)])
def test_merge_of_one_model_and_four_views_is_the_four_flip_merge(N, S):
    from dahitra_amd import ops
    for H, W in ((S, S), (S, S + 5), (S + 8, S)):
        logits = dev(T.random_logits(N, H, W, seed=N * 10 + H + W))
        assert torch.equal(ops.xbd_tta_merge_multi([logits], 4), ops.xbd_tta_merge(logits))
        assert torch.equal(ops.xbd_tta_merge_multi((logits,)), ops.xbd_tta_merge(logits)), "views=4 is the default; a tuple is a list"


@pytest.mark.parametrize("M,V", E.EXACT_MV)
@pytest.mark.parametrize("N,S", SHAPES)
def test_merge_is_exact_on_three_level_logits(M, V, N, S):
    from dahitra_amd import ops
    logits = E.three_level_multi(M, V, N, S, seed=M * 1000 + V * 100 + S + N)
    want = E.check_three_level_multi(logits, V)
    out = torch.full((N, S, S, 5), SENTINEL, dtype=torch.uint8, device=DEV)
    got = ops.xbd_tta_merge_multi([dev(l) for l in logits], V, out=out)
    assert got is out and np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("S", E.SIZES)
def test_merge_undoes_every_view_of_every_model(S):
    """logits[m][v] = view_v(L): the output is the quantisation of sigmoid(L) alone; a wrong un-transpose or a swapped rot90
    direction mixes levels (bytes other than 0 / 127 / 255 appear)"""
    from dahitra_amd import ops
    logits, L = E.equivariant_multi(2, 8, S, seed=S)
    want = E.check_three_level_multi(logits, 8)
    single = np.trunc(T.sigmoid32(L) * np.float32(255)).astype(np.uint8).transpose(1, 2, 0)
    assert np.array_equal(want[0], single) and set(np.unique(single).tolist()) == {0, 127, 255}
    got = ops.xbd_tta_merge_multi([dev(l) for l in logits], 8).cpu().numpy()
    assert got.shape == (1, S, S, 5) and np.array_equal(got[0], single)


@pytest.mark.parametrize("M,V,S,N,seed", E.RANDOM_CASES)
def test_merge_on_random_logits_agrees_with_the_float64_restatement(M, V, S, N, seed):
    from dahitra_amd import ops
    logits = E.random_multi(M, V, N, S, seed)
    got = ops.xbd_tta_merge_multi([dev(l) for l in logits], V).cpu().numpy()
    share = T.check_against_merge64(got, E.merge_multi64(logits, V))
    same = float((got == E.merge_multi(logits, V)).mean())
    print("M V = %d: undecided bytes: %.3f %%; equal to the float32 restatement: %.4f %%" % (M * V, 100 * share, 100 * same))
    assert len(np.unique(got)) > 8


@pytest.mark.parametrize("M,V", [(4, 4), (8, 4), (2, 8), (4, 8)])
def test_every_model_contributes_once_and_in_its_own_slot(M, V):
    from dahitra_amd import ops
    # one-hot regions: at a pixel of region r model r alone says 1: the mean is 1 / M, 255 / M is .75, .875 or .5 above a byte
    S = 36
    logits, region = E.one_hot_models(M, V, S, seed=M + V)
    want = E.check_three_level_multi(logits, V)
    assert (want == 255 // M).all() and abs(255 / M - 255 // M) >= 0.5
    d = [dev(l) for l in logits]
    assert np.array_equal(ops.xbd_tta_merge_multi(d, V).cpu().numpy(), want)
    twice = ops.xbd_tta_merge_multi([d[0]] + d[:-1], V).cpu().numpy()[0].transpose(2, 0, 1)      # model 0 twice, the last one left out
    assert (twice[region == 0] == (2 * 255) // M).all() and (twice[region == M - 1] == 0).all()
    # constant levels, one per model: +40, 0, -40, -40, ...: the mean is 1.5 / M, and 255 * 1.5 / M is .625 or .8125 above a byte
    levels = [40.0, 0.0] + [-40.0] * (M - 2)
    const = [np.full((V, 5, S, S), lv, dtype=np.float32) for lv in levels]
    want = E.check_three_level_multi(const, V)
    v = 255 * 1.5 / M
    assert (want == int(v)).all() and 0.1 < v - int(v) < 0.9
    for order in (list(range(M)), list(range(M))[::-1]):
        got = ops.xbd_tta_merge_multi([dev(const[m]) for m in order], V).cpu().numpy()
        assert np.array_equal(got, want)


def test_refused_arguments_raise_and_write_nothing():
    from dahitra_amd import _lib, ops
    L = _lib.lib()
    P, S = ops.P, ops.S
    pre = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=DEV)
    wide = torch.zeros(1, 8, 12, 3, dtype=torch.uint8, device=DEV)
    inp = torch.full((8, 6, 8, 8), -7.0, device=DEV)
    logits = torch.zeros(8, 5, 8, 8, device=DEV)
    out = torch.full((1, 8, 8, 5), SENTINEL, dtype=torch.uint8, device=DEV)
    good = dict(pre=P(pre), post=P(pre), N=1, H=8, W=8, bgr=1, V=8, inp=P(inp))
    order = ("pre", "post", "N", "H", "W", "bgr", "V", "inp")
    for change in (dict(N=0), dict(N=-1), dict(N=8192), dict(V=4, N=16384), dict(H=0, W=0), dict(V=4, H=0), dict(V=4, W=0),
                   dict(V=4, H=1 << 16, W=1 << 15), dict(H=1 << 16, W=1 << 16), dict(V=0), dict(V=2), dict(V=6), dict(V=16),
                   dict(W=12), dict(H=4), dict(pre=P(None)), dict(post=P(None)), dict(inp=P(None)),
                   dict(inp=ctypes.c_void_p(inp.data_ptr() + 2))):
        args = dict(good, **change)
        assert L.dh_xbd_tta_pack_views_u8(*[args[k] for k in order], S()) != 0, change
        assert L.dh_last_error().decode().startswith("xbd_tta_pack_views"), (change, L.dh_last_error())

    def table(*ptrs):
        return (ctypes.c_void_p * len(ptrs))(*ptrs)

    keep = [table(logits.data_ptr()), table(logits.data_ptr(), logits.data_ptr()), table(logits.data_ptr(), None),
            table(logits.data_ptr(), logits.data_ptr() + 2), table(*[logits.data_ptr()] * 9)]
    tab = lambda i: ctypes.cast(keep[i], ctypes.c_void_p)
    good = dict(table=tab(0), M=1, V=8, N=1, H=8, W=8, out=P(out))
    order = ("table", "M", "V", "N", "H", "W", "out")
    for change in (dict(N=0), dict(N=-1), dict(N=8192), dict(V=4, N=16384), dict(H=0, W=0), dict(V=4, H=0), dict(V=4, W=0),
                   dict(V=4, H=1 << 16, W=1 << 15), dict(V=0), dict(V=2), dict(V=16), dict(W=12), dict(H=4), dict(M=0), dict(M=-1),
                   dict(M=9, table=tab(4)), dict(table=P(None)), dict(out=P(None)), dict(M=2, table=tab(2)), dict(M=2, table=tab(3))):
        args = dict(good, **change)
        assert L.dh_xbd_tta_merge_multi_u8(*[args[k] for k in order], S()) != 0, change
        assert L.dh_last_error().decode().startswith("xbd_tta_merge_multi"), (change, L.dh_last_error())
    # through ops: V N = 65536 reaches the library and is refused there
    big = torch.zeros(8192, 1, 1, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.HipLibraryError):
        ops.xbd_tta_pack_views(big, big, views=8)
    with pytest.raises(_lib.HipLibraryError):
        ops.xbd_tta_merge_multi([torch.zeros(65536, 5, 1, 1, device=DEV)], views=8)
    with pytest.raises((_lib.HipLibraryError, ValueError)):
        ops.xbd_tta_pack_views(pre[:0], pre[:0])
    with pytest.raises((_lib.HipLibraryError, ValueError)):
        ops.xbd_tta_merge_multi([logits[:0]])
    # ... and what ops itself refuses before any launch
    for bad in (torch.zeros(8, 7, 8, 8, device=DEV),                        # 7 channels
                torch.zeros(12, 5, 8, 8, device=DEV),                       # not eight views per image
                torch.zeros(8, 5, 8, 8),                                    # CPU
                torch.zeros(8, 5, 8, 8, device=DEV, dtype=torch.float16),
                torch.zeros(5, 8, 8, device=DEV),
                torch.zeros(8, 5, 8, 12, device=DEV),                       # another shape; alone: not square
                torch.zeros(8, 5, 8, 16, device=DEV)[..., ::2]):            # not contiguous
        with pytest.raises(ValueError):
            ops.xbd_tta_merge_multi([bad], 8, out=out)
        with pytest.raises(ValueError):
            ops.xbd_tta_merge_multi([logits, bad], 8, out=out)              # ... in any slot of the list
    for lst, kw in (([], {}), ([logits] * 9, {}), (logits, {}), ([logits], dict(views=6)), ([logits], dict(views=16)),
                    ([logits], dict(views=8, out=out.cpu())),
                    ([logits], dict(views=8, out=torch.zeros(1, 5, 8, 8, dtype=torch.uint8, device=DEV)))):
        with pytest.raises(ValueError):
            ops.xbd_tta_merge_multi(lst, **dict(dict(views=8, out=out), **kw))
    with pytest.raises(ValueError, match="square"):
        ops.xbd_tta_pack_views(wide, wide, views=8)
    for a, b, kw in ((pre, pre, dict(order="grb")), (pre, pre, dict(views=2)), (pre, pre, dict(views=16)), (pre.cpu(), pre.cpu(), {}),
                     (pre, pre.cpu(), {}), (pre[0], pre[0], {}), (pre.float(), pre.float(), {}), (pre, pre[:, :4], {}),
                     (pre.permute(0, 2, 1, 3)[:, :, ::2], ) * 2 + ({},), (pre, pre, dict(out=torch.zeros(8, 6, 8, 4, device=DEV))),
                     (pre, pre, dict(views=4))):                                # out holds eight views
        with pytest.raises(ValueError):
            ops.xbd_tta_pack_views(a, b, **dict(dict(views=8, out=inp), **kw))
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((inp == -7.0).all())
    # the good calls do write
    ops.xbd_tta_pack_views(pre, pre, views=8, out=inp)
    ops.xbd_tta_merge_multi([logits, logits], 8, out=out)
    assert bool((inp == -1.0).all()) and bool((out == 127).all())          # byte 0 -> -1; sigmoid(0) = 0.5 -> trunc(127.5)


# ---- model level -------------------------------------------------------------------------------------------------------
def build_net(salt):
    from dahitra_amd.models import xbd
    net = xbd.BASE_Transformer_UNet(input_nc=3, output_nc=5, token_len=4, resnet_stages_num=4, with_pos='learned',
                                    with_decoder_pos=None, enc_depth=1, dec_depth=8).cuda()
    net.load_state_dict(O.deterministic_state(NAME, salt=salt))
    return net.eval()


@pytest.fixture(scope="module")
def model_case():
    """two nets (fp32 compute, deterministic weights of two seeds), two pairs of random 256 x 256 sources, and per pair the
    eager 8-view prediction and the nets' own eager logits on ops.xbd_tta_pack_views' output (computed once)"""
    from dahitra_amd import ops
    from dahitra_amd.models import xbd
    nets = [build_net(0), build_net(1)]
    pairs, eager, logits = [], [], []
    for seed in (31, 32):
        pre, post = (dev(a) for a in T.sources(1, 256, 256, seed=seed))
        pairs.append((pre, post))
        eager.append(xbd.predict_ensemble(nets, pre, post, views=8, graph=False).clone())
        with torch.no_grad():
            inp = ops.xbd_tta_pack_views(pre, post, views=8)
            logits.append([net(inp).float().cpu().numpy() for net in nets])
    return {"nets": nets, "pairs": pairs, "eager": eager, "logits": logits}


def test_eager_ensemble_is_the_restatement_on_the_nets_own_logits(model_case):
    from dahitra_amd.models import xbd
    nets = model_case["nets"]
    for (pre, post), got, logits in zip(model_case["pairs"], model_case["eager"], model_case["logits"]):
        assert len(logits) == 2 and logits[0].shape == (8, 5, 256, 256) and logits[0].dtype == np.float32
        assert not np.array_equal(logits[0], logits[1]), "two seeds, two nets"
        got = got.cpu().numpy()
        assert got.shape == (1, 256, 256, 5) and got.dtype == np.uint8
        share = T.check_against_merge64(got, E.merge_multi64(logits, 8))
        want = E.merge_multi(logits, 8)
        print("undecided bytes: %.3f %%; differ from the float32 restatement: %d of %d; distinct bytes: %d"
              % (100 * share, int((got != want).sum()), got.size, len(np.unique(got))))
        assert len(np.unique(got)) > 8, "a degenerate net cannot pass"
    assert not torch.equal(model_case["eager"][0], model_case["eager"][1])
    # one net, four views: predict_tta's bytes, eagerly and through the recorded step
    pre, post = model_case["pairs"][0]
    single = xbd.predict_tta(nets[0], pre, post, graph=False)
    assert torch.equal(xbd.predict_ensemble([nets[0]], pre, post, views=4, graph=False), single)
    assert torch.equal(xbd.predict_ensemble((nets[0],), pre, post), single)
    assert not torch.equal(single, model_case["eager"][0])
    # the same net twice is the script's behaviour for a repeated snapshot: eight terms, each map twice
    logits4 = model_case["logits"][0][0][:4]
    twice = xbd.predict_ensemble([nets[0], nets[0]], pre, post, views=4, graph=False).cpu().numpy()
    T.check_against_merge64(twice, E.merge_multi64([logits4, logits4], 4))


def test_graphed_ensemble_replays_bit_equal_to_the_eager_path_and_checks_its_inputs(model_case):
    from dahitra_amd.graph import GraphedXbdEnsembleStep
    from dahitra_amd.models import xbd
    nets, pairs, eager = model_case["nets"], model_case["pairs"], model_case["eager"]
    nets[0].__dict__.pop('_xbd_ensemble_steps', None)
    got = xbd.predict_ensemble(nets, *pairs[0], views=8)
    assert got.shape == (1, 256, 256, 5) and got.dtype == torch.uint8 and torch.equal(got, eager[0])
    steps = nets[0]._xbd_ensemble_steps
    assert len(steps) == 1 and not hasattr(nets[1], '_xbd_ensemble_steps')
    step = next(iter(steps.values()))
    assert isinstance(step, GraphedXbdEnsembleStep) and got is step.out
    again = xbd.predict_ensemble(nets, *pairs[1], views=8)          # a second replay, other sources
    assert again is step.out and torch.equal(again, eager[1]) and len(steps) == 1
    assert torch.equal(step.step(*pairs[0]), eager[0])
    # a pair of another shape is refused, nothing is broadcast
    pre, post = pairs[0]
    for bad in ((pre[:, :128, :128], post[:, :128, :128]), (pre, post[:, :, :128]),
                (pre.expand(2, -1, -1, -1), post.expand(2, -1, -1, -1)), (pre.float(), post.float()), (pre, None)):
        with pytest.raises(ValueError):
            step.step(*bad)
    assert torch.equal(step.out, eager[0])
    # one net in training mode
    nets[1].train()
    with pytest.raises(RuntimeError, match="eval-mode forward"):
        step.step(pre, post)
    nets[1].eval()
    # the second net's arena is rebuilt (a parameter replaced): predict_ensemble records a new step, the stale one refuses
    p = next(nets[1].parameters())
    p.data = p.data.clone()
    fresh = xbd.predict_ensemble(nets, *pairs[1], views=8)
    new = next(iter(steps.values()))
    assert len(steps) == 1 and new is not step and not new.stale() and step.stale()
    assert fresh is new.out and torch.equal(fresh, eager[1])
    with pytest.raises(RuntimeError, match="rebuilt"):
        step.step(pre, post)


def test_predict_dir_ensemble_writes_the_scripts_files(model_case, tmp_path, capsys):
    from PIL import Image
    from dahitra_amd.models import xbd
    nets = model_case["nets"]
    src, dst = tmp_path / "images", tmp_path / "pred" / "cls_"
    src.mkdir()
    names = []
    for i, (h, w) in enumerate(((128, 128), (128, 128), (128, 192))):
        pre, post = T.sources(1, h, w, seed=40 + i)
        f = "area_%08d_pre_disaster.png" % i
        Image.fromarray(pre[0]).save(str(src / f))
        Image.fromarray(post[0]).save(str(src / f.replace("_pre_", "_post_")))
        names.append((f, pre, post))
    written = xbd.predict_dir_ensemble(nets, str(src), str(dst), views=8)
    assert written == [names[0][0], names[1][0]], "the pair that is not square is skipped under views=8"
    assert names[2][0] in capsys.readouterr().out
    assert sorted(os.listdir(str(dst))) == sorted(n for f in written for n in xbd.predict_names(f))
    for f, pre, post in names[:2]:
        want = xbd.predict_ensemble(nets, dev(pre), dev(post), views=8, graph=False)[0].cpu().numpy()
        full, part1, part2 = xbd.predict_names(f)
        msk = np.load(str(dst / full))
        assert msk.shape == (128, 128, 5) and msk.dtype == np.uint8 and np.array_equal(msk, want)
        for name, part in ((part1, msk[..., :3]), (part2, msk[..., 2:])):
            img = Image.open(str(dst / name))
            assert img.mode == "RGB" and np.array_equal(np.asarray(img)[..., ::-1], part), name
    assert len(np.unique(msk)) > 8


def test_load_snapshot_copies_what_fits_with_or_without_the_module_prefix(model_case, tmp_path, capsys):
    from dahitra_amd import ops
    from dahitra_amd.models import xbd
    a = model_case["nets"][0]
    pre, post = model_case["pairs"][0]
    inp = ops.xbd_tta_pack(pre[:, :64, :64].contiguous(), post[:, :64, :64].contiguous())
    with torch.no_grad():
        want = a(inp).float().clone()
    state = {k: v.detach().cpu().clone() for k, v in a.state_dict().items()}

    def save(tag, sd):
        """evaluate_val's snapshot: its four keys, the score a numpy float64"""
        path = str(tmp_path / ("snap_" + tag))
        torch.save({'epoch': 7, 'state_dict': sd, 'best_score': np.float64(0.625), 'optimizer': {'state': {}, 'param_groups': []}}, path)
        return path

    for tag, prefix in (("plain", ""), ("parallel", "module.")):
        path = save(tag, {prefix + k: v for k, v in state.items()})
        b = build_net(5)
        with torch.no_grad():
            assert not torch.equal(b(inp).float(), want)
        assert xbd.load_snapshot(b, path) == (7, 0.625)
        printed = capsys.readouterr().out
        assert "=> loading checkpoint '%s'" % path in printed and "loaded checkpoint '%s' (epoch 7, best_score 0.625)" % path in printed
        b.eval()
        with torch.no_grad():
            assert torch.equal(b(inp).float(), want), tag
    # a key of another size, and a key the model does not have, are left alone
    odd = next(k for k, v in state.items() if v.dim() == 4)
    kept = b.state_dict()[odd].detach().cpu().clone()
    other = build_net(6).state_dict()
    sd = {k: other[k].detach().cpu().clone() for k in state}
    assert not torch.equal(sd[odd], kept)
    sd[odd] = torch.zeros(3, 3)
    sd["no.such.key"] = torch.zeros(2)
    assert xbd.load_snapshot(b, save("odd", sd)) == (7, 0.625)
    got = b.state_dict()
    assert torch.equal(got[odd].cpu(), kept)
    assert all(torch.equal(got[k].cpu(), other[k].cpu()) for k in state if k != odd)
