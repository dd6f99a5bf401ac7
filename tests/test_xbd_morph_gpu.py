"""The xBD mask morphology on the MI355X (csrc/xbd_morph.hip): the window kernel in its three forms, the hole fill,
models/xbd.clean_footprint, the loader's `dilate` switch and the cleaned footprint through building_damage / building_match,
against the numpy restatements of tests/_xbd_morph_cases.py (themselves held against scipy.ndimage in test_xbd_morph_cpu.py).
Everything is integer: every comparison is exact.  The kernel's tile is 32 x 64, so (1, 70, 130) lies one and two pixels past a
tile edge in both directions; C.SHAPES needs no further shape."""
import functools
import random

import numpy as np
import pytest
import torch

import _xbd_match_cases as M
import _xbd_morph_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL = 0xAA


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def filled_u8(*shape):
    return torch.full(shape, FILL, dtype=torch.uint8, device=DEV)


@functools.lru_cache(maxsize=None)
def window_refs(N, H, W):
    """name -> (input, {(op, k): restatement}), computed once and shared"""
    refs = {}
    for name, a in C.map_cases(N, H, W).items():
        want = {}
        for k in C.KS:
            want["dilate", k], want["erode", k] = C.win_or(a, k), C.erode(a, k)
            want["opening", k], want["closing", k] = C.win_or(want["erode", k], k), C.erode(want["dilate", k], k)
        refs[name] = (a, want)
    return refs


def test_the_tile_is_the_one_the_shapes_were_chosen_for():
    from dahitra_amd import _lib, ops
    assert (_lib.lib().dh_xbd_morph_tile_h(), _lib.lib().dh_xbd_morph_tile_w()) == ops.XBD_MORPH_TILE == (32, 64)
    assert (1, 70, 130) in C.SHAPES and 70 == 2 * 32 + 6 and 130 == 2 * 64 + 2 and (1, 1, 1) in C.SHAPES


@pytest.mark.parametrize("N,H,W", C.SHAPES)
def test_dilate_erode_opening_closing_equal_the_restatement(N, H, W):
    from dahitra_amd import ops
    from dahitra_amd.models import xbd
    grew = shrank = 0
    for name, (a, want) in window_refs(N, H, W).items():
        d = dev(a)
        for k in C.KS:
            for op in ("dilate", "erode"):
                out = filled_u8(N, H, W)
                assert ops.xbd_morph(d, op, k, out=out) is out
                assert np.array_equal(host(out), want[op, k]), (name, op, k)
            got = xbd.dilate(d, k)
            assert got.dtype == torch.uint8 and got.shape == (N, H, W) and np.array_equal(host(got), want["dilate", k])
            assert np.array_equal(host(xbd.erode(d, k)), want["erode", k]), (name, k)
            assert np.array_equal(host(xbd.opening(d, k)), want["opening", k]), (name, k)
            assert np.array_equal(host(xbd.closing(d, k)), want["closing", k]), (name, k)
            grew += int(want["dilate", k].sum()) - int((a != 0).sum())
            shrank += int((a != 0).sum()) - int(want["erode", k].sum())
        assert torch.equal(d, dev(a)), "the input is not written"
    assert (grew > 0 and shrank > 0) or H * W == 1, "a single pixel has nothing to grow into"


@pytest.mark.parametrize("N,H,W", C.SHAPES)
def test_the_mask_form_equals_the_restatement(N, H, W):
    from dahitra_amd import ops
    for name, lbl in C.label_cases(N, H, W).items():
        msk = C.to_msk(lbl)
        d = dev(msk)
        for k in C.MSK_KS:
            want = C.msk_dilate(msk, k)
            out = filled_u8(N, 5, H, W)
            assert ops.xbd_msk_dilate(d, k, out=out) is out
            assert np.array_equal(host(out), want), (name, k)
        assert np.array_equal(host(ops.xbd_msk_dilate(d)), C.msk_dilate(msk, 5)), "k = 5 is the default"
        # channel 0 of the input is not read, and a set byte need not be 1
        other = msk * 255
        other[:, 0] = 7
        assert np.array_equal(host(ops.xbd_msk_dilate(dev(other), 5)), C.msk_dilate(msk, 5)), name


@functools.lru_cache(maxsize=None)
def hole_refs(N, H, W):
    return {name: (a, {bg: C.fill_holes(a, bg) for bg in (4, 8)}) for name, a in C.hole_cases(N, H, W).items()}


@pytest.mark.parametrize("N,H,W", C.HOLE_SHAPES)
def test_fill_holes_equals_the_restatement(N, H, W):
    from dahitra_amd import ops
    from dahitra_amd.models import xbd
    filled = 0
    for name, (a, want) in hole_refs(N, H, W).items():
        d = dev(a)
        for bg in (4, 8):
            out = filled_u8(N, H, W)
            ws = filled_u8(ops.xbd_fill_holes_ws_bytes(N, H, W))
            assert ops.xbd_fill_holes(d, bg, out=out, ws=ws) is out
            assert np.array_equal(host(out), want[bg]), (name, bg)
            filled += int(want[bg].sum()) - int((a != 0).sum())
        assert np.array_equal(host(xbd.fill_holes(d)), want[4]), name
        assert np.array_equal(host(xbd.fill_holes(d, background=8)), want[8]), name
    assert filled > 0
    if (N, H, W) == (1, 256, 256):                              # thousands of complement components: there is no cap
        a, want = hole_refs(N, H, W)["noise50"]
        _, count = ops.xbd_cc_label(dev((a == 0).astype(np.uint8)), 4)
        assert int(count[0]) > 4096 and int(want[4].sum()) - int((a != 0).sum()) > 1000


@pytest.mark.parametrize("N,H,W", [s for s in C.SHAPES if s not in C.HOLE_SHAPES])
def test_fill_holes_on_images_smaller_than_a_ring(N, H, W):
    from dahitra_amd import ops
    for name, a in C.map_cases(N, H, W).items():
        for bg in (4, 8):
            assert np.array_equal(host(ops.xbd_fill_holes(dev(a), bg)), C.fill_holes(a, bg)), (name, bg)


def test_clean_footprint_equals_its_restatement():
    from dahitra_amd.models import xbd
    N, H, W = 1, 70, 130
    for a in (C.noise(N, H, W, 500), C.noise(N, H, W, 30), C.bridged_squares()[0]):
        d = dev(a)
        for kw in (dict(open=3, close=3, fill=True), dict(open=3), dict(close=5), dict(fill=True), dict(fill=True, background=8),
                   dict(open=3, fill=True), dict(open=5, close=3), dict()):
            got = xbd.clean_footprint(d, **kw)
            assert got.dtype == torch.uint8 and np.array_equal(host(got), C.clean_footprint(a, **kw)), kw
    some = C.clean_footprint(C.noise(N, H, W, 500), 3, 3, True)
    assert 0 < some.sum() < some.size
    with pytest.raises(ValueError):
        xbd.clean_footprint(d, open=4)
    with pytest.raises(ValueError):
        xbd.clean_footprint(d, close=33)
    with pytest.raises(ValueError):
        xbd.clean_footprint(d, fill=True, background=6)
    with pytest.raises(ValueError):
        xbd.clean_footprint(d, open=3, ws=torch.empty(16, dtype=torch.uint8, device=DEV))


def test_nothing_is_written_past_the_buffers_and_every_byte_inside():
    """input and output are views into larger buffers whose other bytes are guards; an odd offset also takes the byte-by-byte path
    on a width that is a multiple of four"""
    from dahitra_amd import ops
    N, H, W = 1, 37, 68
    a = C.noise(N, H, W, 500)
    msk = C.to_msk(C.labels3(N, H, W))
    G = 256
    for off in (0, 13):
        def guarded(values):
            buf = filled_u8(G + off + values.size + G)
            view = buf[G + off:G + off + values.size].view(values.shape)
            view.copy_(torch.from_numpy(values))
            return buf, view

        def guards_kept(buf, n):
            return bool((buf[:G + off] == FILL).all()) and bool((buf[G + off + n:] == FILL).all())

        src_buf, src = guarded(a)
        for op, want in (("dilate", C.win_or(a, 9)), ("erode", C.erode(a, 9))):
            out_buf, out = guarded(np.full_like(a, FILL))
            ops.xbd_morph(src, op, 9, out=out)
            assert np.array_equal(host(out), want) and guards_kept(out_buf, a.size) and guards_kept(src_buf, a.size), (off, op)
        out_buf, out = guarded(np.full_like(a, FILL))
        need = ops.xbd_fill_holes_ws_bytes(N, H, W)
        ws_buf = filled_u8(G + 4 + need + G)
        start = G + (-(ws_buf.data_ptr() + G)) % 4              # the workspace holds int32
        ops.xbd_fill_holes(src, 4, out=out, ws=ws_buf[start:start + need])
        assert np.array_equal(host(out), C.fill_holes(a, 4)) and guards_kept(out_buf, a.size)
        assert bool((ws_buf[:start] == FILL).all()) and bool((ws_buf[start + need:] == FILL).all())
        assert torch.equal(src, dev(a)) and guards_kept(src_buf, a.size)
        msk_buf, dmsk = guarded(msk)
        out_buf, out = guarded(np.full_like(msk, FILL))
        ops.xbd_msk_dilate(dmsk, 5, out=out)
        assert np.array_equal(host(out), C.msk_dilate(msk, 5)) and guards_kept(out_buf, msk.size) and guards_kept(msk_buf, msk.size)


def test_clean_footprint_replays_from_a_graph():
    from dahitra_amd import ops
    from dahitra_amd.models import xbd
    N, H, W = 1, 70, 130
    cases = [C.noise(N, H, W, 500), C.spiral(N, H, W, closed=True) | C.noise(N, H, W, 5) // 255]
    src = dev(cases[0])
    out = filled_u8(N, H, W)
    ws = filled_u8(ops.xbd_fill_holes_ws_bytes(N, H, W) + 2 * N * H * W)

    def run():
        assert xbd.clean_footprint(src, open=3, close=3, fill=True, out=out, ws=ws) is out

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                    # warm-up outside the capture: code objects loaded
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for a in (cases[1], cases[0]):
        src.copy_(torch.from_numpy(a))
        out.fill_(FILL)
        ws.fill_(FILL)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(out), C.clean_footprint(a, 3, 3, True))
    assert not np.array_equal(C.clean_footprint(cases[0], 3, 3, True), C.clean_footprint(cases[1], 3, 3, True))


def loader_sources():
    """two 96 x 96 samples; the crop of the rows below is the window [16, 80) x [16, 80).  Sample 0: a class 2 building that
    touches the crop's left edge, a class 3 building that lies entirely in the first column outside it (x = 80 ..), and buildings
    of classes 1 and 4 inside; sample 1: random labels"""
    rng = np.random.RandomState(96)
    pre, post = (rng.randint(0, 256, size=(2, 96, 96, 3)).astype(np.uint8) for _ in range(2))
    label = np.zeros((2, 96, 96), dtype=np.uint8)
    label[0, 20:30, 16:24] = 2
    label[0, 40:50, 80:88] = 3
    label[0, 50:58, 40:52] = 1
    label[0, 54:66, 54:60] = 4
    label[0, 76:80, 30:36] = 1
    label[1] = C.labels3(1, 96, 96)[0]
    pmask = ((label > 0) * 255).astype(np.uint8)
    return pre, post, pmask, label


ROWS = [[16, 16, 0, 0, 0, 0, 0, 64, 64], [16, 16, 1, 1, 0, 0, 0, 64, 64], [16, 16, 0, 0, 1, 5, 7, 50, 40], [3, 29, 1, 0, 1, 0, 0, 64, 33]]
IDX = [0, 0, 0, 1]


def test_the_loader_dilates_the_augmented_crop():
    from dahitra_amd.datasets.xbd_pipeline import GpuXbdPipeline
    src = loader_sources()
    pipe = GpuXbdPipeline(*(torch.from_numpy(a).to(DEV) for a in src), files=["s0", "s1"])
    plain = pipe.make_batch(IDX, 64, ROWS)
    also = pipe.make_batch(IDX, 64, ROWS, dilate=0)
    got = pipe.make_batch(IDX, 64, ROWS, dilate=5)
    assert torch.equal(also["msk"], plain["msk"]) and torch.equal(also["img"], plain["img"])
    base = host(plain["msk"])
    assert np.array_equal(base[0], C.to_msk(src[3][:1, 16:80, 16:80])[0]), "row 0 is the plain crop"
    want = C.msk_dilate(base, 5)
    assert got["msk"].dtype == torch.uint8 and got["msk"].shape == (4, 5, 64, 64)
    assert np.array_equal(host(got["msk"]), want)
    assert want.sum() > base.sum() and (want[:, 1:].sum(axis=1) <= 1).all() and not want.argmax(axis=1).any()
    assert torch.equal(got["img"], plain["img"]) and got["fn"] == plain["fn"]
    assert got["lbl_msk"] is plain["lbl_msk"] and not bool(got["lbl_msk"].any())
    # the building that touches the edge is dilated up to it; the one just outside leaves no mark on the unresized crops
    assert want[0, 2, 2:16, 0:10].all() and not want[0, 2, :, 10:].any()
    assert not want[0, 3].any() and not want[1, 3].any() and src[3][0, 40:50, 80].all()
    assert C.win_or(src[3][:1] == 3, 5)[0, 16:80, 16:80].any(), "dilated before the crop it would have reached columns 78 and 79"
    assert np.array_equal(host(pipe.make_batch(IDX, 64, ROWS, dilate=3)["msk"]), C.msk_dilate(base, 3))
    # an epoch: the same draws with and without the switch
    one = list(pipe.batches(2, 64, train=True, rng=random.Random(7), dilate=5))
    two = list(pipe.batches(2, 64, train=True, rng=random.Random(7)))
    assert len(one) == len(two) == 1
    for x, y in zip(one, two):
        assert x["fn"] == y["fn"] and torch.equal(x["img"], y["img"]) and x["lbl_msk"] is y["lbl_msk"]
        assert np.array_equal(host(x["msk"]), C.msk_dilate(host(y["msk"]), 5))
    with pytest.raises(ValueError, match="dilate"):
        pipe.make_batch(IDX, 64, ROWS, dilate=4)
    with pytest.raises(ValueError, match="dilate"):
        pipe.make_batch(IDX, 64, ROWS, train=False, dilate=5)


def test_the_cleaned_footprint_matches_two_buildings_and_the_raw_one_none():
    from dahitra_amd.models import xbd
    fp, gt = C.bridged_squares()
    _, H, W = fp.shape
    # pinned on the host first (test_xbd_morph_cpu.py holds the same numbers)
    assert M.building_match(C.clean_footprint(fp, open=3, fill=True) * 2, gt)["loc"].tolist() == [2, 0, 0]
    assert M.building_match(fp * 2, gt)["loc"].tolist() == [0, 1, 2]
    msk = np.zeros((1, H, W, 5), dtype=np.uint8)
    msk[..., 2] = 255                                           # every pixel votes class 2
    dmsk, dfp, dgt = dev(msk), dev(fp), dev(gt)
    clean = xbd.clean_footprint(dfp, open=3, fill=True)
    cleaned = xbd.building_match(xbd.building_damage(dmsk, footprint=clean).map, dgt)
    raw = xbd.building_match(xbd.building_damage(dmsk, footprint=dfp).map, dgt)
    assert cleaned.loc.tolist() == [2, 0, 0] and cleaned.confusion[1, 2] == 2 and cleaned.pred_count.tolist() == [2]
    assert raw.loc.tolist() == [0, 1, 2] and raw.pred_count.tolist() == [1]
