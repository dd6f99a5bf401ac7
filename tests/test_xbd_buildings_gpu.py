"""The building step on the MI355X: dh_xbd_cc_label / _stats / _vote / _paint (csrc/xbd_buildings.hip) against the plain-Python
restatement (tests/_xbd_buildings_cases.py, itself checked against scipy in test_xbd_buildings_cpu.py), then models/xbd.buildings /
building_damage / building_confusion on the model, and the whole sequence replayed from a captured graph.  Everything is integer:
every comparison is exact."""
import numpy as np
import pytest
import torch

import _xbd_buildings_cases as B
import _xbd_visual_cases as V
import cdnet_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAME = "xbd_unet_transformer_nodecpos"
SENTINEL = 0xA5
SENT32 = -1515870811          # 0xA5A5A5A5 as int32


def small_shapes():
    from dahitra_amd import ops
    TH, TW = ops.XBD_CC_TILE
    # less than one tile; whole tiles, two images; one-pixel partial tiles on both axes; a fixed shape with partial tiles
    return [(1, 37, 41), (2, TH, 2 * TW), (1, TH + 1, 2 * TW + 3), (1, 130, 200)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def different_images(key):
    """the second image of a batch flipped, so that nothing of image 0 can pass for image 1"""
    key = key.copy()
    if key.shape[0] > 1:
        key[1] = key[1, ::-1, ::-1]
    return key


@pytest.mark.parametrize("shape", range(4))
def test_labels_and_count_equal_the_restatement(shape):
    from dahitra_amd import ops
    N, H, W = small_shapes()[shape]
    for name, key in B.patterns(N, H, W).items():
        key = different_images(key)
        dkey = dev(key)
        for conn in (4, 8):
            for keyed in (False, True):
                want, want_k = B.cc_label(key, conn, keyed)
                out = (torch.full((N, H, W), SENT32, dtype=torch.int32, device=DEV), torch.full((N,), SENT32, dtype=torch.int32, device=DEV))
                got = ops.xbd_cc_label(dkey, conn, keyed, out=out)
                assert got[0] is out[0] and got[1] is out[1]
                assert np.array_equal(out[1].cpu().numpy(), want_k), (name, conn, keyed, out[1].tolist(), want_k.tolist())
                assert np.array_equal(out[0].cpu().numpy(), want), (name, conn, keyed)
                fresh = ops.xbd_cc_label(dkey, conn, keyed)
                assert fresh[0].dtype == fresh[1].dtype == torch.int32 and fresh[0].shape == (N, H, W) and fresh[1].shape == (N,)
                assert torch.equal(fresh[0], out[0]) and torch.equal(fresh[1], out[1]), (name, conn, keyed)


@pytest.mark.parametrize("shape", range(4))
def test_table_votes_and_paint_equal_the_restatement(shape):
    from dahitra_amd import ops
    N, H, W = small_shapes()[shape]
    vote = B.votes(N, H, W)
    assert (vote == 5).any() and (vote == 255).any()
    dvote = dev(vote)
    pats = B.patterns(N, H, W)
    for name in ("noise59", "noise30", "squares", "ones", "zeros", "rings", "classes59"):
        key = different_images(pats[name])
        keyed = name == "classes59"
        labels, count = B.cc_label(key, 8, keyed)
        K = int(count.max())
        dlabels, _ = ops.xbd_cc_label(dev(key), 8, keyed)
        for cap in sorted({K + 3, max(K // 2, 1)}):                       # room to spare; fewer rows than components
            want = B.cc_stats(labels, vote, cap)
            table = torch.full((N, cap, 10), SENT32, dtype=torch.int32, device=DEV)
            assert ops.xbd_cc_stats(dlabels, dvote, cap, out=table) is table
            assert np.array_equal(table.cpu().numpy(), want), (name, cap)
            assert torch.equal(ops.xbd_cc_stats(dlabels, dvote, cap), table)
            if K:
                assert (want[..., 1:6].sum(-1) <= want[..., 0]).all()
            for mode in ("damage", "all"):
                for min_area in (0, 5):
                    want_cls = B.cc_vote(want, min_area, mode)
                    cls = torch.full((N, cap), SENTINEL, dtype=torch.uint8, device=DEV)
                    assert ops.xbd_cc_vote(table, min_area, mode, out=cls) is cls
                    assert np.array_equal(cls.cpu().numpy(), want_cls), (name, cap, mode, min_area)
                    painted = torch.full((N, H, W), SENTINEL, dtype=torch.uint8, device=DEV)
                    assert ops.xbd_cc_paint(dlabels, cls, out=painted) is painted
                    assert np.array_equal(painted.cpu().numpy(), B.cc_paint(labels, want_cls)), (name, cap, mode, min_area)
                    assert torch.equal(ops.xbd_cc_paint(dlabels, cls), painted)
    # a vote byte of 5 and of 255 lands in the area only: one component, every byte odd
    key = B.ones(1, 37, 41)
    odd = np.full((1, 37, 41), 5, dtype=np.uint8)
    odd[0, ::2] = 255
    table = ops.xbd_cc_stats(ops.xbd_cc_label(dev(key))[0], dev(odd), 2).cpu().numpy()
    assert table.tolist() == [[[37 * 41, 0, 0, 0, 0, 0, 0, 0, 36, 40], [0, 0, 0, 0, 0, 0, 37, 41, -1, -1]]]


def test_the_1024_tile_in_closed_form():
    from dahitra_amd import ops
    N, H, W = 1, 1024, 1024
    vote = dev(B.votes(N, H, W, odd_bytes=False))
    for conn in (4, 8):
        key = dev(B.serpentine(N, H, W))
        labels, count = ops.xbd_cc_label(key, conn)
        assert count.tolist() == [1] and torch.equal(labels, key.to(torch.int32)), "the serpentine is one component"
        key = dev(B.ones(N, H, W))
        labels, count = ops.xbd_cc_label(key, conn)
        assert count.tolist() == [1] and bool((labels == 1).all())
        table = ops.xbd_cc_stats(labels, vote, 1).cpu().numpy()
        assert table[0, 0, 0] == H * W and table[0, 0, 1:6].sum() == H * W and table[0, 0, 6:].tolist() == [0, 0, H - 1, W - 1]
        want, want_k, area_box = B.squares_closed_form(N, H, W)
        labels, count = ops.xbd_cc_label(dev(B.squares(N, H, W)), conn)
        assert count.tolist() == want_k.tolist() and np.array_equal(labels.cpu().numpy(), want)
        table = ops.xbd_cc_stats(labels, vote, int(want_k[0])).cpu().numpy()
        assert np.array_equal(table[0, :, 0], area_box[:, 0]) and np.array_equal(table[0, :, 6:], area_box[:, 1:])
        assert np.array_equal(table[0, :, 1:6].sum(1), area_box[:, 0])


def test_the_same_bits_twice():
    """many roots for the compaction (the 4-connectivity checkerboard: 13000 single pixels) and one root with a long path"""
    from dahitra_amd import ops
    N, H, W = 1, 130, 200
    for key, conn, k in ((B.checkerboard(N, H, W), 4, 13000), (B.serpentine(N, H, W), 4, 1), (B.serpentine(N, H, W), 8, 1)):
        dkey = dev(key)
        a, b = ops.xbd_cc_label(dkey, conn), ops.xbd_cc_label(dkey, conn)
        assert a[1].tolist() == b[1].tolist() == [k]
        assert torch.equal(a[0], b[0]) and np.array_equal(a[0].cpu().numpy(), B.cc_label(key, conn)[0])


def test_an_unaligned_key_gives_the_aligned_result():
    from dahitra_amd import ops
    N, H, W = 1, 33, 131
    key, vote = B.noise(N, H, W, 0.59, classes=4), B.votes(N, H, W)
    views = []
    for a in (key, vote):
        buf = torch.full((a.size + 32,), SENTINEL, dtype=torch.uint8, device=DEV)
        view = buf[1:1 + a.size].view(a.shape)
        view.copy_(torch.from_numpy(a))
        assert view.data_ptr() % 4 == 1
        views.append(view)
    for keyed in (False, True):
        want = ops.xbd_cc_label(dev(key), 8, keyed)
        got = ops.xbd_cc_label(views[0], 8, keyed)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert np.array_equal(got[0].cpu().numpy(), B.cc_label(key, 8, keyed)[0])
        cap = int(want[1].max())
        table = ops.xbd_cc_stats(got[0], views[1], cap)
        assert torch.equal(table, ops.xbd_cc_stats(want[0], dev(vote), cap))
        cls = ops.xbd_cc_vote(table)
        out = torch.full((H * W + 32,), SENTINEL, dtype=torch.uint8, device=DEV)
        ops.xbd_cc_paint(got[0], cls, out=out[1:1 + H * W].view(N, H, W))
        assert torch.equal(out[1:1 + H * W].view(N, H, W), ops.xbd_cc_paint(want[0], cls))
        assert bool((out[:1] == SENTINEL).all()) and bool((out[1 + H * W:] == SENTINEL).all())


def test_refused_arguments_return_failure_and_write_nothing():
    from dahitra_amd import _lib, ops
    L = _lib.lib()
    P, S = ops.P, ops.S
    key = torch.ones(1, 8, 8, dtype=torch.uint8, device=DEV)
    labels = torch.full((1, 8, 8), SENT32, dtype=torch.int32, device=DEV)
    count = torch.full((1,), SENT32, dtype=torch.int32, device=DEV)
    ws = torch.full((ops.xbd_cc_ws_bytes(1, 8, 8),), SENTINEL, dtype=torch.uint8, device=DEV)
    table = torch.full((1, 4, 10), SENT32, dtype=torch.int32, device=DEV)
    cls = torch.full((1, 4), SENTINEL, dtype=torch.uint8, device=DEV)
    out = torch.full((1, 8, 8), SENTINEL, dtype=torch.uint8, device=DEV)

    def refused(fn, prefix, order, good, changes):
        for change in changes:
            args = dict(good, **change)
            assert getattr(L, fn)(*[args[k] for k in order], S()) != 0, (fn, change)
            assert L.dh_last_error().decode().startswith(prefix), (fn, change, L.dh_last_error())

    shape = (dict(N=0), dict(N=-1), dict(H=0), dict(W=0), dict(H=1 << 16, W=1 << 15))
    refused("dh_xbd_cc_label", "xbd_cc_label", ("key", "N", "H", "W", "conn", "keyed", "labels", "count", "ws", "ws_bytes"),
            dict(key=P(key), N=1, H=8, W=8, conn=8, keyed=0, labels=P(labels), count=P(count), ws=P(ws), ws_bytes=ws.numel()),
            shape + (dict(conn=6), dict(conn=0), dict(keyed=2), dict(keyed=-1), dict(key=P(None)), dict(labels=P(None)),
                     dict(count=P(None)), dict(ws=P(None)), dict(ws_bytes=ws.numel() - 1), dict(ws_bytes=0)))
    refused("dh_xbd_cc_stats", "xbd_cc_stats", ("labels", "vote", "N", "H", "W", "cap", "table"),
            dict(labels=P(labels), vote=P(key), N=1, H=8, W=8, cap=4, table=P(table)),
            shape + (dict(cap=0), dict(cap=-3), dict(labels=P(None)), dict(vote=P(None)), dict(table=P(None))))
    refused("dh_xbd_cc_vote", "xbd_cc_vote", ("table", "N", "cap", "min_area", "mode", "cls"),
            dict(table=P(table), N=1, cap=4, min_area=0, mode=0, cls=P(cls)),
            (dict(N=0), dict(cap=0), dict(min_area=-1), dict(mode=2), dict(mode=-1), dict(table=P(None)), dict(cls=P(None))))
    refused("dh_xbd_cc_paint", "xbd_cc_paint", ("labels", "cls", "N", "H", "W", "cap", "out"),
            dict(labels=P(labels), cls=P(cls), N=1, H=8, W=8, cap=4, out=P(out)),
            shape + (dict(cap=0), dict(labels=P(None)), dict(cls=P(None)), dict(out=P(None))))
    # what ops refuses before any launch, on device tensors
    for call in (lambda: ops.xbd_cc_label(key.cpu()), lambda: ops.xbd_cc_label(key, 6), lambda: ops.xbd_cc_label(key.to(torch.int32)),
                 lambda: ops.xbd_cc_label(torch.ones(1, 8, 16, dtype=torch.uint8, device=DEV)[:, :, ::2]),
                 lambda: ops.xbd_cc_label(key, out=(labels, count.cpu())), lambda: ops.xbd_cc_label(key, out=(labels[:, :4], count)),
                 lambda: ops.xbd_cc_label(key, out=(labels.float(), count)), lambda: ops.xbd_cc_label(key, ws=ws[:-4]),
                 lambda: ops.xbd_cc_label(key, ws=ws[1:]),
                 lambda: ops.xbd_cc_stats(labels, key.cpu(), 4), lambda: ops.xbd_cc_stats(labels, key, 4, out=table[:, :3]),
                 lambda: ops.xbd_cc_stats(labels, key[:, :4], 4), lambda: ops.xbd_cc_stats(labels, key, 0),
                 lambda: ops.xbd_cc_vote(table, -1), lambda: ops.xbd_cc_vote(table, mode="most"), lambda: ops.xbd_cc_vote(table, out=cls[:, :2]),
                 lambda: ops.xbd_cc_paint(labels, cls.cpu()), lambda: ops.xbd_cc_paint(labels, cls, out=out[:, :4])):
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    for t, s in ((labels, SENT32), (count, SENT32), (table, SENT32), (ws, SENTINEL), (cls, SENTINEL), (out, SENTINEL)):
        assert bool((t == s).all()), "a refused call writes nothing"
    # the good calls do write
    ops.xbd_cc_label(key, out=(labels, count), ws=ws)
    ops.xbd_cc_stats(labels, key, 4, out=table)
    ops.xbd_cc_vote(table, out=cls)
    ops.xbd_cc_paint(labels, cls, out=out)
    assert bool((labels == 1).all()) and count.tolist() == [1] and cls.tolist() == [[1, 0, 0, 0]] and bool((out == 1).all())
    assert table[0, 0].tolist() == [64, 0, 64, 0, 0, 0, 0, 0, 7, 7]


# ---- model level -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_case():
    """the net and the 64 x 64 pair of test_xbd_visual_gpu.py (fp32 compute, deterministic weights)"""
    from dahitra_amd.models import xbd
    net = xbd.BASE_Transformer_UNet(input_nc=3, output_nc=5, token_len=4, resnet_stages_num=4, with_pos='learned',
                                    with_decoder_pos=None, enc_depth=1, dec_depth=8).cuda()
    net.load_state_dict(O.deterministic_state(NAME))
    net.eval()
    pre, post, gt = V.pictures(1, 64, 64, seed=64)
    return {"net": net, "np": (pre, post, gt), "dev": tuple(dev(a) for a in (pre, post, gt))}


def test_building_damage_is_the_restatement_of_the_models_own_prediction(model_case):
    from dahitra_amd import ops
    from dahitra_amd.models import xbd
    pre, post, gt = model_case["np"]
    dpre, dpost, dgt = model_case["dev"]
    msk = xbd.predict_tta(model_case["net"], dpre, dpost).clone()
    m = msk.cpu().numpy()
    assert m.shape == (1, 64, 64, 5) and len(np.unique(m)) > 8, "a degenerate net cannot pass"
    vote = V.damage_map(m, None)
    cut = gt * B.squares(1, 64, 64, s=7)                 # the labels cut into 7 x 7 squares: many buildings, whatever the labels are
    for kw, footprint in ((dict(loc=ops.XBD_LOC_THR), V.damage_map(m, V.SCRIPT_THR)), (dict(footprint=dgt), gt),
                          (dict(footprint=dev(cut)), cut)):
        for conn, min_area in ((8, 0), (4, 3)):
            labels, count, table, cls, painted = B.building_damage(footprint, vote, conn, min_area, 4096)
            got = xbd.building_damage(msk, connectivity=conn, min_area=min_area, **kw)
            assert isinstance(got, xbd.XbdBuildings)
            assert np.array_equal(got.labels.cpu().numpy(), labels) and got.count.tolist() == count.tolist()
            assert got.table.shape == (1, 4096, 10) and np.array_equal(got.table.cpu().numpy(), table)
            assert np.array_equal(got.cls.cpu().numpy(), cls) and np.array_equal(got.map.cpu().numpy(), painted)
            rows, classes = got.rows(0)
            assert np.array_equal(rows, table[0, :count[0]]) and np.array_equal(classes, cls[0, :count[0]])
            for i in range(1, int(count[0]) + 1):                        # one class per label
                assert len(np.unique(got.map.cpu().numpy()[0][labels[0] == i])) == 1
            assert not got.map.cpu().numpy()[labels == 0].any()
    assert int(B.cc_label(cut != 0, 8)[1][0]) >= 2
    with pytest.raises(ValueError, match="components"):
        xbd.building_damage(msk, footprint=dev(cut), max_buildings=1)
    with pytest.raises(ValueError, match="loc=None"):
        xbd.building_damage(msk, loc=None)
    assert xbd.building_damage(msk, loc=None, footprint=dgt).count.tolist() == B.cc_label(gt != 0, 8)[1].tolist()
    lab, cnt = xbd.buildings(dgt, 4, keyed=True)
    want = B.cc_label(gt, 4, True)
    assert np.array_equal(lab.cpu().numpy(), want[0]) and cnt.tolist() == want[1].tolist()


def test_building_confusion_on_a_synthetic_pair():
    from dahitra_amd.models import xbd
    N, H, W = 2, 65, 130
    gt = B.noise(N, H, W, 0.3, classes=4)
    gt[:, 10:30, 10:50], gt[:, 10:30, 50:90], gt[:, 40:60, 20:70] = 1, 3, 4          # some buildings of a size, two of them touching
    pred = B.noise(N, H, W, 0.8, classes=4)
    pred[:, 10:30, 10:90], pred[:, 40:60, 20:70] = 3, 0                              # one hit, one wrong class, one missed
    for conn in (8, 4):
        want = B.building_confusion(pred, gt, conn)
        got = xbd.building_confusion(dev(pred), dev(gt), conn)
        assert got.dtype == np.int64 and got.shape == (4, 5) and np.array_equal(got, want), conn
        assert want[0, 3] >= 1 and want[2, 3] >= 1 and want[3, 0] >= 1
        parts = [xbd.building_confusion(dev(pred[n:n + 1]), dev(gt[n:n + 1]), conn) for n in range(N)]
        assert np.array_equal(parts[0] + parts[1], got), "confusions add over batches"
    with pytest.raises(KeyError):
        xbd.building_confusion(dev(pred), dev(np.maximum(gt, 5)))
    with pytest.raises(ValueError, match="components"):
        xbd.building_confusion(dev(pred), dev(gt), max_buildings=2)
    f1_sc, f1 = xbd.building_f1(want)
    assert f1_sc.shape == (4,) and np.isfinite(f1)


def test_the_sequence_replays_from_a_captured_graph():
    """label + stats + vote + paint recorded once; a second input written into the same buffers gives its own restatement"""
    from dahitra_amd import ops
    N, H, W = small_shapes()[2]
    cap = 4096
    keys = [B.noise(N, H, W, 0.59), B.rings(N, H, W) + B.squares(N, H, W) * (1 - B.rings(N, H, W))]
    votes = [B.votes(N, H, W), B.votes(N, H, W)[:, ::-1].copy()]
    key, vote = dev(keys[0]), dev(votes[0])
    labels = torch.empty(N, H, W, dtype=torch.int32, device=DEV)
    count = torch.empty(N, dtype=torch.int32, device=DEV)
    ws = torch.empty(ops.xbd_cc_ws_bytes(N, H, W), dtype=torch.uint8, device=DEV)
    table = torch.empty(N, cap, 10, dtype=torch.int32, device=DEV)
    cls = torch.empty(N, cap, dtype=torch.uint8, device=DEV)
    out = torch.empty(N, H, W, dtype=torch.uint8, device=DEV)

    def run():
        ops.xbd_cc_label(key, 8, False, out=(labels, count), ws=ws)
        ops.xbd_cc_stats(labels, vote, cap, out=table)
        ops.xbd_cc_vote(table, 2, "damage", out=cls)
        ops.xbd_cc_paint(labels, cls, out=out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                    # warm-up outside the capture: code objects loaded
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for k, v in ((keys[1], votes[1]), (keys[0], votes[0])):
        key.copy_(torch.from_numpy(k))
        vote.copy_(torch.from_numpy(v))
        for t in (labels, count, table):
            t.fill_(SENT32)
        ws.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        want = B.building_damage(k, v, 8, 2, cap)
        for got, w in zip((labels, count, table, cls, out), want):
            assert np.array_equal(got.cpu().numpy(), w)
