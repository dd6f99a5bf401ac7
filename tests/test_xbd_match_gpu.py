"""The building match on the MI355X: dh_xbd_cc_match (csrc/xbd_buildings.hip) against the numpy restatement
(tests/_xbd_match_cases.py, itself checked against a dense table of pairs in test_xbd_match_cpu.py), a closed form at 1024 x 1024,
what is refused, the sequence replayed from a captured graph, and models/xbd.building_match.  Everything is integer: every
comparison is exact."""
import numpy as np
import pytest
import torch

import _xbd_buildings_cases as B
import _xbd_match_cases as M
from test_xbd_buildings_gpu import DEV, SENT32, SENTINEL, dev, model_case, small_shapes  # noqa: F401  (model_case: a fixture)

pytestmark = pytest.mark.gpu


def sentinels(N, cap_a, cap_b):
    from dahitra_amd import ops
    return ((torch.full((N, cap_a, 5), SENT32, dtype=torch.int32, device=DEV), torch.full((N, cap_b), SENT32, dtype=torch.int32, device=DEV)),
            torch.full((ops.xbd_cc_match_ws_bytes(N, cap_a, cap_b),), SENTINEL, dtype=torch.uint8, device=DEV))


@pytest.mark.parametrize("shape", range(4))
def test_match_equals_the_restatement(shape):
    from dahitra_amd import ops
    N, H, W = small_shapes()[shape]
    seen = 0
    for name, (A, B_, ka, kb) in M.all_pairs(N, H, W).items():
        dA, dB = dev(A), dev(B_)
        for cap_a, cap_b in M.cap_choices(ka, kb):
            for thr in M.THRESHOLDS:
                want = M.cc_match_fast(A, B_, cap_a, cap_b, *thr)
                out, ws = sentinels(N, cap_a, cap_b)
                got = ops.xbd_cc_match(dA, dB, cap_a, cap_b, thr, out=out, ws=ws)
                assert got[0] is out[0] and got[1] is out[1]
                assert np.array_equal(out[0].cpu().numpy(), want[0]), (name, cap_a, cap_b, thr)
                assert np.array_equal(out[1].cpu().numpy(), want[1]), (name, cap_a, cap_b, thr)
                fresh = ops.xbd_cc_match(dA, dB, cap_a, cap_b, thr)
                assert fresh[0].dtype == fresh[1].dtype == torch.int32
                assert fresh[0].shape == (N, cap_a, 5) and fresh[1].shape == (N, cap_b)
                assert torch.equal(fresh[0], out[0]) and torch.equal(fresh[1], out[1]), (name, cap_a, cap_b, thr)
                seen += int((want[0][..., 4] != 0).sum())
        if name == "stripes":
            assert ops.xbd_cc_match(dA, dB, 2, 3)[0][0].tolist() == [[A[0].astype(bool).sum() - 6, 0, 0, 0, 0],
                                                                     [6, 2, 6, 5 * W, 0]], "the candidate 3 is rejected"
    assert seen > 0
    assert ops.xbd_cc_match(dA, dB, 2, 3, iou=[1, 2])[1].tolist() == [[0, 0, 0]] * N      # the default threshold, as a list


def test_many_labels_and_high_bits():
    """13000 single-pixel buildings: 14 bits, 32 distinct labels in every wave row, every LDS slot contended"""
    from dahitra_amd import ops
    N, H, W = 1, 130, 200
    cap = 16384
    board, _ = B.cc_label(B.checkerboard(N, H, W), 4)
    squares, _ = B.cc_label(B.squares(N, H, W), 8)
    assert board.max() == 13000 and int(board.max()).bit_length() == 14
    for A, B_ in ((board, board), (board, squares), (squares, board)):
        for thr in ((1, 2), (1, 1)):
            want = M.cc_match_fast(A, B_, cap, cap, *thr)
            out, ws = sentinels(N, cap, cap)
            ops.xbd_cc_match(dev(A), dev(B_), cap, cap, thr, out=out, ws=ws)
            assert np.array_equal(out[0].cpu().numpy(), want[0]) and np.array_equal(out[1].cpu().numpy(), want[1])
            again = ops.xbd_cc_match(dev(A), dev(B_), cap, cap, thr)
            assert torch.equal(again[0], out[0]) and torch.equal(again[1], out[1])
    ma, mb = ops.xbd_cc_match(dev(board), dev(board), cap, cap)
    ids = torch.arange(1, 13001, dtype=torch.int32, device=DEV)
    assert torch.equal(ma[0, :13000, 4], ids) and torch.equal(mb[0, :13000], ids) and not bool(mb[0, 13000:].any())
    # the device's own labels of both sides give the same rows
    la, _ = ops.xbd_cc_label(dev(B.checkerboard(N, H, W)), 4)
    assert torch.equal(ops.xbd_cc_match(la, la, cap, cap)[0], ma)


def test_the_1024_tile_in_closed_form():
    from dahitra_amd import ops
    N, H, W = 1, 1024, 1024
    labels, count, area_box = B.squares_closed_form(N, H, W)
    K = int(count[0])
    ncols = -(-W // 6)
    A = dev(labels)
    Bs = dev(M.shifted(labels))                                  # the same numbers one column to the right
    interior = area_box[:, 0] == 25                              # the 171st square of a row or column is cut to 4 pixels
    assert K == ncols * ncols == 171 * 171 and interior.sum() == 170 * 170
    for thr, matched in (((1, 2), True), ((2, 3), False)):
        ma, mb = ops.xbd_cc_match(A, Bs, K, K, thr)
        ma, mb = ma.cpu().numpy()[0], mb.cpu().numpy()[0]
        assert np.array_equal(ma[:, 0], area_box[:, 0])
        ids = np.flatnonzero(interior) + 1
        assert (ma[interior, :4] == np.stack([np.full(len(ids), 25), ids, np.full(len(ids), 20), np.full(len(ids), 25)], 1)).all()
        assert np.array_equal(ma[interior, 4], ids if matched else np.zeros_like(ids))
        assert np.array_equal(mb[interior], ids if matched else np.zeros_like(ids))
        want = M.cc_match_fast(labels, M.shifted(labels), K, K, *thr)
        assert np.array_equal(ma, want[0][0]) and np.array_equal(mb, want[1][0])


def test_refused_arguments_return_failure_and_write_nothing():
    from dahitra_amd import _lib, ops
    L = _lib.lib()
    P, S = ops.P, ops.S
    la = torch.ones(1, 8, 8, dtype=torch.int32, device=DEV)
    lb = torch.ones(1, 8, 8, dtype=torch.int32, device=DEV)
    (ma, mb), ws = sentinels(1, 4, 4)
    odd = torch.zeros(4 * 64 + 8, dtype=torch.uint8, device=DEV)[1:1 + 4 * 64]
    assert odd.data_ptr() % 4 == 1

    def refused(fn, prefix, order, good, changes):
        for change in changes:
            args = dict(good, **change)
            assert getattr(L, fn)(*[args[k] for k in order], S()) != 0, (fn, change)
            assert L.dh_last_error().decode().startswith(prefix), (fn, change, L.dh_last_error())

    vp = ops._vp
    shape = (dict(N=0), dict(N=-1), dict(N=65536), dict(H=0), dict(W=0), dict(H=1 << 16, W=1 << 15))
    caps = (dict(cap_a=0), dict(cap_b=0), dict(cap_a=-3), dict(cap_a=(1 << 24) + 1), dict(cap_b=(1 << 24) + 1),
            dict(N=1 << 10, cap_a=1 << 19), dict(N=1 << 10, cap_b=1 << 19))
    refused("dh_xbd_cc_match", "xbd_cc_match",
            ("la", "lb", "N", "H", "W", "cap_a", "cap_b", "num", "den", "ma", "mb", "ws", "ws_bytes"),
            dict(la=P(la), lb=P(lb), N=1, H=8, W=8, cap_a=4, cap_b=4, num=1, den=2, ma=P(ma), mb=P(mb), ws=P(ws), ws_bytes=ws.numel()),
            shape + caps + (dict(num=0), dict(num=-1), dict(num=3, den=2), dict(num=32768, den=32769), dict(num=1, den=3),
                            dict(num=16383, den=32768), dict(la=P(None)), dict(lb=P(None)), dict(ma=P(None)), dict(mb=P(None)),
                            dict(ws=P(None)), dict(la=vp(odd.data_ptr())), dict(lb=vp(odd.data_ptr())), dict(ma=vp(odd.data_ptr())),
                            dict(mb=vp(odd.data_ptr())), dict(ws=vp(odd.data_ptr())), dict(ws_bytes=ws.numel() - 1), dict(ws_bytes=0)))
    # what ops refuses before any launch, on device tensors
    for call in (lambda: ops.xbd_cc_match(la.cpu(), lb, 4, 4), lambda: ops.xbd_cc_match(la, lb.cpu(), 4, 4),
                 lambda: ops.xbd_cc_match(la.to(torch.int64), lb, 4, 4), lambda: ops.xbd_cc_match(la, lb.to(torch.uint8), 4, 4),
                 lambda: ops.xbd_cc_match(la[0], lb[0], 4, 4), lambda: ops.xbd_cc_match(la, lb[:, :4], 4, 4),
                 lambda: ops.xbd_cc_match(torch.ones(1, 8, 16, dtype=torch.int32, device=DEV)[:, :, ::2], lb, 4, 4),
                 lambda: ops.xbd_cc_match(la, lb, 0, 4), lambda: ops.xbd_cc_match(la, lb, 4, 4.0),
                 lambda: ops.xbd_cc_match(la, lb, 4, 4, iou=0.5), lambda: ops.xbd_cc_match(la, lb, 4, 4, iou=(2.0, 3)),
                 lambda: ops.xbd_cc_match(la, lb, 4, 4, iou=(1, 3)), lambda: ops.xbd_cc_match(la, lb, 4, 4, iou=(0, 1)),
                 lambda: ops.xbd_cc_match(la, lb, 4, 4, iou=(3, 2)), lambda: ops.xbd_cc_match(la, lb, 4, 4, iou=(32768, 32769)),
                 lambda: ops.xbd_cc_match(la, lb, 4, 4, iou=(1, 2, 3)),
                 lambda: ops.xbd_cc_match(la, lb, 4, 4, out=(ma, mb.cpu())), lambda: ops.xbd_cc_match(la, lb, 4, 4, out=(ma[:, :3], mb)),
                 lambda: ops.xbd_cc_match(la, lb, 4, 4, out=(ma, mb.float())), lambda: ops.xbd_cc_match(la, lb, 4, 4, out=ma),
                 lambda: ops.xbd_cc_match(la, lb, 4, 4, ws=ws[:-4]), lambda: ops.xbd_cc_match(la, lb, 4, 4, ws=ws[1:])):
        with pytest.raises(ValueError, match="xbd_cc_match"):
            call()
    torch.cuda.synchronize()
    for t, s in ((ma, SENT32), (mb, SENT32), (ws, SENTINEL)):
        assert bool((t == s).all()), "a refused call writes nothing"
    assert not bool(odd.any())
    # the good call does write: one building on each side, the same pixels
    ops.xbd_cc_match(la, lb, 4, 4, (1, 2), out=(ma, mb), ws=ws)
    assert ma.tolist() == [[[64, 1, 64, 64, 1]] + [[0] * 5] * 3] and mb.tolist() == [[1, 0, 0, 0]]
    ops.xbd_cc_match(la, lb, 4, 4, (1, 1), out=(ma, mb), ws=ws)
    assert ma.tolist() == [[[64, 1, 64, 64, 0]] + [[0] * 5] * 3] and mb.tolist() == [[0, 0, 0, 0]], "strict: nothing lies above 1 / 1"


def test_the_sequence_replays_from_a_captured_graph():
    """label (both sides) + stats + vote + match recorded once; a second input written into the same buffers gives its own
    restatement"""
    from dahitra_amd import ops
    N, H, W = small_shapes()[2]
    cap = 4096
    preds = [B.noise(N, H, W, 0.3, classes=4), (B.squares(N, H, W) * 3).astype(np.uint8)]
    gts = [M.shifted(B.noise(N, H, W, 0.3, classes=4)), M.shifted(B.squares(N, H, W) * B.noise(N, H, W, 0.9, classes=2)).astype(np.uint8)]
    pred, gt = dev(preds[0]), dev(gts[0])
    lab = [torch.empty(N, H, W, dtype=torch.int32, device=DEV) for _ in range(2)]
    cnt = [torch.empty(N, dtype=torch.int32, device=DEV) for _ in range(2)]
    ws = torch.empty(ops.xbd_cc_ws_bytes(N, H, W), dtype=torch.uint8, device=DEV)
    table = torch.empty(N, cap, 10, dtype=torch.int32, device=DEV)
    cls = torch.empty(N, cap, dtype=torch.uint8, device=DEV)
    (ma, mb), mws = sentinels(N, cap, cap)

    def run():
        ops.xbd_cc_label(pred, 8, False, out=(lab[0], cnt[0]), ws=ws)
        ops.xbd_cc_label(gt, 8, True, out=(lab[1], cnt[1]), ws=ws)
        ops.xbd_cc_stats(lab[0], pred, cap, out=table)
        ops.xbd_cc_vote(table, 0, "damage", out=cls)
        ops.xbd_cc_match(lab[0], lab[1], cap, cap, (1, 2), out=(ma, mb), ws=mws)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                    # warm-up outside the capture: code objects loaded
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    matched = []
    for p, g in ((preds[1], gts[1]), (preds[0], gts[0])):
        pred.copy_(torch.from_numpy(p))
        gt.copy_(torch.from_numpy(g))
        for t in lab + cnt + [table, ma, mb]:
            t.fill_(SENT32)
        for t in (ws, mws, cls):
            t.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        want = M.building_match(p, g, 1, 2, 8, cap)
        for got, k in ((lab[0], "pred_labels"), (cnt[0], "pred_count"), (lab[1], "gt_labels"), (cnt[1], "gt_count"),
                       (ma, "match_pred"), (mb, "match_gt"), (cls, "pred_cls")):
            assert np.array_equal(got.cpu().numpy(), want[k]), k
        matched.append(int(want["loc"][0]))
    assert matched[0] > 0 and matched[1] > 0 and matched[0] != matched[1]


# ---- model level -------------------------------------------------------------------------------------------------------
def same_as_restatement(got, want):
    for k in ("pred_labels", "pred_count", "gt_labels", "gt_count", "match_pred", "match_gt", "pred_cls", "gt_cls"):
        t = getattr(got, k)
        assert t.is_cuda and np.array_equal(t.cpu().numpy(), want[k]), k
    for k in ("loc", "confusion", "spurious"):
        v = getattr(got, k)
        assert isinstance(v, np.ndarray) and v.dtype == np.int64 and v.shape == want[k].shape and np.array_equal(v, want[k]), k


def test_building_match_on_a_synthetic_pair():
    from dahitra_amd.models import xbd
    pred, gt = M.synthetic_pair()
    for conn in (8, 4):
        for thr in ((1, 2), (9, 10)):
            want = M.building_match(pred, gt, *thr, conn=conn)
            got = xbd.building_match(dev(pred), dev(gt), thr, conn)
            assert isinstance(got, xbd.XbdMatch)
            assert got.match_pred.shape == (2, 4096, 5) and got.match_gt.shape == (2, 4096) and got.pred_cls.shape == (2, 4096)
            same_as_restatement(got, want)
            assert got.spurious.sum() == got.loc[1] and got.confusion.sum() == got.loc[0] + got.loc[2]
            parts = [xbd.building_match(dev(pred[n:n + 1]), dev(gt[n:n + 1]), thr, conn) for n in range(2)]
            for k in ("loc", "confusion", "spurious"):
                assert np.array_equal(getattr(parts[0], k) + getattr(parts[1], k), getattr(got, k)), "the tables add over batches"
        assert want["loc"][0] < M.building_match(pred, gt, conn=conn)["loc"][0], "the hit at IoU 35 / 40 is lost at 9 / 10"
    got = xbd.building_match(dev(pred), dev(gt))
    assert got.loc.min() >= 2 and got.confusion[2, 1] >= 1 and got.confusion[3, 4] >= 1 and got.spurious[2] >= 2
    loc_f1, f1_sc, f1 = xbd.building_match_f1(got.loc, got.confusion, got.spurious)
    assert 0 < loc_f1 < 1 and f1_sc.shape == (4,) and np.isfinite(f1)
    with pytest.raises(KeyError):
        xbd.building_match(dev(pred), dev(np.maximum(gt, 5)))
    with pytest.raises(ValueError, match="components"):
        xbd.building_match(dev(pred), dev(gt), max_buildings=4)                  # too many on the true side
    few = np.zeros_like(gt)
    few[:, 5:9, 5:9] = 2
    assert xbd.building_match(dev(few), dev(few), max_buildings=4).loc.tolist() == [2, 0, 0]
    with pytest.raises(ValueError, match="components"):
        xbd.building_match(dev(gt), dev(few), max_buildings=4)                   # and on the predicted side
    for bad in (0.5, (1, 3), (1.0, 2)):
        with pytest.raises(ValueError, match="building_match"):
            xbd.building_match(dev(pred), dev(gt), iou=bad)


def test_building_match_is_the_restatement_of_the_models_own_prediction(model_case):
    from dahitra_amd.models import xbd
    pre, post, gt = model_case["np"]
    dpre, dpost, dgt = model_case["dev"]
    msk = xbd.predict_tta(model_case["net"], dpre, dpost).clone()
    cut = (gt * B.squares(1, 64, 64, s=7)).astype(np.uint8)      # the labels cut into 7 x 7 squares: many true buildings
    for kw, truth in ((dict(), gt), (dict(min_area=3), cut), (dict(footprint=dgt), gt), (dict(footprint=dgt, min_area=3), cut)):
        painted = xbd.building_damage(msk, **kw).map
        p = painted.cpu().numpy()
        assert p.any() or "footprint" not in kw, "a prediction without buildings cannot pass"
        for conn in (8, 4):
            same_as_restatement(xbd.building_match(painted, dev(truth), connectivity=conn), M.building_match(p, truth, conn=conn))
