"""The plain-Python restatement of the building step (tests/_xbd_buildings_cases.py) against scipy.ndimage.label and against closed
forms, mutation checks that show those comparisons can fail, building_f1 on a hand-made confusion, and what the interface refuses
without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import _xbd_buildings_cases as B

SHAPES = [(1, 37, 41), (2, 32, 128), (1, 33, 131)]
S4 = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
S8 = np.ones((3, 3), dtype=int)


def scipy_label(key, conn, keyed):
    """scipy's labels of every image; keyed: every value labelled on its own, the components renumbered by first pixel"""
    ndi = pytest.importorskip("scipy.ndimage")
    st = S8 if conn == 8 else S4
    out, counts = [], []
    for img in key:
        if not keyed:
            lab, k = ndi.label(img != 0, structure=st)
        else:
            firsts, parts = [], []
            for v in np.unique(img[img != 0]):
                lv, kv = ndi.label(img == v, structure=st)
                for i in range(1, kv + 1):
                    m = lv == i
                    firsts.append(int(np.flatnonzero(m.ravel())[0]))
                    parts.append(m)
            lab, k = np.zeros(img.shape, dtype=np.int32), len(parts)
            for rank, j in enumerate(np.argsort(firsts)):
                lab[parts[j]] = rank + 1
        out.append(lab.astype(np.int32))
        counts.append(k)
    return np.stack(out), np.array(counts, dtype=np.int32)


@pytest.mark.parametrize("N,H,W", SHAPES)
def test_the_restatement_numbers_components_as_scipy_does(N, H, W):
    for name, key in B.patterns(N, H, W).items():
        for conn in (4, 8):
            for keyed in (False, True):
                want, want_k = scipy_label(key, conn, keyed)
                got, got_k = B.cc_label(key, conn, keyed)
                assert np.array_equal(got, want) and np.array_equal(got_k, want_k), (name, conn, keyed)


def test_closed_forms():
    for N, H, W in SHAPES + [(1, 130, 200)]:
        for conn in (4, 8):
            lab, k = B.cc_label(B.zeros(N, H, W), conn)
            assert not lab.any() and not k.any()
            lab, k = B.cc_label(B.ones(N, H, W), conn)
            assert (lab == 1).all() and (k == 1).all()
            key = B.serpentine(N, H, W)
            lab, k = B.cc_label(key, conn)
            assert np.array_equal(lab, key) and (k == 1).all(), "the serpentine is one component"
            want, want_k, area_box = B.squares_closed_form(N, H, W)
            lab, k = B.cc_label(B.squares(N, H, W), conn)
            assert np.array_equal(lab, want) and np.array_equal(k, want_k)
            table = B.cc_stats(lab, B.votes(N, H, W), int(want_k[0]) + 2)
            assert np.array_equal(table[0, :want_k[0], 0], area_box[:, 0]) and np.array_equal(table[0, :want_k[0], 6:], area_box[:, 1:])
            assert np.array_equal(table[0, want_k[0]:], np.tile([0, 0, 0, 0, 0, 0, H, W, -1, -1], (2, 1))), "rows of labels that do not exist"
            assert (B.cc_label(B.u_shape(N, H, W), conn)[1] == 1).all()
            assert (B.cc_label(B.rings(N, H, W), conn)[1] == 2).all()
        lab, k = B.cc_label(B.checkerboard(N, H, W), 8)
        assert (k == 1).all()
        lab, k = B.cc_label(B.checkerboard(N, H, W), 4)
        assert (k == -(-H * W // 2)).all() and np.array_equal(lab[0][lab[0] > 0], np.arange(1, k[0] + 1))
        blocks = B.touching_blocks(N, H, W)
        assert (B.cc_label(blocks, 8, True)[1] == 4).all() and (B.cc_label(blocks, 4, True)[1] == 4).all()
        assert (B.cc_label(blocks, 8, False)[1] == 2).all() and (B.cc_label(blocks, 4, False)[1] == 2).all()


def test_the_comparisons_catch_wrong_restatements():
    N, H, W = 1, 33, 131
    pats = B.patterns(N, H, W)
    # 4 and 8 swapped: the checkerboard and the noise differ
    for name in ("checkerboard", "noise59"):
        for conn in (4, 8):
            want = scipy_label(pats[name], conn, False)
            got = B.cc_label(pats[name], conn, False, mutate="swap")
            assert not np.array_equal(got[0], want[0]), (name, conn)
    # one union dropped: the pixel where the U's right bar meets its bottom row, and a connector of the serpentine
    for name, at in (("u", (H - 2, (3 * W) // 4)), ("serpentine", (2, W - 1))):
        for conn in (4, 8):
            want = scipy_label(pats[name], conn, False)
            assert np.array_equal(B.cc_label(pats[name], conn)[0], want[0])
            got = B.cc_label(pats[name], conn, mutate=("drop", at))
            assert not np.array_equal(got[0], want[0]) and got[1][0] > want[1][0], (name, conn)
    # numbered in reverse root order: the same partition, other numbers
    for name in ("squares", "noise30"):
        want = scipy_label(pats[name], 8, False)
        got = B.cc_label(pats[name], 8, mutate="reverse")
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0] > 0, want[0] > 0) and not np.array_equal(got[0], want[0]), name
    # and the closed form of the squares catches them too
    want = B.squares_closed_form(N, H, W)[0]
    assert not np.array_equal(B.cc_label(pats["squares"], 8, mutate="reverse")[0], want)


def test_table_votes_and_paint_of_the_restatement():
    ndi = pytest.importorskip("scipy.ndimage")
    N, H, W = 2, 32, 128
    key, vote = B.noise(N, H, W, 0.59), B.votes(N, H, W)
    labels, count = B.cc_label(key, 8)
    cap = int(count.max()) + 3
    table = B.cc_stats(labels, vote, cap)
    for n in range(N):
        k = int(count[n])
        idx = np.arange(1, k + 1)
        assert np.array_equal(table[n, :k, 0], ndi.sum(key[n], labels[n], idx).astype(np.int32))
        for c in range(5):
            assert np.array_equal(table[n, :k, 1 + c], ndi.sum(vote[n] == c, labels[n], idx).astype(np.int32))
        boxes = ndi.find_objects(labels[n])
        assert [tuple(r) for r in table[n, :k, 6:]] == [(b[0].start, b[1].start, b[0].stop - 1, b[1].stop - 1) for b in boxes]
        assert (table[n, :k, 1:6].sum(1) < table[n, :k, 0]).any(), "bytes above 4 count in the area only"
    # votes by hand: ties go to the lowest class; all-zero damage votes give 0; min_area
    t = np.zeros((1, 6, B.COLS), dtype=np.int32)
    t[0, :, :6] = [[9, 3, 2, 2, 1, 1], [4, 4, 0, 0, 0, 0], [7, 0, 1, 3, 3, 0], [0, 0, 0, 0, 0, 0], [6, 1, 0, 0, 0, 5], [3, 1, 1, 0, 0, 0]]
    assert B.cc_vote(t, 0, "damage").tolist() == [[1, 0, 2, 0, 4, 1]]
    assert B.cc_vote(t, 0, "all").tolist() == [[0, 0, 2, 0, 4, 0]]
    assert B.cc_vote(t, 5, "damage").tolist() == [[1, 0, 2, 0, 4, 0]]
    lab = np.array([[[0, 1, 1, 3], [5, 5, 7, 0]]], dtype=np.int32)
    assert B.cc_paint(lab, B.cc_vote(t, 0, "damage")).tolist() == [[[0, 1, 1, 2], [4, 4, 0, 0]]], "a label above cap paints 0"
    # the confusion: additive, KeyError above 4
    gt, pred = B.noise(2, 33, 40, 0.5, classes=4), B.noise(2, 33, 40, 0.8, classes=4)
    whole = B.building_confusion(pred, gt)
    assert whole.sum() == B.cc_label(gt, 8, True)[1].sum()
    assert np.array_equal(whole, B.building_confusion(pred[:1], gt[:1]) + B.building_confusion(pred[1:], gt[1:]))
    with pytest.raises(KeyError):
        B.building_confusion(pred, np.maximum(gt, 5))


def test_building_f1_on_a_hand_made_confusion():
    from dahitra_amd.models import xbd
    conf = np.array([[1, 8, 1, 0, 0],          # class 1: tp 8, fn 2
                     [0, 2, 6, 2, 0],          # class 2: tp 6, fn 4, fp 1 (row 1) + 1 (row 3)
                     [1, 0, 1, 3, 0],          # class 3: tp 3, fn 2, fp 2
                     [0, 0, 0, 0, 4]])         # class 4: tp 4
    f1_sc, f1 = xbd.building_f1(conf)
    want = np.array([2 * 8 / (16 + 2 + 2), 2 * 6 / (12 + 2 + 4), 2 * 3 / (6 + 2 + 2), 1.0])
    assert np.allclose(f1_sc, want, rtol=0, atol=1e-15)
    assert f1 == 4 / np.sum(1.0 / (want + 1e-6))
    # additive: the F1 of a sum of confusions is that of the sum; an absent class is nan, as val_score's
    assert np.array_equal(xbd.building_f1(conf + conf)[0], f1_sc)
    none = xbd.building_f1(np.zeros((4, 5), dtype=np.int64))
    assert np.isnan(none[0]).all() and np.isnan(none[1])


def test_the_binding_and_what_is_refused_without_a_gpu():
    from dahitra_amd import _lib, ops
    from dahitra_amd.models import xbd
    p = _lib.prototypes()
    i, vp, lg = ctypes.c_int, ctypes.c_void_p, ctypes.c_long
    assert p["dh_xbd_cc_label"] == (i, [vp, i, i, i, i, i, vp, vp, vp, lg, vp])
    assert p["dh_xbd_cc_stats"] == (i, [vp, vp, i, i, i, i, vp, vp])
    assert p["dh_xbd_cc_vote"] == (i, [vp, i, i, i, i, vp, vp])
    assert p["dh_xbd_cc_paint"] == (i, [vp, vp, i, i, i, i, vp, vp])
    assert p["dh_xbd_cc_ws_bytes"] == (i, [i, i, i, vp])
    L = _lib.lib()
    assert ops.XBD_CC_TILE == (L.dh_xbd_cc_tile_h(), L.dh_xbd_cc_tile_w())
    assert ops.XBD_CC_TILE[0] * ops.XBD_CC_TILE[1] <= 65536
    assert ops.xbd_cc_ws_bytes(2, 33, 131) == 4 * 2 * (33 * 131 + 5)
    for shape in ((1, 1 << 16, 1 << 15), (0, 8, 8), (1, 0, 8), (70000, 8, 8)):
        with pytest.raises(ValueError, match="xbd_cc_ws_bytes"):
            ops.xbd_cc_ws_bytes(*shape)
    assert ops.XBD_CC_COLS == B.COLS
    key = torch.zeros(1, 8, 8, dtype=torch.uint8)
    lab = torch.zeros(1, 8, 8, dtype=torch.int32)
    for bad in (dict(key_u8=key), dict(key_u8=key, connectivity=6), dict(key_u8=key.float()), dict(key_u8=key[0]), dict(key_u8=key[:0])):
        with pytest.raises(ValueError):
            ops.xbd_cc_label(**bad)
    for call in (lambda: ops.xbd_cc_stats(lab, key, 4), lambda: ops.xbd_cc_stats(lab, key, 0), lambda: ops.xbd_cc_stats(key, key, 4),
                 lambda: ops.xbd_cc_vote(torch.zeros(1, 4, 10, dtype=torch.int32)),
                 lambda: ops.xbd_cc_vote(torch.zeros(1, 4, 10, dtype=torch.int32), mode="most"),
                 lambda: ops.xbd_cc_vote(torch.zeros(1, 4, 10, dtype=torch.int32), min_area=-1),
                 lambda: ops.xbd_cc_vote(torch.zeros(1, 4, 9, dtype=torch.int32)),
                 lambda: ops.xbd_cc_paint(lab, torch.zeros(1, 4, dtype=torch.uint8)),
                 lambda: ops.xbd_cc_paint(lab, torch.zeros(2, 4, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            call()
    msk = torch.zeros(1, 8, 8, 5, dtype=torch.uint8)
    for call in (lambda: xbd.buildings(key), lambda: xbd.building_damage(msk), lambda: xbd.building_damage(msk, footprint=key),
                 lambda: xbd.building_confusion(key, key)):
        with pytest.raises(_lib.HipLibraryError, match="runs on MI355X only"):
            call()
