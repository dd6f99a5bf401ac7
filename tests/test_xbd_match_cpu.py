"""The numpy restatement of the building match (tests/_xbd_match_cases.py) against an independent dense contingency table, the
majority-bit argument on every pattern pair, mutation checks that show those comparisons can fail, the counts of the named cases
pinned so that no test passes on empty ground, building_match_f1 on a hand-made example, and what the interface refuses without
a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import _xbd_match_cases as M

SHAPES = [(1, 37, 41), (2, 32, 128), (1, 33, 131)]


def dense_match(A, B_, cap_a, cap_b, num, den):
    """the definition over a dense [cap_a + 1, cap_b + 1] table of pairs, filled with np.add.at"""
    N = A.shape[0]
    match_a = np.zeros((N, cap_a, M.COLS), dtype=np.int32)
    match_b = np.zeros((N, cap_b), dtype=np.int32)
    for n in range(N):
        a = np.where((A[n] < 1) | (A[n] > cap_a), 0, A[n]).ravel()
        b = np.where((B_[n] < 1) | (B_[n] > cap_b), 0, B_[n]).ravel()
        table = np.zeros((cap_a + 1, cap_b + 1), dtype=np.int64)
        np.add.at(table, (a, b), 1)
        area_a, area_b = table.sum(1), table.sum(0)
        for i in range(1, cap_a + 1):
            over = np.flatnonzero(2 * table[i, 1:] > area_a[i]) + 1
            assert len(over) <= 1
            if area_a[i] == 0 or len(over) == 0:
                match_a[n, i - 1, 0] = area_a[i]
                continue
            j = int(over[0])
            inter = int(table[i, j])
            hit = inter * den > num * (int(area_a[i]) + int(area_b[j]) - inter)
            match_a[n, i - 1] = (area_a[i], j, inter, area_b[j], j if hit else 0)
            if hit:
                assert match_b[n, j - 1] == 0, "one-to-one"
                match_b[n, j - 1] = i
    return match_a, match_b


@pytest.mark.parametrize("N,H,W", SHAPES)
def test_the_restatement_equals_a_dense_table_of_pairs(N, H, W):
    for name, (A, B_, ka, kb) in M.all_pairs(N, H, W).items():
        for caps in M.cap_choices(ka, kb):
            for thr in M.THRESHOLDS:
                want = dense_match(A, B_, *caps, *thr)
                for fn in (M.cc_match, M.cc_match_fast):
                    got = fn(A, B_, *caps, *thr)
                    assert got[0].dtype == got[1].dtype == np.int32
                    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, caps, thr, fn.__name__)
                # both directions of the match agree, and no true building has two partners
                ma, mb = want
                for n in range(N):
                    hit = np.flatnonzero(ma[n, :, 4])
                    assert len(np.unique(ma[n, hit, 4])) == len(hit)
                    assert np.array_equal(mb[n, ma[n, hit, 4] - 1], hit + 1) and (mb[n] != 0).sum() == len(hit)


@pytest.mark.parametrize("N,H,W", SHAPES + [(1, 130, 200)])
def test_the_majority_bits_name_the_majority_label(N, H, W):
    for name, (A, B_, ka, kb) in M.all_pairs(N, H, W).items():
        for caps in M.cap_choices(ka, kb):
            maj = M.cc_match_fast(A, B_, *caps)[0][..., 1]
            cand = M.bit_candidates(A, B_, *caps)
            assert np.array_equal(cand[maj != 0], maj[maj != 0]), (name, caps)


def counts(A, B_, ka, kb, thr):
    """(rows with a maj, matched rows, rows whose candidate is a label of B that exists but is not their maj)"""
    ma, mb = M.cc_match_fast(A, B_, ka + 3, kb + 3, *thr)
    cand = M.bit_candidates(A, B_, ka + 3, kb + 3)
    rejected = 0
    for n in range(A.shape[0]):
        exists = np.bincount(M._clamped(B_[n], kb + 3), minlength=kb + 4) > 0
        exists[0] = False
        ok = (cand[n] >= 1) & (cand[n] <= kb + 3)
        rejected += int((ok & exists[np.where(ok, cand[n], 0)] & (ma[n, :, 1] == 0) & (ma[n, :, 0] > 0)).sum())
    assert (mb != 0).sum() == (ma[..., 4] != 0).sum()
    return int((ma[..., 1] != 0).sum()), int((ma[..., 4] != 0).sum()), rejected


def test_the_named_cases_are_not_empty_ground():
    sq = ("squares", "squares>")
    # interior 5 x 5 squares meet their shifted copies at 20 of 30 pixels: IoU exactly 2 / 3
    assert counts(*M.pair_labels(1, 130, 200, *sq), (1, 2)) == (726, 726, 0)
    assert counts(*M.pair_labels(1, 130, 200, *sq), (2, 3)) == (726, 0, 0)
    assert counts(*M.pair_labels(1, 130, 200, *sq), (13, 20)) == (726, 726, 0)
    assert counts(*M.pair_labels(1, 37, 41, *sq), (2, 3)) == (49, 7, 0), "7 of the 49 edge-cut squares lie above 2 / 3"
    assert counts(*M.pair_labels(1, 37, 41, *sq), (1, 1)) == (49, 0, 0)
    assert counts(*M.pair_labels(1, 37, 41, "squares", "squares"), (13, 20)) == (49, 49, 0), "every square matches itself at IoU 1"
    assert counts(*M.pair_labels(1, 37, 41, "squares", "squares"), (1, 1)) == (49, 0, 0), "the comparison is strict: nothing is above 1"
    # noise against keyed classes: majorities that fail the IoU, matches, and candidates the verify pass has to reject
    nc = ("noise59", "classes59")
    assert counts(*M.pair_labels(2, 32, 128, *nc), (1, 2)) == (6, 3, 4)
    assert counts(*M.pair_labels(1, 33, 131, *nc), (1, 2)) == (2, 2, 2)
    assert counts(*M.pair_labels(1, 130, 200, *nc), (1, 2)) == (18, 5, 4)
    # one true blob under many predicted squares: a majority everywhere, a match nowhere
    assert counts(*M.pair_labels(1, 130, 200, "squares", "noise70"), (1, 2)) == (735, 0, 1)
    assert counts(*M.pair_labels(2, 32, 128, "squares", "noise70"), (1, 2)) == (257, 0, 0)
    assert counts(*M.pair_labels(1, 37, 41, "zeros", "squares"), (1, 2)) == (0, 0, 0)
    # the stripes: the bits name label 3, which covers 40 %
    A, B_ = M.stripes(1, 37, 41)
    assert M.bit_candidates(A, B_, 2, 3).tolist() == [[3, 2]]
    assert M.cc_match(A, B_, 2, 3)[0].tolist() == [[[740, 0, 0, 0, 0], [6, 2, 6, 205, 0]]]
    assert counts(A, B_, 2, 3, (1, 2)) == (1, 0, 1)


def test_the_comparisons_catch_wrong_restatements():
    differs = {m: set() for m in M.MUTANTS}
    for shape in ((1, 37, 41), (1, 33, 131)):
        for name, (A, B_, ka, kb) in M.all_pairs(*shape).items():
            for thr in M.THRESHOLDS:
                want = M.cc_match(A, B_, ka + 3, kb + 3, *thr)
                for m in M.MUTANTS:
                    got = M.cc_match(A, B_, ka + 3, kb + 3, *thr, mutate=m)
                    if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])):
                        differs[m].add((shape, name, thr))
    assert ((1, 37, 41), "squares|squares>", (2, 3)) in differs["ge"], ">= matches the squares that sit exactly at 2 / 3"
    assert ((1, 37, 41), "squares|squares", (1, 1)) in differs["ge"]
    assert ((1, 37, 41), "squares|noise70", (1, 2)) in differs["ratio"], "a square inside the blob is covered, not matched"
    assert ((1, 37, 41), "stripes", (1, 2)) in differs["ratio"]
    assert ((1, 37, 41), "stripes", (1, 2)) in differs["noverify"], "the candidate 3 covers 40 % of the rectangle"
    assert ((1, 33, 131), "noise59|classes59", (1, 2)) in differs["noverify"]
    assert ((1, 37, 41), "squares|squares>", (1, 2)) in differs["no_match_b"]
    # and at the model level, on the synthetic pair
    pred, gt = M.synthetic_pair()
    want = M.building_match(pred, gt, conn=4)
    assert want["loc"][0] >= 2 and want["loc"][1] >= 2 and want["loc"][2] >= 2 and want["confusion"][2, 1] >= 1
    for m in ("ge", "ratio", "no_match_b"):
        got = M.building_match(pred, gt, conn=4, mutate=m)
        assert not all(np.array_equal(got[k], want[k]) for k in ("loc", "confusion", "spurious")), m


def test_the_restated_building_match_adds_up():
    pred, gt = M.synthetic_pair()
    for conn in (8, 4):
        r = M.building_match(pred, gt, conn=conn)
        assert r["spurious"].sum() == r["loc"][1] and r["confusion"].sum() == r["loc"][0] + r["loc"][2]
        assert r["loc"][0] + r["loc"][1] == r["pred_count"].sum() and r["loc"][0] + r["loc"][2] == r["gt_count"].sum()
        parts = [M.building_match(pred[n:n + 1], gt[n:n + 1], conn=conn) for n in range(2)]
        for k in ("loc", "confusion", "spurious"):
            assert np.array_equal(parts[0][k] + parts[1][k], r[k]), (conn, k)
    # the block on empty ground and the block over two true buildings are spurious, the two buildings under it are missed
    r = M.building_match(pred[:1], gt[:1])
    la, lb = r["pred_labels"][0], r["gt_labels"][0]
    assert r["match_pred"][0, la[36, 100] - 1].tolist() == [8 * 14, 0, 0, 0, 0]
    assert r["match_pred"][0, la[50, 100] - 1].tolist() == [10 * 22, 0, 0, 0, 0]
    assert r["match_gt"][0, lb[50, 100] - 1] == 0 and r["match_gt"][0, lb[50, 110] - 1] == 0
    assert r["match_pred"][0, la[60, 100] - 1].tolist() == [40, lb[60, 100], 35, 35, lb[60, 100]]
    with pytest.raises(KeyError):
        M.building_match(pred, np.maximum(gt, 5))
    with pytest.raises(ValueError):
        M.building_match(pred, gt, cap=2)


def test_building_match_f1_on_three_buildings():
    from dahitra_amd.models import xbd
    # three true buildings: class 1 matched as 1, class 1 matched as 2, class 3 unmatched; one spurious predicted building of class 2
    loc = np.array([2, 1, 1])
    conf = np.zeros((4, 5), dtype=np.int64)
    conf[0, 1], conf[0, 2], conf[2, 0] = 1, 1, 1
    spur = np.array([0, 0, 1, 0, 0])
    loc_f1, f1_sc, f1 = xbd.building_match_f1(loc, conf, spur)
    assert loc_f1 == 2 * 2 / (2 * 2 + 1 + 1)
    # class 1: tp 1, fn 1, fp 0; class 2: tp 0, fn 0, fp 1 + 1; class 3: tp 0, fn 1, fp 0; class 4: nothing at all
    assert f1_sc[:3].tolist() == [2 / 3, 0.0, 0.0] and np.isnan(f1_sc[3]) and np.isnan(f1)
    # without the spurious building class 2 keeps its false positive from the confusion's column
    assert xbd.building_match_f1(loc, conf, np.zeros(5))[1][1] == 0.0
    # all four classes present: the harmonic mean of val_score, 1e-6 included
    conf = np.diag([3, 2, 4, 1])
    conf = np.concatenate([np.zeros((4, 1), dtype=np.int64), conf], axis=1)
    conf[1, 0], conf[3, 3] = 1, 1
    spur = np.array([1, 2, 0, 0, 1])
    loc_f1, f1_sc, f1 = xbd.building_match_f1([11, 4, 1], conf, spur)
    want = np.array([2 * 3 / (6 + 2 + 0), 2 * 2 / (4 + 0 + 1), 2 * 4 / (8 + 1 + 0), 2 * 1 / (2 + 1 + 1)])
    assert loc_f1 == 22 / 27 and np.allclose(f1_sc, want, rtol=0, atol=1e-15) and f1 == 4 / np.sum(1.0 / (want + 1e-6))
    # with no spurious buildings and every true building matched, the class scores are building_f1's
    assert np.array_equal(xbd.building_match_f1([11, 0, 0], conf, np.zeros(5))[1], xbd.building_f1(conf)[0])
    none = xbd.building_match_f1(np.zeros(3), np.zeros((4, 5)), np.zeros(5))
    assert np.isnan(none[0]) and np.isnan(none[1]).all() and np.isnan(none[2])


def test_the_binding_and_what_is_refused_without_a_gpu():
    from dahitra_amd import _lib, ops
    from dahitra_amd.models import xbd
    p = _lib.prototypes()
    i, vp, lg = ctypes.c_int, ctypes.c_void_p, ctypes.c_long
    assert p["dh_xbd_cc_match_ws_bytes"] == (i, [i, i, i, vp])
    assert p["dh_xbd_cc_match"] == (i, [vp, vp, i, i, i, i, i, i, i, vp, vp, vp, lg, vp])
    assert ops.XBD_CC_MATCH_COLS == M.COLS == 5
    # rows [cap_a][NB + 1], candidates and intersections [cap_a], the areas of B [cap_b]; NB = bit_length(cap_b)
    assert ops.xbd_cc_match_ws_bytes(2, 100, 4096) == 4 * 2 * (100 * (13 + 3) + 4096)
    assert ops.xbd_cc_match_ws_bytes(1, 7, 1) == 4 * (7 * 4 + 1)
    assert ops.xbd_cc_match_ws_bytes(1, 1, 1 << 24) == 4 * (28 + (1 << 24))
    for bad in ((0, 4, 4), (70000, 4, 4), (1, 0, 4), (1, 4, 0), (1, (1 << 24) + 1, 4), (1, 4, (1 << 24) + 1), (1 << 10, 1 << 19, 4)):
        with pytest.raises(ValueError, match="xbd_cc_match"):
            ops.xbd_cc_match_ws_bytes(*bad)
    lab = torch.zeros(1, 8, 8, dtype=torch.int32)
    for call in (lambda: ops.xbd_cc_match(lab, lab, 4, 4),                       # not on the device
                 lambda: ops.xbd_cc_match(lab, lab, 0, 4), lambda: ops.xbd_cc_match(lab, lab, 4, True),
                 lambda: ops.xbd_cc_match(lab.to(torch.int64), lab, 4, 4), lambda: ops.xbd_cc_match(lab, lab[:, :4], 4, 4),
                 lambda: ops.xbd_cc_match(lab[0], lab[0], 4, 4), lambda: ops.xbd_cc_match(lab, lab, 4, 4, iou=0.5),
                 lambda: ops.xbd_cc_match(lab, lab, 4, 4, iou=(1.0, 2)), lambda: ops.xbd_cc_match(lab, lab, 4, 4, iou=(1, 3)),
                 lambda: ops.xbd_cc_match(lab, lab, 4, 4, iou=(0, 1)), lambda: ops.xbd_cc_match(lab, lab, 4, 4, iou=(3, 2)),
                 lambda: ops.xbd_cc_match(lab, lab, 4, 4, iou=(32768, 32769)), lambda: ops.xbd_cc_match(lab, lab, 4, 4, iou=(1, 2, 3)),
                 lambda: ops.xbd_cc_match(lab, lab, 4, 4, iou=(True, 1))):
        with pytest.raises(ValueError, match="xbd_cc_match"):
            call()
    key = torch.zeros(1, 8, 8, dtype=torch.uint8)
    with pytest.raises(_lib.HipLibraryError, match="runs on MI355X only"):
        xbd.building_match(key, key)
