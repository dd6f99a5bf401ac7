"""The host side of the xBD validation score (models/xbd.val_score) and the numpy restatement of the reference's validate()
that the GPU tests compare the kernel with (tests/_xbd_val_cases.py).  No GPU."""
import math

import numpy as np
import pytest
import torch

import _xbd_val_cases as V


def test_val_score_is_the_references_expression_on_the_counts():
    """train.py:281-288 typed out: d0 = mean dice, f1_sc = 2 tp / (2 tp + fp + fn), f1 = 4 / sum(1 / (f1_sc + 1e-6)),
    score = 0.3 d0 + 0.7 f1, all float64"""
    from dahitra_amd.models.xbd import val_score
    image_counts = np.array([[100, 80, 60], [7, 0, 0], [0, 5, 0], [123456789012, 123456789000, 123456788000]], dtype=np.int64)
    class_counts = np.array([[50, 4, 6], [30, 10, 0], [1, 0, 9], [3000000007, 11, 13]], dtype=np.int64)       # tp, fn, fp
    sc, parts = val_score(image_counts, class_counts)
    dices0 = [2. * 60 / (100 + 80), 2. * 0 / 7, 2. * 0 / 5, 2. * 123456788000 / (123456789012 + 123456789000)]
    d0 = np.mean(dices0)
    tp, fn, fp = class_counts[:, 0].astype(np.float64), class_counts[:, 1].astype(np.float64), class_counts[:, 2].astype(np.float64)
    f1_sc = np.zeros((4,))
    for c in range(4):
        f1_sc[c] = 2 * tp[c] / (2 * tp[c] + fp[c] + fn[c])
    f1 = 4 / np.sum(1.0 / (f1_sc + 1e-6))
    assert sc == 0.3 * d0 + 0.7 * f1
    assert parts["dice"] == d0 and parts["f1"] == f1 and np.array_equal(parts["f1_per_class"], f1_sc)
    assert (sc, parts["dice"], parts["f1"]) == V.score(image_counts, class_counts)[:3]
    # torch tensors (what a caller reads back) give the same number
    sc_t, _ = val_score(torch.from_numpy(image_counts), torch.from_numpy(class_counts))
    assert sc_t == sc


def test_val_score_without_a_counted_pixel_is_nan_and_beats_nothing():
    from dahitra_amd.models.xbd import val_score
    sc, parts = val_score(np.array([[10, 10, 5]]), np.zeros((4, 3), dtype=np.int64))
    assert math.isnan(sc) and math.isnan(parts["f1"]) and np.isnan(parts["f1_per_class"]).all()
    assert parts["dice"] == 0.5
    assert not sc > -1.0 and not sc > float("-inf")          # evaluate_val's `d > best_score`
    # one class without a pixel is enough: 0 / 0 is nan in numpy and the harmonic mean carries it
    sc, parts = val_score(np.array([[10, 10, 5]]), np.array([[5, 1, 1], [5, 1, 1], [0, 0, 0], [5, 1, 1]]))
    assert math.isnan(sc) and np.isnan(parts["f1_per_class"]).tolist() == [False, False, True, False]


def test_val_score_empty_truth_and_empty_prediction_is_dice_one():
    from dahitra_amd.models.xbd import val_score
    cc = np.array([[5, 1, 1]] * 4)
    _, parts = val_score(np.array([[0, 0, 0]]), cc)
    assert parts["dice"] == 1.0
    _, parts = val_score(np.array([[0, 0, 0], [4, 4, 2]]), cc)
    assert parts["dice"] == np.mean([1.0, 0.5])
    _, parts = val_score(np.array([[0, 3, 0]]), cc)            # an empty truth alone is not the empty case
    assert parts["dice"] == 0.0


def test_restated_row_selection_is_the_references_boolean_index():
    """train.py:271 and 274 literally, on a random 6 x 6 label image: lbl[j][lbl[j, 0] > 0]"""
    rng = np.random.RandomState(5)
    for trial in range(20):
        lbl = (rng.randint(0, 4, (2, 6, 6)) * (rng.rand(2, 6, 6) < 0.6)).astype(np.int64)
        pred = rng.randint(0, 4, (6, 6))
        for j in range(2):
            sel = V.row_selection(lbl[j])
            assert np.array_equal(lbl[j][sel].reshape(-1, 6), lbl[j][lbl[j, 0] > 0]), trial
            assert np.array_equal(pred[sel].reshape(-1, 6), pred[lbl[j, 0] > 0]), trial
            assert np.array_equal(sel.any(axis=1), lbl[j, 0] > 0)       # row r iff lbl[j, 0, r] > 0 (a COLUMN of the first row)
    # and the counts built on it equal the loop of train.py:269-279 written with the literal index
    x = (np.round(rng.randn(2, 5, 6, 6) * 16) / 8).astype(np.float32)
    msk0 = (rng.rand(2, 6, 6) < 0.5).astype(np.uint8)
    lbl = rng.randint(0, 4, (2, 6, 6)).astype(np.uint8)
    s = V.sigmoid32(x)
    tp, fn, fp = np.zeros((4,)), np.zeros((4,)), np.zeros((4,))
    for j in range(2):
        targ = lbl[j][lbl[j, 0] > 0]
        pred = s[j, 1:].argmax(axis=0)
        pred = pred * (s[j, 0] > 0.3)
        pred = pred[lbl[j, 0] > 0]
        for c in range(4):
            tp[c] += np.logical_and(pred == c, targ == c).sum()
            fn[c] += np.logical_and(pred != c, targ == c).sum()
            fp[c] += np.logical_and(pred == c, targ != c).sum()
    _, cc = V.counts(x, msk0, lbl)
    assert np.array_equal(cc, np.stack([tp, fn, fp], axis=1).astype(np.int64))


def test_non_square_image_raises():
    """lbl[j][lbl[j, 0] > 0] on [H, W] with H != W: numpy raises IndexError; the restatement and the library refuse it too"""
    lbl = np.ones((4, 6), dtype=np.int64)
    with pytest.raises(IndexError):
        lbl[lbl[0] > 0]
    with pytest.raises(IndexError):
        V.row_selection(lbl)
    from dahitra_amd import ops
    logits = torch.zeros(1, 5, 4, 6)
    msk, lab = torch.zeros(1, 5, 4, 6, dtype=torch.uint8), torch.zeros(1, 4, 6, dtype=torch.uint8)
    ic, cc = torch.zeros(1, 3, dtype=torch.int64), torch.zeros(4, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="H == W"):
        ops.xbd_val_count(logits, msk, lab, ic, cc)
    with pytest.raises(ValueError, match="lbl_msk"):
        ops.xbd_val_count(logits, msk, lab[:, :, :4], ic, cc, select="building")
    with pytest.raises(ValueError, match="select"):
        ops.xbd_val_count(logits, msk, lab, ic, cc, select="rows")


def test_synthetic_inputs_meet_their_conditions():
    for B, S in ((3, 37), (2, 40)):
        V.check_synthetic(*V.synthetic(B, S, seed=B * 100 + S))
