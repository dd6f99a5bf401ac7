"""The histograms of dh_xbd_val_sweep / models/xbd.validate_sweep restated in numpy straight from their definition, the
three-threshold rule of xBD_code/visualize_results.py:209 typed out on the sigmoids, and the threshold grid the tests share.

Per pixel of image j, with s = torch.sigmoid(out) in float32 (as tests/_xbd_val_cases.py takes it):
    bin = #{k : s[j, 0] > thr[k]}              float32 comparisons, strict; 0 .. T
    arg = s[j, 1:].argmax(axis=0)              the first maximum of the float32 sigmoids; 0 .. 3
    g0  = msk0[j] != 0
    image_hist[j, bin, arg, g0] += 1           over every pixel
    class_hist[bin, arg, min(lbl, 4)] += 1     over the selected pixels (the reference's rows, or the building pixels)"""
import numpy as np

import _xbd_val_cases as V


def hist(logits, msk0, lbl, thresholds, select="reference", s=None):
    """logits float32 [B, 5, H, W], msk0 [B, H, W], lbl [B, H, W], thresholds [T] ascending.
    Returns image_hist int64 [B, T + 1, 4, 2] and class_hist int64 [T + 1, 4, 5]."""
    s = V.sigmoid32(logits) if s is None else s
    assert s.dtype == np.float32
    thr = np.asarray(thresholds, dtype=np.float32)
    B, T = s.shape[0], thr.size
    image_hist = np.zeros((B, T + 1, 4, 2), dtype=np.int64)
    class_hist = np.zeros((T + 1, 4, 5), dtype=np.int64)
    for j in range(B):
        bins = np.zeros(s[j, 0].shape, dtype=np.int64)
        for k in range(T):
            bins += s[j, 0] > thr[k]
        arg = s[j, 1:].argmax(axis=0)
        g0 = (np.asarray(msk0[j]) != 0).astype(np.int64)
        np.add.at(image_hist[j], (bins, arg, g0), 1)
        sel = V.row_selection(np.asarray(lbl[j])) if select == "reference" else np.asarray(msk0[j]) > 0
        t = np.minimum(np.asarray(lbl[j]).astype(np.int64), 4)
        np.add.at(class_hist, (bins[sel], arg[sel], t[sel]), 1)
    return image_hist, class_hist


def rule_counts(logits, msk0, lbl, t0, t1, t2, select="reference", s=None):
    """visualize_results.py:209 on the float32 sigmoids, msk_dmg = argmax + 1 (line 206):
        msk_loc = (loc_preds > _thr[0]) | ((loc_preds > _thr[1]) & (msk_dmg > 1) & (msk_dmg < 4)) | ((loc_preds > _thr[2]) & (msk_dmg > 1))
    then the dice and tp / fn / fp counting of _xbd_val_cases.counts with that mask as `loc` (handed over as a 0 / 1 plane
    thresholded at 0.5)."""
    s = V.sigmoid32(logits) if s is None else s
    _thr = [np.float32(t0), np.float32(t1), np.float32(t2)]
    loc_preds = s[:, 0]
    msk_dmg = s[:, 1:].argmax(axis=1) + 1
    msk_loc = (loc_preds > _thr[0]) | ((loc_preds > _thr[1]) & (msk_dmg > 1) & (msk_dmg < 4)) | ((loc_preds > _thr[2]) & (msk_dmg > 1))
    s = s.copy()
    s[:, 0] = msk_loc.astype(np.float32)
    return V.counts(logits, msk0, lbl, thr=0.5, select=select, s=s)


def logit_sigmoids():
    """sigmoid32 of every value a free logit of _xbd_val_cases.synthetic takes: the multiples of 1/8 in [-8, 8], ascending"""
    return V.sigmoid32(np.arange(-64, 65, dtype=np.float32) / 8)


def grid():
    """64 thresholds for the synthetic logits: the float32 midpoints of every second adjacent pair of sigmoid32(k / 8) -- the
    first 62 of them -- with float32(0.3) and float32(0.5), sorted.  0.5 IS sigmoid32(0): a logit of 0 sits on a threshold and
    must stay below it (the comparison is strict); every other threshold is far from every sigmoid (check_grid)."""
    sg = logit_sigmoids()
    mid = ((sg[0:-1:2].astype(np.float64) + sg[1::2].astype(np.float64)) / 2).astype(np.float32)[:62]
    return np.sort(np.concatenate([mid, np.asarray([0.3, 0.5], dtype=np.float32)]))


def check_grid(thr):
    """the conditions under which the comparison with the restatement may be exact"""
    sg = logit_sigmoids().astype(np.float64)
    assert thr.dtype == np.float32 and thr.shape == (64,)
    assert V.sigmoid32(np.zeros(1))[0] == np.float32(0.5) and (thr == np.float32(0.5)).sum() == 1
    dist = np.abs(thr.astype(np.float64)[:, None] - sg[None, :])
    dist[thr == np.float32(0.5), 64] = 1.0            # the one exception: 0.5 equals sigmoid32(0) exactly
    assert dist.min() >= 1e-5, dist.min()
    assert np.diff(thr.astype(np.float64)).min() > 0, "neighbouring thresholds differ"
    assert (thr > 0).all() and (thr < 1).all()
