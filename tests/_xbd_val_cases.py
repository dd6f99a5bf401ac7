"""validate() of the reference's xBD loop (xBD_code/train.py:247-290, dice: xBD_code/utils.py:124-154) restated in numpy for
the tests of dh_xbd_val_count / models/xbd.validate, and the synthetic inputs those tests share.

What the reference does per image j of a batch, with s = torch.sigmoid(out) in float32 (train.py:266-279):
    loc   = s[j, 0] > 0.3                      a float32 comparison: the Python float becomes float32(0.3); strict
    dice(msks[j, 0], loc)                      2 |a & b| / (|a| + |b|) in float64, 1.0 when both are empty
    pred  = s[j, 1:].argmax(axis=0) * loc      numpy's argmax: the first maximum wins, on the float32 SIGMOIDS
    targ  = lbl_msk[j][lbl_msk[j, 0] > 0]      lbl_msk[j] is [H, W]: lbl_msk[j, 0] is its first ROW, a boolean index on axis 0
    pred  = pred[lbl_msk[j, 0] > 0]
    tp[c] += (pred == c) & (targ == c); fn[c] += (pred != c) & (targ == c); fp[c] += (pred == c) & (targ != c)
`counts` below returns the integers; `score` finishes as train.py:281-288 does."""
import numpy as np
import torch

THR = 0.3


def sigmoid32(x):
    """torch.sigmoid on float32, the function the reference calls"""
    return torch.sigmoid(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))).numpy()


def row_selection(lbl_j):
    """the [H, W] mask of the pixels train.py:271 / 274 keep: row r, with all its columns, iff lbl_j[0, r] > 0.  Written out
    row by row; test_xbd_val_cpu checks it against the literal expression."""
    H, W = lbl_j.shape
    if H != W:
        raise IndexError("boolean index of length %d on an axis of length %d" % (W, H))
    sel = np.zeros((H, W), dtype=bool)
    for r in range(H):
        if lbl_j[0, r] > 0:
            sel[r, :] = True
    return sel


def counts(logits, msk0, lbl, thr=THR, select="reference", s=None):
    """logits float32 [B, 5, H, W], msk0 [B, H, W] (nonzero = building), lbl [B, H, W] (0 .. 3).
    Returns image_counts int64 [B, 3] = |gt0|, |loc|, |gt0 & loc| and class_counts int64 [4, 3] = tp, fn, fp per class."""
    s = sigmoid32(logits) if s is None else s
    assert s.dtype == np.float32
    B = s.shape[0]
    image_counts = np.zeros((B, 3), dtype=np.int64)
    class_counts = np.zeros((4, 3), dtype=np.int64)
    for j in range(B):
        loc = s[j, 0] > np.float32(thr)
        gt0 = np.asarray(msk0[j]).astype(bool)
        image_counts[j] = gt0.sum(), loc.sum(), np.logical_and(gt0, loc).sum()
        pred = s[j, 1:].argmax(axis=0) * loc
        sel = row_selection(np.asarray(lbl[j])) if select == "reference" else np.asarray(msk0[j]) > 0
        targ, pred = np.asarray(lbl[j])[sel], pred[sel]
        for c in range(4):
            class_counts[c, 0] += np.logical_and(pred == c, targ == c).sum()
            class_counts[c, 1] += np.logical_and(pred != c, targ == c).sum()
            class_counts[c, 2] += np.logical_and(pred == c, targ != c).sum()
    return image_counts, class_counts


def score(image_counts, class_counts):
    """train.py:281-288 and utils.py:147-154, typed out on the counts: (score, d0, f1, f1_sc)"""
    dices0 = []
    for gt0, loc, both in np.asarray(image_counts):
        dices0.append(1.0 if gt0 + loc == 0 else 2. * both / (gt0 + loc))
    d0 = np.mean(dices0)
    tp, fn, fp = (np.asarray(class_counts)[:, k].astype(np.float64) for k in range(3))
    f1_sc = np.zeros((4,))
    with np.errstate(divide="ignore", invalid="ignore"):
        for c in range(4):
            f1_sc[c] = 2 * tp[c] / (2 * tp[c] + fp[c] + fn[c])
        f1 = 4 / np.sum(1.0 / (f1_sc + 1e-6))
    return 0.3 * d0 + 0.7 * f1, d0, f1, f1_sc


# ---- synthetic inputs the CPU restatement cannot read differently from the kernel ------------------------------------
SAT = (30.0, 35.0)        # two damage logits whose float32 sigmoids are both exactly 1.0f


def synthetic(B, S, seed):
    """logits [B, 5, S, S] float32, msk [B, 5, S, S] uint8 (channel 0 = the localisation truth, as the loader lays it out),
    lbl [B, S, S] uint8, and `planted`, what check_synthetic asserts.
    Logits are multiples of 1/8 inside [-8, 8]: the neighbours of logit(0.3) = -0.8473 are -0.875 and -0.75 (sigmoids 0.2942 and
    0.3208), distinct values differ by >= 4e-5 after the sigmoid (the closest pair is 7.875 / 8), equal values tie on both sides.
    A block of every image holds 30 / 35 in damage channels 2 / 3 (both sigmoids are 1.0f: the first must win) under a set
    localisation.  Image 0's first row has positive and zero labels; with B > 1 the last image has an all-zero first row, an
    empty mask and an empty prediction."""
    rng = np.random.RandomState(seed)
    x = np.clip(np.round(rng.randn(B, 5, S, S) * 3.0 * 8.0) / 8.0, -8.0, 8.0).astype(np.float32)
    msk = (rng.rand(B, 5, S, S) < 0.4).astype(np.uint8)
    lbl = rng.randint(0, 4, (B, S, S)).astype(np.uint8)
    h = max(S // 4, 2)
    x[:, 0, h:2 * h, h:2 * h] = 8.0
    x[:, 1, h:2 * h, h:2 * h] = -8.0
    x[:, 2, h:2 * h, h:2 * h] = SAT[0]
    x[:, 3, h:2 * h, h:2 * h] = SAT[1]
    x[:, 4, h:2 * h, h:2 * h] = 8.0
    lbl[0, 0, ::2] = 0
    lbl[0, 0, 1::2] = 1 + (np.arange(S)[1::2] % 3)
    lbl[0, h:2 * h, h:2 * h] = np.arange(h * h).reshape(h, h) % 4
    if B > 1:
        lbl[B - 1, 0, :] = 0
        msk[B - 1, 0] = 0
        x[B - 1, 0] = -8.0
    planted = {"block": (slice(h, 2 * h), slice(h, 2 * h)), "empty_image": B - 1 if B > 1 else None}
    return x, msk, lbl, planted


def check_synthetic(x, msk, lbl, planted):
    """the conditions under which the comparison may be exact"""
    B, _, S, _ = x.shape
    blk = planted["block"]
    free = np.ones(x.shape, dtype=bool)
    free[:, 2, blk[0], blk[1]] = free[:, 3, blk[0], blk[1]] = False
    v = x[free].astype(np.float64)
    assert np.all(v * 8 == np.round(v * 8)) and np.all(np.abs(v) <= 8), "logits are multiples of 1/8 inside [-8, 8]"
    assert not np.any((x[:, 0] > -0.875) & (x[:, 0] < -0.75)), "no localisation logit between the threshold's neighbours"
    s = sigmoid32(np.unique(x))
    assert s[np.unique(x) <= -0.875].max() < np.float32(THR) - 5e-3 and s[np.unique(x) >= -0.75].min() > np.float32(THR) + 5e-3
    grid = sigmoid32(np.arange(-64, 65, dtype=np.float32) / 8)
    assert np.diff(grid.astype(np.float64)).min() >= 4e-5, "distinct values stay distinct by >= 4e-5 after the sigmoid"
    sat = sigmoid32(np.asarray(SAT, dtype=np.float32))
    assert sat[0] == np.float32(1.0) and sat[1] == np.float32(1.0), "both planted damage logits saturate to 1.0f"
    assert np.all(x[:, 2, blk[0], blk[1]] == SAT[0]) and np.all(x[:, 3, blk[0], blk[1]] == SAT[1])
    # an argmax over the LOGITS picks channel 3 (damage index 2) there, the sigmoids' first maximum is damage index 1
    assert np.all(x[:, 1:, blk[0], blk[1]].argmax(axis=1) == 2)
    assert np.all(sigmoid32(x)[:, 1:, blk[0], blk[1]].argmax(axis=1) == 1)
    assert (lbl[0, 0] > 0).any() and (lbl[0, 0] == 0).any(), "image 0: a first row with and without positive labels"
    assert lbl.max() <= 3
    e = planted["empty_image"]
    if B > 1:
        assert not (lbl[e, 0] > 0).any(), "an image whose first row selects nothing"
        assert not msk[e, 0].any() and not (sigmoid32(x[e, 0]) > np.float32(THR)).any(), "an empty mask and an empty prediction"
