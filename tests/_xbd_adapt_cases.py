"""xBD_code/train_adapt.py restated on the host for tests/test_xbd_adapt_cpu.py and tests/test_xbd_adapt_gpu.py: its loss (lines
332-342) in float64 numpy with the gradient written out, the masks of its two datasets (lines 147-175, 216-236) as the literal
numpy of the script and as the closed form the kernel computes, its file set (lines 369-391), its loader's bytes and its
validation counts (lines 262-280).  Written from the script and from the formulas of include/dahitra_hip.h, not from the kernels.

The loss, with s_c = sigmoid(x_c), t_c the mask byte, N the number of pixels:
    I, S, T = sum s_c t_c, sum s_c, sum t_c;  dice_c = 1 - (2 I + eps) / (S + T + eps)
    o = clamp(s_c, eps, 1 - eps), tt = clamp(t_c, eps, 1 - eps), pt = (1 - tt)(1 - o) + tt o;  focal_c = mean(-(1 - pt)^2 log pt)
    l_c = dice_c + 8 focal_c
    y = the first maximum of (1 - t_0, t_1, t_2, t_3);  nll = logsumexp(x) - x_y;  ce = sum(w_y nll) / sum(w_y)
    loss = 0.1 l_0 + 0.8 l_1 + 2 l_2 + 8 l_3 + 5 ce
As in tests/_xbd_unet_loss_cases.py, FocalLoss2d converts the targets with `.float()` BEFORE it clamps them (losses.py:284-288):
`tt` is the float32 neighbour of 1e-6 or of 1 - 1e-6 and `1 - tt` a float32 difference, whatever the precision of the logits."""
import numpy as np
import torch

EPS = 1e-6
CHANNEL_WEIGHTS = (0.1, 0.8, 2.0, 8.0)
CE_WEIGHTS = (0.1, 0.5, 1.5, 1.5)
CE_SCALE = 5.0
CASES = ("train", "val")

# (B, H, W, saturated) of the GPU tests; the GPU test appends the two shapes past one grid pass and the unaligned one
SHAPES = ((2, 15, 17, True),         # the fixture's shape, H * W odd: the one-pixel form, with saturated logits
          (1, 8, 12, False))         # the 4-pixel form, less than one workgroup


# ---- the loss ---------------------------------------------------------------------------------------------------------------
def label(msk):
    """lines 338-339 on integers: msks[:, 0] = 1 - msks[:, 0]; argmax(msks, dim=1) -- the first maximum"""
    m = np.asarray(msk).astype(np.int64).copy()
    m[:, 0] = 1 - m[:, 0]
    return m.argmax(axis=1)


def restate(logits, msk, upstream=1.0):
    """float64 numpy: {'loss', 'parts' [6] = l_0 .. l_3, ce, 0, 'grad' = d(upstream * loss) / dlogits, 'label'}"""
    x = np.asarray(logits, dtype=np.float64)
    t = np.asarray(msk).astype(np.float64)
    B, C, H, W = x.shape
    assert C == 4 and t.shape == x.shape
    N = B * H * W
    tt32 = np.clip(np.asarray(msk).astype(np.float32), np.float32(EPS), np.float32(1.0 - EPS))      # the reference's float32 clamp
    tt, omtt = tt32.astype(np.float64), (np.float32(1) - tt32).astype(np.float64)                   # ... and its float32 1 - tt
    s = 1.0 / (1.0 + np.exp(-x))
    channel, grad = [], np.zeros_like(x)
    for c in range(4):
        I, S, T = (s[:, c] * t[:, c]).sum(), s[:, c].sum(), t[:, c].sum()
        U = S + T + EPS
        dice = 1 - (2 * I + EPS) / U
        o = np.clip(s[:, c], EPS, 1.0 - EPS)
        pt = omtt[:, c] * (1 - o) + tt[:, c] * o
        focal = (-(1.0 - pt) ** 2 * np.log(pt)).mean()
        channel.append(dice + 8.0 * focal)
        ddice = -(2 * t[:, c] * U - (2 * I + EPS)) / (U * U)
        inside = (s[:, c] >= EPS) & (s[:, c] <= 1.0 - EPS)                  # clamp's gradient
        dfocal = (2 * (1 - pt) * np.log(pt) - (1 - pt) ** 2 / pt) * (tt[:, c] - omtt[:, c]) * inside / N
        grad[:, c] = CHANNEL_WEIGHTS[c] * (ddice + 8.0 * dfocal) * s[:, c] * (1 - s[:, c])
    y = label(msk)
    mx = x.max(axis=1, keepdims=True)
    e = np.exp(x - mx)
    se = e.sum(axis=1, keepdims=True)
    logp = x - mx - np.log(se)
    onehot = (np.arange(4)[None, :, None, None] == y[:, None]).astype(np.float64)
    nll = -(logp * onehot).sum(axis=1)
    w = np.asarray(CE_WEIGHTS, dtype=np.float64)[y]
    ce = (w * nll).sum() / w.sum()
    grad += CE_SCALE * (w / w.sum())[:, None] * (e / se - onehot)
    loss = sum(cw * l for cw, l in zip(CHANNEL_WEIGHTS, channel)) + CE_SCALE * ce
    return {"loss": float(loss), "parts": np.array(channel + [ce, 0.0], dtype=np.float64), "grad": grad * upstream, "label": y}


def fixture_reference(golden, name):
    """the reference's float64 results of a fixture case in restate's layout"""
    return {"loss": float(golden[name + "_loss64"]), "grad": golden[name + "_grad64"],
            "parts": np.concatenate([golden[name + "_channel64"], [golden[name + "_ce64"]], [0.0]])}


def yardstick(golden):
    """The reference's own float32 error on the fixture, the measure of the GPU tests: the distance of its float32 CPU results
    from its float64 ones, the largest over the fixture's cases per quantity -- 'loss', 'channel', 'ce' relative, 'grad' as the
    largest error over the largest gradient."""
    out = {k: 0.0 for k in ("loss", "channel", "ce", "grad")}
    for name in CASES:
        for k in ("loss", "channel", "ce"):
            a, b = golden["%s_%s32" % (name, k)].astype(np.float64), golden["%s_%s64" % (name, k)]
            out[k] = max(out[k], float(np.max(np.abs(a - b) / np.abs(b))))
        a, b = golden[name + "_grad32"].astype(np.float64), golden[name + "_grad64"]
        out["grad"] = max(out["grad"], float(np.abs(a - b).max() / np.abs(b).max()))
    return out


def make_case(golden, B, H, W, saturated, seed):
    """(logits fp32, msk uint8) of a test shape: every pixel -- its four logits and its four mask bytes -- is a pixel of the
    fixture, drawn with replacement from its two cases, for the reason tests/_xbd_unet_loss_cases.make_case gives (the yardstick
    is the reference's float32 error on those pixels; fresh inputs hold more or fewer of the few pixels that carry it).
    saturated: with the fixture's +25 / -25 pixels, at least one of each; without them otherwise."""
    x = np.concatenate([golden[n + "_logits"].transpose(0, 2, 3, 1).reshape(-1, 4) for n in CASES])
    m = np.concatenate([golden[n + "_msk"].transpose(0, 2, 3, 1).reshape(-1, 4) for n in CASES])
    if not saturated:
        keep = (np.abs(x) != 25.0).all(1)
        x, m = x[keep], m[keep]
    idx = np.random.RandomState(seed).randint(0, len(x), size=B * H * W)
    if saturated:
        idx[:2] = np.nonzero((x == 25.0).any(1))[0][0], np.nonzero((x == -25.0).any(1))[0][0]
    logits = np.ascontiguousarray(x[idx].reshape(B, H, W, 4).transpose(0, 3, 1, 2))
    msk = np.ascontiguousarray(m[idx].reshape(B, H, W, 4).transpose(0, 3, 1, 2))
    return torch.from_numpy(logits), torch.from_numpy(msk)


# ---- the masks ----------------------------------------------------------------------------------------------------------------
def train_masks_literal(msk0, lbl_msk1):
    """train_adapt.py:147-175, typed out: (msk [H, W, 4] of 0 / 1, lbl_msk [H, W])"""
    msk1 = np.zeros_like(lbl_msk1)
    msk2 = np.zeros_like(lbl_msk1)
    msk3 = np.zeros_like(lbl_msk1)
    msk2[lbl_msk1 == 2] = 255
    msk3[lbl_msk1 == 3] = 255
    msk3[lbl_msk1 == 4] = 255
    msk1[lbl_msk1 == 1] = 255

    msk0 = msk0[..., np.newaxis]
    msk1 = msk1[..., np.newaxis]
    msk2 = msk2[..., np.newaxis]
    msk3 = msk3[..., np.newaxis]

    msk = np.concatenate([msk0, msk1, msk2, msk3], axis=2)
    msk = (msk > 127)

    msk[..., 0] = False
    msk[..., 1][msk[..., 2:].max(axis=2)] = False
    msk[..., 3][msk[..., 2]] = False
    msk[..., 0][msk[..., 1:].max(axis=2)] = True
    msk = msk * 1

    lbl_msk = msk[..., 1:].argmax(axis=2)
    return msk, lbl_msk


def val_masks_literal(msk0, lbl_msk1):
    """train_adapt.py:216-236, typed out"""
    msk1 = np.zeros_like(lbl_msk1)
    msk2 = np.zeros_like(lbl_msk1)
    msk3 = np.zeros_like(lbl_msk1)
    msk1[lbl_msk1 == 1] = 255
    msk2[lbl_msk1 == 2] = 255
    msk3[lbl_msk1 == 3] = 255
    msk3[lbl_msk1 == 4] = 255

    msk0 = msk0[..., np.newaxis]
    msk1 = msk1[..., np.newaxis]
    msk2 = msk2[..., np.newaxis]
    msk3 = msk3[..., np.newaxis]

    msk = np.concatenate([msk0, msk1, msk2, msk3], axis=2)
    msk = (msk > 127)

    msk = msk * 1

    lbl_msk = msk[..., 1:].argmax(axis=2)
    return msk, lbl_msk


def masks_closed(pre_mask, label, train):
    """the closed form the loader computes, per pixel from the post label byte l (and, for ValData, the pre mask byte):
    m1 = l == 1, m2 = l == 2, m3 = l in (3, 4), m0 = m1 | m2 | m3 (train) or pre_mask > 127 (val); lbl = 1 where m2, 2 where m3,
    else 0.  Returns (msk uint8 [4, H, W], lbl uint8 [H, W])"""
    l = np.asarray(label)
    m1, m2, m3 = l == 1, l == 2, (l == 3) | (l == 4)
    m0 = (m1 | m2 | m3) if train else np.asarray(pre_mask) > 127
    lbl = np.where(m2, 1, np.where(m3, 2, 0))
    return np.stack([m0, m1, m2, m3]).astype(np.uint8), lbl.astype(np.uint8)


def batch_reference(pre, post, pre_mask, label, indices, crop, origins, train):
    """make_adapt_batch on the host: img float32 [n, 6, c, c] = preprocess_inputs (x /= 127; x -= 1 in float32), and the masks of
    the script's literal code on every crop"""
    n = len(indices)
    img = np.empty((n, 6, crop, crop), dtype=np.float32)
    msk = np.empty((n, 4, crop, crop), dtype=np.uint8)
    lbl = np.empty((n, crop, crop), dtype=np.uint8)
    literal = train_masks_literal if train else val_masks_literal
    for k, i in enumerate(indices):
        x0, y0 = (0, 0) if origins is None else origins[k]
        win = (slice(y0, y0 + crop), slice(x0, x0 + crop))
        x = np.concatenate([pre[i][win], post[i][win]], axis=2).astype(np.float32)
        x /= 127
        x -= 1
        img[k] = x.transpose(2, 0, 1)
        m, l = literal(pre_mask[i][win], label[i][win])
        msk[k], lbl[k] = m.transpose(2, 0, 1), l
    return img, msk, lbl


# ---- the file set ---------------------------------------------------------------------------------------------------------------
def trainset_literal(names, labels, split):
    """train_adapt.py:369-391 on a list of names and their label arrays; split(n) -> (train_idxs, val_idxs) stands for
    train_test_split(np.arange(n), test_size=0.15, random_state=seed).  Returns (train names in the script's order, val names)."""
    xbd_files = []
    aoi_files = []
    for fn, msk in zip(names, labels):
        msk = msk[msk > 0]
        if msk.sum() > 500:
            if 'AOI' in fn:
                aoi_files.append(fn)
            else:
                xbd_files.append(fn)
    train_idxs, val_idxs = split(len(aoi_files))
    train_aoi = [aoi_files[x] for x in train_idxs]
    xbd_files.extend(train_aoi)
    return xbd_files, [aoi_files[x] for x in val_idxs]


# ---- validation (lines 262-280) ---------------------------------------------------------------------------------------------------
def val_counts(logits, msk0, lbl, thr=0.3, select="reference"):
    """logits float32 [B, 4, H, W], msk0 [B, H, W], lbl [B, H, W] (0 .. 2) -> image_counts int64 [B, 3] = |gt0|, |loc|, |gt0 & loc|
    and class_counts int64 [3, 3] = tp, fn, fp: lines 267-279 with the sigmoid in float32, as tests/_xbd_val_cases.counts"""
    import _xbd_val_cases as V
    s = V.sigmoid32(logits)
    B = s.shape[0]
    image_counts = np.zeros((B, 3), dtype=np.int64)
    class_counts = np.zeros((3, 3), dtype=np.int64)
    for j in range(B):
        msk_pred = s[j, 0]
        msk_damage_pred = s[j, 1:]
        loc = msk_pred > np.float32(thr)
        gt0 = np.asarray(msk0[j]).astype(bool)
        image_counts[j] = gt0.sum(), loc.sum(), np.logical_and(gt0, loc).sum()
        pred = msk_damage_pred.argmax(axis=0)
        pred = pred * loc
        lj = np.asarray(lbl[j])
        sel = (lj[0] > 0) if select == "reference" else (np.asarray(msk0[j]) > 0)
        targ = lj[sel]
        pred = pred[sel]
        for c in range(3):
            class_counts[c, 0] += np.logical_and(pred == c, targ == c).sum()
            class_counts[c, 1] += np.logical_and(pred != c, targ == c).sum()
            class_counts[c, 2] += np.logical_and(pred == c, targ != c).sum()
    return image_counts, class_counts


def val_score_literal(image_counts, class_counts):
    """lines 282-289 on the counts: (score, d0, f1, f1_sc)"""
    dices0 = [1.0 if gt0 + loc == 0 else 2. * both / (gt0 + loc) for gt0, loc, both in np.asarray(image_counts)]
    d0 = np.mean(dices0)
    tp, fn, fp = (np.asarray(class_counts)[:, k].astype(np.float64) for k in range(3))
    f1_sc = np.zeros((3,))
    with np.errstate(divide="ignore", invalid="ignore"):
        for c in range(3):
            f1_sc[c] = 2 * tp[c] / (2 * tp[c] + fp[c] + fn[c])
        f1 = 3 / np.sum(1.0 / (f1_sc + 1e-6))
    sc = 0.3 * d0 + 0.7 * f1
    return sc, d0, f1, f1_sc
