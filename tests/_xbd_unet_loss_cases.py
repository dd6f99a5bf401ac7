"""The loss of xBD_code/train_unettransformer.py:438-461 restated in float64 torch, with autograd for the gradient, and the shapes
the GPU tests run it at.  Written from the formulas of include/dahitra_hip.h (dh_xbd_unet_loss_fwd), not from the kernel:

    s_c = sigmoid(x_c);  I, S, T = sum s_c t_c, sum s_c, sum t_c;  dice_c = 1 - (2 I + eps) / (S + T + eps)
    o = clamp(s_c, eps, 1 - eps), tt = clamp(t_c, eps, 1 - eps), pt = (1 - tt)(1 - o) + tt o;  focal_c = mean(-(1 - pt)^2 log pt)
    channel_c = dice_w dice_c + focal_w focal_c
    m = y > 0;  z = m x;  nll = logsumexp(z) - z_y;  ce = sum(w_y nll) / sum(w_y) over every pixel whose label is 0 .. 4
    meter = (2 I' + eps) / (S' + T_0 + eps) with s' = sigmoid(z_0)
    loss = sum_c cw_c channel_c + ce_w ce

One detail is the reference's and not a formula: FocalLoss2d converts the targets with `.float()` BEFORE it clamps them
(losses.py:284-288), so `tt` is the float32 neighbour of 1e-6 or of 1 - 1e-6, and `1 - tt` a float32 difference, whatever the
precision of the logits.  The kernels form both in float32 too.  tests/test_xbd_unet_step_cpu.py holds this restatement to the
reference's own float64 results."""
import math

import numpy as np
import torch

EPS = 1e-6
CHANNEL_WEIGHTS = (0.1, 0.1, 0.6, 0.3, 1.0)
CE_WEIGHTS = (0.01, 0.10, 1.0, 0.80, 1.0)
LN5 = math.log(5.0)

# (B, H, W, saturated): what the GPU tests run; the last one is appended by the GPU test from ops.XBD_UNET_LOSS_PASS
SHAPES = ((2, 35, 37, True),         # H * W odd: the one-pixel form, with saturated logits
          (1, 1, 1, False),
          (3, 8, 4, False),          # less than a wavefront, 4-pixel form
          (2, 32, 36, False))        # the 4-pixel form with a ragged last workgroup (576 quads = 2 workgroups + 64 lanes)


def damage_label(msk):
    """numpy's statement of the 'damage' label: the first set channel among 1 .. 4, 0 where none is set"""
    m = np.asarray(msk)[:, 1:]
    return np.where(m.any(1), m.argmax(1) + 1, 0).astype(np.uint8)


def make_case(golden, B, H, W, saturated, seed):
    """(logits fp32, msk uint8, damage label uint8) of a test shape.  Every pixel -- its five logits and its five mask bytes -- is
    a pixel of the fixture `golden`, drawn with replacement from its two cases.  The reason: the GPU tests measure the kernels
    against float64 with the reference's own float32 error ON THE FIXTURE as the yardstick, and that error is carried by a few
    pixels -- logits of 8 .. 13.8 in magnitude, where float32 resolves 1 - sigmoid(x) to a few percent and the focal gradient
    feels it.  Inputs drawn afresh hold more or fewer such pixels than the fixture by chance, and the yardstick then says
    nothing about them (measured: randn * 3 at 2 x 5 x 32 x 36 puts the kernel 5.9e-05 of the largest gradient from float64,
    the fixture's float32 reference 8.0e-06); on the fixture's own pixels it is the reference's error on the same arithmetic.
    saturated: with the fixture's +25 / -25 pixels (both clamps of the focal term), at least one of each; without them otherwise."""
    x = np.concatenate([golden[n + "_logits"].transpose(0, 2, 3, 1).reshape(-1, 5) for n in ("zero", "damage")])
    m = np.concatenate([golden[n + "_msk"].transpose(0, 2, 3, 1).reshape(-1, 5) for n in ("zero", "damage")])
    if not saturated:
        keep = (np.abs(x) != 25.0).all(1)
        x, m = x[keep], m[keep]
    idx = np.random.RandomState(seed).randint(0, len(x), size=B * H * W)
    if saturated:
        idx[:2] = np.nonzero((x == 25.0).any(1))[0][0], np.nonzero((x == -25.0).any(1))[0][0]
    logits = np.ascontiguousarray(x[idx].reshape(B, H, W, 5).transpose(0, 3, 1, 2))
    msk = np.ascontiguousarray(m[idx].reshape(B, H, W, 5).transpose(0, 3, 1, 2))
    return torch.from_numpy(logits), torch.from_numpy(msk), torch.from_numpy(damage_label(msk))


def restate(logits, msk, lbl, channel_weights=CHANNEL_WEIGHTS, ce_weights=CE_WEIGHTS, dice_w=1.0, focal_w=8.0, ce_w=8.0,
            upstream=1.0, combo_only=False):
    """float64: {'loss', 'parts' [8], 'grad' = d(upstream * loss) / dlogits} as numpy arrays.  lbl: integer labels [B, H, W]; a
    label above 4 has no cross-entropy term and is counted in parts[7].  combo_only leaves the cross-entropy term out of the
    loss (the five weighted channel terms alone)."""
    x = torch.as_tensor(np.asarray(logits), dtype=torch.float64).clone().requires_grad_(True)
    t = torch.as_tensor(np.asarray(msk)).to(torch.float64)
    y = torch.as_tensor(np.asarray(lbl)).to(torch.int64)
    tt32 = torch.as_tensor(np.asarray(msk)).float().clamp(EPS, 1.0 - EPS)                          # the reference's float32 clamp
    tt, one_minus_tt = tt32.to(torch.float64), (1 - tt32).to(torch.float64)                        # ... and its float32 1 - tt
    s = torch.sigmoid(x)
    channel = []
    for c in range(5):
        I, S, T = (s[:, c] * t[:, c]).sum(), s[:, c].sum(), t[:, c].sum()
        dice = 1 - (2 * I + EPS) / (S + T + EPS)
        o = s[:, c].clamp(EPS, 1.0 - EPS)
        pt = one_minus_tt[:, c] * (1 - o) + tt[:, c] * o
        focal = (-(1.0 - pt) ** 2 * torch.log(pt)).mean()
        channel.append(dice_w * dice + focal_w * focal)
    m = (y > 0).to(torch.float64).unsqueeze(1)
    z = x * m
    valid = y <= 4
    yc = y.clamp(max=4)
    nll = torch.logsumexp(z, dim=1) - z.gather(1, yc.unsqueeze(1)).squeeze(1)
    w = torch.tensor(ce_weights, dtype=torch.float64)[yc] * valid.to(torch.float64)
    ce = (w * nll).sum() / w.sum()
    s0 = torch.sigmoid(z[:, 0])
    meter = (2 * (s0 * t[:, 0]).sum() + EPS) / (s0.sum() + t[:, 0].sum() + EPS)
    loss = sum(cw * l for cw, l in zip(channel_weights, channel))
    if not combo_only:
        loss = loss + ce_w * ce
    (loss * upstream).backward()
    parts = np.array([float(l.detach()) for l in channel] + [float(ce.detach()), float(meter.detach()), float((~valid).sum())],
                     dtype=np.float64)
    return {"loss": float(loss.detach()), "parts": parts, "grad": x.grad.numpy()}


def yardstick(golden):
    """The reference's own float32 error on the fixture, the measure of the GPU tests: the distance of its float32 CPU results
    from its float64 ones, the largest over the fixture's cases per quantity -- 'loss', 'channel', 'ce', 'dice' relative, 'grad'
    as the largest error over the largest gradient."""
    out = {k: 0.0 for k in ("loss", "channel", "ce", "dice", "grad")}
    for name in ("zero", "damage"):
        for k in ("loss", "channel", "ce", "dice"):
            a, b = golden["%s_%s32" % (name, k)].astype(np.float64), golden["%s_%s64" % (name, k)]
            out[k] = max(out[k], float(np.max(np.abs(a - b) / np.abs(b))))
        a, b = golden[name + "_grad32"].astype(np.float64), golden[name + "_grad64"]
        out["grad"] = max(out["grad"], float(np.abs(a - b).max() / np.abs(b).max()))
    return out
