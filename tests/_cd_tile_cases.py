"""dh_cd_tile_stitch restated in float32 numpy, in the kernel's stated order, and the inputs the tile tests share.

For pixel (Y, X) and class c, over the covering iy ascending, then ix ascending, then f in plan order:
    ly = Y - ys[iy], lx = X - xs[ix], g = wy[ly] * wx[lx]
    v  = logits[(iy * nx + ix) * nf + f, c, ly' , lx'],  ly' = h - 1 - ly if flip bit 0, lx' = w - 1 - lx if flip bit 1
    acc = acc + g * v;  ws = ws + g           each operation rounded to float32 on its own
    out = acc / ws
Walking the views in the order (iy, ix, f) and adding each un-flipped window into its place gives every pixel its covering views
in exactly that order; numpy rounds g * v and the sum separately.  The mask is dh_argmax_nchw's rule on out.  This file is the
oracle for the kernel; the kernel's own output is never the yardstick."""
import os

import numpy as np

from _xbd_tta_cases import flip

# the stitch shapes of the GPU tests: (C, H, W, window, stride, flips, weight)
ODD = (2, 19, 23, (8, 8), (5, 6), (0, 1, 2, 3), "triangle")          # odd, non-square, clamped last window, cover 1..3 per axis
IDENTITY = (5, 64, 96, (32, 32), (32, 32), (0,), "mean")             # output bits are the input bits moved into place
MAXC = (8,) + ODD[1:]
BIG = (2, 1024, 1024, (256, 256), (128, 128), (0, 1, 2, 3), "triangle")          # P = 196
LOOP = (2, 2048, 1280, (256, 256), (256, 256), (0, 3), "triangle")   # 655 360 quads: more than the 2048 x 256 of one grid pass
SHAPES = {"odd": ODD, "identity": IDENTITY, "maxc": MAXC, "big": BIG, "loop": LOOP}


def make_plan(case):
    from dahitra_amd.tiles import TilePlan
    C, H, W, window, stride, flips, weight = case
    return TilePlan(H, W, window=window, stride=stride, flips=flips, weight=weight)


def stitch(logits, plan, wy=None, wx=None, mutate=None):
    """logits [P, C, h, w] float32 -> (out [C, H, W] float32, ws [H, W] float32).  wy, wx: other weight profiles than the plan's.
    mutate: a deliberately WRONG restatement, for the tests that show the properties catch it --
      'flips'   the two flip bits swapped,
      'weight'  the weight indexed by the flipped (stored) coordinate instead of the un-flipped one,
      'order'   the covering views taken in the reverse order."""
    logits = np.asarray(logits)
    assert logits.dtype == np.float32 and logits.shape[0] == plan.P and logits.shape[2:] == (plan.h, plan.w)
    pwy, pwx = plan.weights()
    wy = pwy if wy is None else np.asarray(wy, dtype=np.float32)
    wx = pwx if wx is None else np.asarray(wx, dtype=np.float32)
    g = wy[:, None] * wx[None, :]
    assert g.dtype == np.float32
    C, h, w = logits.shape[1], plan.h, plan.w
    acc = np.zeros((C, plan.H, plan.W), dtype=np.float32)
    ws = np.zeros((plan.H, plan.W), dtype=np.float32)
    views = [(iy, ix, f) for iy in range(plan.ny) for ix in range(plan.nx) for f in range(plan.nf)]
    if mutate == "order":
        views = views[::-1]
    for iy, ix, f in views:
        y0, x0, k = plan.ys[iy], plan.xs[ix], plan.flips[f]
        v = logits[(iy * plan.nx + ix) * plan.nf + f]
        gk = g
        if mutate == "flips":
            k = ((k & 1) << 1) | ((k >> 1) & 1)
        if mutate == "weight":
            gk = flip(g, k)          # after the un-flip below, position (ly, lx) carries the weight of its stored coordinate
        v = flip(v, k)               # flip_k is its own inverse: the window as it lies in the tile
        t = gk * v
        assert t.dtype == np.float32
        acc[:, y0:y0 + h, x0:x0 + w] = acc[:, y0:y0 + h, x0:x0 + w] + t
        ws[y0:y0 + h, x0:x0 + w] = ws[y0:y0 + h, x0:x0 + w] + gk
    with np.errstate(invalid="ignore", divide="ignore"):
        out = acc / ws
    assert out.dtype == np.float32
    return out, ws


def stitch_literal(logits, plan, wy=None, wx=None):
    """the same statement pixel by pixel in float32 scalars, literally as written at the top (small shapes only): a second,
    independently ordered form that the vectorised one above must equal bit for bit"""
    f32 = np.float32
    pwy, pwx = plan.weights()
    wy = pwy if wy is None else np.asarray(wy, dtype=f32)
    wx = pwx if wx is None else np.asarray(wx, dtype=f32)
    C, h, w = logits.shape[1], plan.h, plan.w
    out = np.empty((C, plan.H, plan.W), dtype=f32)
    for Y in range(plan.H):
        for X in range(plan.W):
            acc, ws = [f32(0)] * C, f32(0)
            for iy in range(plan.ny):
                ly = Y - plan.ys[iy]
                if not 0 <= ly < h:
                    continue
                for ix in range(plan.nx):
                    lx = X - plan.xs[ix]
                    if not 0 <= lx < w:
                        continue
                    g = f32(wy[ly] * wx[lx])
                    for f, k in enumerate(plan.flips):
                        sy, sx = (h - 1 - ly if k & 1 else ly), (w - 1 - lx if k & 2 else lx)
                        p = (iy * plan.nx + ix) * plan.nf + f
                        for c in range(C):
                            acc[c] = f32(acc[c] + f32(g * logits[p, c, sy, sx]))
                        ws = f32(ws + g)
            for c in range(C):
                out[c, Y, X] = f32(acc[c] / ws)
    return out


def relabel(logits, plan, flips):
    """(logits', plan') with the same windows under the flip codes `flips` (a permutation of the plan's, position by position):
    view (window, f) keeps its content as it lies in the tile and is stored under code flips[f] instead of plan.flips[f]"""
    from dahitra_amd.tiles import TilePlan
    other = TilePlan(plan.H, plan.W, (plan.h, plan.w), (plan.sy, plan.sx), flips, plan.weight)
    out = np.empty_like(logits)
    for p in range(plan.P):
        f = p % plan.nf
        out[p] = flip(flip(logits[p], plan.flips[f]), flips[f])
    return out, other


def stitch64(logits, plan):
    """the same blend in float64 (no stated order: float64 sums of at most 36 float32 products of small integers)"""
    wy, wx = (a.astype(np.float64) for a in plan.weights())
    g = wy[:, None] * wx[None, :]
    acc = np.zeros((logits.shape[1], plan.H, plan.W))
    ws = np.zeros((plan.H, plan.W))
    cover = np.zeros((plan.H, plan.W), dtype=np.int64)
    mag = np.zeros((plan.H, plan.W))
    for iy in range(plan.ny):
        for ix in range(plan.nx):
            for f in range(plan.nf):
                y0, x0 = plan.ys[iy], plan.xs[ix]
                v = flip(np.asarray(logits[(iy * plan.nx + ix) * plan.nf + f], dtype=np.float64), plan.flips[f])
                sl = (slice(y0, y0 + plan.h), slice(x0, x0 + plan.w))
                acc[(slice(None),) + sl] += g * v
                ws[sl] += g
                cover[sl] += 1
                mag[sl] += g * np.abs(v).max(axis=0)
    return acc / ws, cover, mag / ws, ws


def first_max(out):
    """dh_argmax_nchw's rule over axis 0 of [C, H, W]: class 0 to begin with, a later class wins only if strictly greater (so a
    NaN never wins and a NaN in class 0 is never beaten)"""
    best = out[0].copy()
    arg = np.zeros(out.shape[1:], dtype=np.uint8)
    for c in range(1, out.shape[0]):
        with np.errstate(invalid="ignore"):
            win = out[c] > best
        best = np.where(win, out[c], best)
        arg[win] = c
    return arg


def confusion(label, mask, C):
    """counts[label, class] as dh_confusion_matrix orients them; a label >= C counts nowhere"""
    label, mask = np.asarray(label).reshape(-1).astype(np.int64), np.asarray(mask).reshape(-1).astype(np.int64)
    keep = label < C
    return np.bincount(label[keep] * C + mask[keep], minlength=C * C).reshape(C, C).astype(np.int64)


# ---- inputs --------------------------------------------------------------------------------------------------------------
def random_logits(plan, C, seed):
    return (np.random.RandomState(seed).randn(plan.P, C, plan.h, plan.w) * 3).astype(np.float32)


def field(C, H, W, seed, bits=10, span=8):
    """F [C, H, W] float32, multiples of 2^-bits in [-span, span), asymmetric under both flips"""
    rng = np.random.RandomState(seed)
    F = (rng.randint(-span << bits, span << bits, (C, H, W)).astype(np.float64) / (1 << bits)).astype(np.float32)
    assert not np.array_equal(F, F[:, ::-1]) and not np.array_equal(F, F[:, :, ::-1])
    return F


def views_of(F, plan):
    """logits [P, C, h, w]: view p = flip_k of the crop of F at the view's origin, what a perfectly equivariant net returns"""
    out = np.empty((plan.P, F.shape[0], plan.h, plan.w), dtype=np.float32)
    for iy in range(plan.ny):
        for ix in range(plan.nx):
            crop = F[:, plan.ys[iy]:plan.ys[iy] + plan.h, plan.xs[ix]:plan.xs[ix] + plan.w]
            for f in range(plan.nf):
                out[(iy * plan.nx + ix) * plan.nf + f] = flip(crop, plan.flips[f])
    return out


def check_exact(F, plan, wy=None, wx=None, bits=10):
    """the condition under which every partial sum of the blend of views_of(F) is exact in float32: |F| * sum(g) in units of
    2^-bits stays below 2^24"""
    pwy, pwx = plan.weights()
    wy, wx = (pwy if wy is None else wy), (pwx if wx is None else wx)
    g = np.asarray(wy, dtype=np.float64)[:, None] * np.asarray(wx, dtype=np.float64)[None, :]
    assert np.array_equal(g, np.round(g)) and g.min() >= 1
    total = np.zeros((plan.H, plan.W))
    for y0 in plan.ys:
        for x0 in plan.xs:
            total[y0:y0 + plan.h, x0:x0 + plan.w] += g * plan.nf
    assert float(np.abs(F).max()) * float(total.max()) * (1 << bits) < (1 << 24)
    assert np.array_equal(F.astype(np.float64) * (1 << bits), np.round(F.astype(np.float64) * (1 << bits)))


def plant(logits, plan, seed, ties=0.2, nans=0.02):
    """ties and NaNs planted at TILE positions so that they survive the blend.  At a share `ties` of the pixels every covering
    view gets, in all classes, the value of its class 0: the classes then go through the same operations on the same numbers
    and the blended pixel is an exact tie.  At a share `nans` of the (class, pixel) positions every covering view holds a NaN."""
    rng = np.random.RandomState(seed)
    P, C, h, w = logits.shape
    tie = views_of((rng.rand(1, plan.H, plan.W) < ties).astype(np.float32), plan) > 0
    nan = views_of((rng.rand(C, plan.H, plan.W) < nans).astype(np.float32), plan) > 0
    out = np.where(tie, logits[:, :1], logits)
    out[nan] = np.nan
    return np.ascontiguousarray(out, dtype=np.float32)


# ---- model level ---------------------------------------------------------------------------------------------------------
LEVIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "levir")


def levir_pairs():
    """the four shipped LEVIR pairs: (A, B [4, 256, 256, 3] uint8, L [4, 256, 256] uint8 in {0, 1}, names)"""
    from PIL import Image
    names = sorted(os.listdir(os.path.join(LEVIR, "train", "A")))
    load = lambda d, n, mode: np.asarray(Image.open(os.path.join(LEVIR, "train", d, n)).convert(mode))
    A = np.stack([load("A", n, "RGB") for n in names])
    B = np.stack([load("B", n, "RGB") for n in names])
    L = np.stack([np.array(Image.open(os.path.join(LEVIR, "train", "label", n)), dtype=np.uint8) for n in names]) // 255
    assert A.shape == (4, 256, 256, 3) and L.shape == (4, 256, 256)
    return A, B, L.astype(np.uint8), names


def mosaic(x, order, cols):
    """the images x[order] laid out row by row, `cols` per row: [rows * 256, cols * 256, ...]"""
    rows = [np.concatenate([x[i] for i in order[r:r + cols]], axis=1) for r in range(0, len(order), cols)]
    return np.concatenate(rows, axis=0)
