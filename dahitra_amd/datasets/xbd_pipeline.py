"""Pre-decoded xBD samples resident in HBM + TrainData / ValData.__getitem__ on the device (ops.xbd_augment: dh_xbd_augment_u8,
dh_xbd_augment_jitter_u8).

The reference's xBD loader opens four 1024x1024 PNGs per sample (pre and post image, pre mask, post label) and, in training,
crops, flips and bilinearly resizes all four in Pillow before it builds the mask channels (xBD_code/train.py:99-183); DataLoader
workers do not feed the MI355X xBD step that way.  Here the four uint8 stacks are decoded once and stay on the device, and ONE
kernel per batch produces what `GraphedXbdStep(net, opt, imgs, msks)` consumes: crop, flips, TF.resized_crop -- Pillow's
two-pass fixed-point BILINEAR resize, byte for byte, on the masks as well -- the five mask channels and preprocess_inputs.
With `jitter_gen` the 9 % of the samples that draw it also get the reference's ColorJitter (train.py:138-139), byte for byte what
PIL's ImageEnhance chain computes; a batch with such a sample takes a second launch for contrast's whole-image mean.

    pipe = GpuXbdPipeline.from_image_dir('/data/xbd/train/images', device='cuda:0')
    for batch in pipe.batches(4, 1024, train=True, rng=random.Random(0), jitter_gen=torch.Generator().manual_seed(0)):
        loss = step(batch['img'], batch['msk'])                                  # {'img', 'msk', 'lbl_msk', 'fn'}

Differences from the reference, all deliberate:
  * `msk` is uint8 (0 / 1), not long: the step casts it to float where it always did (graph.py, GraphedXbdStep._loss_and_grad;
    models/xbd.xbd_loss), and 5 bytes per pixel instead of 40 is most of the batch's mask traffic.  `lbl_msk` is uint8 too.
  * `lbl_msk` of a TRAINING batch is zeros, as in the reference: there msk[0] is set wherever any other channel is, so
    msk.argmax(axis=2) is 0 at every pixel (train.py:171-174).  One zero tensor is kept and returned; do not write to it.
  * ColorJitter is applied only to an epoch that is given `jitter_gen`, the torch.Generator its draws come from (the reference
    draws them from torch's global generator, in its worker processes); without one the flag `draw_train_params` reports is
    dropped, as before.  The draws are torchvision's (>= 0.8: one randperm(4), then the three factors) and the arithmetic is
    Pillow's (`jitter_reference_u8` states it).
  * `dilate=k` (off by default) replaces `msk` of a training batch by the dilated, prioritised channels that
    xBD_code/train_unettransformer.py:262-273 builds with dilation(., square(5)) -- lines that train.py, which this loader
    follows, has commented out -- in one more launch (dh_xbd_msk_dilate_u8).

xBD_code/train_unettransformer.py, the script that trains DAHiTra proper, augments differently: vertical flip, np.rot90, a
reflect-101 shift, a cv2.warpAffine rotate / scale and shift_channels.  `make_unet_batch` / `unet_batches` are that loader,
one launch per batch as well (dh_xbd_augment_warp_u8), with `draw_unet_params` for its draws:

    for batch in pipe.unet_batches(16, 256, random.Random(0)):                    # dilate=5: the script's targets
        loss = step(batch['img'], batch['msk'])

  * The byte contract of the warp is `warp_affine_u8`, a numpy restatement of OpenCV's fixed-point path for 8-bit images
    (INTER_LINEAR, BORDER_REFLECT_101; OpenCV 4.x up to 4.10, imgwarp.cpp), and `unet_reference_u8` around it.  It was written
    from that code, not compared with it: no OpenCV is installed where this was built and tested, so equality with a cv2 build
    has not been run.  OpenCV 4.11 and later take another path for linear warpAffine, and the matrix's cos / sin come from the
    libm of the host that writes the tables.
  * The script's colour stage (lines 211-244: change_hsv, then gauss_noise, cv2.blur, saturation, brightness or contrast) is
    opt-in: `unet_batches(16, 256, rng, colour=True, np_rng=np.random.RandomState(0))` draws with `draw_unet_colour` --
    `draw_unet_params`' stream -- and applies it in place in two more launches per batch that drew any (dh_xbd_unet_colour_u8),
    byte for byte `unet_colour_reference_u8`.  The blends and the noise equal the reference's utils.py on a committed fixture;
    contrast's mean is defined from the exact channel sums (`contrast_mean`: against numpy's pairwise mean a byte can move only
    where a blended value lies within about 1e-11 of an integer); cv2.blur and change_hsv's 8-bit cv2.cvtColor are restated from
    OpenCV 4.x's scalar paths, and equality with a cv2 build has not been run (a vectorised build may fuse multiply-adds and
    differ by one in a byte).  Without `colour=True` the operations are drawn, reported as `skipped` and not applied.
  * Not built: clahe (OpenCV's 8-bit Lab tables) and imgaug's elastic transform, each drawn by under 2 % of the samples.  Both
    draw functions draw them, so the `random` stream stands where the script's does, and report them as `skipped`.

The set the scripts train on comes from the same resident pipeline.  Both scan every post-disaster label for the classes it
holds, cut their one folder 90 / 10 with sklearn's train_test_split and train on an index list in which files with damage repeat
(train.py:397-429, train_unettransformer.py:499-522).  `class_table` / `file_classes` read that scan off the resident labels in
one launch (ops.xbd_class_table, dh_xbd_class_table_u8); `split_indices`, `train_indices` and `unet_train_indices` are the split
and the two lists on the host; `trainset` / `unet_trainset` do a script's lines in one call; and `indices=` / `drop_last=` of
`batches`, `unet_batches` and models/xbd.unet_val_batches run an epoch over such a list, a repeated index reading the same
resident source again:

    train_idxs, val_idxs = pipe.unet_trainset(seed)
    for batch in pipe.unet_batches(16, 256, random.Random(seed + 321), indices=train_idxs, drop_last=True): ...
    for batch in xbd.unet_val_batches(pipe, 16, 256, indices=val_idxs): ...
"""
import collections
import functools
import glob
import math
import os
import random

import numpy as np
import torch
from PIL import Image

from .. import ops

PRECISION_BITS = 22        # Pillow's 8-bit resize: coefficients in 2.22 fixed point (Resample.c)
PARAM_FIELDS = ("x0", "y0", "hflip", "vflip", "resize", "top", "left", "height", "width")


@functools.lru_cache(maxsize=None)
def _resize_coeffs(in_size, out_size):
    if in_size < 1 or out_size < 1:
        raise ValueError("resize_coeffs: %d -> %d: empty axis" % (in_size, out_size))
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs                                        # the bilinear filter's support is 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    lo = np.maximum((center - support + 0.5).astype(np.int64), 0)            # C's (int): truncation
    cnt = np.minimum((center + support + 0.5).astype(np.int64), in_size) - lo
    t = np.arange(3, dtype=np.int64)[None, :]
    arg = ((t + lo[:, None]) - center[:, None] + 0.5) * (1.0 / fs)
    w = np.maximum(1.0 - np.abs(arg), 0.0)
    w[t >= cnt[:, None]] = 0.0
    if (cnt > 3).any():
        raise ValueError("resize_coeffs: %d -> %d needs %d taps, the table holds three" % (in_size, out_size, cnt.max()))
    ww = w[:, 0] + w[:, 1] + w[:, 2]                          # Pillow sums the taps in this order
    w = np.where(ww[:, None] != 0, w / ww[:, None], w)
    k = (0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)
    # what the kernel's 32-bit accumulator and its unclipped byte rely on: 255 * sum(k) + (1 << 21) < 256 << 22
    if (k < 0).any() or (k.sum(axis=1) > (1 << PRECISION_BITS) + 8192).any():
        raise ValueError("resize_coeffs: %d -> %d: coefficients outside 0 <= k, sum(k) <= 2^22 + 8192" % (in_size, out_size))
    out = np.concatenate([lo[:, None], k], axis=1).astype(np.int32)
    out.setflags(write=False)
    return out


def resize_coeffs(in_size, out_size):
    """[out_size, 4] int32 rows (first source index, k0, k1, k2) of Pillow's Image.resize(..., Image.BILINEAR) along one axis
    of an 8-bit image.  Three taps hold every in_size <= out_size -- all the loader asks for -- and a source up to half as
    long again; ValueError for one that needs more.
    Derived as Pillow's precompute_coeffs / normalize_coeffs_8bpc do, in float64: scale = in / out, support = max(scale, 1);
    output index o has center = (o + 0.5) * scale, first tap lo = max(int(center - support + 0.5), 0), count =
    min(int(center + support + 0.5), in) - lo; tap t < count weighs max(0, 1 - |(t + lo - center + 0.5) / support|), the weights are
    divided by their sum and each becomes int(0.5 + w * (1 << 22)); taps at or past `count` are 0 and may lie outside the
    source.  An output byte of a pass is clip8(((1 << 21) + sum_t in[lo + t] * k[t]) >> 22).  in == out gives (o, 1 << 22, 0, 0).
    Byte for byte Pillow on nine odd shapes (tests/test_xbd_loader_cpu.py).  The array is cached and read-only."""
    return _resize_coeffs(int(in_size), int(out_size))


def draw_train_params(rng, H, W, crop):
    """One training sample's draws from `rng` (a random.Random, or the `random` module), exactly the reference's and in its
    order (xBD_code/train.py:110-138): x0, y0; then, if random() > 0.7: hflip, vflip (each random() > 0.3); if random() > 0.3
    the two randint(0, 200) of TF.resized_crop(img, x, y, crop - x, crop - y, (crop, crop)) -- top = x, left = y in
    torchvision's argument order; and the ColorJitter decision random() > 0.7.  Returns (params row in PARAM_FIELDS order,
    jitter flag).  ColorJitter itself is not applied (module docstring); its own draws come from torch's generator, so the
    Python stream stands where the reference's does after the sample."""
    if crop > H or crop > W:
        raise ValueError("crop %d is larger than the %dx%d image" % (crop, H, W))
    x0 = rng.randint(0, W - crop)
    y0 = rng.randint(0, H - crop)
    hf = vf = rs = top = left = 0
    bh = bw = crop
    jitter = False
    if rng.random() > 0.7:
        hf = int(rng.random() > 0.3)
        vf = int(rng.random() > 0.3)
        if rng.random() > 0.3:
            x = rng.randint(0, 200)
            y = rng.randint(0, 200)
            if crop - x < 1 or crop - y < 1:
                raise ValueError("resized_crop box (%d, %d) leaves nothing of a %d crop" % (x, y, crop))
            rs, top, left, bh, bw = 1, x, y, crop - x, crop - y
        jitter = rng.random() > 0.7
    return [x0, y0, hf, vf, rs, top, left, bh, bw], jitter


def draw_jitter_params(gen=None):
    """One ColorJitter(brightness=[0.8, 1.2], contrast=[0.8, 1.2], saturation=[0.8, 1.2]) call's draws (train.py:139;
    torchvision >= 0.8, ColorJitter.get_params), from the torch.Generator `gen` or, as the reference does, from torch's global
    one: fn_idx = randperm(4), then the brightness, contrast and saturation factors, each float(empty(1).uniform_(0.8, 1.2)).
    Hue is None: it draws nothing.  Returns (order, (b, c, s)): the order as drawn, a permutation of 0 .. 3 (0 brightness,
    1 contrast, 2 saturation, 3 hue = nothing), and the factors, float32 values."""
    order = torch.randperm(4, generator=gen).tolist()
    factors = tuple(float(torch.empty(1).uniform_(0.8, 1.2, generator=gen)) for _ in range(3))
    return order, factors


def _luma(img):
    """PIL's convert("L") of [..., 3] uint8 -> int64"""
    c = img.astype(np.int64)
    return (c[..., 0] * 19595 + c[..., 1] * 38470 + c[..., 2] * 7471 + 0x8000) >> 16


def _blend_u8(d, i, factor):
    """PIL's Image.blend(degenerate, image, factor) on uint8 arrays (Blend.c): per byte t = (float)d + alpha * (float)(i - d)
    with alpha = (float)factor -- the product is rounded to float32, then the sum (numpy does not fuse them); for 0 <= alpha <= 1
    the byte is (int)t, otherwise t is clipped to 0 .. 255 first."""
    alpha = np.float32(factor)
    d = np.broadcast_to(d, i.shape).astype(np.int32)
    prod = alpha * (i.astype(np.int32) - d).astype(np.float32)
    t = d.astype(np.float32) + prod
    assert prod.dtype == np.float32 and t.dtype == np.float32
    if not 0 <= alpha <= 1:
        t = np.clip(t, np.float32(0), np.float32(255))
    return t.astype(np.int32).astype(np.uint8)


def jitter_reference_u8(img_u8, order, factors):
    """What ColorJitter computes on an [h, w, 3] uint8 RGB image with PIL: the operations of `order` (0 brightness, 1 contrast,
    2 saturation, 3 hue = skipped; any sequence of them) in turn, each ImageEnhance.X(img).enhance(f) = Image.blend(degenerate,
    img, f) with f = factors[op].  The degenerate image is 0 (Brightness), L of each pixel on all three channels (Color, L =
    (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16) or, for Contrast, int(mean + 0.5) of L over the whole image AS IT
    STANDS when contrast is applied: with the exact sum s over n pixels, (2 s + n) // (2 n).  Byte for byte PIL on all 24
    orders (tests/test_xbd_jitter_cpu.py); the kernel's statement of the arithmetic (csrc/augment_xbd.hip)."""
    img = np.ascontiguousarray(img_u8)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("jitter_reference_u8: an [h, w, 3] uint8 image, got %s %s" % (img.shape, img.dtype))
    for op in order:
        if op == 0:
            img = _blend_u8(np.uint8(0), img, factors[0])
        elif op == 1:
            lum = _luma(img)
            s, n = int(lum.sum()), lum.size
            img = _blend_u8(np.uint8((2 * s + n) // (2 * n)), img, factors[1])
        elif op == 2:
            img = _blend_u8(_luma(img)[..., None].astype(np.uint8), img, factors[2])
        elif op != 3:
            raise ValueError("jitter_reference_u8: operation %r is none of 0 .. 3" % (op,))
    return img


JITTER_WORDS = ops.XBD_JITTER_WORDS        # int32 words of a row of dh_xbd_augment_jitter_u8's table


def jitter_table(jitter):
    """[n, 2, 8] int32 numpy table for dh_xbd_augment_jitter_u8 from one entry per sample, None or (pre, post) with each a
    draw_jitter_params result: row = (1, the three operations in applied order -- the drawn order without hue --, the float32
    bits of the three factors, 0); rows of samples without jitter stay 0.  None when every entry is None.  ValueError for an
    entry that is no pair, an order that is no permutation of 0 .. 3 or a factor that is not finite."""
    if all(j is None for j in jitter):
        return None
    table = np.zeros((len(jitter), 2, JITTER_WORDS), dtype=np.int32)
    for n, entry in enumerate(jitter):
        if entry is None:
            continue
        if len(entry) != 2:
            raise ValueError("jitter[%d]: None or a (pre, post) pair of draw_jitter_params results" % n)
        for im, (order, factors) in enumerate(entry):
            order = [int(o) for o in order]
            if sorted(order) != [0, 1, 2, 3]:
                raise ValueError("jitter[%d]: order %r is not a permutation of 0 .. 3" % (n, order))
            with np.errstate(over='ignore'):                 # a factor beyond float32 becomes inf and is refused below
                f = np.asarray([float(x) for x in factors], dtype=np.float32)
            if f.shape != (3,) or not all(math.isfinite(float(x)) for x in factors) or not np.isfinite(f).all():
                raise ValueError("jitter[%d]: factors %r are not three finite numbers" % (n, tuple(factors)))
            table[n, im, 0] = 1
            table[n, im, 1:4] = [o for o in order if o != 3]
            table[n, im, 4:7] = f.view(np.int32)
    return table


jitter_workspace_bytes = ops.xbd_augment_jitter_ws_bytes


def check_params(params, H, W, crop):
    """[n, 9] int32 tensor of parameter rows; ValueError for a crop window outside the image, a flag that is not 0 / 1 or a
    resize box that is empty or leaves the crop (the kernel trusts the rows)"""
    p = torch.as_tensor(params, dtype=torch.int32).reshape(-1, len(PARAM_FIELDS))
    if crop < 1 or crop > H or crop > W:
        raise ValueError("crop %d does not fit the %dx%d image" % (crop, H, W))
    for row in p.tolist():
        x0, y0, hf, vf, rs, top, left, bh, bw = row
        if not (0 <= x0 <= W - crop and 0 <= y0 <= H - crop):
            raise ValueError("crop window (%d, %d) + %d leaves the %dx%d image" % (x0, y0, crop, H, W))
        if hf not in (0, 1) or vf not in (0, 1) or rs not in (0, 1):
            raise ValueError("flags %r are not 0 / 1" % ([hf, vf, rs],))
        if rs and not (top >= 0 and left >= 0 and bh >= 1 and bw >= 1 and top + bh <= crop and left + bw <= crop):
            raise ValueError("resize box top %d left %d height %d width %d leaves the %d crop" % (top, left, bh, bw, crop))
    return p


def coef_table(params, crop):
    """[n, 2, crop, 4] int32 host tensor for dh_xbd_augment_u8 (axis 0 along x from the box width, axis 1 along y from its
    height), or None when no row of `params` (checked rows) has the resize flag; rows of samples without it stay 0"""
    rows = params.tolist()
    if not any(r[4] for r in rows):
        return None
    table = np.zeros((len(rows), 2, crop, 4), dtype=np.int32)
    for i, r in enumerate(rows):
        if r[4]:
            table[i, 0], table[i, 1] = resize_coeffs(r[8], crop), resize_coeffs(r[7], crop)
    return torch.from_numpy(table)


# ---- xBD_code/train_unettransformer.py's TrainData: vflip, rot90, shift_image, rotate_image, shift_channels ----

UNET_SKIPPED = tuple("%s_%s" % (op, im) for op in ("change_hsv", "clahe", "gauss_noise", "blur", "saturation", "brightness",
                                                   "contrast", "elastic") for im in ("pre", "post"))
UNET_MAX_SHIFT = 1 << 20   # |sx|, |sy| the kernel takes as they are (the script draws -320 .. 320)


def draw_unet_params(rng, H, W, crop):
    """One training sample's draws of xBD_code/train_unettransformer.py:109-253 from `rng` (a random.Random, or the `random`
    module), in the script's order and count, so the stream stands where the script's stands after the sample.  Returns
    (row, skipped).
    row: a dict of the operations that are built --
        x0, y0   the crop origin (randint(0, W - crop), randint(0, H - crop))
        vflip    0 / 1: random() > 0.5
        rot      k of np.rot90, 0 .. 3: randrange(4) if random() > 0.05
        shift    None or (sx, sy), two randint(-320, 320): if random() > 0.9
        warp     None or (angle, scale, (cx, cy)): if random() > 0.6 the centre crop // 2 + randint(-320, 320) twice, scale =
                 0.9 + random() * 0.2, angle = randint(0, 20) - 10; the script skips the warp, not its draws, when angle == 0
                 and scale == 1 (line 160)
        channels None or (image, b, g, r), image 1 = pre, 2 = post, three randint(-5, 5) in the script's (BGR) order: the
                 if / elif pair of lines 206-209, whose second random() is drawn only when the first test fails.
    skipped: the names (UNET_SKIPPED) of the operations the sample drew that a batch of these rows does NOT apply (draw_unet_colour
    keeps the values of those that are built, for make_unet_batch's `colour`; clahe and elastic are not built): change_hsv (three
    randint(-5, 5)), clahe, gauss_noise, blur, saturation / brightness / contrast (one random() each) and elastic, each
    with _pre or _post.  (gauss_noise and elastic draw their own numbers from numpy's generators, not from `random`.)"""
    row, drawn = _draw_unet_sample(rng, H, W, crop)
    return row, [name for name, _ in drawn]


def _draw_unet_sample(rng, H, W, crop):
    """the draws of draw_unet_params and draw_unet_colour: (row, drawn) with `drawn` the colour operations and elastic transforms
    the sample drew, in the script's order, as (name, value): the (h, s, v) of change_hsv, the factor 0.9 + random() * 0.2 of
    saturation / brightness / contrast, None for the others"""
    if crop > H or crop > W:
        raise ValueError("crop %d is larger than the %dx%d image" % (crop, H, W))
    row = {"x0": rng.randint(0, W - crop), "y0": rng.randint(0, H - crop), "vflip": 0, "rot": 0, "shift": None, "warp": None,
           "channels": None}
    drawn = []
    row["vflip"] = int(rng.random() > 0.5)
    if rng.random() > 0.05:
        row["rot"] = rng.randrange(4)
    if rng.random() > 0.9:
        row["shift"] = (rng.randint(-320, 320), rng.randint(-320, 320))
    if rng.random() > 0.6:
        centre = (crop // 2 + rng.randint(-320, 320), crop // 2 + rng.randint(-320, 320))
        scale = 0.9 + rng.random() * 0.2
        angle = rng.randint(0, 20) - 10
        if angle != 0 or scale != 1:
            row["warp"] = (angle, scale, centre)
    three = lambda: (rng.randint(-5, 5), rng.randint(-5, 5), rng.randint(-5, 5))
    if rng.random() > 0.985:
        row["channels"] = (1,) + three()
    elif rng.random() > 0.985:
        row["channels"] = (2,) + three()
    if rng.random() > 0.985:
        drawn.append(("change_hsv_pre", three()))
    elif rng.random() > 0.985:
        drawn.append(("change_hsv_post", three()))
    for im in ("pre", "post"):                                # lines 216-244: the same nested block for either image
        if rng.random() > 0.98:
            if rng.random() > 0.985:
                drawn.append(("clahe_" + im, None))
            elif rng.random() > 0.985:
                drawn.append(("gauss_noise_" + im, None))
            elif rng.random() > 0.985:
                drawn.append(("blur_" + im, None))
        elif rng.random() > 0.98:
            for op in ("saturation", "brightness", "contrast"):
                if rng.random() > 0.985:
                    drawn.append(("%s_%s" % (op, im), 0.9 + rng.random() * 0.2))
                    break
    for im in ("pre", "post"):
        if rng.random() > 0.983:
            drawn.append(("elastic_" + im, None))
    return row, drawn


def rotation_matrix(centre, angle, scale):
    """cv2.getRotationMatrix2D(centre, angle, scale) as a [2, 3] float64 array; cos / sin are this libm's"""
    a = angle * math.pi / 180.0
    alpha, beta = math.cos(a) * scale, math.sin(a) * scale
    cx, cy = float(centre[0]), float(centre[1])
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]], dtype=np.float64)


def shift_matrix(shift):
    """the matrix of the script's shift_image(img, (sx, sy))"""
    return np.array([[1.0, 0.0, float(shift[0])], [0.0, 1.0, float(shift[1])]], dtype=np.float64)


def warp_tables(M, width, height):
    """(adelta[width], bdelta[width], X0[height], Y0[height]) int64: the tables of cv2.warpAffine(img, M, (width, height),
    flags=INTER_LINEAR) without WARP_INVERSE_MAP (OpenCV 4.x up to 4.10, imgwarp.cpp).  M [2, 3] float64 is inverted as
    warpAffine does it -- D = M0 M4 - M1 M3, D = 1 / D if D != 0 else 0, A11 = M4 D, A22 = M0 D, M0 = A11, M1 *= -D, M3 *= -D,
    M4 = A22, b1 = -M0 M2 - M1 M5, b2 = -M3 M2 - M4 M5 --, then adelta[x] = rint(M0 x 1024), bdelta[x] = rint(M3 x 1024), X0[y] =
    rint((M1 y + M2) 1024) + 16, Y0[y] = rint((M4 y + M5) 1024) + 16, rint to even.  An output pixel reads the taps at ((X0[y] +
    adelta[x]) >> 10, (Y0[y] + bdelta[x]) >> 10); OpenCV saturates that origin to int16, which no warp of the script comes near:
    ValueError where an origin leaves -32768 .. 32767, or a table entry int32."""
    m = [float(v) for v in np.asarray(M, dtype=np.float64).reshape(6)]
    if not all(math.isfinite(v) for v in m):
        raise ValueError("warp_tables: the matrix %r is not finite" % (m,))
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0], m[1], m[3], m[4] = A11, m[1] * -D, m[3] * -D, A22
    b1, b2 = -m[0] * m[2] - m[1] * m[5], -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    x, y = np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        f = [m[0] * x * 1024, m[3] * x * 1024, (m[1] * y + m[2]) * 1024, (m[4] * y + m[5]) * 1024]
    if not all(np.isfinite(t).all() and (np.abs(t) < 2.0 ** 30).all() for t in f):
        raise ValueError("warp_tables: a table entry leaves the int32 range")
    ad, bd, X0, Y0 = (np.rint(t).astype(np.int64) for t in f)
    X0, Y0 = X0 + 16, Y0 + 16
    # rint is monotone, so the extremes of X0[y] + adelta[x] are sums of the tables' extremes
    for a, b in ((X0, ad), (Y0, bd)):
        if (int(a.min()) + int(b.min())) >> 10 < -32768 or (int(a.max()) + int(b.max())) >> 10 > 32767:
            raise ValueError("warp_tables: a tap origin leaves the int16 range (OpenCV saturates there; not built)")
    return ad, bd, X0, Y0


def _reflect101(p, n):
    """cv2.BORDER_REFLECT_101 of an integer array into 0 .. n - 1"""
    if n == 1:
        return np.zeros_like(p)
    m = 2 * (n - 1)
    p = np.mod(p, m)
    return np.where(p >= n, m - p, p)


def warp_affine_u8(img_u8, M):
    """cv2.warpAffine(img, M, (w, h), flags=cv2.INTER_LINEAR, borderMode=cv2.BORDER_REFLECT_101) of an [h, w] or [h, w, c]
    uint8 image, restated from OpenCV's fixed-point path for CV_8U (4.x up to 4.10; 4.11 and later take another path for
    linear warpAffine): with warp_tables' four tables, X = (X0[y] + adelta[x]) >> 5 and Y = (Y0[y] + bdelta[x]) >> 5; the four
    taps are (X >> 5, Y >> 5), its right, lower and lower-right neighbour, each coordinate reflected (101) into the image; fx =
    X & 31, fy = Y & 31; the weights are (32 - fx)(32 - fy) 32, fx (32 - fy) 32, (32 - fx) fy 32, fx fy 32 (OpenCV's 32 x 32
    bilinear table scaled by 32768; exact products here, the sum is 32768); byte = (sum w v + 16384) >> 15.  This restatement,
    not an installed OpenCV, is the byte contract of dh_xbd_augment_warp_u8; tests/test_xbd_unet_cpu.py holds it to identities
    that do not depend on it."""
    img = np.asarray(img_u8)
    if img.dtype != np.uint8 or img.ndim not in (2, 3):
        raise ValueError("warp_affine_u8: an [h, w] or [h, w, c] uint8 image, got %s %s" % (img.shape, img.dtype))
    h, w = img.shape[:2]
    ad, bd, X0, Y0 = warp_tables(M, w, h)
    X, Y = (X0[:, None] + ad[None, :]) >> 5, (Y0[:, None] + bd[None, :]) >> 5
    u0, v0, fx, fy = _reflect101(X >> 5, w), _reflect101(Y >> 5, h), X & 31, Y & 31
    u1, v1 = _reflect101((X >> 5) + 1, w), _reflect101((Y >> 5) + 1, h)
    a = img.astype(np.int64).reshape(h, w, -1)
    acc = (((32 - fx) * (32 - fy) * 32)[..., None] * a[v0, u0] + (fx * (32 - fy) * 32)[..., None] * a[v0, u1]
           + ((32 - fx) * fy * 32)[..., None] * a[v1, u0] + (fx * fy * 32)[..., None] * a[v1, u1])
    return ((acc + 16384) >> 15).astype(np.uint8).reshape(img.shape)


def check_unet_rows(rows, H, W, crop):
    """the rows of a batch (draw_unet_params' dicts) as they are; ValueError for a crop that does not fit the image, a window
    outside it, a flip that is not 0 / 1, a rot outside 0 .. 3, a shift that is no pair of integers within +-2^20, a warp that is
    no (angle, scale, (cx, cy)) of finite numbers, or channels that are no (1 or 2, b, g, r) with integer shifts within +-255"""
    if crop < 1 or crop > H or crop > W:
        raise ValueError("crop %d does not fit the %dx%d image" % (crop, H, W))
    is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
    for n, row in enumerate(rows):
        if not isinstance(row, dict) or set(row) != {"x0", "y0", "vflip", "rot", "shift", "warp", "channels"}:
            raise ValueError("rows[%d]: a dict of x0, y0, vflip, rot, shift, warp, channels (draw_unet_params), got %r" % (n, row))
        if not (is_int(row["x0"]) and is_int(row["y0"]) and 0 <= row["x0"] <= W - crop and 0 <= row["y0"] <= H - crop):
            raise ValueError("rows[%d]: crop window (%r, %r) + %d leaves the %dx%d image" % (n, row["x0"], row["y0"], crop, H, W))
        if row["vflip"] not in (0, 1) or not is_int(row["rot"]) or not 0 <= row["rot"] <= 3:
            raise ValueError("rows[%d]: vflip %r is not 0 / 1 or rot %r not 0 .. 3" % (n, row["vflip"], row["rot"]))
        s = row["shift"]
        if s is not None and not (len(s) == 2 and all(is_int(v) and abs(v) <= UNET_MAX_SHIFT for v in s)):
            raise ValueError("rows[%d]: shift %r is no pair of integers within +-%d" % (n, s, UNET_MAX_SHIFT))
        w = row["warp"]
        if w is not None:
            ok = len(w) == 3 and len(w[2]) == 2 and all(isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(v)
                                                         for v in (w[0], w[1]) + tuple(w[2]))
            if not ok:
                raise ValueError("rows[%d]: warp %r is no (angle, scale, (cx, cy)) of finite numbers" % (n, w))
        c = row["channels"]
        if c is not None and not (len(c) == 4 and c[0] in (1, 2) and all(is_int(v) and abs(v) <= 255 for v in c[1:])):
            raise ValueError("rows[%d]: channels %r is no (1 = pre or 2 = post, b, g, r) with shifts within +-255" % (n, c))
    return rows


def unet_param_rows(rows):
    """[n, 12] int32 numpy rows of dh_xbd_augment_warp_u8 from checked rows: x0, y0, vflip, rot, sx, sy, warp, chan, dR, dG, dB,
    0.  The pipeline stores RGB and the script's images are BGR: its b_shift goes to plane 2."""
    p = np.zeros((len(rows), ops.XBD_WARP_PARAM_WORDS), dtype=np.int32)
    for n, row in enumerate(rows):
        sx, sy = row["shift"] or (0, 0)
        chan, b, g, r = row["channels"] or (0, 0, 0, 0)
        p[n, :11] = [row["x0"], row["y0"], row["vflip"], row["rot"], sx, sy, int(row["warp"] is not None), chan, r, g, b]
    return p


def unet_warp_table(rows, crop):
    """[n, 4, crop] int32 numpy tables (adelta, bdelta, X0, Y0: warp_tables of rotation_matrix(centre, angle, scale)) for
    dh_xbd_augment_warp_u8, or None when no row warps; rows of samples without a warp stay 0 and are not read.  A shift needs
    no table: shift_image's matrix [[1, 0, sx], [0, 1, sy]] through the same tables is the single tap (x - sx, y - sy) at full
    weight, which the kernel takes from the row (tests/test_xbd_unet_cpu.py shows the two equal).  ValueError where a tap origin
    would leave the int16 range (OpenCV saturates there)."""
    if not any(row["warp"] is not None for row in rows):
        return None
    table = np.zeros((len(rows), 4, crop), dtype=np.int32)
    for n, row in enumerate(rows):
        if row["warp"] is not None:
            angle, scale, centre = row["warp"]
            table[n] = np.stack(warp_tables(rotation_matrix(centre, angle, scale), crop, crop))
    return table


def unet_reference_u8(pre, post, label, row, crop):
    """What TrainData.__getitem__ of xBD_code/train_unettransformer.py computes for one sample, line by line and through every
    intermediate image, on the operations that are built: pre, post [H, W, 3] uint8 RGB and label [H, W] uint8 -> (img uint8
    [6, crop, crop], the planes pre R G B, post R G B in front of preprocess_inputs; msk uint8 [5, crop, crop], 0 / 1, in front of
    the dilation of lines 265-273).  The crop; [::-1] if vflip; np.rot90(., rot); shift_image and rotate_image as
    warp_affine_u8 of shift_matrix / rotation_matrix, on both images and on the four 0 / 255 planes of (label == c), which are
    thresholded > 127 afterwards (channel 0 = any of them); shift_channels on the image that drew it (b to plane 2: RGB here).
    dh_xbd_augment_warp_u8 equals it byte for byte (tests/test_xbd_unet_gpu.py)."""
    x0, y0 = row["x0"], row["y0"]
    win = lambda a: a[y0:y0 + crop, x0:x0 + crop]
    planes = [win(np.asarray(pre)), win(np.asarray(post))] + [((win(np.asarray(label)) == c) * 255).astype(np.uint8) for c in (1, 2, 3, 4)]
    if row["vflip"]:
        planes = [a[::-1] for a in planes]
    planes = [np.ascontiguousarray(np.rot90(a, row["rot"])) for a in planes]
    if row["shift"] is not None:
        planes = [warp_affine_u8(a, shift_matrix(row["shift"])) for a in planes]
    if row["warp"] is not None:
        angle, scale, centre = row["warp"]
        planes = [warp_affine_u8(a, rotation_matrix(centre, angle, scale)) for a in planes]
    if row["channels"] is not None:
        chan, b, g, r = row["channels"]
        planes[chan - 1] = np.clip(planes[chan - 1].astype(np.int64) + np.array([r, g, b]), 0, 255).astype(np.uint8)
    img = np.concatenate([planes[0], planes[1]], axis=2).transpose(2, 0, 1)
    m = np.stack(planes[2:]) > 127
    msk = np.concatenate([m.any(axis=0, keepdims=True), m]).astype(np.uint8)
    return np.ascontiguousarray(img), msk


# ---- the script's colour stage (lines 211-244): change_hsv, gauss_noise, cv2.blur, saturation, brightness, contrast ----
# Images here are [h, w, 3] uint8 in the pipeline's R, G, B order; the script's are BGR, so its channel 0 is plane 2.

UNET_COLOUR_OPS = {"gauss_noise": 1, "blur": 2, "saturation": 3, "brightness": 4, "contrast": 5}    # the kernel's op codes
UNET_COLOUR_NOT_BUILT = ("clahe", "elastic")
HSV_SHIFT = 12


def _rgb_u8(img, who):
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("%s: an [h, w, 3] uint8 image, got %s %s" % (who, img.shape, img.dtype))
    return img


def _grey(img):
    """the script's _grayscale of an RGB image, float64 [h, w]: (0.114 b + 0.587 g) + 0.299 r, the order in which numpy sums
    the three products"""
    c = img.astype(np.float64)
    return (0.114 * c[..., 2] + 0.587 * c[..., 1]) + 0.299 * c[..., 0]


def _blend(img, gs, alpha):
    """the script's _blend: clip(img * alpha + (1 - alpha) * gs, 0, 255) in float64, truncated.  (A NaN, which only a factor
    near the end of the float64 range can give, becomes 0.)"""
    alpha = float(alpha)
    with np.errstate(over='ignore', invalid='ignore'):
        x = img.astype(np.float64) * alpha + (1 - alpha) * gs
    return np.clip(np.nan_to_num(x, nan=0.0, posinf=255.0, neginf=0.0), 0, 255).astype(np.uint8)


def saturation_u8(img, alpha):
    """utils.saturation: every channel blended with the pixel's grey"""
    img = _rgb_u8(img, "saturation_u8")
    return _blend(img, _grey(img)[..., None], alpha)


def brightness_u8(img, alpha):
    """utils.brightness: every channel blended with 0"""
    return _blend(_rgb_u8(img, "brightness_u8"), 0.0, alpha)


def contrast_mean(img):
    """the grey mean contrast blends with, DEFINED from the exact channel sums: ((0.114 Sb + 0.587 Sg) + 0.299 Sr) / (h w).  The
    script takes numpy's pairwise mean of the per-pixel greys, which may differ in the last bits; that moves a byte only where a
    blended value lies within about 1e-11 of an integer."""
    img = _rgb_u8(img, "contrast_mean")
    sr, sg, sb = (int(v) for v in img.reshape(-1, 3).astype(np.int64).sum(axis=0))
    return ((0.114 * float(sb) + 0.587 * float(sg)) + 0.299 * float(sr)) / float(img.shape[0] * img.shape[1])


def contrast_u8(img, alpha):
    """utils.contrast: every channel blended with contrast_mean"""
    img = _rgb_u8(img, "contrast_u8")
    return _blend(img, contrast_mean(img), alpha)


def draw_unet_noise(np_rng, S):
    """utils.gauss_noise's draw for an S x S image from `np_rng` (a np.random.RandomState, or the np.random module: the
    RandomState(k) stream is the one np.random.seed(k) gives): normal(30, 30 ** 0.5, (S, S, 3)) minus its minimum, truncated to
    uint8, in the script's (BGR) channel order"""
    g = np_rng.normal(30, 30 ** 0.5, (S, S, 3))
    return (g - g.min()).astype(np.uint8)


def gauss_noise_u8(img, noise_u8):
    """utils.gauss_noise with the noise already drawn (draw_unet_noise, BGR): min(img + noise, 255)"""
    img = _rgb_u8(img, "gauss_noise_u8")
    noise = np.asarray(noise_u8)
    if noise.dtype != np.uint8 or noise.shape != img.shape:
        raise ValueError("gauss_noise_u8: noise %s %s is not uint8 %s" % (noise.shape, noise.dtype, img.shape))
    return np.minimum(img.astype(np.int32) + noise[..., ::-1], 255).astype(np.uint8)


def blur_u8(img):
    """cv2.blur(img, (3, 3)): the 3 x 3 sum under BORDER_REFLECT_101, rounded to the nearest ninth as (2 sum + 9) // 18 (no sum
    of nine bytes over nine is a tie, and float64, float32 and OpenCV's fixed-point forms agree with it on every sum)"""
    img = _rgb_u8(img, "blur_u8")
    h, w = img.shape[:2]
    ys, xs = _reflect101(np.arange(-1, h + 1), h), _reflect101(np.arange(-1, w + 1), w)
    p = img.astype(np.int64)[ys][:, xs]
    total = sum(p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))
    return ((2 * total + 9) // 18).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _hsv_div_tables():
    i = np.arange(1, 256, dtype=np.float64)
    sdiv, hdiv = np.zeros(256, dtype=np.int64), np.zeros(256, dtype=np.int64)
    sdiv[1:] = np.rint((255 << HSV_SHIFT) / (1. * i))
    hdiv[1:] = np.rint((180 << HSV_SHIFT) / (6. * i))
    return sdiv, hdiv


def rgb_to_hsv_u8(img):
    """8-bit cv2.COLOR_BGR2HSV of an RGB-ordered image -> [h, w, 3] uint8 H (0 .. 179), S, V: OpenCV's integer path with
    hsv_shift = 12.  V = max, d = V - min, S = (d sdiv[V] + 2048) >> 12, H0 = g - b where V == r, else b - r + 2 d where V == g,
    else r - g + 4 d; H = (H0 hdiv[d] + 2048) >> 12 (arithmetic), plus 180 where negative."""
    c = _rgb_u8(img, "rgb_to_hsv_u8").astype(np.int64)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    sdiv, hdiv = _hsv_div_tables()
    V = np.maximum(np.maximum(b, g), r)
    d = V - np.minimum(np.minimum(b, g), r)
    S = (d * sdiv[V] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT
    H0 = np.where(V == r, g - b, np.where(V == g, b - r + 2 * d, r - g + 4 * d))
    H = (H0 * hdiv[d] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT
    H = H + np.where(H < 0, 180, 0)
    return np.clip(np.stack([H, S, V], axis=-1), 0, 255).astype(np.uint8)


_HSV_SECTORS = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])     # (b, g, r) of a sector


def hsv_to_rgb_u8(hsv):
    """8-bit cv2.COLOR_HSV2BGR into an RGB-ordered image: OpenCV's scalar float32 path, every product and difference rounded to
    float32 on its own (no fused multiply-add).  h = H float32(6 / 180), s = S float32(1 / 255), v = V float32(1 / 255); h =
    fmod(h, 6), k = floor(h), f = h - k (a sector outside 0 .. 5 is sector 0 with f = 0); t = [v, v (1 - s), v (1 - s f),
    v (1 - s (1 - f))] and (b, g, r) = t[_HSV_SECTORS[k]]; s == 0 gives b = g = r = v; a byte is rint(x 255) saturated."""
    c = np.asarray(hsv)
    if c.dtype != np.uint8 or c.ndim != 3 or c.shape[2] != 3:
        raise ValueError("hsv_to_rgb_u8: an [h, w, 3] uint8 image, got %s %s" % (c.shape, c.dtype))
    f32, one = np.float32, np.float32(1)
    h = c[..., 0].astype(f32) * f32(6 / 180)
    s, v = c[..., 1].astype(f32) * f32(1 / 255), c[..., 2].astype(f32) * f32(1 / 255)
    h = np.fmod(h, f32(6))
    k = np.floor(h)
    f = h - k
    sector = k.astype(np.int64)
    outside = (sector < 0) | (sector > 5)
    sector, f = np.where(outside, 0, sector), np.where(outside, f32(0), f)
    t = np.stack([v, v * (one - s), v * (one - s * f), v * (one - s * (one - f))])
    assert t.dtype == np.float32
    bgr = np.take_along_axis(t, np.moveaxis(_HSV_SECTORS[sector], -1, 0), axis=0)
    bgr = np.where((s == 0)[None], v[None], bgr)
    byte = np.clip(np.rint(bgr * f32(255)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.moveaxis(byte[::-1], 0, -1))


def change_hsv_u8(img, h, s, v):
    """utils.change_hsv: rgb_to_hsv_u8, the three shifts added and clipped to 0 .. 255 (hue as well, as the script does: a hue
    above 179 then wraps in the return, one below 0 stays 0), hsv_to_rgb_u8.  Written from OpenCV 4.x's scalar path; equality
    with a cv2 build has not been run, and a vectorised build may use fused multiply-adds and differ by one in a byte."""
    hsv = rgb_to_hsv_u8(img).astype(np.int64) + np.array([int(h), int(s), int(v)])
    return hsv_to_rgb_u8(np.clip(hsv, 0, 255).astype(np.uint8))


def draw_unet_colour(rng, H, W, crop, np_rng=None):
    """draw_unet_params with the colour operations kept: the same draws from `rng`, in the same order and count.  Returns
    (row, colour, skipped).  row: draw_unet_params' dict.  colour: {"hsv": None or (image, h, s, v), "pre": None or (op, value),
    "post": None or (op, value)}, image 1 = pre, 2 = post, op one of gauss_noise, blur, saturation, brightness, contrast (an
    image draws one of them at most) and value the factor 0.9 + random() * 0.2, the noise array (draw_unet_noise(np_rng, crop),
    drawn as the sample reaches it, pre before post) or None.  skipped: the names of what is NOT applied -- clahe_*, elastic_*
    and, when np_rng is None, gauss_noise_*."""
    row, drawn = _draw_unet_sample(rng, H, W, crop)
    colour, skipped = {"hsv": None, "pre": None, "post": None}, []
    for name, value in drawn:
        op, im = name.rsplit("_", 1)
        if op == "change_hsv":
            colour["hsv"] = (1 if im == "pre" else 2,) + tuple(value)
        elif op in UNET_COLOUR_NOT_BUILT or (op == "gauss_noise" and np_rng is None):
            skipped.append(name)
        else:
            colour[im] = (op, draw_unet_noise(np_rng, crop) if op == "gauss_noise" else value)
    return row, colour, skipped


def unet_colour_names(colour):
    """the operations of one sample's colour dict under draw_unet_params' names (change_hsv_pre, blur_post, ..)"""
    colour = colour or {}
    names = ["change_hsv_" + ("pre", "post")[colour["hsv"][0] - 1]] if colour.get("hsv") is not None else []
    return names + ["%s_%s" % (colour[im][0], im) for im in ("pre", "post") if colour.get(im) is not None]


def check_unet_colour(colour, crop):
    """the colour dicts of a batch (draw_unet_colour's; None or a missing key is no operation) as they are; ValueError for an
    entry that is no dict of hsv, pre, post, an hsv that is no (1 or 2, h, s, v) with integer shifts within +-255, an operation
    that is none of UNET_COLOUR_OPS, a factor that is no finite number or a noise array that is not [crop, crop, 3] uint8"""
    is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
    for n, col in enumerate(colour):
        if col is None:
            continue
        if not isinstance(col, dict) or not set(col) <= {"hsv", "pre", "post"}:
            raise ValueError("colour[%d]: None or a dict of hsv, pre, post (draw_unet_colour), got %r" % (n, col))
        c = col.get("hsv")
        if c is not None and not (isinstance(c, (tuple, list)) and len(c) == 4 and c[0] in (1, 2)
                                  and all(is_int(v) and abs(v) <= 255 for v in c[1:])):
            raise ValueError("colour[%d]: hsv %r is no (1 = pre or 2 = post, h, s, v) with shifts within +-255" % (n, c))
        for im in ("pre", "post"):
            e = col.get(im)
            if e is None:
                continue
            if not (isinstance(e, (tuple, list)) and len(e) == 2 and isinstance(e[0], str) and e[0] in UNET_COLOUR_OPS):
                raise ValueError("colour[%d]: %s %r is no (op, value) with op one of %s" % (n, im, e, sorted(UNET_COLOUR_OPS)))
            op, value = e
            if op == "gauss_noise":
                if not (isinstance(value, np.ndarray) and value.dtype == np.uint8 and value.shape == (crop, crop, 3)):
                    raise ValueError("colour[%d]: the noise of %s is no uint8 array [%d, %d, 3] (draw_unet_noise), got %s"
                                     % (n, im, crop, crop, getattr(value, "shape", type(value))))
            elif op == "blur":
                if value is not None:
                    raise ValueError("colour[%d]: blur of %s takes no value, got %r" % (n, im, value))
            elif not (isinstance(value, (int, float, np.integer, np.floating)) and not isinstance(value, bool)
                      and math.isfinite(value)):
                raise ValueError("colour[%d]: the %s factor %r of %s is no finite number" % (n, op, value, im))
    return colour


def unet_colour_jobs(colour, crop):
    """(jobs, noise) for dh_xbd_unet_colour_u8 from checked colour dicts: jobs [J, 12] int32 numpy, one row per (sample, image)
    that drew anything = sample, image (0 pre, 1 post), hsv flag, h, s, v, op code, the factor's float64 bits (low word, high
    word), the noise plane, 0, 0; noise [K, crop, crop, 3] uint8 (BGR, as drawn) or None.  (None, None) without a job."""
    rows, planes = [], []
    for n, col in enumerate(colour):
        col = col or {}
        for im in (0, 1):
            hsv = col.get("hsv")
            hsv = hsv if hsv is not None and hsv[0] == im + 1 else None
            e = col.get(("pre", "post")[im])
            if hsv is None and e is None:
                continue
            job = [n, im, int(hsv is not None)] + [int(v) for v in (hsv[1:] if hsv is not None else (0, 0, 0))] + [0] * 6
            if e is not None:
                job[6] = UNET_COLOUR_OPS[e[0]]
                if e[0] == "gauss_noise":
                    job[9] = len(planes)
                    planes.append(e[1])
                elif e[0] != "blur":
                    job[7:9] = np.array([float(e[1])], dtype=np.float64).view(np.int32).tolist()
            rows.append(job)
    if not rows:
        return None, None
    return np.array(rows, dtype=np.int32).reshape(-1, ops.XBD_COLOUR_JOB_WORDS), (np.stack(planes) if planes else None)


def unet_colour_reference_u8(img6_u8, colour):
    """The script's colour stage on one sample: img6_u8 [6, S, S] uint8 (unet_reference_u8's img, shift_channels inside) and the
    sample's colour dict -> [6, S, S] uint8.  Per image the script's order: change_hsv, then the one block operation it drew.
    clahe and the elastic transform are never applied.  dh_xbd_unet_colour_u8 equals it byte for byte
    (tests/test_xbd_unet_colour_gpu.py)."""
    img6 = np.asarray(img6_u8)
    if img6.dtype != np.uint8 or img6.ndim != 3 or img6.shape[0] != 6:
        raise ValueError("unet_colour_reference_u8: a [6, S, S] uint8 image pair, got %s %s" % (img6.shape, img6.dtype))
    check_unet_colour([colour], img6.shape[1])
    out, colour = img6.copy(), colour or {}
    for im in (0, 1):
        a = np.ascontiguousarray(img6[3 * im:3 * im + 3].transpose(1, 2, 0))
        hsv = colour.get("hsv")
        if hsv is not None and hsv[0] == im + 1:
            a = change_hsv_u8(a, *hsv[1:])
        e = colour.get(("pre", "post")[im])
        if e is not None:
            op, value = e
            a = {"gauss_noise": lambda: gauss_noise_u8(a, value), "blur": lambda: blur_u8(a),
                 "saturation": lambda: saturation_u8(a, value), "brightness": lambda: brightness_u8(a, value),
                 "contrast": lambda: contrast_u8(a, value)}[op]()
        out[3 * im:3 * im + 3] = a.transpose(2, 0, 1)
    return out


# ---- the scripts' training set: the 90 / 10 split and the oversampled index lists (train.py:397-429, ----
# ---- train_unettransformer.py:499-522) ----

def split_indices(n, test_size=0.1, seed=0):
    """(train_idxs0, val_idxs), int64 arrays: what sklearn.model_selection.train_test_split(np.arange(n), test_size=test_size,
    random_state=seed) returns, restated on numpy so that the product does not import sklearn: n_test = ceil(test_size * n),
    perm = np.random.RandomState(seed).permutation(n), validation = perm[:n_test], training = perm[n_test:].  Equal to sklearn
    on a committed fixture (tests/golden/xbd_split.json, written by tools/make_xbd_split_golden.py).  test_size is a fraction
    inside (0, 1), as the scripts pass it (sklearn also takes a count; this does not).  ValueError where sklearn raises one: a
    test_size outside (0, 1), n < 1, or a split that leaves no training sample (n = 1 is one)."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError("split_indices: n %r is no positive integer" % (n,))
    if isinstance(test_size, bool) or not isinstance(test_size, (float, np.floating)) or not 0 < test_size < 1:
        raise ValueError("split_indices: test_size %r is no fraction inside (0, 1)" % (test_size,))
    n_test = int(math.ceil(test_size * n))
    if n - n_test < 1:
        raise ValueError("split_indices: with n = %d and test_size = %r the training set is empty" % (n, test_size))
    perm = np.random.RandomState(seed).permutation(int(n)).astype(np.int64)
    return perm[n_test:], perm[:n_test]


def _class_rows(file_classes, who):
    fc = np.asarray(file_classes)
    if fc.ndim != 2 or fc.shape[1] != 4 or fc.dtype != np.bool_:
        raise ValueError("%s: file_classes is a bool array [n, 4] (GpuXbdPipeline.file_classes), got %s %s" % (who, fc.shape, fc.dtype))
    return fc


def _index_list(idxs, rows, who):
    idxs = [int(i) for i in idxs]
    if any(not 0 <= i < rows for i in idxs):
        raise ValueError("%s: an index of train_idxs0 lies outside the %d rows of file_classes" % (who, rows))
    return idxs


def unet_train_indices(file_classes, train_idxs0):
    """train_idxs of xBD_code/train_unettransformer.py:513-520, an int64 array: every index of train_idxs0 once, once more if
    the file holds any of classes 2 to 4 (file_classes[i, 1:].max()), once more if it holds class 4 (file_classes[i, 3]), in
    the order of train_idxs0.  file_classes: the bool [n, 4] array of GpuXbdPipeline.file_classes.  It draws nothing."""
    fc = _class_rows(file_classes, "unet_train_indices")
    out = []
    for i in _index_list(train_idxs0, len(fc), "unet_train_indices"):
        out += [i] * (1 + int(fc[i, 1:].any()) + int(fc[i, 3]))
    return np.asarray(out, dtype=np.int64)


def train_indices(file_classes, train_idxs0, rng, files=None):
    """(train_idxs, non_zero_bldg, non_zero_dmg) of xBD_code/train.py:414-425 (train_loc.py and train_GAN.py use the same
    lines): in the order of train_idxs0, an index is taken if its file holds any building -- a file without one is dropped --
    and taken (again) if `rng.random() > 0.5` and the file holds any of classes 2 to 4.  The draw is made for EVERY index,
    whether or not the file has damage (`and` evaluates it first), so afterwards `rng` (a random.Random, or the `random` module)
    stands len(train_idxs0) calls of random() further.  The two counters are the script's.
    files: None -- row i of file_classes is file i, the set the script MEANT.  With the list of the files' paths -- the script
    AS EXECUTED: train.py:405-406 appends a file's row a second time when its path contains 'AOI', so file_classes[i] there is
    the row of an earlier file for every i behind the first such path; `files` rebuilds that doubled table and indexes it as the
    script does.  The two are the same list when no path contains 'AOI'."""
    fc = _class_rows(file_classes, "train_indices")
    if files is not None:
        files = [str(f) for f in files]
        if len(files) != len(fc):
            raise ValueError("train_indices: %d files for %d rows of file_classes" % (len(files), len(fc)))
        fc = np.repeat(fc, [2 if 'AOI' in f else 1 for f in files], axis=0)
    out, non_zero_bldg, non_zero_dmg = [], 0, 0
    for i in _index_list(train_idxs0, len(fc), "train_indices"):
        if fc[i].any():
            out.append(i)
            non_zero_bldg += 1
        if rng.random() > 0.5 and fc[i, 1:].any():
            out.append(i)
            non_zero_dmg += 1
    return np.asarray(out, dtype=np.int64), non_zero_bldg, non_zero_dmg


def adapt_files(names):
    """the name filter of xBD_code/train_adapt.py:75 on a list of file names or paths, order kept: a name stays if it contains
    '_pre_disaster.png' and 'hurricane-michael' or 'AOI' -- xBD's hurricane-michael tiles plus the Ida-BD (AOI) tiles.  What the
    caller applies to `files` before GpuXbdPipeline.from_image_dir(..., files=...)."""
    return [f for f in names if ('_pre_disaster.png' in f) and (('hurricane-michael' in f) or ('AOI' in f))]


def adapt_train_indices(class_table, files, seed=0):
    """(train_idxs, val_idxs, n_xbd, n_train_aoi) of xBD_code/train_adapt.py:369-391 from a class table [n, 6] (GpuXbdPipeline.
    class_table) and the n file names: a file is kept if the sum of its non-zero label bytes, sum(c * table[:, c]), exceeds 500;
    the kept files are split by name into 'AOI' and the rest; split_indices(len(aoi), 0.15, seed) splits the AOI files;
    train_idxs = the rest, then the training AOI files, val_idxs = the held-out AOI files -- all as row indices of the table,
    int64 arrays.  ValueError if column 5 is non-zero (the sum of a byte above 4 cannot be read from the table), if the names do
    not match the rows, or where split_indices refuses the AOI files (none, or one)."""
    table = np.asarray(class_table)
    if table.ndim != 2 or table.shape[1] != 6 or table.dtype.kind not in "iu":
        raise ValueError("adapt_train_indices: class_table is an integer array [n, 6], got %s %s" % (table.shape, table.dtype))
    files = [str(f) for f in files]
    if len(files) != len(table):
        raise ValueError("adapt_train_indices: %d files for %d rows of class_table" % (len(files), len(table)))
    if table[:, 5].any():
        raise ValueError("adapt_train_indices: %d files hold label bytes above 4; their sum is not in the class table"
                         % int((table[:, 5] != 0).sum()))
    sums = (table[:, :5].astype(np.int64) * np.arange(5, dtype=np.int64)[None, :]).sum(axis=1)
    xbd_files, aoi_files = [], []
    for i, fn in enumerate(files):
        if sums[i] > 500:
            (aoi_files if 'AOI' in fn else xbd_files).append(i)
    tr, va = split_indices(len(aoi_files), 0.15, seed)
    train_aoi = [aoi_files[x] for x in tr]
    return (np.asarray(xbd_files + train_aoi, dtype=np.int64), np.asarray([aoi_files[x] for x in va], dtype=np.int64),
            len(xbd_files), len(train_aoi))


def epoch_order(n, indices):
    """the source indices of an epoch over n samples as a fresh list: every sample once (indices None), or `indices`, which may
    repeat; ValueError for an empty list or an index outside the samples"""
    if indices is None:
        return list(range(n))
    order = [int(i) for i in indices]
    if not order:
        raise ValueError("indices: an epoch over no sample")
    outside = [i for i in order if not 0 <= i < n]
    if outside:
        raise ValueError("indices: %d lies outside the %d samples" % (outside[0], n))
    return order


def _check_dilate(dilate, train=True):
    if isinstance(dilate, bool) or not isinstance(dilate, int) or (dilate != 0 and not (3 <= dilate <= ops.XBD_MORPH_MAX_K
                                                                                         and dilate % 2 == 1)):
        raise ValueError("dilate: %r is neither 0 nor an odd window of 3 .. %d" % (dilate, ops.XBD_MORPH_MAX_K))
    if dilate and not train:
        raise ValueError("dilate: the dilated masks are training targets; the reference's ValData does not dilate (train=False)")


class GpuXbdPipeline:
    def __init__(self, pre_u8, post_u8, pre_mask_u8, post_label_u8, files=None):
        """pre_u8, post_u8: [n_src, H, W, 3] uint8 device tensors; pre_mask_u8 (0 / 255) and post_label_u8 (0 .. 4):
        [n_src, H, W] uint8"""
        assert pre_u8.is_cuda and pre_u8.dtype == torch.uint8 and pre_u8.dim() == 4 and pre_u8.shape[-1] == 3
        assert post_u8.shape == pre_u8.shape and post_u8.dtype == torch.uint8
        for m in (pre_mask_u8, post_label_u8):
            assert m.dtype == torch.uint8 and m.shape == pre_u8.shape[:3]
        self.pre, self.post = pre_u8.contiguous(), post_u8.contiguous()
        self.pre_mask, self.post_label = pre_mask_u8.contiguous(), post_label_u8.contiguous()
        self.files = list(files) if files is not None else [str(i) for i in range(pre_u8.shape[0])]
        self._zero_lbl = None
        self._jitter_ws = None
        self.unet_skipped = collections.Counter()      # unet_batches: the drawn operations of the last epoch that are not built
        self.unet_applied = collections.Counter()      # ... and, with colour=True, the colour operations that were applied
        self._colour_ws = None
        self._class_table = None

    @classmethod
    def from_image_dir(cls, images_dir, device='cuda:0', files=None):
        """the reference's naming (xBD_code/train.py:79-83, 102-108): every `*_pre_disaster.png` of `images_dir` (or the
        paths in `files`), its post image under `_post_disaster`, and both masks under the same names with `/images/`
        replaced by `/masks/`"""
        if files is None:
            files = sorted(glob.glob(os.path.join(images_dir, '*_pre_disaster.png')))
        files = [str(f) for f in files]
        if not files:
            raise ValueError("no *_pre_disaster.png under %s" % images_dir)
        for fn in files:
            if '/images/' not in fn or '_pre_disaster' not in fn:
                raise ValueError("%s: expected .../images/..._pre_disaster.png (the masks are found by replacing /images/)" % fn)
        rgb = lambda fn: np.asarray(Image.open(fn).convert('RGB'))

        def gray(fn):
            m = np.asarray(Image.open(fn))
            if m.ndim != 2 or m.dtype != np.uint8:
                raise ValueError("%s: a mask is one 8-bit channel, got %s %s" % (fn, m.shape, m.dtype))
            return m

        post = lambda fn: fn.replace('_pre_disaster', '_post_disaster')
        mask = lambda fn: fn.replace('/images/', '/masks/')
        to = lambda xs: torch.from_numpy(np.ascontiguousarray(np.stack(xs))).to(device)
        return cls(to([rgb(f) for f in files]), to([rgb(post(f)) for f in files]), to([gray(mask(f)) for f in files]),
                   to([gray(mask(post(f))) for f in files]), files)

    def __len__(self):
        return self.pre.shape[0]

    def _sources(self, indices, allow_empty=False):
        """a batch's source indices as a list of ints; ValueError for one outside the samples (or for none at all)"""
        ind = [int(i) for i in indices]
        if (not ind and not allow_empty) or any(not 0 <= i < len(self) for i in ind):
            raise ValueError("indices %r outside the %d samples" % (list(indices), len(self)))
        return ind

    def _zero_label(self, n, crop):
        """the ONE zero `lbl_msk` every training batch of a shape shares (module docstring): read it, never write to it"""
        if self._zero_lbl is None or self._zero_lbl.shape != (n, crop, crop):
            self._zero_lbl = torch.zeros(n, crop, crop, dtype=torch.uint8, device=self.pre.device)
        return self._zero_lbl

    def _grown(self, attr, need):
        """the workspace kept under `attr`, replaced by a larger one when it holds fewer than `need` bytes"""
        ws = getattr(self, attr, None)
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=self.pre.device)
            setattr(self, attr, ws)
        return ws

    def _batch(self, img, msk, lbl, ind):
        return {'img': img, 'msk': msk, 'lbl_msk': lbl, 'fn': [self.files[i] for i in ind]}

    def _epoch_chunks(self, batch_size, crop, train, rng, indices, drop_last):
        """the source indices of every batch of one epoch, what `batches`, `adapt_batches` and `unet_batches` share: epoch_order
        of `indices`, shuffled with `rng` in a training epoch and nothing drawn otherwise, in slices of batch_size; drop_last
        stops in front of a short one.  ValueError, at the first next(), for a validation crop that is not the whole image, a
        crop that does not fit, an empty or outside index list, or a training epoch without `rng`."""
        _, H, W, _ = self.pre.shape
        if not train and not crop == H == W:
            raise ValueError("a validation epoch takes whole images: crop %d is not the %dx%d image" % (crop, H, W))
        if not 1 <= crop <= min(H, W):
            raise ValueError("crop: %r does not fit the %dx%d images" % (crop, H, W))
        order = epoch_order(len(self), indices)
        if train:
            if rng is None:
                raise ValueError("a training epoch draws from `rng` (a random.Random)")
            rng.shuffle(order)
        for s in range(0, len(order), batch_size):
            ind = order[s:s + batch_size]
            if drop_last and len(ind) < batch_size:
                break
            yield ind

    def class_table(self):
        """[len(self), 6] int64 host array, read-only: how many pixels of every resident post-disaster label equal 0, 1, 2, 3, 4
        or lie above 4 (ops.XBD_CLASS_COLUMNS) -- ops.xbd_class_table on the resident stack, one launch and one device-to-host
        read.  Kept on the pipeline: a second call returns the same array without a launch (the sources do not change)."""
        if self._class_table is None:
            table = ops.xbd_class_table(self.post_label).cpu().numpy().astype(np.int64)
            table.setflags(write=False)
            self._class_table = table
        return self._class_table

    def file_classes(self):
        """the bool [len(self), 4] array the training scripts call file_classes (train.py:397-407,
        train_unettransformer.py:499-506): fl[c - 1] = c in msk1 for c = 1 .. 4, here class_table()[:, 1:5] > 0 -- no label
        is opened or copied back.  (train.py's table holds the rows of 'AOI' paths twice; train_indices' `files` restates
        that.)"""
        return self.class_table()[:, 1:5] > 0

    def unet_trainset(self, seed=0):
        """(train_idxs, val_idxs) of xBD_code/train_unettransformer.py:499-520 from this one folder: file_classes from the
        resident labels, split_indices(len(self), 0.1, seed), and unet_train_indices on the training part -- train_idxs is
        already oversampled and repeats indices; val_idxs is the held-out tenth.  Feed them to unet_batches(..., indices=
        train_idxs, drop_last=True) and models.xbd.unet_val_batches(self, ..., indices=val_idxs).  No image is copied.  (The
        script then seeds `random` and numpy with seed + 321: the epochs' rng is the caller's.)"""
        train_idxs0, val_idxs = split_indices(len(self), 0.1, seed)
        return unet_train_indices(self.file_classes(), train_idxs0), val_idxs

    def trainset(self, seed=0, rng=None):
        """(train_idxs, val_idxs, rng) of xBD_code/train.py:397-429 from this one folder, the script as executed:
        file_classes from the resident labels, split_indices(len(self), 0.1, seed), then train_indices with `files=self.files`
        -- so the doubled rows of paths that contain 'AOI' (train.py:405-406) are reproduced; call train_indices(
        self.file_classes(), train_idxs0, rng) for the set the script meant.  rng defaults to random.Random(seed + 321), the
        state the script's random.seed(seed + 321) leaves, and is returned so that the caller's epochs go on drawing from it as
        the script's loader does.  Prints the script's counts line: non_zero_bldg non_zero_dmg len(train_idxs) len(val_idxs)."""
        if rng is None:
            rng = random.Random(seed + 321)
        train_idxs0, val_idxs = split_indices(len(self), 0.1, seed)
        train_idxs, non_zero_bldg, non_zero_dmg = train_indices(self.file_classes(), train_idxs0, rng, self.files)
        print(non_zero_bldg, non_zero_dmg, len(train_idxs), len(val_idxs))
        return train_idxs, val_idxs, rng

    def make_batch(self, indices, crop, params=None, train=True, jitter=None, dilate=0):
        """indices: source samples of the batch; params: one row per sample in PARAM_FIELDS order (draw_train_params), or None
        for the crop at the origin without augmentation.  train=False builds ValData's masks (msk[0] from the pre mask,
        lbl_msk = label - 1 on the buildings); the reference validates whole images, i.e. crop == H == W and params=None.
        Returns {'img': fp32 [n, 6, crop, crop], 'msk': uint8 [n, 5, crop, crop], 'lbl_msk': uint8 [n, crop, crop], 'fn'}.
        `lbl_msk` of a training batch is all zeros (module docstring) and is ONE tensor shared by every training batch of
        that shape: read it, never write to it in place.
        jitter: one entry per sample, None or the pair (pre, post) of draw_jitter_params results applied to the sample's two
        images (ColorJitter, train.py:139; training batches only).  None, or every entry None, is dh_xbd_augment_u8 exactly
        as without the argument; otherwise one call of dh_xbd_augment_jitter_u8 (ops.xbd_augment makes either).
        dilate: 0 (default) is the batch as above, with the same launches and the same bytes.  An odd k of 3 .. 31 (training
        batches only; 5 is the script's value) gives the targets xBD_code/train_unettransformer.py trains on: after the augment
        launch ONE more launch (ops.xbd_msk_dilate) replaces `msk` by the four damage channels dilated with square(k) and put
        through the priority rule of its lines 262-273 (class 2 over 3 over 4, any of them over 1; channel 0 = any).  The
        dilation acts on the augmented crop, as in the script, which dilates after its crop and flips: a building just outside
        the crop window contributes nothing.  `img`, `lbl_msk` (still all zeros: channel 0 is set wherever another is) and `fn`
        are untouched.  What this is NOT: that script's geometry -- the switch gives train.py's geometry with
        train_unettransformer.py's targets; make_unet_batch is the script's own loader (rot90, reflect-101 shift,
        cv2.warpAffine rotate / scale, shift_channels).  The script's ValData does not dilate: train=False is refused.
        ValueError for a crop larger than the image, a window outside it, a resize box that leaves the crop, jitter in a
        validation batch, jitter rows that do not match the samples, an order that is no permutation, a factor that is not
        finite, a `dilate` that is not 0 or an odd integer of 3 .. 31, or `dilate` in a validation batch."""
        n = len(indices)
        _check_dilate(dilate, train)
        table = None
        if jitter is not None:
            if not train:
                raise ValueError("jitter: ColorJitter belongs to the training augmentation (train=False)")
            if len(jitter) != n:
                raise ValueError("jitter: %d entries for %d samples" % (len(jitter), n))
            table = jitter_table(jitter)
        _, H, W, _ = self.pre.shape
        if params is None:
            params = [[0, 0, 0, 0, 0, 0, 0, crop, crop]] * n
        p = check_params(params, H, W, crop)
        if p.shape[0] != n:
            raise ValueError("params: %d rows for %d samples" % (p.shape[0], n))
        ind = self._sources(indices, allow_empty=True)          # (an empty batch is the entry's to refuse)
        coef = coef_table(p, crop)
        dev = self.pre.device
        idx = torch.as_tensor(ind, dtype=torch.int32).to(dev)
        p = p.contiguous().to(dev)
        coef = coef.to(dev) if coef is not None else None
        # the jitter table is host memory: the entry checks it and copies it into the workspace before it returns
        ws = self._grown('_jitter_ws', jitter_workspace_bytes(n, crop)) if table is not None else None
        img, msk, lbl = ops.xbd_augment(self.pre, self.post, self.pre_mask, self.post_label, idx, p, coef, crop, train, table,
                                        out_lbl=self._zero_label(n, crop) if train else None, ws=ws)
        if dilate:
            msk = ops.xbd_msk_dilate(msk, dilate)
        return self._batch(img, msk, lbl, ind)

    def batches(self, batch_size, crop, train=True, rng=None, jitter_gen=None, dilate=0, indices=None, drop_last=False):
        """one epoch.  train: `rng` (a random.Random) shuffles the samples, then every sample draws its parameters with
        draw_train_params, in batch order (the reference's DataLoader shuffles with torch's generator and draws in its worker
        processes: the order of the samples is this loader's own, a sample's draws are the reference's).  Otherwise the
        samples in order with ValData's masks, as ValData takes them: whole images, so `crop` must be the (square) image
        size -- ValueError otherwise; a validation crop is make_batch(..., params, train=False).
        jitter_gen: a torch.Generator; every training sample whose draw_train_params flag is set then draws its ColorJitter
        parameters from it (draw_jitter_params, pre then post, in sample order) and gets them applied.  None: no ColorJitter
        and no draw from any torch generator.
        dilate: make_batch's, for every batch of a training epoch (0: off; ValueError with train=False).  It draws nothing.
        indices: None -- every sample once -- or the epoch's source indices, which may repeat (trainset / unet_trainset's
        oversampled train_idxs, or val_idxs): a training epoch shuffles a copy of the list with `rng`, a validation epoch takes
        it in the order given.  A repeated index reads the same resident source again; nothing is copied.  ValueError, before
        any launch, for an empty list or an index outside the samples.
        drop_last: stop in front of a batch shorter than batch_size, as the scripts' DataLoader(drop_last=True): the epoch then
        has len(indices) // batch_size batches, their steps_per_epoch."""
        _, H, W, _ = self.pre.shape
        _check_dilate(dilate, train)
        for ind in self._epoch_chunks(batch_size, crop, train, rng, indices, drop_last):
            if not train:
                yield self.make_batch(ind, crop, None, train)
                continue
            params, jitter = [], []
            for _ in ind:
                row, flag = draw_train_params(rng, H, W, crop)
                params.append(row)
                jitter.append((draw_jitter_params(jitter_gen), draw_jitter_params(jitter_gen))
                              if flag and jitter_gen is not None else None)
            yield self.make_batch(ind, crop, params, train, jitter if jitter_gen is not None else None, dilate)

    def adapt_trainset(self, seed=0):
        """(train_idxs, val_idxs) of xBD_code/train_adapt.py:72-78, 369-391 from this one folder (adapt_train_indices on the
        resident class table and self.files): the files whose non-zero label bytes sum above 500, the AOI ones split 85 / 15 with
        split_indices(len(aoi), 0.15, seed); train_idxs = the other files, then the training AOI files; val_idxs = the held-out
        AOI files.  Indices into this pipeline: feed them to adapt_batches(..., indices=train_idxs, drop_last=True) and
        adapt_batches(..., train=False, indices=val_idxs).  The name filter of line 75 is adapt_files(), applied by the caller
        to `files` before the pipeline is built.  Prints the script's two count lines.  Host code on the class table: no image
        is copied, no label is opened.  (The script then seeds `random` and numpy with seed + 321: the epochs' rng is the
        caller's.)"""
        train_idxs, val_idxs, n_xbd, n_train_aoi = adapt_train_indices(self.class_table(), self.files, seed)
        print(n_xbd)
        print(n_train_aoi, len(train_idxs))
        return train_idxs, val_idxs

    def make_adapt_batch(self, indices, crop, origins=None, train=True):
        """A batch of xBD_code/train_adapt.py's TrainData (lines 97-184; train=True) or ValData (196-245), the Ida-BD adaptation
        of the FOUR-output net, in ONE launch (ops.xbd_adapt_batch, dh_xbd_adapt_batch_u8).  indices: the source samples;
        origins: one (x0, y0) per sample, the corner of its crop x crop window, or None for (0, 0) -- the script's crop is the
        whole 1024 tile, where (0, 0) is the only origin.  Returns {'img': fp32 [n, 6, crop, crop] = x / 127 - 1, 'msk': uint8
        [n, 4, crop, crop], 'lbl_msk': uint8 [n, crop, crop], 'fn'}.  The mask planes are a pure function of the post label
        byte l: m1 = (l == 1), m2 = (l == 2), m3 = (l in (3, 4)) -- destroyed merged with class 3 --, and m0 = m1 | m2 | m3 for a
        training batch, whose pre-disaster mask is NOT read (line 165 clears channel 0, line 172 sets the union), or
        pre_mask > 127 for a validation batch; lbl_msk = argmax(m1, m2, m3), 0 .. 2.  A label byte above 4 sets no plane.  The
        script's priority lines 170-171 (m1 cleared where m2 or m3 is set, m3 where m2 is) cannot fire on planes cut from one
        byte, which equals at most one of 1, 2 and 3 / 4; they would matter behind a dilation, which the script has commented
        out.  The training augmentation of lines 115-146 sits inside a string literal: it is not executed and not built.
        ValueError for a crop that does not fit, origins that do not match the samples or leave the image, or indices outside
        the samples."""
        n = len(indices)
        _, H, W, _ = self.pre.shape
        if isinstance(crop, bool) or not isinstance(crop, (int, np.integer)) or not 1 <= crop <= min(H, W):
            raise ValueError("crop: %r does not fit the %dx%d images" % (crop, H, W))
        crop = int(crop)
        ind = self._sources(indices)
        dev = self.pre.device
        org = None
        if origins is not None:
            rows = [tuple(int(v) for v in o) for o in origins]
            if len(rows) != n or any(len(o) != 2 for o in rows):
                raise ValueError("origins: %d rows for %d samples, each (x0, y0)" % (len(rows), n))
            if any(not (0 <= x0 <= W - crop and 0 <= y0 <= H - crop) for x0, y0 in rows):
                raise ValueError("origins: a %dx%d window at one of %r leaves the %dx%d image" % (crop, crop, rows, H, W))
            org = torch.as_tensor(rows, dtype=torch.int32).reshape(n, 2).to(dev)
        idx = torch.as_tensor(ind, dtype=torch.int32).to(dev)
        return self._batch(*ops.xbd_adapt_batch(self.pre, self.post, self.pre_mask, self.post_label, idx, org, crop, train), ind)

    def adapt_batches(self, batch_size, crop, train=True, rng=None, indices=None, drop_last=False):
        """one epoch of xBD_code/train_adapt.py's loader, make_adapt_batch's dicts.  train: `rng` (a random.Random) shuffles the
        samples (the sample order is this loader's own, as in `batches`), then every sample draws x0 = rng.randint(0, W - crop)
        and y0 = rng.randint(0, H - crop), in that order: the two draws of lines 108-109, consumed even at the script's crop of
        the whole tile, where both are 0 -- a shared `rng` stays in step with the script.  Nothing else is drawn.  Otherwise
        (ValData) the samples in order, whole images: `crop` must be the (square) image size, ValueError otherwise.
        indices, drop_last: as in `batches` -- the script's epochs are adapt_batches(1, 1024, True, rng, train_idxs,
        drop_last=True) and adapt_batches(1, 1024, False, indices=val_idxs) with adapt_trainset's lists."""
        _, H, W, _ = self.pre.shape
        for ind in self._epoch_chunks(batch_size, crop, train, rng, indices, drop_last):
            origins = [(rng.randint(0, W - crop), rng.randint(0, H - crop)) for _ in ind] if train else None     # x0, then y0
            yield self.make_adapt_batch(ind, crop, origins, train)

    def make_unet_batch(self, indices, crop, rows, dilate=5, colour=None):
        """A training batch of xBD_code/train_unettransformer.py's TrainData, the script that trains DAHiTra proper: rows is one
        draw_unet_params dict per sample (crop, vflip, rot90, reflect-101 shift, cv2.warpAffine rotate / scale, shift_channels),
        applied in ONE launch (ops.xbd_augment_warp, dh_xbd_augment_warp_u8), byte for byte unet_reference_u8.  dilate: the
        script's square(5) dilation and priority rule of lines 262-273 on top (ops.xbd_msk_dilate, one more launch; any odd
        window of 3 .. 31), 0 for the undilated channels.  Returns make_batch's dict; `lbl_msk` is the shared zero tensor, as
        the script's argmax gives it (channel 0 is set wherever another one is): read it, never write to it.
        colour: None, or one draw_unet_colour dict (or None) per sample: the script's colour stage of lines 211-244 --
        change_hsv, then gauss_noise, cv2.blur, saturation, brightness or contrast -- on the images the warp launch wrote, in
        place, in two more launches whatever the jobs (ops.xbd_unet_colour, dh_xbd_unet_colour_u8), byte for byte
        unet_colour_reference_u8.  None, or dicts that hold no operation, is the batch as without the argument: the same bytes
        and the same launches.  The limits of that contract: change_hsv restates OpenCV 4.x's scalar 8-bit path and equality
        with a cv2 build has not been run (a vectorised build may fuse multiply-adds and differ by one in a byte); contrast's
        mean is defined from the exact channel sums (contrast_mean), which can move a byte against numpy's pairwise mean only
        where a blended value lies within about 1e-11 of an integer.  Not built and never applied: clahe and imgaug's elastic
        transform, which draw_unet_colour reports as skipped.  The script's ValData is
        make_batch(ind, 256, [[512, 512, 0, 0, 0, 0, 0, 256, 256]] * len(ind), train=False) as it stands.
        ValueError for rows that do not fit (check_unet_rows), a warp whose taps leave the int16 range, indices outside the
        samples, a `dilate` that is not 0 or an odd integer of 3 .. 31, or colour entries that do not match the samples or do
        not fit (check_unet_colour)."""
        n = len(indices)
        _check_dilate(dilate)
        _, H, W, _ = self.pre.shape
        rows = check_unet_rows(list(rows), H, W, crop)
        if len(rows) != n:
            raise ValueError("rows: %d rows for %d samples" % (len(rows), n))
        ind = self._sources(indices)
        jobs = noise = None
        if colour is not None:
            colour = check_unet_colour(list(colour), crop)
            if len(colour) != n:
                raise ValueError("colour: %d entries for %d samples" % (len(colour), n))
            jobs, noise = unet_colour_jobs(colour, crop)
        tab = unet_warp_table(rows, crop)
        dev = self.pre.device
        idx = torch.as_tensor(ind, dtype=torch.int32).to(dev)
        p = torch.from_numpy(unet_param_rows(rows)).to(dev)
        tab = torch.from_numpy(tab).to(dev) if tab is not None else None
        img, msk = ops.xbd_augment_warp(self.pre, self.post, self.post_label, idx, p, tab, crop)
        if jobs is not None:
            ops.xbd_unet_colour(img, torch.from_numpy(jobs).to(dev), torch.from_numpy(noise).to(dev) if noise is not None else None,
                                ws=self._grown('_colour_ws', ops.xbd_unet_colour_ws_bytes(len(jobs), crop)))
        lbl = self._zero_label(n, crop)
        if dilate:
            msk = ops.xbd_msk_dilate(msk, dilate)
        return self._batch(img, msk, lbl, ind)

    def unet_batches(self, batch_size, crop, rng, dilate=5, colour=False, np_rng=None, indices=None, drop_last=False):
        """one training epoch of xBD_code/train_unettransformer.py's loader: `rng` (a random.Random) shuffles the samples, then
        every sample draws with draw_unet_params, in batch order (the sample order is this loader's own, as in `batches`; a
        sample's draws are the script's).  Yields make_unet_batch's dicts.  `self.unet_skipped` counts, over the epoch, the
        drawn operations that are not applied (collections.Counter of draw_unet_params' names).
        colour=True draws with draw_unet_colour instead -- the same stream -- and applies the colour operations
        (make_unet_batch's `colour`); `self.unet_applied` counts them under the same names.  np_rng: the np.random.RandomState
        gauss_noise draws from (the script draws from numpy's global legacy generator); without one gauss_noise stays skipped.
        indices, drop_last: as in `batches` -- the script's epoch is unet_batches(16, 256, rng, indices=train_idxs,
        drop_last=True) with unet_trainset's train_idxs."""
        _, H, W, _ = self.pre.shape
        self.unet_skipped = collections.Counter()
        self.unet_applied = collections.Counter()
        for ind in self._epoch_chunks(batch_size, crop, True, rng, indices, drop_last):
            rows, colours = [], []
            for _ in ind:
                if colour:
                    row, col, skipped = draw_unet_colour(rng, H, W, crop, np_rng)
                    colours.append(col)
                    self.unet_applied.update(unet_colour_names(col))
                else:
                    row, skipped = draw_unet_params(rng, H, W, crop)
                rows.append(row)
                self.unet_skipped.update(skipped)
            yield self.make_unet_batch(ind, crop, rows, dilate, colours if colour else None)
