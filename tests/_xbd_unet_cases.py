"""Cases shared by test_xbd_unet_cpu.py and test_xbd_unet_gpu.py: the loader of xBD_code/train_unettransformer.py on the device
(dh_xbd_augment_warp_u8, datasets/xbd_pipeline.make_unet_batch).

    sources          seeded pre / post images and a label with class rectangles and a per-pixel checkerboard of classes, where the
                     warp's weight-1/2 ties occur
    param_rows       the parameter rows every shape is tested with: each operation alone, and all composed
    composed_u8      the kernel's ONE gather in numpy -- four taps, each an index chain back to the source -- which the CPU test
                     holds against unet_reference_u8's explicit intermediate images
    script_draws     the script's draws, line by line, with the branches it took
"""
import numpy as np

from dahitra_amd.datasets import xbd_pipeline as X


def sources(n, H, W, seed=7):
    """(pre, post [n, H, W, 3] uint8, pre_mask [n, H, W] 0 / 255, label [n, H, W] 0 .. 4).  The label: 5 x 7 rectangles of random
    classes, and in the upper left quarter a checkerboard that changes class at every pixel in both directions (1 / 2 on the
    even rows of 2 x 2 cells, 3 / 4 / 0 below), so that class boundaries lie on every pixel row and column of the region."""
    rng = np.random.RandomState(seed)
    pre = rng.randint(0, 256, size=(n, H, W, 3)).astype(np.uint8)
    post = rng.randint(0, 256, size=(n, H, W, 3)).astype(np.uint8)
    y, x = np.mgrid[:H, :W]
    cls = rng.randint(0, 5, size=(n, H // 5 + 1, W // 7 + 1))
    label = cls[:, y // 5, x // 7]
    board = np.where((y // 8) % 2 == 0, 1 + (x + y) % 2, np.array([3, 4, 0])[(x + 2 * y) % 3])
    region = (y < (H + 1) // 2) & (x < (W + 1) // 2)
    label = np.where(region[None], board[None], label).astype(np.uint8)
    pre_mask = ((label > 0) * 255).astype(np.uint8)
    return pre, post, pre_mask, label


def row(x0=0, y0=0, vflip=0, rot=0, shift=None, warp=None, channels=None):
    return {"x0": x0, "y0": y0, "vflip": vflip, "rot": rot, "shift": shift, "warp": warp, "channels": channels}


def shifts(S):
    return [(0, 0), (1, 0), (-1, 3), (S - 1, -(S - 1)), (S, -S), (320, -320), (-317, 5)]


ANGLES = (-10, -1, 0, 1, 10)
SCALES = (0.9, 1, 1.0999)
CENTRE_OFFSETS = ((0, 0), (320, -320), (-320, 320))


def warps(S):
    return [(a, s, (S // 2 + dx, S // 2 + dy)) for a in ANGLES for s in SCALES for dx, dy in CENTRE_OFFSETS
            if a != 0 or s != 1]                                    # angle 0 at scale 1 is no warp: the script skips it


def param_rows(S, H, W):
    """every operation alone, then all composed; the crop origin is the far corner (not 0 wherever the source is larger)"""
    x0, y0 = W - S, H - S
    rows = [row(x0, y0, vflip=v, rot=k) for v in (0, 1) for k in range(4)]
    rows += [row(x0, y0, shift=s) for s in shifts(S)]
    rows += [row(x0, y0, warp=w) for w in warps(S)]
    rows += [row(x0, y0, channels=c) for c in ((1, 5, -5, 5), (2, -5, 5, -5), (1, -5, -5, -5), (2, 5, 5, 5))]
    ws, ss = warps(S), shifts(S)
    for i, (v, k) in enumerate((v, k) for v in (0, 1) for k in range(4)):
        rows.append(row((x0 * (i + 1)) // 8, (y0 * (8 - i)) // 8, v, k, ss[1 + i % 6], ws[(5 * i + 3) % len(ws)],
                        (1 + i % 2, 5 - i, i - 4, (-5) ** (i % 2))))
    return rows


def normalise(img_u8):
    """preprocess_inputs: x /= 127, x -= 1 in float32"""
    x = img_u8.astype(np.float32)
    x /= np.float32(127)
    x -= np.float32(1)
    return x


def composed_u8(pre, post, label, r, crop):
    """the kernel's statement: one gather.  Tap -> reflect-101 -> minus the shift -> reflect-101 -> undo rot90 -> undo vflip ->
    plus the crop origin; a sample without a warp is the single tap (x, y) at weight 32768."""
    S = crop
    y, x = np.mgrid[:S, :S]
    if r["warp"] is not None:
        angle, scale, centre = r["warp"]
        ad, bd, X0, Y0 = X.warp_tables(X.rotation_matrix(centre, angle, scale), S, S)
        XX, YY = (X0[:, None] + ad[None, :]) >> 5, (Y0[:, None] + bd[None, :]) >> 5
        u, v, fx, fy = XX >> 5, YY >> 5, XX & 31, YY & 31
        taps = [(u, v, (32 - fx) * (32 - fy) * 32), (u + 1, v, fx * (32 - fy) * 32), (u, v + 1, (32 - fx) * fy * 32),
                (u + 1, v + 1, fx * fy * 32)]
    else:
        taps = [(x, y, np.full((S, S), 32768))]
    sx, sy = r["shift"] or (0, 0)
    acc = np.zeros((S, S, 6), dtype=np.int64)
    wc = np.zeros((4, S, S), dtype=np.int64)
    for u, v, w in taps:
        c = X._reflect101(X._reflect101(u, S) - sx, S)
        rr = X._reflect101(X._reflect101(v, S) - sy, S)
        a, b = [(rr, c), (c, S - 1 - rr), (S - 1 - rr, S - 1 - c), (S - 1 - c, rr)][r["rot"]]
        if r["vflip"]:
            a = S - 1 - a
        yy, xx = r["y0"] + a, r["x0"] + b
        acc[..., :3] += w[..., None] * pre[yy, xx].astype(np.int64)
        acc[..., 3:] += w[..., None] * post[yy, xx].astype(np.int64)
        for k in range(4):
            wc[k] += np.where(label[yy, xx] == k + 1, w, 0)
    img = (acc + 16384) >> 15
    if r["channels"] is not None:
        chan, bb, g, rd = r["channels"]
        sl = slice(3 * (chan - 1), 3 * chan)
        img[..., sl] = np.clip(img[..., sl] + np.array([rd, g, bb]), 0, 255)
    m = ((255 * wc + 16384) >> 15) > 127
    msk = np.concatenate([m.any(axis=0, keepdims=True), m]).astype(np.uint8)
    return np.ascontiguousarray(img.astype(np.uint8).transpose(2, 0, 1)), msk


def script_draws(rng, H, W, crop):
    """TrainData.__getitem__'s calls of `random`, xBD_code/train_unettransformer.py:109-253, in the script's order, with the
    branches taken (a set of names) -> (row, skipped, branches)"""
    took = set()
    skipped = []
    r = row()
    r["x0"] = rng.randint(0, W - crop)                                          # 109
    r["y0"] = rng.randint(0, H - crop)                                          # 110
    if rng.random() > 0.5:                                                      # 126
        r["vflip"] = 1
        took.add("vflip")
    else:
        took.add("no vflip")
    if rng.random() > 0.05:                                                     # 135
        r["rot"] = rng.randrange(4)
        took.add("rot %d" % r["rot"])
    else:
        took.add("no rot")
    if rng.random() > 0.9:                                                      # 146
        r["shift"] = (rng.randint(-320, 320), rng.randint(-320, 320))
        took.add("shift")
    else:
        took.add("no shift")
    if rng.random() > 0.6:                                                      # 156
        pnt = (crop // 2 + rng.randint(-320, 320), crop // 2 + rng.randint(-320, 320))
        scale = 0.9 + rng.random() * 0.2
        angle = rng.randint(0, 20) - 10
        if (angle != 0) or (scale != 1):                                        # 160
            r["warp"] = (angle, scale, pnt)
            took.add("warp")
        else:
            took.add("warp drawn and skipped")
    else:
        took.add("no warp")
    if rng.random() > 0.985:                                                    # 206
        r["channels"] = (1, rng.randint(-5, 5), rng.randint(-5, 5), rng.randint(-5, 5))
        took.add("channels pre")
    elif rng.random() > 0.985:
        r["channels"] = (2, rng.randint(-5, 5), rng.randint(-5, 5), rng.randint(-5, 5))
        took.add("channels post")
    else:
        took.add("no channels")
    if rng.random() > 0.985:                                                    # 211
        rng.randint(-5, 5), rng.randint(-5, 5), rng.randint(-5, 5)
        skipped.append("change_hsv_pre")
    elif rng.random() > 0.985:
        rng.randint(-5, 5), rng.randint(-5, 5), rng.randint(-5, 5)
        skipped.append("change_hsv_post")
    else:
        took.add("no change_hsv")
    for im in ("pre", "post"):                                                  # 216-229, 231-244
        if rng.random() > 0.98:
            if rng.random() > 0.985:
                skipped.append("clahe_" + im)
            elif rng.random() > 0.985:
                skipped.append("gauss_noise_" + im)
            elif rng.random() > 0.985:
                skipped.append("blur_" + im)
            else:
                took.add("first block, nothing, " + im)
        elif rng.random() > 0.98:
            if rng.random() > 0.985:
                rng.random()
                skipped.append("saturation_" + im)
            elif rng.random() > 0.985:
                rng.random()
                skipped.append("brightness_" + im)
            elif rng.random() > 0.985:
                rng.random()
                skipped.append("contrast_" + im)
            else:
                took.add("second block, nothing, " + im)
        else:
            took.add("neither block, " + im)
    if rng.random() > 0.983:                                                    # 247
        skipped.append("elastic_pre")
    else:
        took.add("no elastic pre")
    if rng.random() > 0.983:                                                    # 251
        skipped.append("elastic_post")
    else:
        took.add("no elastic post")
    return r, skipped, took | set(skipped)


# every branch script_draws can take, but "warp drawn and skipped": scale == 1 needs random() == 0.5 exactly, which no seed
# gives in 20 000 samples -- test_xbd_unet_cpu.py takes that branch with a scripted stream
BRANCHES = ({"vflip", "no vflip", "no rot", "shift", "no shift", "warp", "no warp", "channels pre", "channels post", "no channels",
             "no change_hsv", "no elastic pre", "no elastic post"} | {"rot %d" % k for k in range(4)} | set(X.UNET_SKIPPED)
            | {"%s, %s" % (b, im) for b in ("first block, nothing", "second block, nothing", "neither block") for im in ("pre", "post")})
