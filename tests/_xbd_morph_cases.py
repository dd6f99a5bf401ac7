"""Square-window morphology, the dilated training masks and the hole fill (csrc/xbd_morph.hip, models/xbd.clean_footprint)
restated in plain numpy, and the named inputs their tests share.  Nothing here needs a GPU.

The definitions: win_or(a, k) is the OR over the k x k window centred on a pixel with everything outside the image clear;
erode(a, k) is the AND with everything outside the image set (skimage's convention), which is the window OR of the complement,
complemented; msk_dilate applies the priority rule of xBD_code/train_unettransformer.py:262-273 to the four dilated damage
channels; fill_holes(a) is a plus every component of the complement that has no pixel on the image border.  The `mutate`
arguments build the WRONG variants with which test_xbd_morph_cpu.py shows that its comparisons can fail."""
import numpy as np

import _xbd_buildings_cases as B

SHAPES = [(1, 1, 1), (1, 1, 7), (1, 5, 3), (2, 37, 67), (1, 70, 130), (1, 256, 256)]
HOLE_SHAPES = [(2, 37, 67), (1, 70, 130), (1, 256, 256)]          # the shapes the rings and the spiral fit into
KS = (1, 3, 5, 9, 31)
MSK_KS = (3, 5)
MUTANTS = ("offcentre", "border0", "swap34", "noleft", "conn")


# ---- the restatements ------------------------------------------------------------------------------------------------
def _window(b, k, outside, off=0):
    """bool [N, H, W]: OR over the k x k window of b, positions outside the image taken as `outside`; off shifts the window's
    columns (the off-centre mutant).  Shifted ORs over a padded array, along the rows and then along the columns."""
    N, H, W = b.shape
    r = k // 2
    pad = np.full((N, H + 2 * r, W + 2 * r + 2), bool(outside))
    pad[:, r:r + H, r + 1:r + 1 + W] = b
    rows = np.zeros((N, H + 2 * r, W), dtype=bool)
    for dx in range(k):
        rows |= pad[:, :, 1 + off + dx:1 + off + dx + W]
    out = np.zeros((N, H, W), dtype=bool)
    for dy in range(k):
        out |= rows[:, dy:dy + H]
    return out


def win_or(a, k, mutate=None):
    """uint8 0 / 1 [N, H, W]: binary_dilation(a, structure=ones((k, k)))"""
    assert a.ndim == 3 and k % 2 == 1 and 1 <= k <= 31
    return _window(a != 0, k, False, 1 if mutate == "offcentre" else 0).astype(np.uint8)


def erode(a, k, mutate=None):
    """uint8 0 / 1: binary_erosion(a, structure=ones((k, k)), border_value=1).  A pixel survives when no pixel of its window is
    clear, and nothing outside the image is clear."""
    assert a.ndim == 3 and k % 2 == 1 and 1 <= k <= 31
    return (~_window(a == 0, k, mutate == "border0")).astype(np.uint8)            # WRONG with border0: the outside clear


def opening(a, k):
    return win_or(erode(a, k), k)


def closing(a, k):
    return erode(win_or(a, k), k)


def msk_dilate(msk, k=5, mutate=None):
    """msk uint8 [N, 5, H, W] -> uint8 [N, 5, H, W]; channel 0 of the input is not read"""
    assert msk.ndim == 4 and msk.shape[1] == 5
    d1, d2, d3, d4 = (win_or(msk[:, c], k).astype(bool) for c in range(1, 5))
    m2 = d2
    if mutate == "swap34":                                      # WRONG: class 4 over class 3
        m4 = d4 & ~d2
        m3 = d3 & ~d2 & ~d4
    else:
        m3 = d3 & ~d2
        m4 = d4 & ~d2 & ~d3
    m1 = d1 & ~(d2 | d3 | d4)
    return np.stack([m1 | m2 | m3 | m4, m1, m2, m3, m4], axis=1).astype(np.uint8)


def fill_holes(a, background=4, mutate=None):
    """uint8 0 / 1: binary_fill_holes(a, structure=generate_binary_structure(2, 1 if background == 4 else 2))"""
    assert a.ndim == 3 and background in (4, 8)
    conn = 12 - background if mutate == "conn" else background            # WRONG with conn: 4 and 8 swapped
    labels, count = B.cc_label((a == 0).astype(np.uint8), conn, False)
    out = (a != 0)
    for n in range(a.shape[0]):
        L = labels[n]
        edge = np.concatenate([L[0], L[-1], L[:, -1]] + ([] if mutate == "noleft" else [L[:, 0]]))      # WRONG with noleft: column 0 not looked at
        open_ = np.zeros(int(count[n]) + 1, dtype=bool)
        open_[edge] = True
        open_[0] = True
        out[n] |= ~open_[L]
    return out.astype(np.uint8)


def clean_footprint(a, open=0, close=0, fill=False, background=4):
    """opening with square(open), then closing with square(close), then the hole fill: the order of models/xbd.clean_footprint"""
    cur = (a != 0).astype(np.uint8)
    if open:
        cur = opening(cur, open)
    if close:
        cur = closing(cur, close)
    if fill:
        cur = fill_holes(cur, background)
    return cur


# ---- named inputs ------------------------------------------------------------------------------------------------------
def marks(N, H, W):
    """the (y, x) of the four corners, the middle of each edge and the centre (fewer distinct ones on tiny images)"""
    ys, xs = (0, H // 2, H - 1), (0, W // 2, W - 1)
    return sorted({(y, x) for y in ys for x in xs})


def points(N, H, W):
    a = B.zeros(N, H, W)
    for y, x in marks(N, H, W):
        a[:, y, x] = 1
    return a


def pits(N, H, W):
    """one clear pixel in a set field at each of the marks"""
    return 1 - points(N, H, W)


def noise(N, H, W, permille):
    rng = np.random.RandomState(B.seed_of(N, H, W, permille, 4242))
    return (rng.random_sample((N, H, W)) < permille / 1000.0).astype(np.uint8) * 255          # nonzero = set, not only 1


def map_cases(N, H, W):
    """name -> uint8 [N, H, W]"""
    return {"zeros": B.zeros(N, H, W), "ones": B.ones(N, H, W), "points": points(N, H, W), "pits": pits(N, H, W),
            "checkerboard": B.checkerboard(N, H, W), "noise0.5": noise(N, H, W, 5), "noise50": noise(N, H, W, 500),
            "noise97": noise(N, H, W, 970)}


def labels3(N, H, W):
    """random labels 0 .. 5 at 3 % coverage; label 5 sets no channel"""
    rng = np.random.RandomState(B.seed_of(N, H, W, 3, 555))
    on = rng.random_sample((N, H, W)) < 0.03
    return (on * rng.randint(1, 6, size=(N, H, W))).astype(np.uint8)


PRIORITY_PAIRS = ((2, 3), (2, 4), (3, 4), (2, 1), (3, 1), (4, 1))


def rects(N, H, W):
    """3 x 3 rectangles of two classes side by side, one row of them per priority pair and one column per gap of 1 .. 4 pixels,
    so that at k = 3 and 5 every pair overlaps somewhere (drawn as far as the image reaches)"""
    a = B.zeros(N, H, W)
    for i, (hi, lo) in enumerate(PRIORITY_PAIRS):
        for g in range(1, 5):
            y, x = 1 + 6 * i, 1 + 15 * (g - 1)
            a[:, y:y + 3, x:x + 3] = hi if (i + g) % 2 else lo
            a[:, y:y + 3, x + 3 + g:x + 6 + g] = lo if (i + g) % 2 else hi
    return a


def label_cases(N, H, W):
    return {"labels3": labels3(N, H, W), "rects": rects(N, H, W)}


def to_msk(lbl):
    """the training mask channels of a label map, uint8 [N, 5, H, W]: msk[c] = (lbl == c) for c = 1 .. 4, msk[0] = any of them"""
    ch = [(lbl == c) for c in range(1, 5)]
    return np.stack([ch[0] | ch[1] | ch[2] | ch[3]] + ch, axis=1).astype(np.uint8)


def _outline(a, y0, x0, y1, x1):
    a[:, y0, x0:x1 + 1] = 1
    a[:, y1, x0:x1 + 1] = 1
    a[:, y0:y1 + 1, x0] = 1
    a[:, y0:y1 + 1, x1] = 1


def ring(N, H, W):
    a = B.zeros(N, H, W)
    _outline(a, 3, 3, H - 4, W - 4)
    return a


def ring_in_ring(N, H, W):
    """a ring inside a ring's hole: the whole interior fills, the inner ring's hole too"""
    a = ring(N, H, W)
    _outline(a, 8, 8, H - 9, W - 9)
    return a


def ring_open(N, H, W):
    """the ring with one pixel of its top side missing: its inside is the outside"""
    a = ring(N, H, W)
    a[:, 3, W // 2] = 0
    return a


def ring_diag(N, H, W):
    """the ring without its upper left corner pixel: the inside touches that pixel only diagonally, so the hole is closed for a
    4-connected background and open for an 8-connected one"""
    a = ring(N, H, W)
    a[:, 3, 3] = 0
    return a


def ring_left(N, H, W):
    """a ring that the image cuts on the left: its hole owns pixels of column 0, and of no other border"""
    a = B.zeros(N, H, W)
    a[:, 3, 0:W - 3] = 1
    a[:, H - 4, 0:W - 3] = 1
    a[:, 3:H - 3, W - 4] = 1
    return a


def spiral(N, H, W, closed=False):
    """walls one pixel thick around a corridor one pixel wide that winds inwards: concentric rings every two pixels, ring t + 1
    opened at one pixel of its top side, and the corridor outside it plugged next to that opening, so that the way from one
    opening to the next runs once round.  Open: the outermost ring is opened too and the whole corridor is the outside.
    Closed: everything inside the outermost ring fills."""
    a = B.zeros(N, H, W)
    s, t = 2, 0
    while H - 1 - 2 * s >= 4 and W - 1 - 2 * s >= 4:
        _outline(a, s, s, H - 1 - s, W - 1 - s)
        if t > 0 or not closed:
            a[:, s, s + 2] = 0                                  # the opening of ring t ...
        if t > 0:
            a[:, s - 1, s + 1] = 1                              # ... and the plug between the last opening and this one
        s, t = s + 2, t + 1
    return a


def hole_cases(N, H, W):
    """name -> uint8 [N, H, W], for H, W >= 32"""
    assert H >= 32 and W >= 32
    return {"ring": ring(N, H, W), "ring_in_ring": ring_in_ring(N, H, W), "ring_open": ring_open(N, H, W),
            "ring_diag": ring_diag(N, H, W), "ring_left": ring_left(N, H, W), "spiral_open": spiral(N, H, W),
            "spiral_closed": spiral(N, H, W, closed=True), "noise50": noise(N, H, W, 500)}


def bridged_squares(H=40, W=72):
    """(footprint, ground truth) uint8 [1, H, W]: two 12 x 12 squares joined by a one-pixel bridge, a pin-hole in the first; the
    truth is the two squares, class 2"""
    gt = np.zeros((1, H, W), dtype=np.uint8)
    gt[:, 10:22, 8:20] = 2
    gt[:, 10:22, 30:42] = 2
    fp = (gt != 0).astype(np.uint8)
    fp[:, 15, 20:30] = 1                                        # the bridge
    fp[:, 14, 12] = 0                                           # the pin-hole
    return fp, gt
