"""The building step of the xBD side (csrc/xbd_buildings.hip: dh_xbd_cc_label / _stats / _vote / _paint, models/xbd.buildings /
building_damage / building_confusion) restated in plain Python and numpy, and the patterns its tests share.

The definition: two neighbouring pixels (4: left / right / up / down; 8: and the diagonals) belong together when both keys are
nonzero (keyed: nonzero and equal); a component's number is its rank, from 1, in raster order of its first pixel; every image
is labelled on its own.  cc_label is a raster union-find over exactly that.  Its `mutate` argument builds the WRONG variants that
test_xbd_buildings_cpu.py uses to show that its comparisons can fail."""
import functools

import numpy as np

COLS = 10          # area, h0 .. h4, y0, x0, y1, x1


# ---- the restatement -------------------------------------------------------------------------------------------------
def _label_image(key, conn, keyed, mutate=None):
    H, W = key.shape
    if mutate == "swap":                                        # 4 and 8 swapped
        conn = 12 - conn
    skip = mutate[1] if isinstance(mutate, tuple) and mutate[0] == "drop" else None      # the unions of ONE pixel dropped
    k = key.ravel().tolist()
    parent = list(range(H * W))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for p in range(H * W):
        kp = k[p]
        if not kp:
            continue
        y, x = divmod(p, W)
        if skip == (y, x):
            continue
        before = []                                             # the neighbours that come before p in raster order
        if x > 0:
            before.append(p - 1)
        if y > 0:
            before.append(p - W)
            if conn == 8:
                if x > 0:
                    before.append(p - W - 1)
                if x < W - 1:
                    before.append(p - W + 1)
        for q in before:
            if k[q] and (not keyed or k[q] == kp):
                a, b = find(p), find(q)
                if a != b:
                    parent[max(a, b)] = min(a, b)               # union by minimum index: a root is its component's first pixel
    labels = np.zeros(H * W, dtype=np.int32)
    ids = {}
    for p in range(H * W):
        if k[p]:
            r = find(p)
            if r not in ids:
                ids[r] = len(ids) + 1                           # r == p here: the first pixel is met first
            labels[p] = ids[r]
    if mutate == "reverse":                                     # numbered from the last root backwards
        labels[labels > 0] = len(ids) + 1 - labels[labels > 0]
    return labels.reshape(H, W), len(ids)


@functools.lru_cache(maxsize=None)
def _label_cached(data, shape, conn, keyed):
    key = np.frombuffer(data, dtype=np.uint8).reshape(shape)
    out = [_label_image(key[n], conn, keyed) for n in range(shape[0])]
    labels = np.stack([o[0] for o in out])
    labels.setflags(write=False)
    return labels, np.array([o[1] for o in out], dtype=np.int32)


def cc_label(key, conn=8, keyed=False, mutate=None):
    """key uint8 [N, H, W] -> (labels int32 [N, H, W], count int32 [N]).  Unmutated results are computed once per input and
    shared (read-only); keyed is the same as unkeyed when the key has one nonzero value."""
    key = np.ascontiguousarray(key, dtype=np.uint8)
    assert key.ndim == 3 and conn in (4, 8)
    if mutate is not None:
        out = [_label_image(key[n], conn, bool(keyed), mutate) for n in range(key.shape[0])]
        return np.stack([o[0] for o in out]), np.array([o[1] for o in out], dtype=np.int32)
    keyed = bool(keyed) and len(np.unique(key[key != 0])) > 1
    return _label_cached(key.tobytes(), key.shape, conn, keyed)


def cc_stats(labels, vote, cap):
    """table int32 [N, cap, 10]: row i describes label i + 1"""
    N, H, W = labels.shape
    table = np.zeros((N, cap, COLS), dtype=np.int32)
    table[:, :, 6], table[:, :, 7], table[:, :, 8:] = H, W, -1
    for n in range(N):
        ys, xs = np.nonzero((labels[n] >= 1) & (labels[n] <= cap))
        rows = labels[n][ys, xs] - 1
        v = vote[n][ys, xs]
        np.add.at(table[n, :, 0], rows, 1)
        for c in range(5):
            np.add.at(table[n, :, 1 + c], rows[v == c], 1)
        np.minimum.at(table[n, :, 6], rows, ys.astype(np.int32))
        np.minimum.at(table[n, :, 7], rows, xs.astype(np.int32))
        np.maximum.at(table[n, :, 8], rows, ys.astype(np.int32))
        np.maximum.at(table[n, :, 9], rows, xs.astype(np.int32))
    return table


def cc_vote(table, min_area=0, mode="damage"):
    """cls uint8 [N, cap]: 'damage' 1 + first maximum of h1 .. h4 (0 when all are zero), 'all' first maximum of h0 .. h4;
    np.argmax returns the FIRST maximum; area 0 or below min_area gives 0"""
    area, h = table[..., 0], table[..., 1:6]
    if mode == "damage":
        cls = np.where(h[..., 1:].max(-1) > 0, 1 + h[..., 1:].argmax(-1), 0)
    else:
        assert mode == "all"
        cls = h.argmax(-1)
    return np.where((area > 0) & (area >= min_area), cls, 0).astype(np.uint8)


def cc_paint(labels, cls):
    N, cap = cls.shape
    out = np.zeros(labels.shape, dtype=np.uint8)
    for n in range(N):
        ok = (labels[n] >= 1) & (labels[n] <= cap)
        out[n][ok] = cls[n][labels[n][ok] - 1]
    return out


def building_damage(footprint, vote, conn=8, min_area=0, cap=4096):
    """(labels, count, table, cls, map) of a footprint (nonzero = building) and the per-pixel vote"""
    labels, count = cc_label((footprint != 0).astype(np.uint8), conn, False)
    table = cc_stats(labels, vote, cap)
    cls = cc_vote(table, min_area, "damage")
    return labels, count, table, cls, cc_paint(labels, cls)


def building_confusion(pred_map, gt, conn=8):
    """int64 [4, 5]: [g - 1, p] counts the ground-truth buildings (keyed components of gt) of class g whose pixels vote p"""
    if gt.size and int(gt.max()) > 4:
        raise KeyError(int(gt.max()))
    labels, count = cc_label(gt, conn, True)
    conf = np.zeros((4, 5), dtype=np.int64)
    for n in range(gt.shape[0]):
        for i in range(1, int(count[n]) + 1):
            m = labels[n] == i
            g = int(gt[n][m][0])
            votes = np.bincount(pred_map[n][m], minlength=256)[:5]
            conf[g - 1, int(votes.argmax())] += 1
    return conf


# ---- patterns: uint8 [N, H, W], every image of a batch different -------------------------------------------------------
def seed_of(*ints):
    s = 12345
    for i in ints:
        s = (s * 1000003 + int(i)) % (2 ** 31 - 1)
    return s


def zeros(N, H, W):
    return np.zeros((N, H, W), dtype=np.uint8)


def ones(N, H, W):
    return np.ones((N, H, W), dtype=np.uint8)


def noise(N, H, W, density, classes=1):
    """set with probability `density`; classes > 1: the set pixels carry a random class 1 .. classes (for keyed)"""
    rng = np.random.RandomState(seed_of(N, H, W, int(density * 100), classes))
    on = rng.random_sample((N, H, W)) < density
    val = rng.randint(1, classes + 1, size=(N, H, W)) if classes > 1 else 1
    return (on * val).astype(np.uint8)


def checkerboard(N, H, W):
    """one component at 8-connectivity, ceil(H W / 2) single pixels at 4"""
    y, x = np.mgrid[:H, :W]
    return np.broadcast_to(((y + x) % 2 == 0).astype(np.uint8), (N, H, W)).copy()


def serpentine(N, H, W):
    """ONE component at either connectivity: every even row is set, and the odd rows between them hold one pixel, at the right
    end and at the left end by turns, so that the path runs through the rows boustrophedon"""
    a = np.zeros((N, H, W), dtype=np.uint8)
    a[:, 0::2] = 1
    a[:, 1::4, W - 1] = 1
    a[:, 3::4, 0] = 1
    if H % 2 == 0:                     # the last row is odd: its connector would be a dead end, harmless, but keep the path clean
        a[:, H - 1] = 0
    return a


def u_shape(N, H, W):
    """two vertical bars joined only by the bottom row: the bars lie in tiles where nothing connects them"""
    a = np.zeros((N, H, W), dtype=np.uint8)
    x1, x2 = W // 4, (3 * W) // 4
    a[:, 1:H - 1, x1] = 1
    a[:, 1:H - 1, x2] = 1
    a[:, H - 2, x1:x2 + 1] = 1
    return a


def rings(N, H, W):
    """two nested rectangular outlines, 3 pixels apart: two components that cross every tile border they meet twice"""
    a = np.zeros((N, H, W), dtype=np.uint8)
    for inset in (1, 4):
        y0, x0, y1, x1 = inset, inset, H - 1 - inset, W - 1 - inset
        if y1 - y0 < 2 or x1 - x0 < 2:
            continue
        a[:, y0, x0:x1 + 1] = 1
        a[:, y1, x0:x1 + 1] = 1
        a[:, y0:y1 + 1, x0] = 1
        a[:, y0:y1 + 1, x1] = 1
    return a


def squares(N, H, W, s=5):
    """s x s squares with 1-pixel gaps (the last ones of a row or column are cut by the image): closed form below"""
    y, x = np.mgrid[:H, :W]
    return np.broadcast_to(((y % (s + 1) < s) & (x % (s + 1) < s)).astype(np.uint8), (N, H, W)).copy()


def squares_closed_form(N, H, W, s=5):
    """(labels, count, table rows area / box of every square) of squares(N, H, W, s) at either connectivity"""
    y, x = np.mgrid[:H, :W]
    ncols, nrows = -(-W // (s + 1)), -(-H // (s + 1))
    on = (y % (s + 1) < s) & (x % (s + 1) < s)
    labels = np.where(on, (y // (s + 1)) * ncols + x // (s + 1) + 1, 0).astype(np.int32)
    area_box = np.zeros((nrows * ncols, 5), dtype=np.int32)
    for i in range(nrows):
        for j in range(ncols):
            ya, xa = i * (s + 1), j * (s + 1)
            yb, xb = min(ya + s, H) - 1, min(xa + s, W) - 1
            area_box[i * ncols + j] = ((yb - ya + 1) * (xb - xa + 1), ya, xa, yb, xb)
    return np.broadcast_to(labels, (N, H, W)).copy(), np.full(N, nrows * ncols, dtype=np.int32), area_box


def touching_blocks(N, H, W):
    """ground-truth classes: a block of class 1 and a block of class 3 that share an edge, a block of class 2 under the second
    that touches the first at a corner only, and a second block of class 1 apart from all: keyed 4 components, unkeyed 2"""
    a = np.zeros((N, H, W), dtype=np.uint8)
    my, mx = H // 2, W // 2
    a[:, 2:my, 2:mx] = 1
    a[:, 2:my, mx:W - 2] = 3
    a[:, my:H - 2, mx:W - 8] = 2
    a[:, my + 2:H - 2, 1:mx - 4] = 1
    return a


def votes(N, H, W, odd_bytes=True):
    """a per-pixel vote 0 .. 4, with a few bytes 5 and 255 that count in the area only"""
    rng = np.random.RandomState(seed_of(N, H, W, 77))
    v = rng.randint(0, 5, size=(N, H, W)).astype(np.uint8)
    # make large patches of one class too, so that a vote has a clear winner somewhere
    v[:, : H // 2, : W // 2] = 2
    if odd_bytes:
        sel = rng.random_sample((N, H, W))
        v[sel < 0.02] = 5
        v[sel > 0.98] = 255
    return v


def patterns(N, H, W):
    """name -> key, the binary patterns and the multi-class ones"""
    return {
        "zeros": zeros(N, H, W), "ones": ones(N, H, W),
        "noise30": noise(N, H, W, 0.3), "noise59": noise(N, H, W, 0.59), "noise70": noise(N, H, W, 0.7),
        "checkerboard": checkerboard(N, H, W), "serpentine": serpentine(N, H, W), "u": u_shape(N, H, W),
        "rings": rings(N, H, W), "squares": squares(N, H, W), "blocks": touching_blocks(N, H, W),
        "classes59": noise(N, H, W, 0.59, classes=4), "classes90": noise(N, H, W, 0.9, classes=2),
    }
