"""TilePlan: the windows a net of fixed input size takes over a whole tile, and the tables that put its answers back together.

newUNetTrans (DAHiTra proper) runs at 256 x 256 only (hard-coded positional embeddings) and the BiT nets are trained at 256,
while LEVIR and xBD tiles are 1024 x 1024.  A plan lists the views of one tile -- window origins, optionally each window under
several flips -- in the form dh_augment_pairs_u8 cuts them (`params()`), and the per-axis weights and cover tables
dh_cd_tile_stitch blends the per-view logits with (`tables()`).  Pure numpy: importable and testable without a GPU.

    plan = TilePlan(1024, 1024, window=(256, 256), stride=(128, 128), flips=(0, 3), weight='triangle')
    plan.P, plan.params()             # 49 * 2 views; [P, 4] int32 rows (x0, y0, hflip, vflip)

Flip codes are those of models/xbd.py's 4-flip prediction (ops.xbd_tta_pack): bit 0 reverses the rows, bit 1 the columns.  In a
`params()` row, `vflip` (rows reversed) is therefore bit 0 and `hflip` (columns reversed) bit 1."""
import numpy as np

WEIGHTS = ("mean", "triangle")


def axis_origins(size, win, stride):
    """origins of the windows of length `win` along an axis of length `size`: range(0, size - win + 1, stride), plus size - win
    when the last of them does not already end at the edge (the last window is clamped to the edge, never padded)"""
    o = list(range(0, size - win + 1, stride))
    if o[-1] != size - win:
        o.append(size - win)
    return o


def axis_cover(size, win, origins):
    """[size, 2] int32 (first, count): the windows `first .. first + count - 1` are exactly those that hold the position.
    Origins ascend, so the windows over one position are consecutive."""
    o = np.asarray(origins, dtype=np.int64)
    t = np.arange(size, dtype=np.int64)
    first = np.searchsorted(o, t - win, side="right")          # the first origin > t - win, i.e. origin + win > t
    last = np.searchsorted(o, t, side="right")                 # one past the last origin <= t
    return np.stack([first, last - first], axis=1).astype(np.int32)


def axis_weight(win, weight):
    t = np.arange(win)
    if weight == "mean":
        return np.ones(win, dtype=np.float32)
    return np.minimum(t + 1, win - t).astype(np.float32)        # small integers: exact in float32, and so is every product


class TilePlan:
    """The views of one H x W tile.

    window (h, w), stride (sy, sx): per axis the origins are axis_origins(); view p = (iy * nx + ix) * nf + f is the window at
    (ys[iy], xs[ix]) under flip code flips[f].  weight: 'mean' (every view counts 1) or 'triangle' (wy[t] = min(t + 1, h - t),
    the same for x; a view counts wy * wx, which favours the middle of a window over its rim).
    ValueError: a window larger than the tile, a stride < 1 or larger than the window (gaps), a flip code outside 0 .. 3,
    repeated flip codes, an unknown weight."""

    def __init__(self, H, W, window=(256, 256), stride=(256, 256), flips=(0,), weight="mean"):
        H, W = int(H), int(W)
        (h, w), (sy, sx) = (int(v) for v in window), (int(v) for v in stride)
        flips = tuple(int(f) for f in flips)
        if h < 1 or w < 1 or h > H or w > W:
            raise ValueError("TilePlan: window %dx%d does not fit the %dx%d tile" % (h, w, H, W))
        if sy < 1 or sx < 1:
            raise ValueError("TilePlan: stride (%d, %d) is below 1" % (sy, sx))
        if sy > h or sx > w:
            raise ValueError("TilePlan: stride (%d, %d) exceeds the window %dx%d and would leave gaps" % (sy, sx, h, w))
        if not flips or any(f < 0 or f > 3 for f in flips):
            raise ValueError("TilePlan: flip codes %r are not in 0 .. 3" % (flips,))
        if len(set(flips)) != len(flips):
            raise ValueError("TilePlan: flip codes %r repeat" % (flips,))
        if weight not in WEIGHTS:
            raise ValueError("TilePlan: weight %r is not one of %s" % (weight, list(WEIGHTS)))
        self.H, self.W, self.h, self.w, self.sy, self.sx = H, W, h, w, sy, sx
        self.flips, self.weight = flips, weight
        self.ys, self.xs = axis_origins(H, h, sy), axis_origins(W, w, sx)
        self.ny, self.nx, self.nf = len(self.ys), len(self.xs), len(flips)
        self.P = self.ny * self.nx * self.nf
        self.stitchable = True
        self._origins = None

    @classmethod
    def eval_cd(cls, H, W, size=256):
        """The sixteen views the reference's eval_cd.py:49-55 evaluates, as executed: one CDEvaluator per `patch` index p in
        0 .. 15, each over the window CDDataAugmentation.transform cuts (datasets/data_utils.py:65-68),
            (x0, y0) = (256 * (p // 4), 256 * (p % 4))   if p else   (256, 256).
        The reference's `if patch:` is false for patch 0, so view 0 REPEATS view 5 and the window at (0, 0) is never evaluated.
        That is kept here: the plan reproduces what the script scores.  No flips.  Not stitchable: its views repeat and do not
        cover the tile; it serves the per-view counts (ops.cd_view_counts, models.tiles.evaluate_tiles).
        ValueError unless size < W // 2 (the reference crops only then) and every window lies inside the tile."""
        H, W, size = int(H), int(W), int(size)
        if size < 1 or not size < W // 2:
            raise ValueError("TilePlan.eval_cd: the reference cuts patches only when size < width // 2; %d, %d" % (size, W))
        origins = [(256 * (p // 4), 256 * (p % 4)) if p else (256, 256) for p in range(16)]
        for x0, y0 in origins:
            if x0 + size > W or y0 + size > H:
                raise ValueError("TilePlan.eval_cd: window (%d, %d) + %d leaves the %dx%d tile" % (x0, y0, size, H, W))
        self = cls.__new__(cls)
        self.H, self.W, self.h, self.w, self.sy, self.sx = H, W, size, size, 256, 256
        self.flips, self.weight = (0,), "mean"
        self.ys = self.xs = None
        self.ny = self.nx = None
        self.nf, self.P = 1, 16
        self.stitchable = False
        self._origins = origins
        return self

    # a plan is a value: equal plans share their device tables (ops.cd_tile_stitch) and their recorded steps
    def key(self):
        return (self.H, self.W, self.h, self.w, self.sy, self.sx, self.flips, self.weight,
                tuple(self._origins) if self._origins is not None else None)

    def __eq__(self, other):
        return isinstance(other, TilePlan) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        if not self.stitchable:
            return "TilePlan.eval_cd(%d, %d, size=%d)" % (self.H, self.W, self.h)
        return "TilePlan(%d, %d, window=(%d, %d), stride=(%d, %d), flips=%r, weight=%r)" % (
            self.H, self.W, self.h, self.w, self.sy, self.sx, self.flips, self.weight)

    def origins(self):
        """[(x0, y0)] per window, in view order without the flips"""
        if self._origins is not None:
            return list(self._origins)
        return [(x0, y0) for y0 in self.ys for x0 in self.xs]

    def params(self):
        """[P, 4] int32 rows (x0, y0, hflip, vflip) as dh_augment_pairs_u8 reads them: hflip reverses the columns (bit 1 of the
        flip code), vflip the rows (bit 0)"""
        rows = [(x0, y0, (f >> 1) & 1, f & 1) for x0, y0 in self.origins() for f in self.flips]
        return np.asarray(rows, dtype=np.int32).reshape(self.P, 4)

    def weights(self):
        """(wy [h], wx [w]) float32"""
        return axis_weight(self.h, self.weight), axis_weight(self.w, self.weight)

    def cover(self):
        """(rows [H, 2], cols [W, 2]) int32: per output row (first iy, count), per output column (first ix, count)"""
        self._need_stitchable("cover")
        return axis_cover(self.H, self.h, self.ys), axis_cover(self.W, self.w, self.xs)

    def x_align(self):
        """4 if the tile width, the window width and every x origin are multiples of 4 (a run of 4 output columns then has one
        cover and its sources are 4 consecutive floats at a multiple of 4), else 1"""
        self._need_stitchable("x_align")
        return 4 if all(v % 4 == 0 for v in [self.W, self.w] + self.xs) else 1

    def _need_stitchable(self, what):
        if not self.stitchable:
            raise ValueError("TilePlan.%s: %r is not stitchable (its views repeat and do not cover the tile)" % (what, self))
