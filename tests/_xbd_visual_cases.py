"""The damage map and the 4-panel picture of the reference's xBD visualiser (xBD_code/visualize_results.py:204-220) restated in
numpy for the tests of dh_xbd_damage_map_u8 / dh_xbd_vis_grid_u8 / models/xbd.visual_grid, and the inputs those tests share.

What is computed for a prediction msk [H, W, 5] uint8, channels last:
    dmg  = 1 + index of the first maximum among msk[..., 1] .. msk[..., 4]          1 .. 4; a tie goes to the lowest channel
    loc  = None: out = dmg (the script as executed)
    loc  = (t0, t1, t2), or one float for all three: p = msk[..., 0] / 255 in float64,
           keep = (p > t0) | ((p > t1) & (dmg > 1) & (dmg < 4)) | ((p > t2) & (dmg > 1)),  out = dmg * keep
    grid = pre | post | colour(gt) | colour(out) side by side, [H, 4W, 3] uint8 RGB; a label outside 0 .. 4 is painted MAGENTA
Two forms: the vectorised one the GPU tests compare with, and a per-pixel loop (explicit first-maximum search, a dict of colours)
to check the first against.  Everything is integer or an exact float64 comparison: there is no tolerance anywhere."""
import numpy as np

SCRIPT_THR = (0.38, 0.13, 0.14)                      # the script's _thr
# the bytes on either side of the three thresholds (96 | 97, 33 | 34, 35 | 36) and the two ends; ten symbols force ties
ALPHABET = (0, 1, 33, 34, 35, 36, 96, 97, 254, 255)
COLOURS = {0: (0, 0, 0), 1: (0, 255, 0), 2: (255, 255, 0), 3: (255, 127, 0), 4: (255, 0, 0)}          # RGB
MAGENTA = (255, 0, 255)
LOCS = (None, SCRIPT_THR, 0.3)
SMALL = ((1, 37, 41), (2, 40, 40))


def seed_of(N, H, W):
    return N * 100 + H


def masks(N, H, W, seed):
    """[N, H, W, 5] uint8 drawn from ALPHABET"""
    rs = np.random.RandomState(seed)
    return np.asarray(ALPHABET, dtype=np.uint8)[rs.randint(0, len(ALPHABET), size=(N, H, W, 5))]


def pictures(N, H, W, seed):
    """pre, post [N, H, W, 3] random bytes and gt [N, H, W] in 0 .. 4"""
    rs = np.random.RandomState(seed + 7919)
    pre = rs.randint(0, 256, size=(N, H, W, 3)).astype(np.uint8)
    post = rs.randint(0, 256, size=(N, H, W, 3)).astype(np.uint8)
    gt = rs.randint(0, 5, size=(N, H, W)).astype(np.uint8)
    return pre, post, gt


def thresholds(loc):
    if loc is None:
        return None
    t = tuple(float(v) for v in loc) if isinstance(loc, (tuple, list)) else (float(loc),) * 3
    assert len(t) == 3
    return t


def first_max(msk):
    """1 + the number of channels in front of the first maximum of msk[..., 1:], [..., H, W]"""
    best = msk[..., 1:].max(axis=-1, keepdims=True)
    return 1 + (np.cumsum(msk[..., 1:] == best, axis=-1) == 0).sum(axis=-1)


def clauses(msk, loc):
    """the three clauses of the rule, each [..., H, W]"""
    t0, t1, t2 = thresholds(loc)
    dmg = first_max(msk)
    p = msk[..., 0].astype(np.float64) / 255
    return p > t0, (p > t1) & (dmg > 1) & (dmg < 4), (p > t2) & (dmg > 1)


def damage_map(msk, loc=None):
    """msk [..., H, W, 5] uint8 -> [..., H, W] uint8"""
    dmg = first_max(msk)
    if loc is not None:
        c1, c2, c3 = clauses(msk, loc)
        dmg = dmg * (c1 | c2 | c3)
    return dmg.astype(np.uint8)


def paint(cls):
    table = np.asarray([COLOURS[c] for c in range(5)] + [MAGENTA], dtype=np.uint8)
    return table[np.minimum(cls, 5)]


def vis_grid(pre, post, gt, msk, loc=None):
    """-> [..., H, 4W, 3] uint8 RGB"""
    return np.concatenate([pre, post, paint(gt), paint(damage_map(msk, loc))], axis=-2)


# ---- the slow form -------------------------------------------------------------------------------------------------------
def damage_map_slow(msk, loc=None):
    flat = msk.reshape(-1, 5)
    out = np.empty(len(flat), dtype=np.uint8)
    t = thresholds(loc)
    for i, (m0, m1, m2, m3, m4) in enumerate(flat.tolist()):
        d, best = 1, m1
        for k, v in ((2, m2), (3, m3), (4, m4)):
            if v > best:
                d, best = k, v
        if t is not None:
            p = m0 / 255
            if not (p > t[0] or (p > t[1] and 1 < d < 4) or (p > t[2] and d > 1)):
                d = 0
        out[i] = d
    return out.reshape(msk.shape[:-1])


def vis_grid_slow(pre, post, gt, msk, loc=None):
    N, H, W, _ = msk.shape
    cls = damage_map_slow(msk, loc)
    out = np.empty((N, H, 4 * W, 3), dtype=np.uint8)
    for n in range(N):
        for y in range(H):
            for x in range(W):
                out[n, y, x] = pre[n, y, x]
                out[n, y, W + x] = post[n, y, x]
                out[n, y, 2 * W + x] = COLOURS.get(int(gt[n, y, x]), MAGENTA)
                out[n, y, 3 * W + x] = COLOURS.get(int(cls[n, y, x]), MAGENTA)
    return out


def input_conditions(msk):
    """what makes these inputs able to tell a wrong tie rule, a swapped threshold or a missing clause from the right one, as
    counts over the pixels of msk under the script's thresholds"""
    dmg = first_max(msk)
    c1, c2, c3 = clauses(msk, SCRIPT_THR)
    best = msk[..., 1:].max(axis=-1, keepdims=True)
    return {"pixels": int(dmg.size),
            "classes": sorted(np.unique(dmg).tolist()),
            "tie_share": float(((msk[..., 1:] == best).sum(axis=-1) > 1).mean()),
            "clause1": int(c1.sum()),
            "clause2_alone": int((c2 & ~c1 & ~c3).sum()),
            "clause3_alone": int((c3 & ~c1 & ~c2).sum()),
            "clause3_alone_classes": sorted(np.unique(dmg[c3 & ~c1 & ~c2]).tolist()),
            "dropped": int((~(c1 | c2 | c3)).sum())}
