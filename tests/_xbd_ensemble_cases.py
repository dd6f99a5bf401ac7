"""The xBD predictor for a list of M snapshots and V = 4 or 8 views, restated in numpy for the tests of
dh_xbd_tta_pack_views_u8 / dh_xbd_tta_merge_multi_u8 / models/xbd.predict_ensemble, and the inputs those tests share.

What the script's loop does with a list `models` (xBD_code/predict_test_cls.py:81-94), here for V views instead of its four:
    inp  = [view_0(x), ..., view_{V-1}(x)]                     one batch, the same for every model
    pred = []
    for model in models:
        s = sigmoid(model(inp)) in float32                     [V, 5, H, W]
        for v in range(V): pred.append(unview_v(s[v]))
    msk  = (asarray(pred).mean(axis=0) * 255).astype('uint8')  moved to [H, W, 5]
numpy's mean over axis 0 of a float32 stack adds the M * V slices one after the other, model-major and view-minor, and divides by
M * V, all in float32.

view_v = flip_v for v < 4 (_xbd_tta_cases.flip: bit 0 reverses the rows, bit 1 the columns); view_{4+k} is the transpose of
flip_k, view_{4+k}(x)[c][i][j] = flip_k(x)[c][j][i], and it is undone by flip_k(transpose(s)).

The kernels work on 32 x 32 pixel tiles (csrc/xbd_ensemble.hip, EN_TILE), so the sizes below -- one vector group, around the
tile edge on both paths, a partial tile on the vector path, several tiles plus a partial one -- are the ones at which they can
go wrong."""
import numpy as np

import _xbd_tta_cases as T

TILE = 32
SIZES = (4, 31, 32, 33, 36, 68)          # S = H = W: 31 and 33 take the scalar path (S % 4 != 0)
BATCHES = (1, 2)
RANDOM_CASES = [(M, V, S, 2 if S == 36 else 1, 1000 * M + 100 * V + S)          # (M, V, S, N, seed) of the random-logit tests
                for M, V in ((3, 4), (3, 8), (2, 8)) for S in (33, 36, 68)]
EXACT_MV = ((2, 4), (1, 8), (2, 8), (4, 8))


def view(a, v):
    """view_v on the last two axes"""
    a = T.flip(a, v & 3)
    return np.swapaxes(a, -1, -2) if v >= 4 else a


def unview(s, v):
    """what brings view_v's image back: flip_k for v = k < 4, flip_k(transpose(s)) for v = 4 + k"""
    return T.flip(np.swapaxes(s, -1, -2) if v >= 4 else s, v & 3)


def pack_views(pre, post, order="bgr", V=4):
    """pre, post [N, H, W, 3] uint8 (RGB as stored) -> [V N, 6, H, W] float32, image V n + v = view_v of pair n"""
    if order == "bgr":
        pre, post = pre[..., ::-1], post[..., ::-1]
    elif order != "rgb":
        raise ValueError(order)
    x = np.concatenate([pre, post], axis=3).astype(np.float32)
    x = x / np.float32(127)
    x = x - np.float32(1)
    assert x.dtype == np.float32
    x = x.transpose(0, 3, 1, 2)
    N, _, H, W = x.shape
    assert V == 4 or (V == 8 and H == W)
    out = np.empty((V * N, 6, H, W), dtype=np.float32)
    for n in range(N):
        for v in range(V):
            out[V * n + v] = view(x[n], v)
    return out


def mean32(us):
    """the float32 mean of a list of float32 maps in the order numpy's mean(axis=0) adds them: one after the other, then a
    true division by the count"""
    t = us[0]
    for u in us[1:]:
        t = t + u
    assert t.dtype == np.float32
    return t / np.float32(len(us))


def stack(s_list, V, n):
    """the script's `pred` for image n: model-major, view-minor, every view undone"""
    return [unview(s[V * n + v], v) for s in s_list for v in range(V)]


def merge_multi(logits_list, V=4):
    """logits_list: M arrays [V N, 5, H, W] float32 -> [N, H, W, 5] uint8"""
    s_list = [T.sigmoid32(l) for l in logits_list]
    shape = s_list[0].shape
    assert all(s.dtype == np.float32 and s.shape == shape for s in s_list) and shape[0] % V == 0 and shape[1] == 5
    N = shape[0] // V
    out = np.empty((N,) + shape[2:] + (5,), dtype=np.uint8)
    for n in range(N):
        m = mean32(stack(s_list, V, n)) * np.float32(255)
        assert m.dtype == np.float32
        out[n] = np.trunc(m).astype(np.uint8).transpose(1, 2, 0)
    return out


def merge_multi64(logits_list, V=4):
    """v = 255 * mean of the float64 sigmoids, [N, H, W, 5] float64: the value whose floor the byte is"""
    s_list = [1.0 / (1.0 + np.exp(-np.asarray(l, dtype=np.float64))) for l in logits_list]
    N = s_list[0].shape[0] // V
    v = np.empty((N,) + s_list[0].shape[2:] + (5,), dtype=np.float64)
    for n in range(N):
        v[n] = (255.0 * sum(stack(s_list, V, n)) / float(len(s_list) * V)).transpose(1, 2, 0)
    return v


# ---- inputs --------------------------------------------------------------------------------------------------------------
def three_level_multi(M, V, N, S, seed):
    """M arrays [V N, 5, S, S] float32 with values in {-40, 0, +40}"""
    rng = np.random.RandomState(seed)
    return [rng.choice(np.asarray(T.LEVELS, dtype=np.float32), size=(V * N, 5, S, S)) for _ in range(M)]


def random_multi(M, V, N, S, seed):
    rng = np.random.RandomState(seed)
    return [(rng.randn(V * N, 5, S, S) * 3).astype(np.float32) for _ in range(M)]


def asymmetric(L):
    """no flip and no transpose maps L [..., S, S] to itself"""
    return all(not np.array_equal(view(L, v), L) for v in range(1, 8))


def equivariant_multi(M, V, S, seed):
    """logits[m][v] = view_v(L) for one three-level map L [5, S, S] that is asymmetric under both flips and the transpose: all
    M V un-viewed maps agree, so the output is the quantisation of sigmoid(L) alone.  Returns (list of M [V, 5, S, S], L)."""
    L = T.three_level(1, S, S, seed)[0]
    assert asymmetric(L)
    one = np.ascontiguousarray(np.stack([view(L, v) for v in range(V)]))
    return [one.copy() for _ in range(M)], L


def one_hot_models(M, V, S, seed):
    """logits[m][v] = view_v(L_m), L_m = +40 where an asymmetric random region map equals m and -40 elsewhere: at a pixel of
    region r exactly model r says 1, in every one of its V views, and every other model 0, so the mean is 1 / M there:
    byte trunc(255 / M).  A model read twice, left out or read in another model's place changes whole regions.
    Returns (list of M [V, 5, S, S], region [5, S, S])."""
    region = np.random.RandomState(seed).randint(0, M, size=(5, S, S))
    assert asymmetric(region)
    out = []
    for m in range(M):
        L = np.where(region == m, np.float32(40), np.float32(-40)).astype(np.float32)
        out.append(np.ascontiguousarray(np.stack([view(L, v) for v in range(V)])))
    return out, region


def check_three_level_multi(logits_list, V):
    """the conditions under which the comparison of the merge may be exact, for K = M V terms, K a power of two up to 32: no
    last bit of an expf and no rounding of a sum, the quotient or the product can decide a byte.  Returns the expected bytes."""
    K = len(logits_list) * V
    assert K in (4, 8, 16, 32), "a mean over a count that is no power of two (8 / 24, say) rounds before it is truncated"
    for l in logits_list:
        assert l.dtype == np.float32 and set(np.unique(l).tolist()) <= set(T.LEVELS)
    s = T.sigmoid32(np.asarray(T.LEVELS, dtype=np.float32))
    assert 0 < s[0] < 1e-17 and s[1] == np.float32(0.5) and s[2] == np.float32(1.0), s
    # a device expf that is a few ulp off leaves the three sigmoids where they are, as far as a float32 sum with 0.5 or more sees
    for tiny in (s[0], np.float32(2) * s[0], np.float32(0.5) * s[0]):
        assert np.float32(0.5) + np.float32(K) * tiny == np.float32(0.5) and np.float32(K) * tiny * np.float32(255) < 1e-12
    N = logits_list[0].shape[0] // V
    for n in range(N):
        us = stack([T.sigmoid32(l) for l in logits_list], V, n)
        es = stack([(np.sign(l).astype(np.float64) + 1) / 2 for l in logits_list], V, n)      # the levels' sigmoids: 0, 0.5, 1
        t32, t64 = us[0], es[0]
        for u, e in zip(us[1:], es[1:]):
            t32, t64 = t32 + u, t64 + e
            # every partial sum is exactly representable: a multiple of 0.5 up to 32 (the 4e-18 terms are absorbed by a
            # nonzero level and stay below 1e-15 without one)
            assert t32.dtype == np.float32
            assert np.where(t64 > 0, t32.astype(np.float64) == t64, t32 < 1e-15).all()
        mean = t32 / np.float32(K)
        assert mean.dtype == np.float32 and np.array_equal(mean.astype(np.float64) * K, t32.astype(np.float64)), "the quotient is exact"
        prod = mean * np.float32(255)                     # j * 255 / (2 K), j <= 2 K: 14 bits over a power of two
        assert np.where(t64 > 0, prod.astype(np.float64) == mean.astype(np.float64) * 255.0, prod < 1e-12).all(), "the product is exact"
    v = merge_multi64(logits_list, V)
    steps = v / 255.0 * (2 * K)
    assert np.abs(steps - np.round(steps)).max() < 1e-9
    out = merge_multi(logits_list, V)
    assert np.array_equal(out, np.clip(np.floor(v + 1e-9), 0, 255).astype(np.uint8))
    return out
