"""The 4-flip prediction of the reference's xBD script (xBD_code/predict_test_cls.py:62-94) restated in numpy for the tests
of dh_xbd_tta_pack_u8 / dh_xbd_tta_merge_u8 / models/xbd.predict_tta, and the inputs those tests share.

What the script does for one pre / post pair:
    x    = concatenate([pre, post], axis=2)                   [H, W, 6] uint8; cv2.imread: each image's channels are B, G, R
    x    = float32(x); x /= 127; x -= 1                       preprocess_inputs: two float32 operations
    inp  = [x, x[::-1], x[:, ::-1], x[::-1, ::-1]]            flip_0 .. flip_3, each moved to [6, H, W]
    s    = sigmoid(model(inp)) in float32                     [4, 5, H, W]
    pred = [s[0], s[1][:, ::-1, :], s[2][:, :, ::-1], s[3][:, ::-1, ::-1]]          every flip undone
    msk  = (asarray(pred).mean(axis=0) * 255).astype('uint8') moved to [H, W, 5]
numpy's mean over axis 0 of a float32 stack adds the four slices one after the other and divides by 4, all in float32."""
import numpy as np
import torch

LEVELS = (-40.0, 0.0, 40.0)
BYTES = (0, 31, 63, 95, 127, 159, 191, 223, 255)


def flip(a, k):
    """flip_k on the last two axes ([..., H, W]): bit 0 reverses the rows, bit 1 the columns; each is its own inverse"""
    if k & 1:
        a = a[..., ::-1, :]
    if k & 2:
        a = a[..., :, ::-1]
    return a


def sigmoid32(x):
    """torch.sigmoid on float32, the function the reference calls"""
    return torch.sigmoid(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))).numpy()


def pack(pre, post, order="bgr"):
    """pre, post [N, H, W, 3] uint8 (RGB as stored) -> [4N, 6, H, W] float32, image 4n + k = flip_k of pair n"""
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
    out = np.empty((4 * N, 6, H, W), dtype=np.float32)
    for n in range(N):
        for k in range(4):
            out[4 * n + k] = flip(x[n], k)
    return out


def mean32(u0, u1, u2, u3):
    """the float32 mean of four float32 maps in the order numpy's mean(axis=0) adds them"""
    t = ((u0 + u1) + u2) + u3
    assert t.dtype == np.float32
    return t / np.float32(4)


def merge(logits, s=None):
    """logits [4N, 5, H, W] float32 -> [N, H, W, 5] uint8"""
    s = sigmoid32(logits) if s is None else s
    assert s.dtype == np.float32 and s.shape[0] % 4 == 0 and s.shape[1] == 5
    N = s.shape[0] // 4
    out = np.empty((N,) + s.shape[2:] + (5,), dtype=np.uint8)
    for n in range(N):
        m = mean32(*(flip(s[4 * n + k], k) for k in range(4))) * np.float32(255)
        assert m.dtype == np.float32
        out[n] = np.trunc(m).astype(np.uint8).transpose(1, 2, 0)
    return out


def merge64(logits):
    """v = 255 * mean of the float64 sigmoids, [N, H, W, 5] float64: the value whose floor the byte is"""
    x = np.asarray(logits, dtype=np.float64)
    s = 1.0 / (1.0 + np.exp(-x))
    N = s.shape[0] // 4
    v = np.empty((N,) + s.shape[2:] + (5,), dtype=np.float64)
    for n in range(N):
        v[n] = (255.0 * sum(flip(s[4 * n + k], k) for k in range(4)) / 4.0).transpose(1, 2, 0)
    return v


BAND = 1e-3        # bytes.  A few ulp of expf (2^-24 relative each) on values <= 1, the four float32 roundings of the sum and
                   # the one of the product, times 255 / 4 per term: below 1e-4 of a byte; the band is ten times that


def check_against_merge64(got, v, cap=0.005):
    """every byte is floor(v), except where v lies within BAND of an integer: there either neighbour passes.  Returns the
    share of such undecided bytes, which must stay under `cap`."""
    got = np.asarray(got).astype(np.int64)
    near = np.abs(v - np.round(v)) < BAND
    lo = np.floor(v).astype(np.int64)
    exact = got == np.clip(lo, 0, 255)
    either = near & ((got == np.clip(np.round(v).astype(np.int64), 0, 255)) | (got == np.clip(np.round(v).astype(np.int64) - 1, 0, 255)))
    share = float(near.mean())
    bad = ~(exact | either)
    assert not bad.any(), "%d bytes differ outside the band, first at %s: got %d, v = %.6f" % (
        bad.sum(), np.argwhere(bad)[0].tolist(), got[bad][0], v[bad][0])
    assert share <= cap, "condition: at most %.1f %% of the bytes may be undecided, %.3f %% are" % (100 * cap, 100 * share)
    return share


# ---- inputs --------------------------------------------------------------------------------------------------------------
def sources(N, H, W, seed):
    """asymmetric random bytes: a swapped or missing flip, a swapped pre / post or a swapped channel order changes them"""
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, (N, H, W, 3)).astype(np.uint8), rng.randint(0, 256, (N, H, W, 3)).astype(np.uint8)


def three_level(N, H, W, seed):
    """logits [4N, 5, H, W] float32 with values in {-40, 0, +40}"""
    rng = np.random.RandomState(seed)
    return rng.choice(np.asarray(LEVELS, dtype=np.float32), size=(4 * N, 5, H, W))


def equivariant(H, W, seed):
    """logits[k] = flip_k(L) for one asymmetric three-level map L [5, H, W]: the four un-flipped maps agree everywhere, so the
    output is the quantisation of sigmoid(L) alone: 0, 127 or 255.  Returns (logits [4, 5, H, W], L)."""
    L = three_level(1, H, W, seed)[0]
    assert not np.array_equal(L, L[:, ::-1]) and not np.array_equal(L, L[:, :, ::-1])
    return np.ascontiguousarray(np.stack([flip(L, k) for k in range(4)])), L


def random_logits(N, H, W, seed):
    return (np.random.RandomState(seed).randn(4 * N, 5, H, W) * 3).astype(np.float32)


def check_three_level(logits):
    """the conditions under which the comparison of the merge may be exact: no last bit of an expf can decide a byte"""
    assert logits.dtype == np.float32 and set(np.unique(logits).tolist()) <= set(LEVELS)
    s = sigmoid32(np.asarray(LEVELS, dtype=np.float32))
    assert 0 < s[0] < 1e-17 and s[1] == np.float32(0.5) and s[2] == np.float32(1.0), s
    # a device expf that is a few ulp off leaves the three sigmoids where they are, as far as a float32 sum with 0.5 or 1 sees
    for tiny in (s[0], np.float32(2) * s[0], np.float32(0.5) * s[0]):
        assert np.float32(0.5) + np.float32(4) * tiny == np.float32(0.5) and np.float32(4) * tiny * np.float32(255) < 1e-12
    # every mean is a multiple of 1/8 (up to the 4e-18 terms, which a sum with a nonzero level absorbs): partial sums are exact
    v = merge64(logits)
    eighths = v / 255.0 * 8
    assert np.abs(eighths - np.round(eighths)).max() < 1e-12
    # v is at least 0.125 from an integer unless all four un-flipped values agree; then it is 0, 127.5 or 255
    N = logits.shape[0] // 4
    U = np.stack([np.stack([flip(logits[4 * n + k], k) for k in range(4)]) for n in range(N)])          # [N, 4, 5, H, W]
    all_same = (U == U[:, :1]).all(axis=1).transpose(0, 2, 3, 1)
    frac = np.abs(v - np.round(v))
    assert (frac[~all_same] >= 0.125 - 1e-9).all()
    assert np.isin(np.round(v[all_same] * 2), (0, 255, 510)).all() and np.abs(v[all_same] * 2 - np.round(v[all_same] * 2)).max() < 1e-9
    out = merge(logits)
    assert set(np.unique(out).tolist()) <= set(BYTES), np.unique(out)
    assert np.array_equal(out, np.clip(np.floor(v + 1e-9), 0, 255).astype(np.uint8))
    return out
