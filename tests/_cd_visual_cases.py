"""The picture the reference's CDEvaluator saves per batch (models/evaluator.py:118-131) restated in numpy for the tests of
dh_cd_eval_vis_u8 / ops.cd_eval_vis / CDEvaluator.vis_picture, and the inputs those tests share.

    vis_input  = make_numpy_grid(de_norm(A))              float32 [rows H, cols W, 3]
    vis_input2 = make_numpy_grid(de_norm(B))              float32
    vis_pred   = make_numpy_grid(argmax(G_pred, 1, keepdim) * 255)      int64
    vis_gt     = make_numpy_grid(L)                       int64
    vis = clip(concatenate([...], axis=0), 0, 1)          float64
    plt.imsave(file, vis)                                 which stores (vis * 255).astype(uint8)

make_numpy_grid and de_norm are the package's restatements of the reference's utils (torchvision's make_grid, padding 0, 8
tiles per row).  The argmax is the first maximum (torch.argmax's and dh_argmax_nchw's rule).  Two forms: the composed one
the GPU tests compare with, and a per-pixel loop to check it against.  Everything ends in bytes: no tolerance anywhere."""
import numpy as np
import torch

from dahitra_amd.utils import de_norm, make_numpy_grid

F32 = np.float32
# (N, C, H, W): one tile with odd sizes, less than a workgroup (pixel-by-pixel path) | cols = 3 | a full row, five classes |
# a second row with seven empty tiles | three rows | the vector path at the evaluator's size, 64 units of 1024 pixels an image
SHAPES = [(1, 2, 5, 7), (3, 2, 16, 12), (8, 5, 8, 8), (9, 2, 16, 16), (17, 2, 4, 4), (2, 2, 256, 256)]
SMALL = [(1, 2, 5, 7), (3, 2, 4, 4), (9, 5, 3, 4)]
LABELS = (-1, 0, 1, 2, 255)
LOGIT_ALPHABET = (-1.0, 0.0, 0.5, 1.0)               # four values: a quarter of the two-class pixels tie


def loader_values():
    """the 256 values the loader makes of a byte: to_tensor's v / 255, then (x - 0.5) / 0.5, in float32"""
    v = np.arange(256, dtype=F32)
    return ((v / F32(255) - F32(0.5)) / F32(0.5)).astype(F32)


def grid_dims(N):
    cols = min(8, N)
    return (N + cols - 1) // cols, cols


def inputs(N, C, H, W, seed=None):
    """a, b float32 [N, 3, H, W]: loader values, one in 16 pushed outside [-1, 1]; logits float32 [N, C, H, W] from
    LOGIT_ALPHABET (planted ties); label int64 [N, 1, H, W], mostly 0 / 1 with -1, 2 and 255 among them"""
    rs = np.random.RandomState(1000 * N + 10 * H + C if seed is None else seed)
    lv = loader_values()

    def image():
        x = lv[rs.randint(0, 256, size=(N, 3, H, W))]
        return np.where(rs.randint(0, 16, size=x.shape) == 0, x * F32(1.25), x).astype(F32)
    a, b = image(), image()
    logits = np.asarray(LOGIT_ALPHABET, dtype=F32)[rs.randint(0, len(LOGIT_ALPHABET), size=(N, C, H, W))]
    label = np.asarray((0, 1, 0, 1, 0, 1) + LABELS, dtype=np.int64)[rs.randint(0, 6 + len(LABELS), size=(N, 1, H, W))]
    return a, b, logits, label


def first_max(logits):
    """[N, C, H, W] -> [N, H, W] int64: the lowest class that holds the maximum"""
    return np.argmax(logits, axis=1).astype(np.int64)


def float_picture(a, b, logits, label):
    """the reference's `vis` after the clip: float64 [4 rows H, cols W, 3] in [0, 1]"""
    label = label.reshape(label.shape[0], 1, *label.shape[-2:])
    vis_input = make_numpy_grid(de_norm(torch.from_numpy(a)))
    vis_input2 = make_numpy_grid(de_norm(torch.from_numpy(b)))
    vis_pred = make_numpy_grid(torch.from_numpy(first_max(logits)[:, None] * 255))
    vis_gt = make_numpy_grid(torch.from_numpy(label))
    assert vis_input.dtype == vis_input2.dtype == F32 and vis_pred.dtype == vis_gt.dtype == np.int64
    vis = np.concatenate([vis_input, vis_input2, vis_pred, vis_gt], axis=0)
    assert vis.dtype == np.float64
    return np.clip(vis, a_min=0.0, a_max=1.0)


def to_bytes(vis):
    """what plt.imsave stores of a float RGB array in [0, 1]"""
    return (vis * 255).astype(np.uint8)


def picture(a, b, logits, label):
    """-> [4 rows H, cols W, 3] uint8 RGB"""
    return to_bytes(float_picture(a, b, logits, label))


# ---- the slow form -------------------------------------------------------------------------------------------------------
def byte_slow(x):
    t = F32(F32(x) * F32(0.5)) + F32(0.5)
    assert type(t) is F32
    t = min(max(float(t), 0.0), 1.0)
    return int(t * 255)                               # float64 product, truncated


def picture_slow(a, b, logits, label):
    N, C, H, W = logits.shape
    label = label.reshape(N, H, W)
    rows, cols = grid_dims(N)
    out = np.zeros((4 * rows * H, cols * W, 3), dtype=np.uint8)
    for n in range(N):
        r, c = divmod(n, cols)
        for y in range(H):
            for x in range(W):
                best, cls = logits[n, 0, y, x], 0
                for k in range(1, C):
                    if logits[n, k, y, x] > best:
                        best, cls = logits[n, k, y, x], k
                for ch in range(3):
                    out[(0 * rows + r) * H + y, c * W + x, ch] = byte_slow(a[n, ch, y, x])
                    out[(1 * rows + r) * H + y, c * W + x, ch] = byte_slow(b[n, ch, y, x])
                out[(2 * rows + r) * H + y, c * W + x] = 255 if cls >= 1 else 0
                out[(3 * rows + r) * H + y, c * W + x] = 255 if label[n, y, x] >= 1 else 0
    return out


# ---- the pinned values ---------------------------------------------------------------------------------------------------
def boundary_t():
    """fl(k / 255) and its two float32 neighbours, k = 1 .. 255: [255, 3] float32 (below, at, above)"""
    t = (np.arange(1, 256, dtype=np.float64) / 255).astype(F32)
    return np.stack([np.nextafter(t, F32(-1)), t, np.nextafter(t, F32(2))], axis=1)


def pinned_x():
    """the float32 inputs whose bytes the tests pin, in four groups:
    loader: the 256 loader values; boundary: for every t of boundary_t() the float32 x nearest to 2 t - 1 and the float32 on
    either side of it (x * 0.5 + 0.5 reaches the float32 values around k / 255 as closely as an input can: the sum rounds
    at 2^-25 and coarser, while k / 255 below 1 / 2 has finer neighbours); ends: 0, 1, -1; outside: just outside and well
    outside [-1, 1]"""
    x = (2.0 * boundary_t().astype(np.float64) - 1.0).astype(F32).ravel()
    boundary = np.stack([np.nextafter(x, F32(-2)), x, np.nextafter(x, F32(2))], axis=1).ravel()
    ends = np.asarray([0.0, 1.0, -1.0], dtype=F32)
    outside = np.asarray([np.nextafter(F32(1), F32(2)), np.nextafter(F32(-1), F32(-2)), 1.5, -1.5, 3e38, -3e38], dtype=F32)
    return {"loader": loader_values(), "boundary": boundary, "ends": ends, "outside": outside}


PINNED_HW = ((27, 32), (32, 27))                      # 3 * 864 = 2592 values: the vector form and the pixel-by-pixel one


def pinned_inputs(H, W):
    """the pinned values as a one-image batch: a holds them in storage order, zero after them; b is a reversed; two classes
    of logits with a tie, a win and a loss in the first three pixels; the labels -1, 0, 1, 2, 255 in the first five"""
    groups = pinned_x()
    flat = np.concatenate([groups[k] for k in ("loader", "boundary", "ends", "outside")])
    assert flat.size == 256 + 255 * 9 + 3 + 6 <= 3 * H * W
    a = np.zeros(3 * H * W, dtype=F32)
    a[:flat.size] = flat
    b = a[::-1].copy()
    logits = np.zeros((1, 2, H, W), dtype=F32)
    logits[0, :, 0, :3] = [[0.25, 0.25, 0.5], [0.25, 0.5, 0.25]]
    label = np.zeros((1, 1, H, W), dtype=np.int64)
    label[0, 0, 0, :5] = LABELS
    return a.reshape(1, 3, H, W), b.reshape(1, 3, H, W), logits, label


def check_pinned(pic, H, W):
    """the bytes of pinned_inputs(H, W) in `pic` [4 H, W, 3], stated without the restatement"""
    assert pic.shape == (4 * H, W, 3) and pic.dtype == np.uint8
    got_a = pic[:H].transpose(2, 0, 1).ravel()                       # back to a's storage order
    got_b = pic[H:2 * H].transpose(2, 0, 1).ravel()
    assert np.array_equal(got_b, got_a[::-1])
    groups = pinned_x()
    at = 0
    got = {}
    for k in ("loader", "boundary", "ends", "outside"):
        got[k] = got_a[at:at + groups[k].size].astype(np.int64)
        at += groups[k].size
    assert (got_a[at:] == 127).all()                                 # x = 0: t = 0.5, 127.5 truncated
    # the loader's bytes come back as themselves or one lower, 63 of them one lower
    v = np.arange(256)
    assert set((v - got["loader"]).tolist()) == {0, 1} and int((v - got["loader"]).sum()) == 63
    assert got["loader"][0] == 0 and got["loader"][255] == 255 and got["loader"][1] == 0 and got["loader"][128] == 128
    # around k / 255: the float64 product of the float32 t, truncated
    x = groups["boundary"]
    t = np.clip((x * F32(0.5) + F32(0.5)).astype(F32).astype(np.float64), 0.0, 1.0)
    want = np.floor(t * 255).astype(np.int64)
    k = np.repeat(np.arange(1, 256), 9)
    assert np.array_equal(got["boundary"], want) and set((want - k).tolist()) == {-1, 0}
    assert ((want == k) == (t * 255 >= k)).all() and 0 < int((want == k).sum()) < want.size
    assert got["ends"].tolist() == [127, 255, 0]
    assert got["outside"].tolist() == [255, 0, 255, 0, 255, 0]
    # prediction: a tie is class 0 (black), class 1 strictly greater is white, smaller is black; every other pixel ties
    pred = pic[2 * H:3 * H]
    assert pred[0, :3].tolist() == [[0] * 3, [255] * 3, [0] * 3] and int(pred.astype(np.int64).sum()) == 3 * 255
    gt = pic[3 * H:]
    assert gt[0, :5].tolist() == [[0] * 3, [0] * 3, [255] * 3, [255] * 3, [255] * 3] and int(gt.astype(np.int64).sum()) == 9 * 255
