"""What tests/test_xbd_jitter_cpu.py and tests/test_xbd_jitter_gpu.py share: the sources, parameter rows and ColorJitter
parameters of the kernel-against-Pillow comparison, and the host chain they are compared with -- window, flips,
crop(box).resize(BILINEAR), the ImageEnhance chain, the mask channels, preprocess_inputs (xBD_code/train.py:99-183)."""
import itertools

import numpy as np
from PIL import Image, ImageEnhance

# float32 factors at which fma(alpha, i - d, d) and Pillow's unfused blend differ (for 123 and 120 of the 65 536 (d, i) pairs)
PINNED = (0.9493669867515564, 1.0305343866348267)
assert [int(np.float32(f).view(np.int32)) for f in PINNED] == [1064503735, 1065609357]

H, W = 80, 96
PERMS = list(itertools.permutations(range(4)))          # 24 drawn orders: 0 brightness, 1 contrast, 2 saturation, 3 hue (nothing)


def pil_jitter(img_u8, order, factors):
    """torchvision's ColorJitter.forward on a PIL image: F.adjust_brightness / contrast / saturation are these three lines"""
    im = Image.fromarray(np.ascontiguousarray(img_u8))
    for op in order:
        if op == 0:
            im = ImageEnhance.Brightness(im).enhance(factors[0])
        elif op == 1:
            im = ImageEnhance.Contrast(im).enhance(factors[1])
        elif op == 2:
            im = ImageEnhance.Color(im).enhance(factors[2])
    return np.asarray(im)


def clips(img_u8, order, factors):
    """{0: .., 255: ..}: whether some operation of the chain brings a byte that was not 0 (255) to 0 (255): Pillow's clip acts"""
    hit = {0: False, 255: False}
    for op in order:
        out = pil_jitter(img_u8, [op], factors)
        for v in hit:
            hit[v] |= bool(((out == v) & (img_u8 != v)).any())
        img_u8 = out
    return hit


def blocky(rng, n, h, w, values):
    small = rng.choice(np.asarray(values, dtype=np.uint8), size=(n, -(-h // 8), -(-w // 8)))
    return np.ascontiguousarray(np.kron(small, np.ones((1, 8, 8), dtype=np.uint8))[:, :h, :w])


def sources(seed=11, h=H, w=W):
    """three samples: 0 bright noise (180 .. 255: brightness, contrast and saturation above 1 clip at 255), 1 dark noise
    (0 .. 59, a fifth of it 0: contrast and saturation above 1 reach 0), 2 plain noise; pre mask 0 / 255, label 0 .. 4"""
    rng = np.random.RandomState(seed)

    def pair(lo, hi):
        return rng.randint(lo, hi, (2, h, w, 3)).astype(np.uint8)

    bright, dark, plain = pair(180, 256), pair(0, 60), pair(0, 256)
    dark[rng.rand(*dark.shape) < 0.2] = 0
    pre, post = (np.ascontiguousarray(np.stack([bright[i], dark[i], plain[i]])) for i in (0, 1))
    return pre, post, blocky(rng, 3, h, w, [0, 255]), blocky(rng, 3, h, w, [0, 1, 2, 3, 4])


def rows_for(S):
    """x0, y0, hflip, vflip, resize, top, left, height, width inside the 80 x 96 sources: without and with the box, both flips"""
    return [[5, 9, 0, 0, 0, 0, 0, S, S],
            [W - S, H - S, 1, 0, 0, 0, 0, S, S],
            [0, 0, 0, 1, 1, 0, 13, S, S - 13],
            [7, 3, 0, 0, 1, 9, 0, S - 9, S],
            [11, 2, 1, 1, 1, 13, 7, S - 13, S - 7],
            [20, 10, 1, 0, 1, 6, 11, 51, 45]]


IDX = [0, 1, 2, 1, 0, 2]                                 # bright, dark, plain, dark, bright, plain


def jitter_cases():
    """one (pre, post) pair per row of rows_for: the pre images take the six effective orders with hue at position 0, 1, 2,
    3, 0, 1 of the permutation, the post images the six in another sequence with hue elsewhere; the pinned factors sit on
    contrast and on saturation (both ways round), the others are 0.8, 1.0, 1.2 and random float32 values in [0.8, 1.2]"""
    rng = np.random.RandomState(5)
    rnd = lambda: float(np.float32(rng.uniform(0.8, 1.2)))
    eff = list(itertools.permutations(range(3)))

    def with_hue(order, at):
        order = list(order)
        order.insert(at, 3)
        return order

    factors = [(1.2, PINNED[0], PINNED[1]), (0.8, PINNED[1], PINNED[0]), (rnd(), PINNED[0], 1.2), (1.0, 1.2, PINNED[1]),
               (rnd(), rnd(), rnd()), (1.2, 0.8, PINNED[0])]
    cases = []
    for k in range(6):
        pre = (with_hue(eff[k], k % 4), factors[k])
        post = (with_hue(eff[(k + 3) % 6], (k + 2) % 4), factors[(k + 1) % 6])
        cases.append((pre, post))
    assert {tuple(o for o in c[0][0] if o != 3) for c in cases} == set(eff) == {tuple(o for o in c[1][0] if o != 3) for c in cases}
    assert {c[0][0].index(3) for c in cases} | {c[1][0].index(3) for c in cases} == {0, 1, 2, 3}
    return cases


def preprocess_inputs(x):
    """xBD_code/utils.py:112-116"""
    x = np.asarray(x, dtype='float32')
    x /= 127
    x -= 1
    return x


def host_windows(src, i, row, S):
    """the four arrays of sample i after crop, flips and resized_crop, as uint8"""
    x0, y0, hf, vf, rs, top, left, bh, bw = row

    def window(a):
        a = a[i, y0:y0 + S, x0:x0 + S]
        a = a[:, ::-1] if hf else a
        a = a[::-1] if vf else a
        a = np.ascontiguousarray(a)
        if rs:
            a = np.asarray(Image.fromarray(a).crop((left, top, left + bw, top + bh)).resize((S, S), Image.BILINEAR))
        return a

    return [window(a) for a in src]


def host_sample(src, i, row, S, jitter, enhance=pil_jitter):
    """one training sample as the reference builds it (train.py:110-183) with `jitter` = None or ((order, factors) of pre,
    of post): (img [6, S, S] float32, msk [5, S, S] uint8)"""
    img1, img2, _, lbl_msk1 = host_windows(src, i, row, S)
    if jitter is not None:
        img1, img2 = enhance(img1, *jitter[0]), enhance(img2, *jitter[1])
    msk = np.stack([np.zeros_like(lbl_msk1)] + [np.where(lbl_msk1 == k, 255, 0).astype(np.uint8) for k in (1, 2, 3, 4)], axis=2) > 127
    msk[..., 0][msk[..., 1:].max(axis=2)] = True
    img = preprocess_inputs(np.concatenate([img1, img2], axis=2)).transpose(2, 0, 1)
    return img, (msk * 1).transpose(2, 0, 1).astype(np.uint8)
