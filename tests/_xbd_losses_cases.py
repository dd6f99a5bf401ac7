"""What tests/test_xbd_losses_cpu.py and tests/test_xbd_losses_gpu.py share: the numpy float64 restatement of the Lovasz terms of
xBD_code/losses.py as csrc/xbd_seg_losses.hip defines them, the restatement of its jaccard / bce / mask_bceavg terms, the inputs
of the kernel tests and the bounds.

The restatement of the Lovasz terms.  x fp32 [B, C, ...], target of its shape.  An element is VALID when its target is 0 or 1;
the value `ignore` and every other value are dropped (the others are counted: `bad`).  A segment is a channel over the batch
(c) or, per image, a plane (b * C + c).  In float32, as the kernel forms them:
    mode 0  e = 1 - x (2 t - 1), weight max(e, 0)      mode 1  e = |t - x|      mode 2  e = |t - p|, p = 1 / (1 + exp(-x))
Order of a segment: np.lexsort over (-e, dropped), stable -- descending e, equal e (+0 == -0) in flat index order, dropped
elements last.  Then everything in float64 from integers: G ones in the segment, c1 / c0 the ones / zeros up to and including an
element, I = G - c1, U = G + c0, g = 1 - I / U for the first element, 1 / U at a one, I / ((U - 1) U) at a zero; segment loss =
sum weight g; channel loss = the segment's, or per image the mean over the B images (an empty one counts 0); loss = sum_c w_c
channel loss; dx = w_c (/ B per image) g d weight / dx with relu'(0) = 0 and sign(0) = 0 as torch has them."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "xbd_losses.npz")
NAMES = os.path.join(HERE, "golden", "xbd_losses_names.json")
ULP = 2.0 ** -23
MODES = {"hinge": 0, "probas": 1, "sigmoid": 2}
TERMS = ("bce", "dice", "focal", "jaccard", "lovasz", "lovasz_sigmoid", "mask_bceavg")
MIX = {'dice': 1, 'focal': 8, 'lovasz': 0.5, 'jaccard': 0.3, 'bce': 0.2}
# gradient bounds of the kernel against the restatement, relative, element by element (plus 1e-12 absolute): modes 0 and 1 carry
# one correctly rounded quotient of integers, at most two roundings of converted integers and a sign; mode 2 also p (1 - p)
GRAD_BOUND = {0: 4 * ULP, 1: 4 * ULP, 2: 8 * ULP}
GRAD_ABS = 1e-12


def golden():
    return np.load(GOLDEN)


def names():
    return json.load(open(NAMES))


def sigmoid32(x):
    one = np.float32(1)
    return (one / (one + np.exp(-np.asarray(x, dtype=np.float32)))).astype(np.float32)


def errors(x, label, mode):
    """the float32 errors and what mode 2 takes them of (the probabilities), for labels 0 / 1"""
    x = np.asarray(x, dtype=np.float32)
    t = label.astype(np.float32)
    if mode == 0:
        return (np.float32(1) - x * (np.float32(2) * t - np.float32(1))).astype(np.float32), x
    p = sigmoid32(x) if mode == 2 else x
    return np.abs(t - p).astype(np.float32), p


def classify(target, ignore):
    """label (0 where dropped), valid, the count of targets that are neither 0, 1 nor `ignore`"""
    t = np.asarray(target).astype(np.float64).reshape(-1)
    valid = (t == 0) | (t == 1)
    dropped = np.zeros_like(valid) if ignore is None else t == float(ignore)
    return np.where(valid, t, 0).astype(np.int64), valid, int((~valid & ~dropped).sum())


def segment_ids(shape, per_image):
    B, C = shape[:2]
    n = int(np.prod(shape))
    plane = np.arange(n) // (n // (B * C))
    return (plane if per_image else plane % C), (B * C if per_image else C)


def closed_form_g(label_sorted):
    """the gradient of the Lovasz extension for the labels of a segment in sorted order, float64"""
    lab = np.asarray(label_sorted, dtype=np.int64)
    if lab.size == 0:
        return np.zeros(0)
    G = float(lab.sum())
    c1 = np.cumsum(lab).astype(np.float64)
    c0 = np.cumsum(1 - lab).astype(np.float64)
    I, U = G - c1, G + c0
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(lab == 1, 1.0 / U, I / ((U - 1.0) * U))
    g[0] = 1.0 - I[0] / U[0]
    return g


def jaccard_differences(label_sorted):
    """lovasz_grad of xBD_code/losses.py:129-141 in float64: the differences of 1 - I / U"""
    lab = np.asarray(label_sorted, dtype=np.float64)
    G = lab.sum()
    jac = 1.0 - (G - np.cumsum(lab)) / (G + np.cumsum(1.0 - lab))
    out = jac.copy()
    out[1:] = jac[1:] - jac[:-1]
    return out, jac


def lovasz_order(x, target, mode, per_image=False, ignore=255):
    x = np.asarray(x, dtype=np.float32)
    label, valid, _ = classify(target, ignore)
    e, _ = errors(x.reshape(-1), label, MODES.get(mode, mode))
    seg, _ = segment_ids(x.shape, per_image)
    key = np.where(valid, -(e + np.float32(0)), np.float32(0))          # -0 + 0 = +0
    return np.lexsort((key, ~valid, seg)).astype(np.int64)


def lovasz(x, target, mode, per_image=False, ignore=255, weights=None, order=None):
    """{'loss', 'channel' [C], 'dx' like x, 'bad', 'order' [n], 'gap': the least distance between sorted neighbours' errors}"""
    mode = MODES.get(mode, mode)
    x = np.asarray(x, dtype=np.float32)
    B, C = x.shape[:2]
    n = x.size
    label, valid, bad = classify(target, ignore)
    e, p = errors(x.reshape(-1), label, mode)
    seg, nseg = segment_ids(x.shape, per_image)
    order = lovasz_order(x, target, mode, per_image, ignore) if order is None else np.asarray(order)
    w = np.ones(C) if weights is None else np.asarray(weights, dtype=np.float32).astype(np.float64)
    L = n // nseg
    seg_loss = np.zeros(nseg)
    dx = np.zeros(n)
    gap = np.inf
    for s in range(nseg):
        idx = order[s * L:(s + 1) * L]
        assert (seg[idx] == s).all()
        idx = idx[valid[idx]]
        if idx.size == 0:
            continue
        lab = label[idx]
        es = e[idx].astype(np.float64)
        if idx.size > 1:
            gap = min(gap, float(np.min(es[:-1] - es[1:])))
        g = closed_form_g(lab)
        sign = 2.0 * lab - 1.0
        if mode == 0:
            weight = np.maximum(es, 0.0)
            slope = np.where(es > 0, -sign, 0.0)
        else:
            pi = p.reshape(-1)[idx].astype(np.float64)
            weight = es
            slope = -np.sign(lab - pi)
            if mode == 2:
                slope = slope * pi * (1.0 - pi)
        seg_loss[s] = float(np.sum(weight * g))
        c = s % C
        dx[idx] = w[c] / (B if per_image else 1) * g * slope
    channel = seg_loss.reshape(B, C).mean(0) if per_image else seg_loss
    return {"loss": float(np.sum(w * channel)), "channel": channel, "dx": dx.reshape(x.shape), "bad": bad, "order": order,
            "gap": gap}


def lovasz_float32(x, target, mode, per_image=False, ignore=255, weights=None):
    """the same loss the way the reference's ten lines form it in float32 (cumulative sums, 1 - I / U, its differences, a dot
    product): its distance from lovasz() is the yardstick of a kernel test's loss"""
    mode = MODES.get(mode, mode)
    x = np.asarray(x, dtype=np.float32)
    B, C = x.shape[:2]
    label, valid, _ = classify(target, ignore)
    e, _ = errors(x.reshape(-1), label, mode)
    seg, nseg = segment_ids(x.shape, per_image)
    order = lovasz_order(x, target, mode, per_image, ignore)
    L = x.size // nseg
    seg_loss = np.zeros(nseg, dtype=np.float32)
    for s in range(nseg):
        idx = order[s * L:(s + 1) * L]
        idx = idx[valid[idx]]
        if idx.size == 0:
            continue
        lab = label[idx].astype(np.float32)
        G = lab.sum(dtype=np.float32)
        jac = np.float32(1) - (G - np.cumsum(lab, dtype=np.float32)) / (G + np.cumsum(np.float32(1) - lab, dtype=np.float32))
        g = jac.copy()
        g[1:] = jac[1:] - jac[:-1]
        es = e[idx]
        seg_loss[s] = np.dot(np.maximum(es, np.float32(0)) if mode == 0 else es, g)
    channel = seg_loss.reshape(B, C).mean(0, dtype=np.float32) if per_image else seg_loss
    w = np.ones(C, dtype=np.float32) if weights is None else np.asarray(weights, dtype=np.float32)
    return float(np.sum(w * channel, dtype=np.float32))


def loss_bound(ref, yardstick):
    """max(2 * yardstick, 2 ulp), absolute, for a loss whose float64 value is `ref`"""
    return max(2.0 * yardstick, 2.0 * float(np.spacing(np.float32(abs(ref)))))


def seg_terms(x, target, weights=None):
    """jaccard, bce, mask_bceavg, dice per channel over the batch in float64 on the float64 sigmoid of the logits x [B, C, ...]:
    {'terms' [C, 4], 'grads' [4] arrays like x (each term's own gradient, times w_c)}"""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    B, C = x64.shape[:2]
    t = np.asarray(target).astype(np.float64).reshape(x64.shape)
    w = np.ones(C) if weights is None else np.asarray(weights, dtype=np.float32).astype(np.float64)
    s = 1.0 / (1.0 + np.exp(-x64))
    ax = tuple(a for a in range(x64.ndim) if a != 1)
    keep = lambda v: np.expand_dims(v, ax)
    I, S, T = (s * t).sum(ax), s.sum(ax), t.sum(ax)
    N = x64.size / C
    eps = 1e-6
    U = S + T - I + eps
    jac = 1.0 - (I + eps) / U
    bce = (np.maximum(x64, 0) - x64 * t + np.log1p(np.exp(-np.abs(x64)))).mean(ax)
    with np.errstate(divide="ignore"):
        mask = -(t * np.maximum(np.log(s), -100.0) + (1.0 - t) * np.maximum(np.log1p(-s), -100.0)).mean(ax)
    D = S + T + eps
    dice = 1.0 - (2.0 * I + eps) / D
    sp = s * (1.0 - s)
    wk = keep(w)
    grads = [wk * (-(t * keep(U) - (keep(I) + eps) * (1.0 - t)) / keep(U) ** 2) * sp,
             wk * (s - t) / N,
             wk * (s - t) / np.maximum(sp, 1e-12) * sp / N,
             wk * (-(2.0 * t * keep(D) - (2.0 * keep(I) + eps)) / keep(D) ** 2) * sp]
    return {"terms": np.stack([jac, bce, mask, dice], 1), "grads": grads}


# ---- inputs of the kernel tests ---------------------------------------------------------------------------------
def hinge_inputs(shape, seed, tile):
    """logits and uint8 labels for modes 0 and 1 (mode 1 reads them as 'probabilities'; the kernel does not mind their range):
    the errors vary in all four key bytes, take both signs, +0 and -0, and hold one run of equal keys longer than 2 * tile where
    the input holds 4 tiles or more"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    t = (rng.random(n) < 0.4).astype(np.uint8)
    x = (rng.standard_normal(n) * np.exp(rng.uniform(-12, 6, n))).astype(np.float32)       # exponents far apart: every key byte
    k = rng.permutation(n)
    q = n // 8
    x[k[:q]] = np.where(t[k[:q]] == 1, 1.0, -1.0)             # e = 1 - 1 = +0 (mode 0)
    x[k[q:2 * q]] = x[k[q]] if n > 8 else x[k[q:2 * q]]       # a run of equal logits
    if n >= 4 * tile:
        run = np.sort(k[2 * q:2 * q + 2 * tile + 2])           # ... and one of equal ERRORS longer than 2 tiles
        x[run] = np.where(t[run] == 1, 0.25, -0.25)
    if n > 4:
        x[k[-1]] = 0.0                                        # mode 1: |0 - 0| = +0 or |1 - 0|
        x[k[-2]] = -0.0
    return x.reshape(shape), t.reshape(shape)


def sigmoid_inputs(shape, seed, per_image, labels=None):
    """logits for mode 2 whose errors no last-bit difference of a sigmoid can reorder: inside every segment the errors are
    DISTINCT points j * 2^-17 of (1/4, 3/4), every element takes part; x = logit(q), q = the point (label 0) or 1 - it (label 1)"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    t = (rng.random(n) < 0.4).astype(np.uint8) if labels is None else np.asarray(labels, dtype=np.uint8).reshape(-1)
    seg, nseg = segment_ids(shape, per_image)
    L = n // nseg
    assert L < 65536, "at most 65535 grid points in (1/4, 3/4)"
    e = np.zeros(n)
    for s in range(nseg):
        e[seg == s] = 0.25 + rng.permutation(np.arange(1, 65536))[:L] * 2.0 ** -17
    q = np.where(t == 1, 1.0 - e, e)
    return np.log(q / (1.0 - q)).astype(np.float32).reshape(shape), t.reshape(shape)
