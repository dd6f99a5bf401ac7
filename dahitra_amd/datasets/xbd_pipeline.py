"""Pre-decoded xBD samples resident in HBM + TrainData / ValData.__getitem__ on the device (dh_xbd_augment_u8).

The reference's xBD loader opens four 1024x1024 PNGs per sample (pre and post image, pre mask, post label) and, in training,
crops, flips and bilinearly resizes all four in Pillow before it builds the mask channels (xBD_code/train.py:99-183); DataLoader
workers do not feed the MI355X xBD step that way.  Here the four uint8 stacks are decoded once and stay on the device, and ONE
kernel per batch produces what `GraphedXbdStep(net, opt, imgs, msks)` consumes: crop, flips, TF.resized_crop -- Pillow's
two-pass fixed-point BILINEAR resize, byte for byte, on the masks as well -- the five mask channels and preprocess_inputs.

    pipe = GpuXbdPipeline.from_image_dir('/data/xbd/train/images', device='cuda:0')
    for batch in pipe.batches(4, 1024, train=True, rng=random.Random(0)):        # {'img', 'msk', 'lbl_msk', 'fn'}
        loss = step(batch['img'], batch['msk'])

Differences from the reference, all deliberate:
  * `msk` is uint8 (0 / 1), not long: the step casts it to float where it always did (graph.py, GraphedXbdStep._loss_and_grad;
    models/xbd.xbd_loss), and 5 bytes per pixel instead of 40 is most of the batch's mask traffic.  `lbl_msk` is uint8 too.
  * `lbl_msk` of a TRAINING batch is zeros, as in the reference: there msk[0] is set wherever any other channel is, so
    msk.argmax(axis=2) is 0 at every pixel (train.py:171-174).  One zero tensor is kept and returned; do not write to it.
  * ColorJitter (train.py:138-139, 9 % of the samples) is not applied: it is torchvision's, drawn from torch's generator.
    `draw_train_params` consumes the reference's Python draws up to and including the one that decides it and reports the flag.
"""
import functools
import glob
import os

import numpy as np
import torch
from PIL import Image

from .. import ops

PRECISION_BITS = 22        # Pillow's 8-bit resize: coefficients in 2.22 fixed point (Resample.c)
PARAM_FIELDS = ("x0", "y0", "hflip", "vflip", "resize", "top", "left", "height", "width")


@functools.lru_cache(maxsize=None)
def _resize_coeffs(in_size, out_size):
    if in_size < 1 or out_size < 1:
        raise ValueError("resize_coeffs: %d -> %d: empty axis" % (in_size, out_size))
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs                                        # the bilinear filter's support is 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    lo = np.maximum((center - support + 0.5).astype(np.int64), 0)            # C's (int): truncation
    cnt = np.minimum((center + support + 0.5).astype(np.int64), in_size) - lo
    t = np.arange(3, dtype=np.int64)[None, :]
    arg = ((t + lo[:, None]) - center[:, None] + 0.5) * (1.0 / fs)
    w = np.maximum(1.0 - np.abs(arg), 0.0)
    w[t >= cnt[:, None]] = 0.0
    if (cnt > 3).any():
        raise ValueError("resize_coeffs: %d -> %d needs %d taps, the table holds three" % (in_size, out_size, cnt.max()))
    ww = w[:, 0] + w[:, 1] + w[:, 2]                          # Pillow sums the taps in this order
    w = np.where(ww[:, None] != 0, w / ww[:, None], w)
    k = (0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)
    # what the kernel's 32-bit accumulator and its unclipped byte rely on: 255 * sum(k) + (1 << 21) < 256 << 22
    if (k < 0).any() or (k.sum(axis=1) > (1 << PRECISION_BITS) + 8192).any():
        raise ValueError("resize_coeffs: %d -> %d: coefficients outside 0 <= k, sum(k) <= 2^22 + 8192" % (in_size, out_size))
    out = np.concatenate([lo[:, None], k], axis=1).astype(np.int32)
    out.setflags(write=False)
    return out


def resize_coeffs(in_size, out_size):
    """[out_size, 4] int32 rows (first source index, k0, k1, k2) of Pillow's Image.resize(..., Image.BILINEAR) along one axis
    of an 8-bit image.  Three taps hold every in_size <= out_size -- all the loader asks for -- and a source up to half as
    long again; ValueError for one that needs more.
    Derived as Pillow's precompute_coeffs / normalize_coeffs_8bpc do, in float64: scale = in / out, support = max(scale, 1);
    output index o has center = (o + 0.5) * scale, first tap lo = max(int(center - support + 0.5), 0), count =
    min(int(center + support + 0.5), in) - lo; tap t < count weighs max(0, 1 - |(t + lo - center + 0.5) / support|), the weights are
    divided by their sum and each becomes int(0.5 + w * (1 << 22)); taps at or past `count` are 0 and may lie outside the
    source.  An output byte of a pass is clip8(((1 << 21) + sum_t in[lo + t] * k[t]) >> 22).  in == out gives (o, 1 << 22, 0, 0).
    Byte for byte Pillow on nine odd shapes (tests/test_xbd_loader_cpu.py).  The array is cached and read-only."""
    return _resize_coeffs(int(in_size), int(out_size))


def draw_train_params(rng, H, W, crop):
    """One training sample's draws from `rng` (a random.Random, or the `random` module), exactly the reference's and in its
    order (xBD_code/train.py:110-138): x0, y0; then, if random() > 0.7: hflip, vflip (each random() > 0.3); if random() > 0.3
    the two randint(0, 200) of TF.resized_crop(img, x, y, crop - x, crop - y, (crop, crop)) -- top = x, left = y in
    torchvision's argument order; and the ColorJitter decision random() > 0.7.  Returns (params row in PARAM_FIELDS order,
    jitter flag).  ColorJitter itself is not applied (module docstring); its own draws come from torch's generator, so the
    Python stream stands where the reference's does after the sample."""
    if crop > H or crop > W:
        raise ValueError("crop %d is larger than the %dx%d image" % (crop, H, W))
    x0 = rng.randint(0, W - crop)
    y0 = rng.randint(0, H - crop)
    hf = vf = rs = top = left = 0
    bh = bw = crop
    jitter = False
    if rng.random() > 0.7:
        hf = int(rng.random() > 0.3)
        vf = int(rng.random() > 0.3)
        if rng.random() > 0.3:
            x = rng.randint(0, 200)
            y = rng.randint(0, 200)
            if crop - x < 1 or crop - y < 1:
                raise ValueError("resized_crop box (%d, %d) leaves nothing of a %d crop" % (x, y, crop))
            rs, top, left, bh, bw = 1, x, y, crop - x, crop - y
        jitter = rng.random() > 0.7
    return [x0, y0, hf, vf, rs, top, left, bh, bw], jitter


def check_params(params, H, W, crop):
    """[n, 9] int32 tensor of parameter rows; ValueError for a crop window outside the image, a flag that is not 0 / 1 or a
    resize box that is empty or leaves the crop (the kernel trusts the rows)"""
    p = torch.as_tensor(params, dtype=torch.int32).reshape(-1, len(PARAM_FIELDS))
    if crop < 1 or crop > H or crop > W:
        raise ValueError("crop %d does not fit the %dx%d image" % (crop, H, W))
    for row in p.tolist():
        x0, y0, hf, vf, rs, top, left, bh, bw = row
        if not (0 <= x0 <= W - crop and 0 <= y0 <= H - crop):
            raise ValueError("crop window (%d, %d) + %d leaves the %dx%d image" % (x0, y0, crop, H, W))
        if hf not in (0, 1) or vf not in (0, 1) or rs not in (0, 1):
            raise ValueError("flags %r are not 0 / 1" % ([hf, vf, rs],))
        if rs and not (top >= 0 and left >= 0 and bh >= 1 and bw >= 1 and top + bh <= crop and left + bw <= crop):
            raise ValueError("resize box top %d left %d height %d width %d leaves the %d crop" % (top, left, bh, bw, crop))
    return p


def coef_table(params, crop):
    """[n, 2, crop, 4] int32 host tensor for dh_xbd_augment_u8 (axis 0 along x from the box width, axis 1 along y from its
    height), or None when no row of `params` (checked rows) has the resize flag; rows of samples without it stay 0"""
    rows = params.tolist()
    if not any(r[4] for r in rows):
        return None
    table = np.zeros((len(rows), 2, crop, 4), dtype=np.int32)
    for i, r in enumerate(rows):
        if r[4]:
            table[i, 0], table[i, 1] = resize_coeffs(r[8], crop), resize_coeffs(r[7], crop)
    return torch.from_numpy(table)


class GpuXbdPipeline:
    def __init__(self, pre_u8, post_u8, pre_mask_u8, post_label_u8, files=None):
        """pre_u8, post_u8: [n_src, H, W, 3] uint8 device tensors; pre_mask_u8 (0 / 255) and post_label_u8 (0 .. 4):
        [n_src, H, W] uint8"""
        assert pre_u8.is_cuda and pre_u8.dtype == torch.uint8 and pre_u8.dim() == 4 and pre_u8.shape[-1] == 3
        assert post_u8.shape == pre_u8.shape and post_u8.dtype == torch.uint8
        for m in (pre_mask_u8, post_label_u8):
            assert m.dtype == torch.uint8 and m.shape == pre_u8.shape[:3]
        self.pre, self.post = pre_u8.contiguous(), post_u8.contiguous()
        self.pre_mask, self.post_label = pre_mask_u8.contiguous(), post_label_u8.contiguous()
        self.files = list(files) if files is not None else [str(i) for i in range(pre_u8.shape[0])]
        self._zero_lbl = None

    @classmethod
    def from_image_dir(cls, images_dir, device='cuda:0', files=None):
        """the reference's naming (xBD_code/train.py:79-83, 102-108): every `*_pre_disaster.png` of `images_dir` (or the
        paths in `files`), its post image under `_post_disaster`, and both masks under the same names with `/images/`
        replaced by `/masks/`"""
        if files is None:
            files = sorted(glob.glob(os.path.join(images_dir, '*_pre_disaster.png')))
        files = [str(f) for f in files]
        if not files:
            raise ValueError("no *_pre_disaster.png under %s" % images_dir)
        for fn in files:
            if '/images/' not in fn or '_pre_disaster' not in fn:
                raise ValueError("%s: expected .../images/..._pre_disaster.png (the masks are found by replacing /images/)" % fn)
        rgb = lambda fn: np.asarray(Image.open(fn).convert('RGB'))

        def gray(fn):
            m = np.asarray(Image.open(fn))
            if m.ndim != 2 or m.dtype != np.uint8:
                raise ValueError("%s: a mask is one 8-bit channel, got %s %s" % (fn, m.shape, m.dtype))
            return m

        post = lambda fn: fn.replace('_pre_disaster', '_post_disaster')
        mask = lambda fn: fn.replace('/images/', '/masks/')
        to = lambda xs: torch.from_numpy(np.ascontiguousarray(np.stack(xs))).to(device)
        return cls(to([rgb(f) for f in files]), to([rgb(post(f)) for f in files]), to([gray(mask(f)) for f in files]),
                   to([gray(mask(post(f))) for f in files]), files)

    def __len__(self):
        return self.pre.shape[0]

    def make_batch(self, indices, crop, params=None, train=True):
        """indices: source samples of the batch; params: one row per sample in PARAM_FIELDS order (draw_train_params), or None
        for the crop at the origin without augmentation.  train=False builds ValData's masks (msk[0] from the pre mask,
        lbl_msk = label - 1 on the buildings); the reference validates whole images, i.e. crop == H == W and params=None.
        Returns {'img': fp32 [n, 6, crop, crop], 'msk': uint8 [n, 5, crop, crop], 'lbl_msk': uint8 [n, crop, crop], 'fn'}.
        `lbl_msk` of a training batch is all zeros (module docstring) and is ONE tensor shared by every training batch of
        that shape: read it, never write to it in place.
        ValueError for a crop larger than the image, a window outside it or a resize box that leaves the crop."""
        n = len(indices)
        _, H, W, _ = self.pre.shape
        if params is None:
            params = [[0, 0, 0, 0, 0, 0, 0, crop, crop]] * n
        p = check_params(params, H, W, crop)
        if p.shape[0] != n:
            raise ValueError("params: %d rows for %d samples" % (p.shape[0], n))
        if any(not 0 <= int(i) < len(self) for i in indices):
            raise ValueError("indices %r outside the %d samples" % (list(indices), len(self)))
        coef = coef_table(p, crop)
        dev = self.pre.device
        idx = torch.as_tensor([int(i) for i in indices], dtype=torch.int32).to(dev)
        p = p.contiguous().to(dev)
        coef = coef.to(dev) if coef is not None else None
        img = torch.empty(n, 6, crop, crop, dtype=torch.float32, device=dev)
        msk = torch.empty(n, 5, crop, crop, dtype=torch.uint8, device=dev)
        if train:
            if self._zero_lbl is None or self._zero_lbl.shape != (n, crop, crop):
                self._zero_lbl = torch.zeros(n, crop, crop, dtype=torch.uint8, device=dev)
            lbl = self._zero_lbl
        else:
            lbl = torch.empty(n, crop, crop, dtype=torch.uint8, device=dev)
        ops._call("dh_xbd_augment_u8", ops.P(self.pre), ops.P(self.post), ops.P(None if train else self.pre_mask),
                  ops.P(self.post_label), ops.P(idx), ops.P(p), ops.P(coef), n, H, W, crop, 0 if train else 1, ops.P(img),
                  ops.P(msk), ops.P(None if train else lbl), ops.S())
        return {'img': img, 'msk': msk, 'lbl_msk': lbl, 'fn': [self.files[int(i)] for i in indices]}

    def batches(self, batch_size, crop, train=True, rng=None):
        """one epoch.  train: `rng` (a random.Random) shuffles the samples, then every sample draws its parameters with
        draw_train_params, in batch order (the reference's DataLoader shuffles with torch's generator and draws in its worker
        processes: the order of the samples is this loader's own, a sample's draws are the reference's).  Otherwise the
        samples in order with ValData's masks, as ValData takes them: whole images, so `crop` must be the (square) image
        size -- ValueError otherwise; a validation crop is make_batch(..., params, train=False)."""
        _, H, W, _ = self.pre.shape
        if not train and not crop == H == W:
            raise ValueError("a validation epoch takes whole images: crop %d is not the %dx%d image" % (crop, H, W))
        order = list(range(len(self)))
        if train:
            if rng is None:
                raise ValueError("a training epoch draws from `rng` (a random.Random)")
            rng.shuffle(order)
        for s in range(0, len(order), batch_size):
            ind = order[s:s + batch_size]
            params = [draw_train_params(rng, H, W, crop)[0] for _ in ind] if train else None
            yield self.make_batch(ind, crop, params, train)
