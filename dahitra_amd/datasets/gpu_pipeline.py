"""Pre-decoded image pairs resident in HBM + crop / flip / blur / normalise on the device (ops.augment_pairs:
dh_augment_pairs_u8, dh_augment_pairs_blur_u8).

The reference's loader decodes two PNGs and runs PIL transforms per sample in DataLoader workers
(datasets/CD_dataset.py:112-134, datasets/data_utils.py:55-111); at the ~7 000 pairs/s of the MI355X train step that is the
bottleneck by an order of magnitude.  A LEVIR-sized training set (7 120 pairs of 256x256x3 uint8 = 2.8 GB, or the 445
1024x1024 tiles) fits the 288 GB of HBM many times over, so: decode once (`from_dataset_root`, same folder layout as
CDDataset), keep uint8 on the device, and produce every batch with ONE kernel -- same crop-window rule, same flip
probabilities, same normalisation as CDDataAugmentation.  With `blur=True` the batch also gets the reference's random
Gaussian blur (ImageFilter.GaussianBlur(radius=random.random()) on both images of a training sample, datasets/data_utils.py:
99-102), byte for byte what Pillow computes: flips + blur is the reference's training augmentation.  The blur is off by
default (the loader then produces what it always did).

    pipe = GpuPairPipeline.from_dataset_root(root, split='train', device='cuda:0')
    for batch in pipe.batches(batch_size=32, img_size=256, train=True, generator=g, blur=True):   # {'A', 'B', 'L', 'name'}
        trainer.train_step(batch)
"""
import os

import numpy as np
import torch
from PIL import Image

from .. import ops
from .CD_dataset import get_img_path, get_img_post_path, get_label_path


def box_blur_weights(radius):
    """(ww, fw) of Pillow's ImageFilter.GaussianBlur(radius) for a radius whose box has integer radius 0 (radius < sqrt(2);
    the reference draws radius = random.random() < 1).  Pillow approximates the Gaussian by three box-blur passes per axis
    (BoxBlur.c); a box of radius 0 + a, 0 <= a < 1, is the 3-tap filter
        out[x] = (in[x] * ww + (in[x - 1] + in[x + 1]) * fw + (1 << 23)) >> 24
    on uint8 with the edge pixel replicated, and (ww, fw) are 8.24 fixed-point weights.  The derivation follows Pillow's
    _gaussian_blur_radius(radius, passes=3) and ImagingLineBoxBlur in ITS precision, float32: a float64 derivation gives
    another ww for some radii (0.25: 16427690 instead of 16427691).  Checked byte for byte against Pillow on random radii in
    [0, sqrt(2)) and on {0, 1e-9, 1e-3, 0.25, 0.5, 0.999999} (tests/test_gpu_blur_cpu.py).  radius == 0 is a special case in
    Pillow (GaussianBlur.filter returns image.copy() without calling the C filter); the formula gives (1 << 24, 0) there,
    the identity, so it needs no special case here.  ValueError for a negative or non-finite radius and for one whose box
    has a non-zero integer radius (radius >= sqrt(2))."""
    ww, fw = _box_blur_weights(np.asarray([radius], dtype=np.float32))
    return int(ww[0]), int(fw[0])


def _box_blur_weights(r):
    """box_blur_weights for a float32 array of radii -> (ww, fw) int64 arrays; every operation rounds to float32"""
    f = np.float32
    bad = ~np.isfinite(r) | (r < 0)
    if bad.any():
        raise ValueError("blur radius %r is negative or not finite" % (float(r[bad][0]),))
    sigma2 = r * r / f(3)
    big_l = np.sqrt(f(12) * sigma2 + f(1))
    l = np.floor((big_l - f(1)) / f(2))
    if (l != 0).any():
        raise ValueError("blur radius %r: its box is not a 3-tap filter (radius must be < sqrt(2))" % (float(r[l != 0][0]),))
    a = (f(2) * l + f(1)) * (l * (l + f(1)) - f(3) * sigma2) / (f(6) * (sigma2 - (l + f(1)) * (l + f(1))))
    ww = (f(1 << 24) / (f(2) * (l + a) + f(1))).astype(np.int64)        # truncation, as the C cast to UINT32
    return ww, ((1 << 24) - ww) // 2


def blur_table(radii):
    """[n, 2] int32 (ww, fw) rows for dh_augment_pairs_blur_u8, with the bounds its 32-bit accumulator relies on checked
    where the table is written: 0 < ww <= 1 << 24, fw >= 0, ww + 2 fw <= 1 << 24 (255 (ww + 2 fw) + (1 << 23) < 2^32)"""
    ww, fw = _box_blur_weights(np.asarray(radii, dtype=np.float32).reshape(-1))
    bad = ~((0 < ww) & (ww <= 1 << 24) & (fw >= 0) & (ww + 2 * fw <= 1 << 24))
    if bad.any():
        raise ValueError("blur weights (%d, %d) outside 0 < ww <= 2^24, ww + 2 fw <= 2^24" % (ww[bad][0], fw[bad][0]))
    return torch.from_numpy(np.stack([ww, fw], axis=1).astype(np.int32))


class GpuPairPipeline:
    def __init__(self, a_u8, b_u8, l_u8, names=None):
        """a_u8, b_u8: [S, H, W, 3] uint8 device tensors; l_u8: [S, H, W] uint8 (already // 255 for 'norm' labels)"""
        assert a_u8.is_cuda and a_u8.dtype == torch.uint8 and a_u8.shape == b_u8.shape and a_u8.shape[-1] == 3
        self.a, self.b, self.l = a_u8.contiguous(), b_u8.contiguous(), l_u8.contiguous()
        self.names = list(names) if names is not None else [str(i) for i in range(a_u8.shape[0])]
        self._plan_params = {}          # TilePlan -> its [P, 4] rows on the device (window_batch)

    @classmethod
    def from_dataset_root(cls, root_dir, split='train', device='cuda:0', label_transform='norm', names=None):
        names = sorted(os.listdir(os.path.join(root_dir, split, 'A'))) if names is None else list(names)
        a = np.stack([np.asarray(Image.open(get_img_path(root_dir, split, n)).convert('RGB')) for n in names])
        b = np.stack([np.asarray(Image.open(get_img_post_path(root_dir, split, n)).convert('RGB')) for n in names])
        lab = np.stack([np.array(Image.open(get_label_path(root_dir, split, n)), dtype=np.uint8) for n in names])
        if label_transform == 'norm':
            lab = lab // 255
        to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)
        return cls(to(a), to(b), to(lab), names)

    def __len__(self):
        return self.a.shape[0]

    def make_batch(self, indices, img_size, flips=None, patch=None, blur=None):
        """indices: source pairs of the batch; flips: [n, 2] 0/1 (hflip, vflip) or None; blur: n Gaussian-blur radii
        (box_blur_weights) applied to A and B of each sample after the crop, or None for no blur (the unblurred kernel).  The
        crop window follows CDDataAugmentation: origin (256, 256) -- or the patch origin for a non-zero patch index -- when
        img_size < width // 2, the whole image otherwise."""
        n = len(indices)
        S, H, W, _ = self.a.shape
        if img_size < W // 2:
            x0, y0 = (256 * (patch // 4), 256 * (patch % 4)) if patch else (256, 256)
            h = w = img_size
            if y0 + h > H or x0 + w > W:
                raise ValueError("crop window (%d, %d) + %d leaves the %dx%d image" % (x0, y0, img_size, H, W))
        else:
            x0 = y0 = 0
            h, w = H, W
        params = torch.zeros(n, 4, dtype=torch.int32)
        params[:, 0], params[:, 1] = x0, y0
        if flips is not None:
            params[:, 2:] = torch.as_tensor(flips, dtype=torch.int32)
        table = None
        if blur is not None:
            if len(blur) != n:
                raise ValueError("blur: %d radii for %d samples" % (len(blur), n))
            table = blur_table(blur)
        dev = self.a.device
        idx = torch.as_tensor(indices, dtype=torch.int32).to(dev)
        out_a, out_b, out_l = ops.augment_pairs(self.a, self.b, self.l, idx, params.to(dev), h, w,
                                                table.to(dev) if table is not None else None)
        return {'A': out_a, 'B': out_b, 'L': out_l, 'name': [self.names[i] for i in indices]}

    def window_batch(self, index, plan, out=None):
        """The P views of source pair `index` under `plan` (tiles.TilePlan): {'A', 'B' float32 [P, 3, h, w], 'L' uint8
        [P, 1, h, w]}, view p cut at the plan's origin and flipped by its code -- ops.augment_pairs (dh_augment_pairs_u8) with the
        pair's index repeated, one launch.  index: an int, or a device int32 tensor of one element (a recorded graph is re-aimed by writing
        into it; it is NOT range-checked, the caller keeps it inside 0 .. len - 1).  out: a dict of such tensors to write into
        (the wrapper checks them; nothing is allocated for the views then)."""
        S, H, W, _ = self.a.shape
        dev = self.a.device
        if (plan.H, plan.W) != (H, W):
            raise ValueError("window_batch: the plan is for %dx%d tiles, the pipeline holds %dx%d" % (plan.H, plan.W, H, W))
        P, h, w = plan.P, plan.h, plan.w
        if torch.is_tensor(index):
            if index.dtype != torch.int32 or index.numel() != 1 or index.device != dev:
                raise ValueError("window_batch: index %s %s on %s is not one int32 on %s"
                                 % (tuple(index.shape), index.dtype, index.device, dev))
            idx = index.reshape(1).expand(P).contiguous()
        else:
            if not 0 <= int(index) < S:
                raise ValueError("window_batch: pair %d of %d" % (index, S))
            idx = torch.full((P,), int(index), dtype=torch.int32, device=dev)
        params = self._plan_params.get(plan)
        if params is None:
            params = self._plan_params[plan] = torch.from_numpy(plan.params()).to(dev)
        if out is None:
            out = {'A': None, 'B': None, 'L': None}
        elif not all(torch.is_tensor(out.get(k)) for k in 'ABL'):
            raise ValueError("window_batch: out is a dict of the tensors 'A', 'B' and 'L'")
        out['A'], out['B'], out['L'] = ops.augment_pairs(self.a, self.b, self.l, idx, params, h, w, out_a=out['A'], out_b=out['B'],
                                                         out_l=out['L'])
        return out

    def batches(self, batch_size, img_size, train=True, generator=None, patch=None, drop_last=False, blur=False):
        """one epoch: shuffled with random flips (p = 0.5 each, as the reference's training augmentation) when `train`; with
        `blur` a training batch also draws one blur radius in [0, 1) per sample, after its flips (evaluation never blurs)"""
        return self._epoch(batch_size, img_size, train, generator, patch, drop_last, blur)

    def _epoch(self, batch_size, img_size, train, generator, patch, drop_last, blur, rank=0, world=1):
        """the epoch body of `batches` and of GpuPairLoader: rank `rank` of `world` takes its shard of the one permutation"""
        S = len(self)
        order = torch.randperm(S, generator=generator).tolist() if train else list(range(S))
        per = S // world
        order = order[rank * per:(rank + 1) * per]
        for s in range(0, len(order), batch_size):
            ind = order[s:s + batch_size]
            if drop_last and len(ind) < batch_size:
                break
            flips = (torch.rand(len(ind), 2, generator=generator) > 0.5).int() if train else None
            radii = torch.rand(len(ind), generator=generator).tolist() if train and blur else None
            yield self.make_batch(ind, img_size, flips, patch, radii)


class GpuPairLoader:
    """A DataLoader-shaped view of a GpuPairPipeline (`for batch in loader`, `len(loader)`): what utils.get_loaders returns
    with args.gpu_loader.  Every epoch draws a fresh permutation and fresh flips from `generator` (train mode), and with
    `blur` one Gaussian-blur radius in [0, 1) per sample after the flips of its batch (train mode only).  With
    world > 1 the epoch's permutation is cut into equal per-rank shards (every rank must pass an equally seeded generator;
    the tail that does not fill a full global batch is dropped so that all ranks take the same number of steps)."""

    def __init__(self, pipe, batch_size, img_size, train, generator=None, drop_last=False, rank=0, world=1, blur=False):
        self.pipe, self.batch_size, self.img_size, self.train = pipe, int(batch_size), img_size, train
        self.blur = bool(blur) and bool(train)
        self.generator, self.drop_last, self.rank, self.world = generator, drop_last or world > 1, rank, world

    def __len__(self):
        per = len(self.pipe) // self.world
        return per // self.batch_size if self.drop_last else -(-per // self.batch_size)

    def __iter__(self):
        return self.pipe._epoch(self.batch_size, self.img_size, self.train, self.generator, None, self.drop_last, self.blur,
                                self.rank, self.world)
