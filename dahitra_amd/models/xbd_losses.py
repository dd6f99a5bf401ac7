"""xBD_code/losses.py on the device: the drop-in for `from losses import ...` (same names, argument meaning and defaults).

    ComboLoss(weights, per_image=False)      losses.py:95-126, all seven terms: bce, dice, focal, jaccard, lovasz, lovasz_sigmoid,
        mask_bceavg.  outputs are LOGITS [B, H, W] (the scripts' call) or [B, C, H, W] (the sum over the channels, as
        xbd.ComboLoss takes it); the sigmoid of the terms in `expect_sigmoid` is taken inside the kernels, lovasz and bce read the
        logits.  dice and focal run through xbd.ComboLoss's kernels (dh_combo_loss_*), jaccard / bce / mask_bceavg through
        dh_xbd_seg_terms_*, the two Lovasz terms through dh_xbd_lovasz_fwd.  per_image reaches the two Lovasz terms only, as in
        the reference (its Dice and Jaccard are built with per_image=False).  .values holds every term of the last call.
    LovaszLoss, LovaszLossSigmoid, JaccardLoss, DiceLoss, StableBCELoss, MaskLoss, FocalLoss2d      the stand-alone classes: like the
        reference's they take what ComboLoss would hand them -- probabilities, except LovaszLoss and StableBCELoss (logits)
    lovasz_hinge, lovasz_sigmoid, lovasz_hinge_flat, lovasz_sigmoid_flat, lovasz_grad, flatten_binary_scores, mean
    jaccard, soft_dice_loss, dice_round, iou_round (per_image=True of the last four is not built and raises)

The Lovasz terms sort with a defined tie order (equal errors keep flat index order; torch.sort promises none) and form the
gradient of the Lovasz extension in closed form from integers, where the reference subtracts two float32 numbers near 0.5.
One call sorts at most 256 segments and 2^30 elements: with per_image=True (the default of lovasz_hinge and of the two Lovasz
classes, as in the reference) a batch of more than 256 images, or B * C > 256 planes in ComboLoss, raises ValueError; the
reference has no such limit.  Targets may be the loaders' uint8 masks or float tensors.  CPU tensors raise HipLibraryError: there is no CPU path."""
import torch
import torch.nn as nn

from .. import _lib, ops
from . import xbd as _xbd

eps = 1e-6


def _device(*tensors):
    for t in tensors:
        if not (torch.is_tensor(t) and t.is_cuda):
            raise _lib.HipLibraryError("dahitra_amd xBD losses run on MI355X only (no CPU fallback)")


def _planes(outputs, targets):
    """x fp32 [B, C, ...] and the target of its shape (uint8 kept, anything else as fp32): a [B, H, W] input is one channel"""
    _device(outputs, targets)
    if outputs.shape != targets.shape:
        raise ValueError("outputs %s and targets %s must have the same shape" % (tuple(outputs.shape), tuple(targets.shape)))
    x = outputs.float().contiguous()
    x = x.unsqueeze(1) if x.dim() <= 3 else x
    t = targets if targets.dtype == torch.uint8 else targets.float()
    return x, t.contiguous().view(x.shape)


def _flat(x, targets):
    """a [P] vector as one segment [1, 1, P]"""
    _device(x, targets)
    t = targets if targets.dtype == torch.uint8 else targets.float()
    return x.float().contiguous().view(1, 1, -1), t.contiguous().view(1, 1, -1)


class _Lovasz(torch.autograd.Function):
    """the forward knows the gradient once it has sorted (as ops.focal_loss(want_grad=True)); backward scales it"""
    @staticmethod
    def forward(ctx, x, target, mode, per_image, ignore, weights_dev):
        loss, channel, dx = ops.xbd_lovasz(x, target, mode, per_image, ignore, weights_dev)
        ctx.save_for_backward(dx)
        ctx.mark_non_differentiable(channel)
        return loss, channel

    @staticmethod
    def backward(ctx, dloss, _dchannel):
        dx, = ctx.saved_tensors
        out = torch.empty_like(dx)
        ops.scale_into(dx, dloss.detach(), out)
        return out, None, None, None, None, None


class _SegTerms(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, target, weights_dev, probs, jaccard_w, bce_w, mask_w, dice_w, focal_w):
        kw = dict(jaccard=jaccard_w, bce=bce_w, mask_bceavg=mask_w, dice=dice_w, focal=focal_w, probs=probs)
        loss, terms, sums = ops.xbd_seg_terms_fwd(x, target, weights_dev, **kw)
        ctx.save_for_backward(x, target, sums)
        ctx.how = (weights_dev, kw)
        ctx.mark_non_differentiable(terms)
        return loss, terms

    @staticmethod
    def backward(ctx, dloss, _dterms):
        x, target, sums = ctx.saved_tensors
        weights_dev, kw = ctx.how
        up = dloss.detach().to(torch.float32).reshape(1).contiguous()
        return (ops.xbd_seg_terms_bwd(x, target, sums, weights_dev, up, **kw),) + (None,) * 8


def _seg_term(outputs, targets, name, probs):
    x, t = _planes(outputs, targets)
    w = {k: 0.0 for k in ("jaccard", "bce", "mask_bceavg", "dice", "focal")}
    w[name] = 1.0
    loss, _ = _SegTerms.apply(x, t, None, probs, w["jaccard"], w["bce"], w["mask_bceavg"], w["dice"], w["focal"])
    return loss


def _one_segment(x, t):
    """every element in ONE sort, whatever the shape: what the reference's functions do with a whole tensor"""
    return x.reshape(1, 1, -1), t.reshape(1, 1, -1)


def _lovasz(outputs, targets, mode, per_image, ignore):
    """the reference's functions: one loss over everything, or with per_image the mean of one loss per leading index"""
    x, t = _planes(outputs, targets)
    if per_image:
        x, t = x.reshape(x.shape[0], 1, -1), t.reshape(x.shape[0], 1, -1)
    else:
        x, t = _one_segment(x, t)
    loss, _ = _Lovasz.apply(x, t, mode, bool(per_image), ignore, None)
    return loss


# ---- the reference's functions -----------------------------------------------------------------------------
def lovasz_grad(gt_sorted):
    """losses.py:129-141 from a sorted label vector [P], on the device: the gradient of the Lovasz extension, fp32 [P].  All
    errors are made equal, so the stable sort keeps the given order, and the gradient's magnitude is read off."""
    _device(gt_sorted)
    t = (gt_sorted if gt_sorted.dtype == torch.uint8 else gt_sorted.float()).contiguous().view(1, 1, -1)
    half = torch.full(t.shape, 0.5, dtype=torch.float32, device=t.device)
    _, _, dx = ops.xbd_lovasz(half, t, "probas", False, None)
    return dx.view(-1).abs()


def lovasz_hinge(logits, labels, per_image=True, ignore=None):
    """losses.py:144-157: logits, labels [B, H, W]"""
    return _lovasz(logits, labels, "hinge", per_image, ignore)


def lovasz_hinge_flat(logits, labels):
    """losses.py:160-177: logits, labels [P]; nothing is ignored"""
    _device(logits, labels)
    if labels.numel() == 0:
        return logits.sum() * 0.
    loss, _ = _Lovasz.apply(*_flat(logits, labels), "hinge", False, None, None)
    return loss


def flatten_binary_scores(scores, labels, ignore=None):
    """losses.py:180-192 (indexing only; the Lovasz functions here drop `ignore` inside the kernel instead)"""
    scores, labels = scores.reshape(-1), labels.reshape(-1)
    if ignore is None:
        return scores, labels
    valid = labels != ignore
    return scores[valid], labels[valid]


def lovasz_sigmoid(probas, labels, per_image=False, ignore=None):
    """losses.py:195-209: probas, labels [B, H, W]"""
    return _lovasz(probas, labels, "probas", per_image, ignore)


def lovasz_sigmoid_flat(probas, labels):
    """losses.py:212-225: probas, labels [P]"""
    _device(probas, labels)
    if labels.numel() == 0:
        return probas.sum() * 0.
    loss, _ = _Lovasz.apply(*_flat(probas, labels), "probas", False, None, None)
    return loss


def mean(l, ignore_nan=False, empty=0):
    """The arithmetic mean of an iterable of numbers or device scalars (a generator too); `empty` when it yields nothing,
    ValueError if that is 'raise'; ignore_nan leaves NaNs out first.  Host arithmetic on what the iterable yields."""
    values = [v for v in l if not (ignore_nan and v != v)]
    if not values:
        if empty == 'raise':
            raise ValueError('Empty mean')
        return empty
    return sum(values[1:], values[0]) / len(values) if len(values) > 1 else values[0]


def _batch_wide(what, per_image):
    if per_image:
        raise NotImplementedError("%s: per_image=True is not built (ComboLoss builds its Dice and Jaccard with per_image=False)" % what)


def soft_dice_loss(outputs, targets, per_image=False):
    """losses.py:24-33 on probabilities"""
    _batch_wide("soft_dice_loss", per_image)
    return _seg_term(*_one_segment(*_planes(outputs, targets)), "dice", True)


def jaccard(outputs, targets, per_image=False):
    """losses.py:36-45 on probabilities"""
    _batch_wide("jaccard", per_image)
    return _seg_term(*_one_segment(*_planes(outputs, targets)), "jaccard", True)


def dice_round(preds, trues):
    return soft_dice_loss(preds.float(), trues)


def iou_round(preds, trues):
    return jaccard(preds.float(), trues)


# ---- the reference's classes ---------------------------------------------------------------------------------
class _BatchWide(nn.Module):
    """DiceLoss / JaccardLoss: the reference's arguments are taken; `weight` and `size_average` have no effect there either"""
    _fn = None

    def __init__(self, weight=None, size_average=True, per_image=False):
        super().__init__()
        self.per_image = per_image

    def forward(self, input, target):
        return type(self)._fn(input, target, per_image=self.per_image)


class DiceLoss(_BatchWide):
    _fn = staticmethod(soft_dice_loss)


class JaccardLoss(_BatchWide):
    _fn = staticmethod(jaccard)


class StableBCELoss(nn.Module):
    def forward(self, input, target):
        return _seg_term(*_one_segment(*_planes(input, target)), "bce", False)


class MaskLoss(nn.Module):
    def forward(self, input, target):
        return _seg_term(*_one_segment(*_planes(input, target)), "mask_bceavg", True)


class FocalLoss2d(nn.Module):
    def __init__(self, gamma=2, ignore_index=255):
        super().__init__()
        if gamma != 2 or ignore_index != 255:
            raise NotImplementedError("FocalLoss2d: gamma=2 and ignore_index=255 (the reference's defaults) are built")
        self.gamma = gamma
        self.ignore_index = ignore_index

    def forward(self, outputs, targets):
        return _seg_term(*_one_segment(*_planes(outputs, targets)), "focal", True)


class _LovaszModule(nn.Module):
    _fn = None

    def __init__(self, ignore_index=255, per_image=True):
        super().__init__()
        self.ignore_index, self.per_image = ignore_index, per_image

    def forward(self, outputs, targets):
        return type(self)._fn(outputs, targets, per_image=self.per_image, ignore=self.ignore_index)


class LovaszLoss(_LovaszModule):
    _fn = staticmethod(lovasz_hinge)


class LovaszLossSigmoid(_LovaszModule):
    _fn = staticmethod(lovasz_sigmoid)


_TERMS = ('bce', 'dice', 'focal', 'jaccard', 'lovasz', 'lovasz_sigmoid', 'mask_bceavg')


class ComboLoss(nn.Module):
    def __init__(self, weights, per_image=False):
        super().__init__()
        unknown = [k for k in weights if k not in _TERMS]
        if unknown:
            raise KeyError("ComboLoss: no term %s; the terms are %s" % (unknown, list(_TERMS)))
        self.weights = weights
        self.per_image = per_image
        self.expect_sigmoid = {'dice', 'focal', 'jaccard', 'lovasz_sigmoid', 'mask_bceavg'}
        self.values = {}

    def forward(self, outputs, targets):
        """outputs: logits [B, H, W] or [B, C, H, W]; targets of that shape, uint8 or float.  The weighted sum of the terms whose
        weight is not zero, every term summed over the channels; .values[k] is term k of this call (a device scalar)."""
        x, t = _planes(outputs, targets)
        w = {k: float(v) for k, v in self.weights.items() if v}
        loss = 0
        if 'dice' in w or 'focal' in w:
            # xbd.ComboLoss's kernels, one call per term so that .values holds each of them; they take float masks
            tf = t.float()
            ones = _xbd.channel_weights_dev(x.device, (1.0,) * x.shape[1])
            for k in ('dice', 'focal'):
                if k in w:
                    val, _ = _xbd._Combo.apply(x, tf, ones, float(k == 'dice'), float(k == 'focal'))
                    self.values[k] = val
                    loss = loss + w[k] * val
        for k in ('jaccard', 'bce', 'mask_bceavg'):
            if k in w:
                val, _ = _SegTerms.apply(x, t, None, False, float(k == 'jaccard'), float(k == 'bce'), float(k == 'mask_bceavg'), 0.0, 0.0)
                self.values[k] = val
                loss = loss + w[k] * val
        for k, mode in (('lovasz', 'hinge'), ('lovasz_sigmoid', 'sigmoid')):
            if k in w:
                val, _ = _Lovasz.apply(x, t, mode, bool(self.per_image), 255, None)
                self.values[k] = val
                loss = loss + w[k] * val
        return loss
