"""The xBD 5-class damage-assessment step on the HIP pipelines.

Mirrored interfaces (same names, argument meaning, error behaviour):
    BASE_Transformer_UNet(input_nc, output_nc, ...)   xBD_code/zoo/model_transformer_encoding.py:242-449
        net(x) with ONE [B, 6, H, W] tensor (pre | post), logits [B, 5, H, W]; built at xBD_code/train.py:44-45
        output_nc=4: the four-output net of xBD_code/train_adapt.py:37-38 (localisation, minor, major, destroyed merged with 3)
    ComboLoss(weights, per_image=False)               xBD_code/losses.py:95-126   (dice + focal on the sigmoid)
    xbd_loss(out, msks)                               xBD_code/train.py:348-353   (the five weighted channel losses)
    unet_loss(out, msks, lbl_msk, labels)             xBD_code/train_unettransformer.py:438-456 (five ComboLoss terms + 8 * the
        class-weighted cross-entropy of the logits masked by lbl_msk > 0; uint8 masks, one pass; labels='damage' derives the label)
    unet_scheduler(optimizer)                         train_unettransformer.py:536      (MultiStepLR, gamma 0.6)
    unet_val_batches(pipe, batch_size, crop, indices) train_unettransformer.py:288-352  (ValData: the fixed crop at (512, 512);
        indices: the val_idxs of pipe.unet_trainset(), the tenth the script holds out of its one folder)
    train_epoch_unet(current_epoch, model, optimizer, scheduler, batches)   train_unettransformer.py:421-486 (no clip; the meters
        Loss / loss2 / loss3 / Dice from ONE host read per epoch; `seg_loss`, `ce_loss` and `scaler` are not arguments here)
    adapt_loss(out, msks)                             xBD_code/train_adapt.py:332-342 (four ComboLoss terms weighted 0.1, 0.8, 2, 8
        + 5 * the class-weighted cross-entropy of the RAW logits; uint8 masks, the label derived from them in the kernel)
    adapt_scheduler(optimizer)                        train_adapt.py:423                (MultiStepLR, gamma 0.6, no 17)
    train_epoch_adapt(current_epoch, model, optimizer, scheduler, batches)   train_adapt.py:313-360 (WITH the clip of line 346;
        the meters Loss / loss1 / loss2 / loss3 from ONE host read per epoch; line 359 as printed; line 331's print and the
        unused GradScaler are not reproduced)
    validate_adapt(model, batches) / evaluate_val_adapt(...)   train_adapt.py:248-310 (validate / evaluate_val with THREE damage
        classes: f1 = 3 / sum(1 / (f1_sc + 1e-6)); the `best_score == 10000` train-score branch is not built)
        the loader and the file set of that script are GpuXbdPipeline.make_adapt_batch / adapt_batches / adapt_trainset; the
        sample order stays this loader's own, and the augmentation inside the script's string literal is not built
    clip_grad_norm_(parameters, max_norm)             torch.nn.utils.clip_grad_norm_ as called at train.py:373
    AdamW(params, lr, weight_decay)                   xBD_code/adamw.py:6-86      (hand-rolled; eps before bias correction)
    validate(model, data_loader)                      xBD_code/train.py:247-290   (dice of the localisation + harmonic F1)
    evaluate_val(data_val, best_score, model, ...)    xBD_code/train.py:293-307   (the snapshot of the best score)
        the reference reads `optimizer` and the snapshot's folder from globals; here they are arguments
    validate_sweep / evaluate_val_sweep               no counterpart: validate for a grid of localisation thresholds in one
        epoch of forwards (the reference's scripts use 0.3, 0.5 and visualize_results.py's 0.38 / 0.13 / 0.14 by turns)
    dice(im1, im2, empty_score=1.0)                   xBD_code/utils.py:124-154   as val_score's per-image term, on counts
    predict_dir(model, test_dir, pred_folder)         xBD_code/predict_test_cls.py:58-97 (the 4-flip TTA loop and its files)
        the reference reads the two folders and its list `models` from globals; here they are arguments
    load_snapshot(model, path)                        xBD_code/predict_test_cls.py:43-53 (the size-matched copy of a snapshot)
    predict_ensemble(models, pre_u8, post_u8)         xBD_code/predict_test_cls.py:81-94 for a list of several snapshots: every
        model's un-flipped sigmoids in one stack, numpy's float32 mean over it; views=8 adds the transposed views
    predict_dir_ensemble(models, test_dir, pred_folder)   predict_dir's loop and files on predict_ensemble
    visualize_dir(model, test_dir, mask_dir, out_dir) xBD_code/visualize_results.py:171-223 (pre | post | truth | prediction PNGs)
        damage_map / visual_grid are its lines 206-211 / 213-220 on device tensors; the folders are arguments here too, and
        the localisation probability is channel 0 of the same prediction (the script's separate localisation net is not built)
    buildings / building_damage / building_confusion / building_f1   no counterpart: connected components of a class map, one
        damage class per building by vote, and the building-level confusion and F1 against the ground truth
    dilate / erode / opening / closing / fill_holes / clean_footprint   no counterpart: square-window morphology and hole
        filling of a footprint before its buildings are counted (scipy.ndimage's binary_* functions are the oracle)
Everything computes through libdahitra_hip.so (csrc/xbd_step.hip, csrc/xbd_script_loss.hip, csrc/xbd_eval.hip, csrc/xbd_predict.hip, csrc/xbd_ensemble.hip, csrc/xbd_visual.hip,
csrc/xbd_buildings.hip, csrc/xbd_morph.hip + the shared model kernels); CPU tensors are refused.  val_score alone is host arithmetic: the reference's float64 numpy expressions on the integer counts."""
import os

import numpy as np
import torch
import torch.nn as nn

from .. import _lib, ops
from ..optim import AdamW as _ArenaAdamW
from .networks import CDNet

CHANNEL_WEIGHTS = (0.05, 0.2, 0.8, 0.7, 0.4)          # xBD_code/train.py:353
UNET_CHANNEL_WEIGHTS = (0.1, 0.1, 0.6, 0.3, 1.0)      # xBD_code/train_unettransformer.py:456
UNET_CE_WEIGHTS = (0.01, 0.10, 1.0, 0.80, 1.0)        # ... :563
UNET_CE_SCALE = 8.0                                   # ... :456 (loss5 * 8)
UNET_MILESTONES = (5, 11, 17, 23, 29, 33, 47, 50, 60, 70, 90, 110, 130, 150, 170, 180, 190)      # ... :536
UNET_GAMMA = 0.6
ADAPT_CHANNEL_WEIGHTS = (0.1, 0.8, 2.0, 8.0)          # xBD_code/train_adapt.py:336
ADAPT_CE_WEIGHTS = (0.1, 0.5, 1.5, 1.5)               # ... :320
ADAPT_CE_SCALE = 5.0                                  # ... :340 (ce_loss(...) * 5)
ADAPT_MILESTONES = (5, 11, 23, 29, 33, 47, 50, 60, 70, 90, 110, 130, 150, 170, 180, 190)      # ... :423 (no 17 in this list)
ADAPT_MAX_NORM = 0.999                                # ... :346
_weights = {}


def BASE_Transformer_UNet(input_nc=3, output_nc=5, with_pos='learned', resnet_stages_num=4, token_len=4, token_trans=True,
                          enc_depth=1, dec_depth=8, dim_head=64, decoder_dim_head=64, tokenizer=True,
                          if_upsample_2x=True, pool_mode='max', pool_size=2, backbone='resnet18', decoder_softmax=True,
                          with_decoder_pos=None, with_decoder=True, compute_dtype=None):
    """Constructor of the xBD copy.  `dec_depth` is accepted and ignored exactly as the reference does (the per-level
    decoder depths 4/4/8/1 are hard-coded, model_transformer_encoding.py:318-334).  Default torch initialisation (the
    xBD scripts never call init_weights).  output_nc: 5 (train.py) or 4 (train_adapt.py: netspec's `..._c4` entries, the same
    state but for the classifier's two shapes); anything else raises NotImplementedError."""
    if (input_nc, with_pos, resnet_stages_num, token_len, enc_depth, dim_head, decoder_dim_head, backbone) != \
            (3, 'learned', 4, 4, 1, 64, 64, 'resnet18') or output_nc not in (4, 5) or \
            not (tokenizer and token_trans and with_decoder and decoder_softmax):
        raise NotImplementedError("only the configurations of xBD_code/train.py:44-45 and train_adapt.py:37-38 are built "
                                  "(input_nc=3, output_nc=5 or 4, token_len=4, with_pos='learned', resnet18)")
    if with_decoder_pos not in (None, 'learned'):
        raise NotImplementedError("with_decoder_pos must be None or 'learned'")
    print("using UNet Transformer !!!!")
    name = "xbd_unet_transformer" if output_nc == 5 else "xbd_unet_transformer_c4"
    return CDNet(name if with_decoder_pos == 'learned' else name + "_nodecpos", compute_dtype)


# ---- loss ------------------------------------------------------------------------------------------------
class _Combo(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, masks, weights_dev, dice_w, focal_w):
        loss, channel, sums = ops.combo_loss_fwd(logits, masks, weights_dev, dice_w, focal_w)
        ctx.save_for_backward(logits, masks, sums, weights_dev)
        ctx.w = (dice_w, focal_w)
        ctx.mark_non_differentiable(channel)
        return loss, channel

    @staticmethod
    def backward(ctx, dloss, _dchannel):
        logits, masks, sums, weights_dev = ctx.saved_tensors
        up = dloss.detach().to(torch.float32).reshape(1).contiguous()
        return ops.combo_loss_bwd(logits, masks, sums, weights_dev, up, *ctx.w), None, None, None, None


def _check(outputs, targets):
    if not (outputs.is_cuda and targets.is_cuda):
        raise _lib.HipLibraryError("dahitra_amd xBD loss runs on MI355X only (no CPU fallback)")
    if outputs.shape != targets.shape:
        raise ValueError("logits %s and masks %s must have the same shape" % (tuple(outputs.shape), tuple(targets.shape)))


class ComboLoss(nn.Module):
    """ComboLoss({'dice': a, 'focal': b}): a * soft dice over the whole batch + b * FocalLoss2d(gamma 2), both on
    sigmoid(outputs) (xBD_code/losses.py:95-126).  Other terms of the reference's mapping (bce, jaccard, lovasz, ...)
    are not on the executed path (train.py:316) and raise."""

    def __init__(self, weights, per_image=False):
        super().__init__()
        extra = [k for k, v in weights.items() if v and k not in ("dice", "focal")]
        if extra or per_image:
            raise NotImplementedError("ComboLoss terms %s / per_image are outside the executed xBD step" % extra)
        self.weights = dict(weights)
        self.values = {}

    def forward(self, outputs, targets):
        """outputs / targets: one channel [B, H, W] (the reference's call, train.py:348-352) or [B, C, H, W]"""
        _check(outputs, targets)
        lo = outputs.float().contiguous()
        lo = lo.unsqueeze(1) if lo.dim() == 3 else lo
        ta = targets.float().contiguous().view(lo.shape)
        key = (str(lo.device), (1.0,) * lo.shape[1])
        ones = _weights.get(key)
        if ones is None:
            ones = _weights[key] = torch.ones(lo.shape[1], dtype=torch.float32, device=lo.device)
        loss, _ = _Combo.apply(lo, ta, ones, float(self.weights.get("dice", 0)), float(self.weights.get("focal", 0)))
        return loss


def channel_weights_dev(device, channel_weights=CHANNEL_WEIGHTS):
    """the channel weights as a cached device tensor (no host-to-device copy inside a HIP-graph capture)"""
    key = (str(device), tuple(float(v) for v in channel_weights))
    w = _weights.get(key)
    if w is None:
        w = _weights[key] = torch.tensor(key[1], dtype=torch.float32, device=device)
    return w


def xbd_loss(out, msks, channel_weights=CHANNEL_WEIGHTS, dice=1.0, focal=8.0, want_channels=False, lovasz=0.0):
    """train.py:348-353 in one pass: sum_c w_c * ComboLoss{dice:1, focal:8}(out[:, c], msks[:, c]).
    lovasz: the weight of ComboLoss's 'lovasz' term in every channel's loss: a non-zero value adds
    lovasz * sum_c w_c * lovasz_hinge(out[:, c], msks[:, c], per_image=False) (xbd_losses, dh_xbd_lovasz_fwd; nothing is
    ignored); the channel losses of want_channels stay those of dice and focal.  0 launches what it always launched."""
    _check(out, msks)
    key = (str(out.device), tuple(float(v) for v in channel_weights))
    w = _weights.get(key)
    if w is None:                    # cached: no host-to-device copy inside a HIP-graph capture
        w = _weights[key] = torch.tensor(key[1], dtype=torch.float32, device=out.device)
    logits = out.float().contiguous()
    loss, channel = _Combo.apply(logits, msks.float().contiguous(), w, float(dice), float(focal))
    if lovasz:
        from .xbd_losses import _Lovasz
        hinge, _ = _Lovasz.apply(logits, (msks if msks.dtype == torch.uint8 else msks.float()).contiguous(), "hinge", False, None, w)
        loss = loss + float(lovasz) * hinge
    return (loss, channel) if want_channels else loss


# ---- losses of xBD_code/train_unettransformer.py (lines 438-461, 562-564) and xBD_code/train_adapt.py (lines 332-342) ----------
class _ScriptLoss(torch.autograd.Function):
    """both scripts' losses: `form` is the row of ops._XBD_LOSS_FORMS, lbl and labels are None where the form has no lbl"""
    @staticmethod
    def forward(ctx, form, logits, msks, lbl, labels, weights_dev, dice_w, focal_w, ce_w):
        loss, parts, sums = ops._xbd_loss_fwd(form, logits, msks, lbl, labels, weights_dev, dice_w, focal_w, ce_w)
        ctx.save_for_backward(logits, msks, lbl, sums, weights_dev)
        ctx.how = (form, labels, dice_w, focal_w, ce_w)
        ctx.mark_non_differentiable(parts)
        return loss, parts

    @staticmethod
    def backward(ctx, dloss, _dparts):
        logits, msks, lbl, sums, weights_dev = ctx.saved_tensors
        form, labels, dice_w, focal_w, ce_w = ctx.how
        up = dloss.detach().to(torch.float32).reshape(1).contiguous()
        return (None, ops._xbd_loss_bwd(form, logits, msks, lbl, labels, sums, weights_dev, up, dice_w, focal_w, ce_w)) + (None,) * 7


def _loss_weights_dev(what, device, n, channel_weights, ce_weights):
    key = (str(device), tuple(float(v) for v in channel_weights), tuple(float(v) for v in ce_weights))
    if len(key[1]) != n or len(key[2]) != n:
        raise ValueError("%s: channel_weights %r and ce_weights %r must hold %d numbers each" % (what, key[1], key[2], n))
    w = _weights.get(key)
    if w is None:
        w = _weights[key] = torch.tensor(key[1] + key[2], dtype=torch.float32, device=device)
    return w


def unet_weights_dev(device, channel_weights=UNET_CHANNEL_WEIGHTS, ce_weights=UNET_CE_WEIGHTS):
    """the 5 channel weights and the 5 class weights as ONE cached device tensor [10], the form ops.xbd_unet_loss_fwd takes (no
    host-to-device copy inside a HIP-graph capture).  ValueError unless both hold 5 numbers."""
    return _loss_weights_dev("unet_loss", device, 5, channel_weights, ce_weights)


def unet_loss(out, msks, lbl_msk=None, labels='lbl_msk', channel_weights=UNET_CHANNEL_WEIGHTS, ce_weights=UNET_CE_WEIGHTS,
              dice=1.0, focal=8.0, ce=UNET_CE_SCALE, want_parts=False):
    """The loss of train_unettransformer.py:438-456 in one pass over the pixels (ops.xbd_unet_loss_fwd; one more for the gradient):
        sum_c channel_weights[c] * ComboLoss{dice, focal}(out[:, c], msks[:, c])
        + ce * CrossEntropyLoss(weight=ce_weights)(out * (y > 0), y)
    out: logits [B, 5, H, W]; msks: uint8 [B, 5, H, W] AS THE LOADER YIELDS THEM (no float copy is made; another dtype is
    refused).  labels='lbl_msk' is the script as executed: y = lbl_msk, uint8 [B, H, W] -- which its TrainData makes zero at
    every pixel, so the cross-entropy term is the constant ln 5 and has no gradient.  labels='damage' is the term as intended
    ("ce loss only on building"): y = the first set channel among 1 .. 4 of msks, 0 where none is set; lbl_msk is not read.
    want_parts: also return the device tensor parts [8] = ops.XBD_UNET_PARTS: the five channel losses, the cross-entropy, the
    script's Dice meter (line 460: on channel 0 AFTER the in-place masking, so 0.5-sigmoids wherever y is 0) and the number of
    label bytes above 4 (they add nothing to the cross-entropy and get no gradient from it; torch raises IndexError there,
    train_epoch_unet does so at the end of the epoch).  No host synchronisation."""
    if not (torch.is_tensor(out) and out.is_cuda):
        raise _lib.HipLibraryError("dahitra_amd xBD loss runs on MI355X only (no CPU fallback)")
    w = unet_weights_dev(out.device, channel_weights, ce_weights)
    lbl = lbl_msk.contiguous() if torch.is_tensor(lbl_msk) and labels != 'damage' else None
    if labels == 'lbl_msk' and lbl is None:
        raise ValueError("unet_loss: labels='lbl_msk' reads lbl_msk, which is %r" % (lbl_msk,))
    loss, parts = _ScriptLoss.apply("unet", out.float().contiguous(), msks.contiguous() if torch.is_tensor(msks) else msks, lbl,
                                    labels, w, float(dice), float(focal), float(ce))
    return (loss, parts) if want_parts else loss


# ---- clip + optimizer ------------------------------------------------------------------------------------
def clip_grad_norm_(parameters, max_norm):
    """torch.nn.utils.clip_grad_norm_(parameters, max_norm) for the parameters of ONE dahitra_amd net: the total L2
    norm over the flat gradient arena and the in-place scaling by min(1, max_norm / (norm + 1e-6)), without a host
    synchronisation.  Returns the total norm as a device scalar."""
    params = [p for p in parameters if p.grad is not None]
    nets = {id(getattr(p, "_dh_arena", (None,))[0]): getattr(p, "_dh_arena", (None,))[0] for p in params}
    if len(nets) != 1 or None in nets.values():
        raise _lib.HipLibraryError("clip_grad_norm_: parameters must belong to one dahitra_amd net on the GPU")
    net = next(iter(nets.values()))
    if len(params) != len(net._active_keys):
        raise ValueError("clip_grad_norm_: pass all of net.parameters() (the norm is taken over the whole arena)")
    _, grad = net.flat_params()
    out = torch.empty(2, dtype=torch.float32, device=grad.device)
    ops.grad_norm_clip_coef(grad, float(max_norm), out)
    ops.scale_into(grad, out[1:2], grad)
    return out[0]


class AdamW(_ArenaAdamW):
    """xBD_code/adamw.py: m, v as Adam; denom = sqrt(v) + eps; step = lr * sqrt(1 - b2^t) / (1 - b1^t);
    w -= weight_decay * lr * w before the Adam term.  One launch over the net's flat arena."""
    _rule = "xbd"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, capturable=False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=capturable)


# ---- validation (xBD_code/train.py:247-307) ----------------------------------------------------------------
def val_score(image_counts, class_counts, empty_score=1.0, classes=4):
    """The reference's score from the counts of ops.xbd_val_count, in its own float64 numpy expressions.
    image_counts: integers [n_images, 3] = |gt0|, |loc|, |gt0 & loc| per image; class_counts: integers [4, 3] = tp, fn, fp per
    class.  dice of an image = 2 |gt0 & loc| / (|gt0| + |loc|), `empty_score` when both are empty (utils.py:147-154);
    d0 = mean of the dices; f1_sc[c] = 2 tp / (2 tp + fp + fn), nan for 0 / 0 as numpy gives it; f1 = 4 / sum(1 / (f1_sc +
    1e-6)); score = 0.3 d0 + 0.7 f1 (train.py:281-288).  A class without a counted pixel makes the score nan, and
    `nan > best_score` is False: the reference's behaviour, kept.  Returns (score, {'dice', 'f1', 'f1_per_class'}).
    The counts are additive: ranks that validate shards sum them before this call.
    classes: the damage classes, 4 (default: all of the above) or 3 -- xBD_code/train_adapt.py:282-289 for its four-output net:
    class_counts [3, 3] and f1 = 3 / sum(1 / (f1_sc + 1e-6)).  ValueError for another number."""
    if classes not in ops.XBD_VAL_CLASSES:
        raise ValueError("val_score: classes %r is not one of %s" % (classes, list(ops.XBD_VAL_CLASSES)))
    ic = np.asarray(image_counts.cpu() if torch.is_tensor(image_counts) else image_counts).astype(np.int64).reshape(-1, 3)
    cc = np.asarray(class_counts.cpu() if torch.is_tensor(class_counts) else class_counts).astype(np.int64).reshape(classes, 3)
    dices0 = []
    for gt0, loc, both in ic:
        im_sum = gt0 + loc
        dices0.append(empty_score if im_sum == 0 else 2. * both / im_sum)
    with np.errstate(divide='ignore', invalid='ignore'):
        d0 = np.mean(dices0) if dices0 else np.float64('nan')
        tp, fn, fp = (cc[:, k].astype(np.float64) for k in range(3))          # np.zeros((4,)) accumulators: float64
        f1_sc = np.zeros((classes,))
        for c in range(classes):
            f1_sc[c] = 2 * tp[c] / (2 * tp[c] + fp[c] + fn[c])
        f1 = classes / np.sum(1.0 / (f1_sc + 1e-6))
        sc = 0.3 * d0 + 0.7 * f1
    return sc, {'dice': d0, 'f1': f1, 'f1_per_class': f1_sc}


def _device_u8(what, *tensors):
    for t in tensors:
        if not (torch.is_tensor(t) and t.is_cuda):
            raise _lib.HipLibraryError("dahitra_amd xBD %s runs on MI355X only (no CPU fallback)" % what)


def _kept_step(owner, slot, key, build, fresh):
    """the recorded step kept in the dictionary `slot` of the model `owner` under `key` (kept: a graph pins its buffers for the
    life of the process, so an epoch must not record a new one); `build()` records it when there is none or `fresh(step)` is
    no longer true"""
    steps = owner.__dict__.setdefault(slot, {})
    step = steps.get(key)
    if step is None or not fresh(step):
        step = steps[key] = build()
    return step


def _eval_step(model, batch, class_counts, thr, select, classes=4):
    """the model's recorded validation step for this batch shape, threshold, selection and device"""
    from ..graph import GraphedXbdEvalStep
    imgs = batch['img']
    return _kept_step(model, '_xbd_eval_steps', (tuple(imgs.shape), float(thr), select, str(imgs.device)),
                      lambda: GraphedXbdEvalStep(model, imgs, batch['msk'], batch['lbl_msk'], class_counts, thr, select,
                                                 classes=classes),
                      lambda step: step._generation == model._arena.generation and step.class_counts is class_counts)


def _next_rows(rows, n, count, row_shape, dtype, device):
    """The rows [n, n + count) of an epoch's device buffer [*, *row_shape], made by the first call (rows=None) and doubled, on the
    device, when it is full: an iterator does not say how long it is.  Returns (the buffer, the view of those rows)."""
    if rows is None:
        rows = torch.zeros((max(64, count),) + row_shape, dtype=dtype, device=device)
    if n + count > rows.shape[0]:
        rows = torch.cat([rows, torch.zeros((max(rows.shape[0], count),) + row_shape, dtype=dtype, device=device)])
    return rows, rows[n:n + count]


def _epoch(what, model, batches, row_shape, accumulator, replay, eager):
    """The epoch loop of validate and validate_sweep.  The first batch fixes the shape and the device; accumulator(device) gives
    the int64 class accumulator (kept on the model: a recorded step holds its address), zeroed here; every image gets one int64
    row of `row_shape` in a device buffer that doubles when it is full.  A batch of the first shape goes through
    replay(batch, accumulator) -> the batch's rows (None: no graph), any other through eager(logits, msk, lbl, rows, accumulator).
    ONE host read when the epoch is over; returns (rows [n_images, *row_shape], accumulator) as numpy integers."""
    model.eval()
    acc, rows, n, first, dev = None, None, 0, None, None
    with torch.no_grad():
        for batch in batches:
            imgs, msk, lbl = batch['img'], batch['msk'], batch['lbl_msk']
            _device_u8("validation", imgs)
            B = imgs.shape[0]
            if first is None:
                dev, first = imgs.device, tuple(imgs.shape)
                acc = accumulator(dev)
                acc.zero_()
            rows, mine = _next_rows(rows, n, B, row_shape, torch.int64, dev)
            if replay is not None and tuple(imgs.shape) == first:
                mine.copy_(replay(batch, acc), non_blocking=True)
            else:
                eager(model(imgs).float(), msk, lbl, mine, acc)
            n += B
    if rows is None:
        raise ValueError("%s: no batches" % what)
    both = torch.cat([rows[:n].reshape(-1), acc.reshape(-1)]).cpu().numpy()        # the epoch's one read
    cut = rows[:n].numel()
    return both[:cut].reshape((n,) + row_shape), both[cut:].reshape(tuple(acc.shape))


def _val_counts(what, model, batches, thr, select, graph, classes):
    """the epoch of validate (classes 4) and validate_adapt (3): (image_counts [n_images, 3], class_counts [classes, 3]) as numpy
    integers, from ONE host read.  The class accumulator is kept on the model: a recorded step holds its address."""
    if select not in ops.XBD_VAL_SELECT:
        raise ValueError("%s: select %r is not one of %s" % (what, select, sorted(ops.XBD_VAL_SELECT)))

    def accumulator(dev):
        cc = model.__dict__.get('_xbd_val_class_counts')
        if cc is None or cc.device != dev or cc.shape[0] != classes:
            cc = model.__dict__['_xbd_val_class_counts'] = torch.zeros(classes, 3, dtype=torch.int64, device=dev)
        return cc

    def replay(batch, cc):
        step = _eval_step(model, batch, cc, thr, select, classes)
        step(batch['img'], batch['msk'], batch['lbl_msk'])
        return step.image_counts
    return _epoch(what, model, batches, (3,), accumulator, replay if graph else None,
                  lambda logits, msk, lbl, rows, cc: ops.xbd_val_count(logits, msk, lbl, rows, cc, thr, select, classes))


def validate(model, batches, thr=0.3, select='reference', graph=True, want_counts=False):
    """validate(model, data_loader) of xBD_code/train.py:247-290 on the device.  batches: dicts {'img' [B, 6, H, W] fp32,
    'msk' [B, 5, H, W], 'lbl_msk' [B, H, W]} as GpuXbdPipeline.batches(b, size, train=False) yields them (uint8; the
    reference's long tensors are converted).  Per batch: the eval-mode forward and ONE count kernel (ops.xbd_val_count); the
    batch's image rows go into the epoch's [n_images, 3] device buffer by an asynchronous device copy.  Nothing is read by the
    host until the epoch is over: ONE read then, and val_score on the integers.  graph=True replays a GraphedXbdEvalStep for
    every batch of the first batch's shape (recorded once per model and shape) and runs other shapes -- a ragged last batch --
    eagerly; the counts are the same bits either way.  select: 'reference' (default; train.py:271-274 as executed: rows chosen
    by the first row of lbl_msk) or 'building' (pixels of msk[:, 0]), see ops.xbd_val_count.
    Prints the reference's `Val Score: ...` line and returns the score (with want_counts: score, parts, image_counts,
    class_counts as numpy integers)."""
    image_counts, cc = _val_counts("validate", model, batches, thr, select, graph, 4)
    sc, parts = val_score(image_counts, cc)
    f1_sc = parts['f1_per_class']
    print("Val Score: {}, Dice: {}, F1: {}, F1_0: {}, F1_1: {}, F1_2: {}, F1_3: {}".format(sc, parts['dice'], parts['f1'], f1_sc[0],
                                                                                          f1_sc[1], f1_sc[2], f1_sc[3]))
    return (sc, parts, image_counts, cc) if want_counts else sc


def _keep_best(d, best_score, model, optimizer, path, current_epoch, thr=None):
    """the second half of evaluate_val (train.py:296-307): when the score `d` beats `best_score` save the snapshot {'epoch':
    current_epoch + 1, 'state_dict', 'best_score', 'optimizer'} -- and 'thr', where one is given -- to `path`; print the
    `score: ... score_best: ...` line and return the best score.  A nan score beats nothing."""
    if d > best_score:
        folder = os.path.dirname(path)
        if folder:
            os.makedirs(folder, exist_ok=True)
        snapshot = {
            'epoch': current_epoch + 1,
            'state_dict': model.state_dict(),
            'best_score': d,
            'optimizer': optimizer.state_dict(),
        }
        if thr is not None:
            snapshot['thr'] = thr
        torch.save(snapshot, path)
        best_score = d
    print("score: {}\tscore_best: {}".format(d, best_score))
    return best_score


def evaluate_val(batches, best_score, model, optimizer, path, current_epoch, thr=0.3, select='reference', graph=True):
    """evaluate_val of xBD_code/train.py:293-307: validate, and when the score beats `best_score` save the snapshot {'epoch':
    current_epoch + 1, 'state_dict', 'best_score', 'optimizer'} to `path` (the reference's models_folder/snapshot_name).  A nan
    score (no counted pixel) beats nothing, as in the reference.  Prints its `score: ... score_best: ...` line and returns the
    best score."""
    model = model.eval()
    d = validate(model, batches, thr=thr, select=select, graph=graph)
    return _keep_best(d, best_score, model, optimizer, path, current_epoch)


# ---- threshold sweep: validate for a whole grid of localisation thresholds from ONE pass ---------------------------------
# ops.xbd_val_sweep files every pixel under bin = the number of grid thresholds its localisation sigmoid exceeds.  The thresholds
# ascend, so "s0 > thresholds[k]" is "bin > k": a localisation rule is a bool table over (bin, arg), and the counts of
# ops.xbd_val_count under that rule are sums of histogram cells -- int64 sums, exact, on the host, without the device.
def sweep_loc_table(T, k):
    """The rule `loc = s0 > thresholds[k]` as a table: bool [T + 1, 4], loc[b, a] = b > k_a.  k: one index into the grid of T
    thresholds, or four -- one per damage arg-max a.  ValueError for an index outside 0 .. T - 1."""
    ks = np.asarray(k)
    if ks.dtype.kind not in "iu" or ks.shape not in ((), (4,)):
        raise ValueError("sweep_loc_table: k %r is neither one grid index nor four" % (k,))
    ks = np.broadcast_to(ks, (4,)).astype(np.int64)
    if T < 1 or ks.min() < 0 or ks.max() >= T:
        raise ValueError("sweep_loc_table: k %r is outside the grid of %d thresholds" % (k, T))
    return np.arange(T + 1, dtype=np.int64)[:, None] > ks[None, :]


def sweep_rule_table(thresholds, t0, t1, t2):
    """The three-threshold rule of xBD_code/visualize_results.py:209 as a table over the grid, with dmg = arg + 1:
        loc = (p > t0) | ((p > t1) & (dmg > 1) & (dmg < 4)) | ((p > t2) & (dmg > 1))
    so arg 0 is kept above t0, arg 1 and arg 2 above min(t0, t1, t2), arg 3 above min(t0, t2).  Each of t0, t1, t2 must equal
    a threshold of the grid after conversion to float32: ValueError otherwise (the histogram cannot split a bin)."""
    thr = ops.xbd_sweep_thresholds(thresholds, "sweep_rule_table")
    t = [np.float32(v) for v in (t0, t1, t2)]
    for name, v in zip(("t0", "t1", "t2"), t):
        if not (thr == v).any():
            raise ValueError("sweep_rule_table: %s=%r is not a threshold of the grid %s" % (name, float(v), thr.tolist()))
    per_arg = (t[0], min(t), min(t), min(t[0], t[2]))
    return sweep_loc_table(thr.size, [int(np.nonzero(thr == v)[0][0]) for v in per_arg])


def sweep_counts(image_hist, class_hist, loc):
    """The counts ops.xbd_val_count would have written under the rule `loc`, from the histograms of ops.xbd_val_sweep.
    image_hist: integers [n, T + 1, 4, 2] = [image, bin, arg, g0]; class_hist: integers [T + 1, 4, 5] = [bin, arg, t];
    loc: bool [T + 1, 4] (sweep_loc_table / sweep_rule_table).  Returns (image_counts int64 [n, 3] = |gt0|, |loc|, |gt0 & loc|,
    class_counts int64 [4, 3] = tp, fn, fp), the layout val_score takes.  pred(bin, arg) = arg where loc, else 0; class c has
    tp over [pred == c][t == c], fn over [pred != c][t == c], fp over [pred == c][t != c]; t = 4 (a label above 3) is no
    class's truth.  The histograms are additive: ranks that validate shards sum them before this call."""
    loc = np.asarray(loc)
    if loc.dtype != np.bool_ or loc.ndim != 2 or loc.shape[1] != 4:
        raise ValueError("sweep_counts: loc %s %s is not a bool [T + 1, 4] table" % (loc.shape, loc.dtype))
    nb = loc.shape[0]
    ih = np.asarray(image_hist.cpu() if torch.is_tensor(image_hist) else image_hist).astype(np.int64)
    ch = np.asarray(class_hist.cpu() if torch.is_tensor(class_hist) else class_hist).astype(np.int64)
    if ih.ndim != 4 or ih.shape[1:] != (nb, 4, 2) or ch.shape != (nb, 4, 5):
        raise ValueError("sweep_counts: image_hist %s / class_hist %s do not fit a [%d, 4] rule" % (ih.shape, ch.shape, nb))
    image_counts = np.stack([ih[..., 1].sum(axis=(1, 2)), ih[:, loc].sum(axis=(1, 2)), ih[:, loc, 1].sum(axis=1)], axis=1)
    pred = np.where(loc, np.arange(4, dtype=np.int64)[None, :], 0)                  # [bin, arg]
    class_counts = np.zeros((4, 3), dtype=np.int64)
    for c in range(4):
        is_c = pred == c
        class_counts[c] = ch[is_c, c].sum(), ch[~is_c, c].sum(), ch[is_c].sum() - ch[is_c, c].sum()
    return image_counts, class_counts


class XbdSweep:
    """An epoch's threshold sweep (validate_sweep): `thresholds` float32 [T], `image_hist` int64 [n_images, T + 1, 4, 2],
    `class_hist` int64 [T + 1, 4, 5] and `scores` float64 [T], scores[k] = the score validate(thr=thresholds[k]) gives."""

    def __init__(self, thresholds, image_hist, class_hist):
        self.thresholds = ops.xbd_sweep_thresholds(thresholds, "XbdSweep")
        T = self.thresholds.size
        self.image_hist = np.asarray(image_hist, dtype=np.int64).reshape(-1, T + 1, 4, 2)
        self.class_hist = np.asarray(class_hist, dtype=np.int64).reshape(T + 1, 4, 5)
        self.scores = np.array([val_score(*self.counts(k))[0] for k in range(T)], dtype=np.float64)

    def counts(self, k):
        """(image_counts [n, 3], class_counts [4, 3]) at thresholds[k]: what validate(thr=thresholds[k], want_counts=True) counts"""
        return sweep_counts(self.image_hist, self.class_hist, sweep_loc_table(self.thresholds.size, k))

    def parts(self, k):
        """{'dice', 'f1', 'f1_per_class'} at thresholds[k] (val_score's second result)"""
        return val_score(*self.counts(k))[1]

    def best(self):
        """(threshold, score) of the highest score: nan scores are ignored, the lowest threshold wins a tie; (None, nan) if every
        score is nan"""
        if np.isnan(self.scores).all():
            return None, float('nan')
        k = int(np.nanargmax(self.scores))          # the first maximum
        return float(self.thresholds[k]), float(self.scores[k])

    def score_rule(self, t0, t1, t2):
        """(score, parts) under the three-threshold rule of visualize_results.py:209 (sweep_rule_table); t0, t1, t2 from the grid"""
        return val_score(*sweep_counts(self.image_hist, self.class_hist, sweep_rule_table(self.thresholds, t0, t1, t2)))


def _sweep_step(model, batch, class_hist, thresholds, select):
    """the model's recorded sweep step for this batch shape, grid, selection and device (kept on the model, as _eval_step does)"""
    from ..graph import GraphedXbdSweepStep
    imgs = batch['img']
    return _kept_step(model, '_xbd_sweep_steps', (tuple(imgs.shape), thresholds.tobytes(), select, str(imgs.device)),
                      lambda: GraphedXbdSweepStep(model, imgs, batch['msk'], batch['lbl_msk'], class_hist, thresholds, select),
                      lambda step: step._generation == model._arena.generation and step.class_hist is class_hist)


def validate_sweep(model, batches, thresholds, select='reference', graph=True):
    """validate for every threshold of a grid from ONE epoch of forwards.  batches, select and graph as validate; thresholds:
    1 .. ops.XBD_SWEEP_MAX floats inside (0, 1), strictly ascending as float32.  Per batch: the eval-mode forward and ONE
    histogram kernel (ops.xbd_val_sweep); the batch's image rows go into the epoch's device buffer by an asynchronous device
    copy, and the host reads ONCE when the epoch is over.  graph=True replays a GraphedXbdSweepStep for every batch of the first
    batch's shape (recorded once per model, shape, grid, selection and device) and runs other shapes eagerly; the integers
    are the same either way.  Prints `thr {thr}: ` and the reference's `Val Score: ...` line for every threshold and returns
    the XbdSweep: .scores[k] is what validate(thr=thresholds[k]) returns, .best() the (threshold, score) to keep."""
    if select not in ops.XBD_VAL_SELECT:
        raise ValueError("validate_sweep: select %r is not one of %s" % (select, sorted(ops.XBD_VAL_SELECT)))
    thr = ops.xbd_sweep_thresholds(thresholds, "validate_sweep")
    T = thr.size

    def accumulator(dev):
        hists = model.__dict__.setdefault('_xbd_sweep_class_hist', {})
        class_hist = hists.get((T, str(dev)))          # one buffer per grid size: a recorded step holds its address
        if class_hist is None:
            class_hist = hists[(T, str(dev))] = torch.zeros(T + 1, 4, 5, dtype=torch.int64, device=dev)
        return class_hist

    def replay(batch, class_hist):
        step = _sweep_step(model, batch, class_hist, thr, select)
        step(batch['img'], batch['msk'], batch['lbl_msk'])
        return step.image_hist
    sweep = XbdSweep(thr, *_epoch("validate_sweep", model, batches, (T + 1, 4, 2), accumulator, replay if graph else None,
                                  lambda logits, msk, lbl, rows, ch: ops.xbd_val_sweep(logits, msk, lbl, rows, ch, thr, select)))
    for k in range(T):
        sc, parts = sweep.scores[k], sweep.parts(k)
        f1_sc = parts['f1_per_class']
        print("thr {}: Val Score: {}, Dice: {}, F1: {}, F1_0: {}, F1_1: {}, F1_2: {}, F1_3: {}".format(
            str(thr[k]), sc, parts['dice'], parts['f1'], f1_sc[0], f1_sc[1], f1_sc[2], f1_sc[3]))
    return sweep


def evaluate_val_sweep(batches, best_score, model, optimizer, path, current_epoch, thresholds, select='reference', graph=True):
    """evaluate_val with the grid's best threshold: validate_sweep, and when the best threshold's score beats `best_score` save
    evaluate_val's snapshot with one more key, 'thr' (that threshold, a Python float), to `path`.  All-nan scores beat nothing.
    Prints the `score: ... score_best: ...` line and returns the best score."""
    model = model.eval()
    thr, d = validate_sweep(model, batches, thresholds, select=select, graph=graph).best()
    return _keep_best(d, best_score, model, optimizer, path, current_epoch, thr)


# ---- the epoch of xBD_code/train_unettransformer.py (lines 421-486, 532-575) ----------------------------------------
def unet_scheduler(optimizer):
    """lr_scheduler.MultiStepLR(optimizer, milestones=[5, 11, 17, 23, 29, 33, 47, 50, 60, ...], gamma=0.6) of line 536"""
    return torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=list(UNET_MILESTONES), gamma=UNET_GAMMA)


def unet_val_batches(pipe, batch_size=16, crop=256, indices=None):
    """The script's ValData (lines 288-352) from a GpuXbdPipeline: the samples in order, the fixed crop at x0 = y0 = 512, no
    augmentation, ValData's masks (train=False) -- what validate / evaluate_val take.  The script's val_batch_size is 16 and its
    DataLoader keeps the ragged last batch.
    indices: None -- every sample -- or the source indices to validate on, in the order given: the `val_idxs` of
    pipe.unet_trainset(), the tenth the script holds out of the one folder it trains on.  ValueError, before any launch, for an
    empty list or an index outside the samples."""
    from ..datasets.xbd_pipeline import epoch_order
    order = epoch_order(len(pipe), indices)
    for s in range(0, len(order), batch_size):
        ind = order[s:s + batch_size]
        yield pipe.make_batch(ind, crop, [[512, 512, 0, 0, 0, 0, 0, crop, crop]] * len(ind), train=False)


def unet_eager_step(model, optimizer, imgs, msks, lbl_msk, labels, update=True):
    """The script's step through autograd (train_unettransformer.py:436-481): zero_grad, forward, unet_loss, backward and --
    with `update` -- optimizer.step(), no clip.  Returns (logits, loss, parts), detached.  What train_epoch_unet runs for a batch
    without a recorded step, and GraphedXbdUnetStep's `_eager_body`."""
    model.zero_grad()
    logits = model(imgs)
    loss, parts = unet_loss(logits, msks, lbl_msk, labels, want_parts=True)
    loss.backward()
    if update:
        optimizer.step()
    return logits.detach(), loss.detach(), parts


def _script_train_step(step_class, eager_step, slot, fields, extra, model, optimizer, first, graph):
    """run(batch) -> (loss, parts) device tensors for the batches of one epoch of a training script: batches of the first batch's
    shape replay the model's recorded step -- graph.<step_class>, kept in the model's `slot` per shape, `extra`, optimizer and
    device -- any other shape -- a ragged last batch -- and graph=False take `eager_step`.  fields: the batch's entries that the
    step takes, in its order; extra: what its constructor and the eager step take after them."""
    _device_u8("training", first['img'], first['msk'])

    def eager(batch):
        return eager_step(model, optimizer, *(batch[f] for f in fields), *extra)[1:]
    if not graph:
        return eager
    from .. import graph as graphs
    imgs = first['img']
    model._ensure_arena(imgs.device)
    step = _kept_step(model, slot, (tuple(imgs.shape),) + extra + (id(optimizer), str(imgs.device)),
                      lambda: getattr(graphs, step_class)(model, optimizer, *(first[f] for f in fields), *extra),
                      lambda step: step._generation == model._arena.generation and step.opt is optimizer)

    def replay(batch):
        if tuple(batch['img'].shape) != tuple(imgs.shape):
            return eager(batch)
        return step(*(batch[f] for f in fields)), step.parts
    return replay


def _unet_train_step(model, optimizer, first, labels, graph):
    """_script_train_step of GraphedXbdUnetStep, kept per shape, label mode, optimizer and device"""
    return _script_train_step('GraphedXbdUnetStep', unet_eager_step, '_xbd_unet_steps', ('img', 'msk', 'lbl_msk'), (labels,),
                              model, optimizer, first, graph)


def _train_epoch(what, current_epoch, model, optimizer, scheduler, batches, step_for, n_parts, columns, printed, check=None):
    """The epoch of train_epoch_unet and train_epoch_adapt.  step_for(first batch) -> run(batch) -> (loss, parts [n_parts]); every
    step's row [loss, parts...] goes into a device buffer, read ONCE when the epoch is over; check(rows), if given, may refuse
    the epoch before the scheduler moves.  columns: meter name -> column of the row, AverageMeter's mean weighted by the batch
    size; printed: the three meters of the script's closing line."""
    model.train()
    run, rows, sizes = None, None, []
    for batch in batches:
        if run is None:
            run = step_for(batch)
        loss, parts = run(batch)
        rows, row = _next_rows(rows, len(sizes), 1, (1 + n_parts,), torch.float32, loss.device)
        row[0, 0:1].copy_(loss.reshape(1), non_blocking=True)
        row[0, 1:].copy_(parts, non_blocking=True)
        sizes.append(int(batch['img'].shape[0]))
    if rows is None:
        raise ValueError("%s: no batches" % what)
    host = rows[:len(sizes)].cpu().numpy().astype(np.float64)          # the epoch's one read
    if check is not None:
        check(host)
    w = np.asarray(sizes, dtype=np.float64)
    meters = {k: float((host[:, col] * w).sum() / w.sum()) for k, col in columns}        # AverageMeter: sum(val * n) / sum(n)
    scheduler.step()
    lr = optimizer.param_groups[-1]['lr']
    print("epoch: {}; lr {:.7f}; Loss {:.4f}; loss2 {:.4f}; Dice {:.4f}".format(current_epoch, lr, *(meters[k] for k in printed)))
    meters.update(lr=lr, steps=len(sizes), samples=int(w.sum()))
    return meters


def train_epoch_unet(current_epoch, model, optimizer, scheduler, batches, labels='lbl_msk', graph=True):
    """train_epoch of xBD_code/train_unettransformer.py:421-486 on the device.  batches: dicts {'img' fp32 [B, 6, H, W], 'msk' uint8
    [B, 5, H, W], 'lbl_msk' uint8 [B, H, W]} as GpuXbdPipeline.unet_batches yields them.  Per batch: forward, unet_loss, backward,
    NO gradient clip (commented out at line 480) and the hand-rolled AdamW -- with graph=True one replay of a GraphedXbdUnetStep
    (optimizer: AdamW(..., capturable=True)).  labels: unet_loss's ('lbl_msk': the script as executed; 'damage': its
    cross-entropy term as intended).  Every step's loss and parts go into a row of a device buffer by asynchronous device copies;
    the host reads ONCE, when the epoch is over, where the script reads four .item() values per step.  The meters are
    AverageMeter's means, weighted by the batch size: Loss, loss2 (channel 2) and loss3 (channel 3) as the script passes them,
    Dice.  Then scheduler.step(), and the script's final line
        epoch: ..; lr ..; Loss ..; loss2 ..; Dice ..
    IndexError if the epoch counted a label byte above 4 (torch raises it at that step), before the scheduler moves.
    Returns {'loss', 'loss2', 'loss3', 'dice', 'ce', 'lr', 'steps', 'samples'}.
    Deliberate differences: the printed lr is optimizer.param_groups[-1]['lr'], the rate the next epoch runs at -- the script's
    deprecated scheduler.get_lr() reports that rate times 0.6 once more at a milestone epoch; amp.autocast and GradScaler (fp16,
    a dynamic loss scale, skipped steps) are not reproduced: the net's compute_dtype decides the precision, nothing is scaled."""
    if labels not in ops.XBD_UNET_LABELS:
        raise ValueError("train_epoch_unet: labels %r is not one of %s" % (labels, sorted(ops.XBD_UNET_LABELS)))

    def no_bad_labels(host):
        bad = int(host[:, 8].sum())
        if bad:
            raise IndexError("train_epoch_unet: %d label bytes above 4 in epoch %s (steps %s); CrossEntropyLoss has 5 classes"
                             % (bad, current_epoch, np.nonzero(host[:, 8])[0].tolist()))
    return _train_epoch("train_epoch_unet", current_epoch, model, optimizer, scheduler, batches,
                        lambda first: _unet_train_step(model, optimizer, first, labels, graph), len(ops.XBD_UNET_PARTS),
                        (('loss', 0), ('loss2', 3), ('loss3', 4), ('dice', 7), ('ce', 6)), ('loss', 'loss2', 'dice'), no_bad_labels)


# ---- the adaptation script xBD_code/train_adapt.py: loss, step, epoch and validation of the FOUR-output net ---------------
def adapt_weights_dev(device, channel_weights=ADAPT_CHANNEL_WEIGHTS, ce_weights=ADAPT_CE_WEIGHTS):
    """the 4 channel weights and the 4 class weights as ONE cached device tensor [8], the form ops.xbd_adapt_loss_fwd takes (no
    host-to-device copy inside a HIP-graph capture).  ValueError unless both hold 4 numbers."""
    return _loss_weights_dev("adapt_loss", device, 4, channel_weights, ce_weights)


def adapt_loss(out, msks, want_parts=False, channel_weights=ADAPT_CHANNEL_WEIGHTS, ce_weights=ADAPT_CE_WEIGHTS, dice=1.0,
               focal=8.0, ce=ADAPT_CE_SCALE):
    """The loss of train_adapt.py:332-342 in one pass over the pixels (ops.xbd_adapt_loss_fwd; one more for the gradient):
        0.1 l0 + 0.8 l1 + 2 l2 + 8 l3 + 5 * CrossEntropyLoss(weight=[0.1, 0.5, 1.5, 1.5])(out, y)
    with l_c = ComboLoss{dice 1, focal 8}(out[:, c], msks[:, c]) and y = the first maximum of (1 - m0, m1, m2, m3) -- the
    script's msks[:, 0] = 1 - msks[:, 0]; argmax(msks, dim=1) -- derived inside the kernel from the mask bytes: msks is not
    written.  out: logits [B, 4, H, W]; msks: uint8 [B, 4, H, W] AS THE LOADER YIELDS THEM (make_adapt_batch; no float copy is
    made; another dtype is refused).  Unlike unet_loss the cross-entropy is taken of the raw logits, nothing is masked: it has
    a gradient on every pixel.  want_parts: also return the device tensor parts [6] = ops.XBD_ADAPT_PARTS: the four channel
    losses, the cross-entropy (before the factor 5), and 0.  No host synchronisation."""
    if not (torch.is_tensor(out) and out.is_cuda):
        raise _lib.HipLibraryError("dahitra_amd xBD loss runs on MI355X only (no CPU fallback)")
    w = adapt_weights_dev(out.device, channel_weights, ce_weights)
    loss, parts = _ScriptLoss.apply("adapt", out.float().contiguous(), msks.contiguous() if torch.is_tensor(msks) else msks, None,
                                    None, w, float(dice), float(focal), float(ce))
    return (loss, parts) if want_parts else loss


def adapt_scheduler(optimizer):
    """lr_scheduler.MultiStepLR(optimizer, milestones=[5, 11, 23, 29, 33, 47, 50, 60, ...], gamma=0.6) of train_adapt.py:423 --
    unet_scheduler's list without the 17"""
    return torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=list(ADAPT_MILESTONES), gamma=UNET_GAMMA)


def adapt_eager_step(model, optimizer, imgs, msks, max_norm=ADAPT_MAX_NORM, update=True):
    """The script's step through autograd (train_adapt.py:329-347): zero_grad, forward, adapt_loss, backward and -- with
    `update` -- clip_grad_norm_(max_norm) and optimizer.step().  Returns (logits, loss, parts), detached.  What
    train_epoch_adapt runs for a batch without a recorded step, and GraphedXbdAdaptStep's `_eager_body`."""
    model.zero_grad()
    logits = model(imgs)
    loss, parts = adapt_loss(logits, msks, want_parts=True)
    loss.backward()
    if update:
        clip_grad_norm_(model.parameters(), max_norm)
        optimizer.step()
    return logits.detach(), loss.detach(), parts


def _adapt_train_step(model, optimizer, first, graph):
    """_script_train_step of GraphedXbdAdaptStep, kept per shape, optimizer and device"""
    return _script_train_step('GraphedXbdAdaptStep', adapt_eager_step, '_xbd_adapt_steps', ('img', 'msk'), (), model, optimizer,
                              first, graph)


def train_epoch_adapt(current_epoch, model, optimizer, scheduler, batches, graph=True):
    """train_epoch of xBD_code/train_adapt.py:313-360 on the device.  batches: dicts {'img' fp32 [B, 6, H, W], 'msk' uint8
    [B, 4, H, W], ...} as GpuXbdPipeline.adapt_batches yields them.  Per batch: forward, adapt_loss, backward,
    clip_grad_norm_(0.999) and the hand-rolled AdamW -- with graph=True one replay of a GraphedXbdAdaptStep (optimizer:
    AdamW(..., capturable=True)).  Every step's loss and parts go into a row of a device buffer by asynchronous device copies;
    the host reads ONCE, when the epoch is over, where the script reads four .item() values per step.  The meters are
    AverageMeter's means, weighted by the batch size, as lines 349-352 feed them: Loss, loss1 (channel 1), loss2 (channel 2) and
    loss3 (channel 3, the script's `lossesgan`).  Then scheduler.step(), and the script's closing line 359 as printed -- its
    `loss2` is the meter of loss1 and its `Dice` the meter of loss3:
        epoch: ..; lr ..; Loss ..; loss2 ..; Dice ..
    Returns {'loss', 'loss1', 'loss2', 'loss3', 'loss0', 'ce', 'lr', 'steps', 'samples'}.
    Not reproduced: the per-step print(out.shape, msks.shape) of line 331 and the GradScaler of line 430, which the script
    never uses.  As in train_epoch_unet the scheduler moves by scheduler.step(), without the script's deprecated epoch argument
    (with `step(current_epoch)` a milestone takes effect one epoch later), and the printed lr is
    optimizer.param_groups[-1]['lr'], the rate the next epoch runs at."""
    return _train_epoch("train_epoch_adapt", current_epoch, model, optimizer, scheduler, batches,
                        lambda first: _adapt_train_step(model, optimizer, first, graph), len(ops.XBD_ADAPT_PARTS),
                        (('loss', 0), ('loss0', 1), ('loss1', 2), ('loss2', 3), ('loss3', 4), ('ce', 5)), ('loss', 'loss1', 'loss3'))


def validate_adapt(model, batches, thr=0.3, select='reference', graph=True, want_counts=False):
    """validate(model, data_loader, best_score) of xBD_code/train_adapt.py:248-294 on the device, for the four-output net.
    batches: dicts {'img' [B, 6, H, W] fp32, 'msk' [B, 4, H, W], 'lbl_msk' [B, H, W]} as GpuXbdPipeline.adapt_batches(b, size,
    train=False) yields them.  Everything is validate's -- one count kernel per batch (ops.xbd_val_count with classes=3), one
    host read per epoch, a recorded GraphedXbdEvalStep per shape, the same `select` -- with THREE damage classes:
    f1 = 3 / sum(1 / (f1_sc + 1e-6)), score = 0.3 d0 + 0.7 f1.  Prints the script's `Val Score: ... F1_2: ...` line and returns
    the score (with want_counts: score, parts, image_counts, class_counts [3, 3] as numpy integers).  The script's
    `best_score == 10000` branch ("Train Score" over a third of the loader) is not built."""
    image_counts, cc = _val_counts("validate_adapt", model, batches, thr, select, graph, 3)
    sc, parts = val_score(image_counts, cc, classes=3)
    f1_sc = parts['f1_per_class']
    print("Val Score: {}, Dice: {}, F1: {}, F1_0: {}, F1_1: {}, F1_2: {}".format(sc, parts['dice'], parts['f1'], f1_sc[0], f1_sc[1],
                                                                                f1_sc[2]))
    return (sc, parts, image_counts, cc) if want_counts else sc


def evaluate_val_adapt(batches, best_score, model, optimizer, path, current_epoch, thr=0.3, select='reference', graph=True):
    """evaluate_val of xBD_code/train_adapt.py:297-310: validate_adapt, and when the score beats `best_score` save the snapshot
    {'epoch': current_epoch + 1, 'state_dict', 'best_score', 'optimizer'} to `path`.  A nan score beats nothing.  Prints the
    `score: ... score_best: ...` line and returns the best score."""
    model = model.eval()
    d = validate_adapt(model, batches, thr=thr, select=select, graph=graph)
    return _keep_best(d, best_score, model, optimizer, path, current_epoch)


# ---- prediction (xBD_code/predict_test_cls.py:58-97) --------------------------------------------------------
def _one_model(model):
    """the script's `models` list has one entry (predict_test_cls.py:39); an ensemble of snapshots is not on the executed path"""
    if isinstance(model, (list, tuple)):
        if len(model) != 1:
            raise NotImplementedError("predict: the reference averages the flips of ONE snapshot (predict_test_cls.py:39); "
                                      "got a list of %d models" % len(model))
        model = model[0]
    return model


def _predict_step(model, pre_u8, post_u8, order):
    """the model's recorded prediction step for this shape, order and device (kept on the model, as _eval_step does)"""
    from ..graph import GraphedXbdPredictStep
    return _kept_step(model, '_xbd_predict_steps', (tuple(pre_u8.shape), order, str(pre_u8.device)),
                      lambda: GraphedXbdPredictStep(model, pre_u8, post_u8, order),
                      lambda step: step._generation == model._arena.generation)


def predict_tta(model, pre_u8, post_u8, order='bgr', graph=True):
    """The prediction of predict_test_cls.py:66-94 for a batch of pairs, on the device.  pre_u8, post_u8: [N, H, W, 3] uint8
    RGB as a decoder stores them.  The four flips of the normalised 6-channel image go through the eval-mode model as one
    batch of 4N; the sigmoids are flipped back, averaged in float32 in the reference's order and written as
    uint8(mean * 255).  Returns the device tensor [N, H, W, 5] uint8, channels last, what the script saves per pair.
    order: 'bgr' (default) is what the script executes: cv2.imread returns BGR, so the net sees each RGB triple reversed;
    'rgb' is the order train.py's PIL loader, and this project's loader, feed the net.  A model trained through this project
    has seen 'rgb'; the default stays with the script as written, the way validate's select='reference' does.
    graph=True replays a GraphedXbdPredictStep recorded once per model, shape, order and device, and the returned tensor is
    that step's static output: valid until the next call with this shape; graph=False runs the three stages eagerly into a new
    tensor.  Both give the same bytes.  `model` may be the script's one-element list `models`; another length raises
    NotImplementedError."""
    model = _one_model(model)
    if order not in ops.XBD_TTA_ORDER:
        raise ValueError("predict_tta: order %r is not one of %s" % (order, sorted(ops.XBD_TTA_ORDER)))
    _device_u8("prediction", pre_u8, post_u8)
    model.eval()
    if graph:
        model._ensure_arena(pre_u8.device)          # a rebuilt arena shows here, before a stale step could be chosen
        return _predict_step(model, pre_u8, post_u8, order).step(pre_u8, post_u8)
    inp = ops.xbd_tta_pack(pre_u8, post_u8, order)
    with torch.no_grad():
        logits = model(inp)
    return ops.xbd_tta_merge(logits.float().contiguous())


def predict_names(f):
    """The three file names predict_test_cls.py:95-97 writes for the pre image `f`, as written: '{0}.png'.format(f.replace(
    '.png', '_full.png')) and np.save's own '.npy' give a doubled extension,
        <stem>_full.png.png.npy, <stem>_part1.png.png, <stem>_part2.png.png
    (the xBD scoring and visualize_results.py look for exactly these)."""
    return ('{0}.png'.format(f.replace('.png', '_full.png')) + '.npy',
            '{0}.png'.format(f.replace('.png', '_part1.png')),
            '{0}.png'.format(f.replace('.png', '_part2.png')))


def predict_dir(model, test_dir, pred_folder, order='bgr', graph=True):
    """The loop of predict_test_cls.py:58-97: every name of sorted(listdir(test_dir)) that contains '_pre_' is paired with the
    name where '_pre_' is replaced by '_post_'; a pair whose two shapes differ is skipped; each pair is predicted by predict_tta
    and written to pred_folder (created) under predict_names(f):
        the .npy          the [H, W, 5] uint8 array
        the _part1 PNG    msk[..., :3]
        the _part2 PNG    msk[..., 2:]
    The images are decoded with PIL (RGB; order='bgr' hands the net what cv2.imread hands it in the script).  The PNGs are written
    so that cv2.imread(..., IMREAD_UNCHANGED) returns exactly those arrays: cv2 stores and returns BGR, so the PIL image is built
    from the channel-reversed slice.  PNG compression level 9; the pixel content is the contract, not the byte stream.
    Returns the list of the pre names whose files were written."""
    model = _one_model(model)
    device = next(model.parameters()).device
    if device.type != 'cuda':
        raise _lib.HipLibraryError("dahitra_amd xBD prediction runs on MI355X only (no CPU fallback): move the model to the GPU")
    return _predict_pairs(lambda pre, post: predict_tta(model, pre, post, order=order, graph=graph), device, test_dir, pred_folder)


def _predict_pairs(predict, device, test_dir, pred_folder, skip=None):
    """the directory loop of predict_dir and predict_dir_ensemble: predict(pre, post) -> [1, H, W, 5] uint8 for every pair of
    test_dir whose two shapes agree and for which skip(f, img) (if given; it prints its own line) is false, the three files of
    each written to pred_folder (created).  Returns the list of the pre names whose files were written."""
    from PIL import Image
    os.makedirs(pred_folder, exist_ok=True)
    written = []
    for f in sorted(os.listdir(test_dir)):
        if '_pre_' not in f:
            continue
        fn = os.path.join(test_dir, f)
        img = np.array(Image.open(fn).convert('RGB'))
        img2 = np.array(Image.open(fn.replace('_pre_', '_post_')).convert('RGB'))
        if img.shape != img2.shape or (skip is not None and skip(f, img)):
            continue
        pre, post = (torch.from_numpy(a).to(device).unsqueeze(0) for a in (img, img2))
        msk = predict(pre, post)[0].cpu().numpy()
        full, part1, part2 = predict_names(f)
        np.save(os.path.join(pred_folder, full), msk)
        for name, part in ((part1, msk[..., :3]), (part2, msk[..., 2:])):
            Image.fromarray(np.ascontiguousarray(part[..., ::-1])).save(os.path.join(pred_folder, name), format='PNG',
                                                                        compress_level=9)
        written.append(f)
    return written


# ---- prediction with several snapshots and 4 or 8 views (predict_test_cls.py:38-55, 81-91) -----------------------------------
def _ensemble(what, models):
    if not isinstance(models, (list, tuple)) or not 1 <= len(models) <= ops.XBD_TTA_MAX_MODELS:
        raise ValueError("%s: models is not a list of 1 .. %d nets (%s)" % (
            what, ops.XBD_TTA_MAX_MODELS, len(models) if isinstance(models, (list, tuple)) else type(models)))
    return list(models)


def _ensemble_step(models, pre_u8, post_u8, order, views):
    """the recorded step of this list of models, shape, order, views and device, kept on the first model (as _predict_step
    keeps one per model); rebuilt when any net's arena generation moved.  A kept step holds its nets, so their ids stay theirs."""
    from ..graph import GraphedXbdEnsembleStep
    key = (tuple(id(m) for m in models), tuple(pre_u8.shape), order, views, str(pre_u8.device))
    return _kept_step(models[0], '_xbd_ensemble_steps', key, lambda: GraphedXbdEnsembleStep(models, pre_u8, post_u8, order, views),
                      lambda step: not step.stale())


def predict_ensemble(models, pre_u8, post_u8, order='bgr', views=4, graph=True):
    """predict_tta for the script's list `models` with more than one snapshot in it, and for 4 or 8 views.  models: a list or
    tuple of 1 .. 8 nets on one device (the same net may appear twice); pre_u8, post_u8 [N, H, W, 3] uint8 as in predict_tta.
    The views of the normalised 6-channel image (ops.xbd_tta_pack_views: views=4 are the script's four flips, views=8 adds
    their transposes -- all eight symmetries of the square, what train_unettransformer.py:135-144 trains with -- and needs
    H == W) go through every eval-mode model as one batch of views * N; every model's sigmoids are brought back, and all
    M * views maps are averaged in float32 in the order `for model in models: pred.append(...)` stacks them and numpy's
    mean(axis=0) adds them, then written as uint8(mean * 255).  Returns the device tensor [N, H, W, 5] uint8, channels last.
    With one model and views=4 the bytes are predict_tta's.  (Averaging several predict_tta results is something else: each is
    already a byte.)
    graph=True replays one GraphedXbdEnsembleStep, kept on the first model and recorded once per list of models, shape, order,
    views and device; the returned tensor is that step's static output, valid until the next call with the same key.
    graph=False runs the stages eagerly into a new tensor.  Both give the same bytes.  ValueError for an empty or too long list,
    an unknown order, views outside {4, 8} or views=8 with H != W; CPU tensors raise HipLibraryError."""
    models = _ensemble("predict_ensemble", models)
    if order not in ops.XBD_TTA_ORDER:
        raise ValueError("predict_ensemble: order %r is not one of %s" % (order, sorted(ops.XBD_TTA_ORDER)))
    if isinstance(views, bool) or views not in ops.XBD_TTA_VIEWS:
        raise ValueError("predict_ensemble: views=%r is not one of %s" % (views, list(ops.XBD_TTA_VIEWS)))
    _device_u8("prediction", pre_u8, post_u8)
    if pre_u8.dim() != 4 or pre_u8.shape != post_u8.shape:
        raise ValueError("predict_ensemble: pre_u8 %s and post_u8 %s are not two [N, H, W, 3] tensors of one shape"
                         % (tuple(pre_u8.shape), tuple(post_u8.shape)))
    if views == 8 and pre_u8.shape[1] != pre_u8.shape[2]:
        raise ValueError("predict_ensemble: views=8 adds the transposes, which need a square image; got %dx%d"
                         % (pre_u8.shape[1], pre_u8.shape[2]))
    for m in models:
        m.eval()
    if graph:
        for m in models:
            m._ensure_arena(pre_u8.device)          # a rebuilt arena shows here, before a stale step could be chosen
        return _ensemble_step(models, pre_u8, post_u8, order, views).step(pre_u8, post_u8)
    inp = ops.xbd_tta_pack_views(pre_u8, post_u8, order, views)
    with torch.no_grad():
        logits = [m(inp).float().contiguous() for m in models]
    return ops.xbd_tta_merge_multi(logits, views)


def predict_dir_ensemble(models, test_dir, pred_folder, order='bgr', views=4, graph=True):
    """predict_dir with predict_ensemble in place of predict_tta: the same loop over sorted(listdir(test_dir)), the same skip of a
    pair whose two shapes differ, the same three files per pair under predict_names(f), written the same way.  With views=8 a
    pair whose image is not square cannot be transposed: it is skipped, and a line says so.  Returns the list of the pre names
    whose files were written."""
    models = _ensemble("predict_dir_ensemble", models)
    device = next(models[0].parameters()).device
    if device.type != 'cuda':
        raise _lib.HipLibraryError("dahitra_amd xBD prediction runs on MI355X only (no CPU fallback): move the models to the GPU")

    def not_square(f, img):
        if views == 8 and img.shape[0] != img.shape[1]:
            print("skipping {}: views=8 needs a square image, got {}x{}".format(f, img.shape[0], img.shape[1]))
            return True
        return False
    return _predict_pairs(lambda pre, post: predict_ensemble(models, pre, post, order=order, views=views, graph=graph), device,
                          test_dir, pred_folder, skip=not_square)


def load_snapshot(model, path):
    """Lines 43-53 of predict_test_cls.py for one snapshot: torch.load(path, map_location='cpu'), take ['state_dict'], copy every
    key the model has with the same size and leave the model's other tensors as they are, print the script's two lines.  The
    script loads into nn.DataParallel(model), whose keys carry a 'module.' prefix; here a snapshot's keys are accepted with or
    without it, so the snapshots evaluate_val and evaluate_val_sweep write load as well as the script's.  The caller moves the
    model to the device and calls eval(), as the script does next.  Returns (epoch, best_score)."""
    print("=> loading checkpoint '{}'".format(path))
    checkpoint = torch.load(path, map_location='cpu', weights_only=False)      # 'best_score' is a numpy scalar, 'optimizer' a dict
    loaded_dict = checkpoint['state_dict']
    sd = model.state_dict()
    for k in model.state_dict():
        for name in (k, 'module.' + k):
            if name in loaded_dict and sd[k].size() == loaded_dict[name].size():
                sd[k] = loaded_dict[name]
                break
    model.load_state_dict(sd)
    print("loaded checkpoint '{}' (epoch {}, best_score {})".format(path, checkpoint['epoch'], checkpoint['best_score']))
    return checkpoint['epoch'], checkpoint['best_score']


# ---- damage map and visual grid (xBD_code/visualize_results.py:171-223) ----------------------------------------------
def damage_map(msk_u8, loc=None):
    """The per-pixel damage class of visualize_results.py:206-211 from a prediction: msk_u8 [N, H, W, 5] uint8 (predict_tta's
    tensor) -> [N, H, W] uint8 on the device, 1 .. 4 = 1 + the first maximum of channels 1 .. 4.  loc=None (default) is the script
    as executed: no pixel is 0.  loc=(t0, t1, t2), or one float for all three, applies the script's three-threshold rule with
    p = msk_u8[..., 0] / 255 and sets the dropped pixels to 0 (ops.xbd_damage_map; ops.XBD_LOC_THR is the script's _thr).  The
    script reads p from a separate localisation net, which is not built here; channel 0 of the same prediction, the channel
    validate thresholds, stands in for it."""
    _device_u8("damage map", msk_u8)
    return ops.xbd_damage_map(msk_u8, loc)


def _check_labels(gt_u8):
    """the script's color_dict has the keys 0 .. 4: another label is its KeyError"""
    top = int(gt_u8.max()) if gt_u8.numel() else 0
    if top > 4:
        raise KeyError(top)


def visual_grid(model, pre_u8, post_u8, gt_u8, order='bgr', loc=None, graph=True):
    """The picture of visualize_results.py:176-220 for a batch of pairs, on the device: predict_tta(model, pre_u8, post_u8, order,
    graph), then ONE kernel that derives the damage class (damage_map's, with the same `loc`) and writes
        pre | post | colour(gt_u8) | colour(class)          [N, H, 4W, 3] uint8, RGB
    pre_u8, post_u8 [N, H, W, 3] uint8 RGB as a decoder stores them, gt_u8 [N, H, W] uint8 with the classes 0 .. 4.  The script's
    array is BGR (cv2): this one with the last axis reversed.  Returns a new device tensor.  A label above 4 raises KeyError, as
    the script's colour table does; CPU tensors are refused.  H and W are what the net takes: multiples of 64 (the decoder
    attention batches the 1/16-scale map of each image in rows of 16; ops.linear asserts on anything else)."""
    _device_u8("visual grid", pre_u8, post_u8, gt_u8)
    ops.xbd_loc_bounds(loc)                                 # a bad threshold shows before the forward runs
    _check_labels(gt_u8)
    msk = predict_tta(model, pre_u8, post_u8, order=order, graph=graph)
    return ops.xbd_vis_grid(pre_u8, post_u8, gt_u8, msk, loc)


def visual_name(f, model_str='TUNet'):
    """The file name visualize_results.py:222 gives the picture of the pre image `f`, as written: '_pre_' becomes '_vis' (no
    second underscore) and a '_part1.png' ending is folded to '.png',
        x_pre_disaster.png -> TUNet_x_visdisaster.png"""
    return model_str + "_" + f.replace('_pre_', '_vis').replace('_part1.png', '.png')


def visualize_dir(model, test_dir, mask_dir, out_dir, model_str='TUNet', crop=512, order='bgr', loc=None, files=None):
    """The loop of visualize_results.py:172-223: every name that contains '_pre_' is paired with the name where '_pre_' is
    replaced by '_post_' and with the ground truth mask_dir/<post name>; the three are decoded with PIL (RGB; the mask as its
    single channel), cut to [:crop, :crop] (crop=None: the whole tile), predicted and painted by visual_grid, and the
    [H, 4W, 3] picture is written to out_dir (created) as visual_name(f, model_str).  The cut tile goes through the net, so its
    sides must be multiples of 64 (see visual_grid): ValueError otherwise, before anything is predicted.
    The script iterates sorted(listdir(test_dir)[100:150]), a slice of an UNSORTED listing, which no two machines need agree on;
    here the default is every name of sorted(listdir(test_dir)), and `files` (any iterable of names) narrows it.
    The PNG is written with PIL from the RGB grid at compress level 9, so cv2.imread returns the array the script hands to
    cv2.imwrite (BGR).  The pixel content is the contract, not the byte stream.  ValueError if the three cropped shapes of a
    pair differ; KeyError for a label above 4.  Returns the list of the pre names whose pictures were written."""
    from PIL import Image
    model = _one_model(model)
    device = next(model.parameters()).device
    if device.type != 'cuda':
        raise _lib.HipLibraryError("dahitra_amd xBD visual grid runs on MI355X only (no CPU fallback): move the model to the GPU")
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for f in sorted(os.listdir(test_dir) if files is None else files):
        if '_pre_' not in f:
            continue
        post_name = f.replace('_pre_', '_post_')
        img = np.array(Image.open(os.path.join(test_dir, f)).convert('RGB'))[:crop, :crop]
        img2 = np.array(Image.open(os.path.join(test_dir, post_name)).convert('RGB'))[:crop, :crop]
        gt = np.array(Image.open(os.path.join(mask_dir, post_name)))
        if gt.ndim != 2 or gt.dtype != np.uint8:
            raise ValueError("visualize_dir: the mask %s is %s %s, expected one uint8 channel" % (post_name, gt.shape, gt.dtype))
        gt = gt[:crop, :crop]
        if not (img.shape == img2.shape == gt.shape + (3,)):
            raise ValueError("visualize_dir: %s: pre %s, post %s and mask %s differ after the crop"
                             % (f, img.shape, img2.shape, gt.shape))
        if gt.shape[0] % 64 or gt.shape[1] % 64:
            raise ValueError("visualize_dir: %s: the net takes tiles whose sides are multiples of 64, got %dx%d after crop=%r"
                             % (f, gt.shape[0], gt.shape[1], crop))
        pre, post, lab = (torch.from_numpy(np.ascontiguousarray(a)).to(device).unsqueeze(0) for a in (img, img2, gt))
        grid = visual_grid(model, pre, post, lab, order=order, loc=loc)[0].cpu().numpy()
        Image.fromarray(grid).save(os.path.join(out_dir, visual_name(f, model_str)), format='PNG', compress_level=9)
        written.append(f)
    return written


# ---- buildings: components, votes and the building-level score (no counterpart in the reference; csrc/xbd_buildings.hip) -----
def buildings(key_u8, connectivity=8, keyed=False):
    """Connected components of a class map on the device: key_u8 [N, H, W] uint8 -> (labels [N, H, W] int32, count [N] int32).
    Neighbouring pixels (connectivity 4 or 8) form one building when both are nonzero, with keyed=True when they are nonzero and
    equal (touching ground-truth buildings of different classes stay apart).  0 is the background; the buildings of each image
    are numbered 1 .. count[n] in raster order of their first pixel, scipy.ndimage.label's numbering (ops.xbd_cc_label)."""
    _device_u8("buildings", key_u8)
    return ops.xbd_cc_label(key_u8, connectivity, keyed)


class XbdBuildings:
    """What building_damage returns, all on the device: labels [N, H, W] int32, count [N] int32, table [N, max_buildings, 10]
    int32 (ops.xbd_cc_stats' rows: area, h0 .. h4, y0, x0, y1, x1), cls [N, max_buildings] uint8 and map [N, H, W] uint8, the
    map with one class per building.  rows(n) copies image n's buildings to the host."""

    def __init__(self, labels, count, table, cls, map, counts_host):
        self.labels, self.count, self.table, self.cls, self.map = labels, count, table, cls, map
        self._counts = counts_host

    def rows(self, n):
        """(table rows [count[n], 10] int32, classes [count[n]] uint8) of image n as numpy arrays"""
        k = int(self._counts[n])
        return self.table[n, :k].cpu().numpy(), self.cls[n, :k].cpu().numpy()


def _check_count(what, count, max_buildings):
    """the one read of `count`: ValueError when an image has more components than the table has rows"""
    counts = count.cpu().numpy()
    if counts.size and int(counts.max()) > max_buildings:
        raise ValueError("%s: an image has %d components, more than max_buildings=%d" % (what, int(counts.max()), max_buildings))
    return counts


def building_damage(msk_u8, loc=ops.XBD_LOC_THR, footprint=None, connectivity=8, min_area=0, max_buildings=4096):
    """One damage class per building from a prediction msk_u8 [N, H, W, 5] uint8 (predict_tta's tensor), on the device.
    The footprint is damage_map(msk_u8, loc) != 0, or the given [N, H, W] uint8 map (nonzero = building); its components
    (connectivity 4 or 8) are the buildings.  Every footprint pixel votes with damage_map(msk_u8, None), and a building's class
    is the first maximum of its votes for 1 .. 4; buildings of fewer than min_area pixels get class 0.  Returns an XbdBuildings.
    loc=None without a footprint is a ValueError (the whole tile would be one building), and so is an image with more than
    max_buildings components (count is read once, after the labelling)."""
    what = "building_damage"
    _device_u8("building damage", msk_u8, *(() if footprint is None else (footprint,)))
    if footprint is None and loc is None:
        raise ValueError("%s: loc=None without a footprint makes the whole tile one building" % what)
    ops._cc_cap(what, max_buildings)
    vote = ops.xbd_damage_map(msk_u8, None)
    if footprint is None:
        footprint = ops.xbd_damage_map(msk_u8, loc)
    elif not (footprint.dtype == torch.uint8 and tuple(footprint.shape) == tuple(vote.shape)):
        raise ValueError("%s: footprint %s %s is not uint8 %s like msk_u8" % (what, tuple(footprint.shape), footprint.dtype,
                                                                            list(vote.shape)))
    labels, count = ops.xbd_cc_label(footprint, connectivity, False)
    table = ops.xbd_cc_stats(labels, vote, max_buildings)
    cls = ops.xbd_cc_vote(table, min_area, "damage")
    painted = ops.xbd_cc_paint(labels, cls)
    counts = _check_count(what, count, max_buildings)
    return XbdBuildings(labels, count, table, cls, painted, counts)


# ---- cleaning the footprint: morphology and hole filling (no counterpart in the reference; csrc/xbd_morph.hip) --------------
def dilate(map_u8, k):
    """map_u8 [N, H, W] uint8 (nonzero = set) dilated by a k x k square (k odd, 1 .. 31), everything outside the image clear:
    [N, H, W] uint8, 0 / 1, on the device.  scipy.ndimage.binary_dilation(a, structure=ones((k, k))); one launch."""
    _device_u8("dilate", map_u8)
    return ops.xbd_morph(map_u8, "dilate", k)


def erode(map_u8, k):
    """map_u8 eroded by a k x k square, everything outside the image set (skimage's convention):
    scipy.ndimage.binary_erosion(a, structure=ones((k, k)), border_value=1); one launch."""
    _device_u8("erode", map_u8)
    return ops.xbd_morph(map_u8, "erode", k)


def opening(map_u8, k):
    """erode, then dilate, with the same k x k square: removes what the square does not fit into (specks, one-pixel bridges).
    Two launches."""
    _device_u8("opening", map_u8)
    return ops.xbd_morph(ops.xbd_morph(map_u8, "erode", k), "dilate", k)


def closing(map_u8, k):
    """dilate, then erode, with the same k x k square: closes gaps and pin-holes narrower than the square.  Two launches."""
    _device_u8("closing", map_u8)
    return ops.xbd_morph(ops.xbd_morph(map_u8, "dilate", k), "erode", k)


def fill_holes(map_u8, background=4):
    """map_u8 with its holes filled: the set pixels plus every component of the clear ones (connectivity `background`, 4 or 8)
    that does not touch the image border.  scipy.ndimage.binary_fill_holes with generate_binary_structure(2, 1) for 4 (its
    default) or (2, 2) for 8.  Nine launches whatever the data, no cap on the number of holes (ops.xbd_fill_holes)."""
    _device_u8("fill holes", map_u8)
    return ops.xbd_fill_holes(map_u8, background)


def clean_footprint(map_u8, open=0, close=0, fill=False, background=4, out=None, ws=None):
    """A footprint cleaned before its buildings are counted, on the device: map_u8 [N, H, W] uint8 (nonzero = building, e.g.
    damage_map(msk_u8, loc)) -> [N, H, W] uint8, 0 / 1.  The order is fixed:
        1. opening with square(open) if open > 0     specks and one-pixel bridges between neighbouring houses go
        2. closing with square(close) if close > 0   gaps narrower than the square close
        3. fill_holes(background) if fill            pin-holes inside roofs fill
    open, close: 0 or an odd window of 1 .. 31.  With open == close == 0 and not fill the result is (map_u8 != 0).  The result goes
    into building_damage(msk_u8, footprint=...), and through its .map into building_match.
    out: a [N, H, W] uint8 buffer for the result; ws: a uint8 device buffer of ops.xbd_fill_holes_ws_bytes(N, H, W) + 2 N H W
    bytes or more (the hole fill's workspace, then two maps for the intermediate results).  With both given nothing is
    allocated, so the call can be recorded in a graph."""
    what = "clean_footprint"
    _device_u8("footprint cleaning", map_u8)
    for name, k in (("open", open), ("close", close)):
        if isinstance(k, bool) or not isinstance(k, int) or k != 0:
            ops._morph_k("%s: %s" % (what, name), k)
    if isinstance(background, bool) or not isinstance(background, int) or background not in (4, 8):
        raise ValueError("%s: background connectivity %r is neither 4 nor 8" % (what, background))
    N, H, W = ops._cc_image(what, "map_u8", map_u8, torch.uint8)
    steps = [(op, k) for k, pair in ((open, ("erode", "dilate")), (close, ("dilate", "erode"))) if k for op in pair]
    fill_ws, tmp = None, [None, None]
    if ws is not None:
        need = ops.xbd_fill_holes_ws_bytes(N, H, W)
        if not torch.is_tensor(ws) or ws.dtype != torch.uint8 or ws.dim() != 1 or ws.numel() < need + 2 * N * H * W:
            raise ValueError("%s: ws is not a uint8 buffer of %d bytes or more" % (what, need + 2 * N * H * W))
        fill_ws = ws[:need]
        tmp = [ws[need + i * N * H * W:need + (i + 1) * N * H * W].view(N, H, W) for i in range(2)]
    if not steps and not fill:
        return ops.xbd_morph(map_u8, "dilate", 1, out=out)           # (map_u8 != 0) as 0 / 1
    cur = map_u8
    for i, (op, k) in enumerate(steps):
        last = i == len(steps) - 1 and not fill
        cur = ops.xbd_morph(cur, op, k, out=out if last else tmp[i % 2])
    if fill:
        cur = ops.xbd_fill_holes(cur, background, out=out, ws=fill_ws)
    return cur


def building_confusion(pred_map_u8, gt_u8, connectivity=8, max_buildings=4096):
    """The building-level confusion of a predicted class map against the ground truth, np.int64 [4, 5]: the ground-truth
    buildings are the keyed components of gt_u8 [N, H, W] uint8 (classes 0 .. 4; a label above 4 raises KeyError, as visual_grid
    does), each predicted as the first maximum of pred_map_u8's classes 0 .. 4 over its pixels (0: missed); [g - 1, p] counts the
    buildings of class g predicted p.  Confusions of batches add.  ValueError for an image with more than max_buildings
    ground-truth buildings."""
    what = "building_confusion"
    _device_u8("building confusion", pred_map_u8, gt_u8)
    ops._cc_cap(what, max_buildings)
    _check_labels(gt_u8)
    labels, count = ops.xbd_cc_label(gt_u8, connectivity, True)
    pred = ops.xbd_cc_vote(ops.xbd_cc_stats(labels, pred_map_u8, max_buildings), 0, "all")
    truth = ops.xbd_cc_vote(ops.xbd_cc_stats(labels, gt_u8, max_buildings), 0, "all")     # a keyed component has one class
    counts = _check_count(what, count, max_buildings)
    pred, truth = pred.cpu().numpy(), truth.cpu().numpy()
    conf = np.zeros((4, 5), dtype=np.int64)
    for n, k in enumerate(counts):
        np.add.at(conf, (truth[n, :k].astype(np.int64) - 1, pred[n, :k].astype(np.int64)), 1)
    return conf


def building_f1(confusion):
    """(the four per-class F1 values, their harmonic mean) of a building_confusion [4, 5], as val_score forms them: for class c,
    tp = [c - 1, c], fn = the rest of the row, fp = the rest of column c; f1_sc = 2 tp / (2 tp + fp + fn), nan for 0 / 0;
    f1 = 4 / sum(1 / (f1_sc + 1e-6))."""
    conf = np.asarray(confusion).astype(np.float64).reshape(4, 5)
    f1_sc = np.zeros((4,))
    with np.errstate(divide='ignore', invalid='ignore'):
        for c in range(1, 5):
            tp = conf[c - 1, c]
            fn = conf[c - 1].sum() - tp
            fp = conf[:, c].sum() - tp
            f1_sc[c - 1] = 2 * tp / (2 * tp + fp + fn)
        f1 = 4 / np.sum(1.0 / (f1_sc + 1e-6))
    return f1_sc, f1


class XbdMatch:
    """What building_match returns.  On the device: pred_labels / gt_labels [N, H, W] int32 and pred_count / gt_count [N] int32
    (the predicted and the true buildings), match_pred [N, max_buildings, 5] int32 and match_gt [N, max_buildings] int32
    (ops.xbd_cc_match's match_a and match_b), pred_cls and gt_cls [N, max_buildings] uint8.  On the host, np.int64 and additive
    over batches: loc [3] = tp, fp, fn buildings; confusion [4, 5], [g - 1, p] the true buildings of class g whose matched
    predicted building has class p (0: unmatched, or a partner of class 0); spurious [5], the unmatched predicted buildings by
    class."""

    def __init__(self, pred_labels, pred_count, gt_labels, gt_count, match_pred, match_gt, pred_cls, gt_cls, loc, confusion, spurious):
        self.pred_labels, self.pred_count, self.gt_labels, self.gt_count = pred_labels, pred_count, gt_labels, gt_count
        self.match_pred, self.match_gt, self.pred_cls, self.gt_cls = match_pred, match_gt, pred_cls, gt_cls
        self.loc, self.confusion, self.spurious = loc, confusion, spurious


def building_match(pred_map_u8, gt_u8, iou=(1, 2), connectivity=8, max_buildings=4096):
    """Predicted buildings matched one-to-one to the true ones at an intersection over union above iou = (num, den), on the
    device.  The predicted buildings are the components of pred_map_u8 != 0 ([N, H, W] uint8; building_damage(...).map drops the
    buildings under min_area first), each with the class its pixels vote for (first maximum of 1 .. 4); the true buildings are
    the keyed components of gt_u8 with their class, as in building_confusion.  A pair matches when inter * den > num * union
    (ops.xbd_cc_match: exact, strict, num / den >= 1 / 2, so no building has two partners).  Returns an XbdMatch.  The two counts
    are read once and the small tables copied once; no label map leaves the device.  A label above 4 raises KeyError, more than
    max_buildings components on either side ValueError."""
    what = "building_match"
    _device_u8("building match", pred_map_u8, gt_u8)
    ops._cc_cap(what, max_buildings)
    ops._cc_iou(what, iou)
    _check_labels(gt_u8)
    cap = max_buildings
    pred_labels, pred_count = ops.xbd_cc_label(pred_map_u8, connectivity, False)
    gt_labels, gt_count = ops.xbd_cc_label(gt_u8, connectivity, True)
    pred_cls = ops.xbd_cc_vote(ops.xbd_cc_stats(pred_labels, pred_map_u8, cap), 0, "damage")
    gt_cls = ops.xbd_cc_vote(ops.xbd_cc_stats(gt_labels, gt_u8, cap), 0, "all")               # a keyed component has one class
    match_pred, match_gt = ops.xbd_cc_match(pred_labels, gt_labels, cap, cap, iou)
    counts = _check_count(what, torch.stack((pred_count, gt_count)), cap)
    m_pred, m_gt = match_pred[:, :, 4].cpu().numpy(), match_gt.cpu().numpy()
    c_pred, c_gt = pred_cls.cpu().numpy().astype(np.int64), gt_cls.cpu().numpy().astype(np.int64)
    loc, conf, spur = np.zeros(3, dtype=np.int64), np.zeros((4, 5), dtype=np.int64), np.zeros(5, dtype=np.int64)
    for n in range(m_gt.shape[0]):
        ka, kb = int(counts[0, n]), int(counts[1, n])
        partner = m_gt[n, :kb]
        p = np.where(partner > 0, c_pred[n][np.maximum(partner, 1) - 1], 0)
        np.add.at(conf, (c_gt[n, :kb] - 1, p), 1)
        free = m_pred[n, :ka] == 0
        spur += np.bincount(c_pred[n, :ka][free], minlength=5)[:5]
        tp = int((partner > 0).sum())
        loc += (tp, int(free.sum()), kb - tp)
    return XbdMatch(pred_labels, pred_count, gt_labels, gt_count, match_pred, match_gt, pred_cls, gt_cls, loc, conf, spur)


def building_match_f1(loc, confusion, spurious):
    """(loc_f1, the four per-class F1 values, their harmonic mean) of building_match's three tables (summed over batches):
    loc_f1 = 2 tp / (2 tp + fp + fn) of the buildings; for class c, tp = confusion[c - 1, c], fn = the rest of the row,
    fp = the rest of column c + spurious[c]; f1_sc = 2 tp / (2 tp + fp + fn), nan for 0 / 0; f1 = 4 / sum(1 / (f1_sc + 1e-6)),
    as building_f1 and val_score form them."""
    tp, fp, fn = (float(v) for v in np.asarray(loc).reshape(3))
    conf = np.asarray(confusion).astype(np.float64).reshape(4, 5)
    spur = np.asarray(spurious).astype(np.float64).reshape(5)
    f1_sc = np.zeros((4,))
    with np.errstate(divide='ignore', invalid='ignore'):
        loc_f1 = np.float64(2 * tp) / np.float64(2 * tp + fp + fn)
        for c in range(1, 5):
            tp = conf[c - 1, c]
            fn = conf[c - 1].sum() - tp
            fp = conf[:, c].sum() - tp + spur[c]
            f1_sc[c - 1] = 2 * tp / (2 * tp + fp + fn)
        f1 = 4 / np.sum(1.0 / (f1_sc + 1e-6))
    return loc_f1, f1_sc, f1
