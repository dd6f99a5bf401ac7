#!/usr/bin/env python
"""Write tests/golden/xbd_unet_loss.npz FROM THE REFERENCE's xBD_code/losses.py (needs the reference tree; no GPU): the loss of
xBD_code/train_unettransformer.py:438-461 on two small seeded cases, for tests/test_xbd_unet_step_cpu.py and
tests/test_xbd_unet_step_gpu.py to hold dahitra_amd's restatement and kernels to.  losses.py is loaded by path (it imports numpy
and torch only).  The composition is the script's: ComboLoss({'dice': 1, 'focal': 8}) on each of the five channels, the in-place
`out[:, c] = out[:, c] * (lbl_msk > 0)` on a NON-LEAF copy of the logits, nn.CrossEntropyLoss(weight=[0.01, 0.10, 1, 0.80, 1]) of
the masked logits, loss = 0.1 l0 + 0.1 l1 + 0.6 l2 + 0.3 l3 + 1 l4 + 8 l5, and the Dice meter 1 - soft_dice_loss(sigmoid(out[:, 0]),
msks[:, 0]) read AFTER the masking (the script goes through dice_round, which only adds a `.float()` of the probabilities; it is
left out so that the float64 evaluation stays float64).  Everything is evaluated in float32 AND in float64 on the CPU: the
distance between the two is the yardstick the GPU tests measure the kernels with.

Cases (2 x 5 x 15 x 17, H * W odd), logits with +25 and -25 patches so that both clamps of FocalLoss2d are hit:
    zero     lbl_msk all zero -- the script as executed (its TrainData's argmax is 0 at every pixel)
    damage   lbl_msk = the first set channel among 1 .. 4 of msk, 0 where none is set; a few pixels carry two damage channels

    python tools/make_unet_loss_golden.py [--reference DIR]       # DIR defaults to $DAHITRA_REFERENCE

Arrays per case <name>: <name>_logits fp32, <name>_msk uint8, <name>_lbl uint8 and, for p in (32, 64): <name>_loss<p>, <name>_channel<p>
[5], <name>_ce<p>, <name>_dice<p>, <name>_grad<p> (d loss / d logits)."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (2, 15, 17)
CHANNEL_WEIGHTS = (0.1, 0.1, 0.6, 0.3, 1.0)          # train_unettransformer.py:456
CE_WEIGHTS = (0.01, 0.10, 1.0, 0.80, 1.0)            # ... :563
CE_SCALE = 8.0


def inputs(seed):
    B, H, W = SHAPE
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, 5, H, W, generator=g) * 3
    logits[0, 1, :3] = 25.0              # the sigmoid saturates: both clamps of FocalLoss2d are hit
    logits[1, 2, :3] = -25.0
    logits[1, 0, 5:7] = 25.0
    lab = torch.randint(0, 5, (B, H, W), generator=g)
    msk = torch.zeros(B, 5, H, W, dtype=torch.uint8)
    for c in range(1, 5):
        msk[:, c] = (lab == c).to(torch.uint8)
    msk[0, 3, 4, :6] = 1                 # two damage channels on one pixel: the first one is the label
    msk[:, 0] = msk[:, 1:].amax(1)
    return logits, msk


def damage_label(msk):
    m = msk.numpy()[:, 1:]
    return torch.from_numpy(np.where(m.any(1), m.argmax(1) + 1, 0).astype(np.uint8))


def evaluate(L, logits, msk, lbl, dtype):
    seg_loss = L.ComboLoss({'dice': 1, 'focal': 8}, per_image=False)
    ce_loss = torch.nn.CrossEntropyLoss(weight=torch.tensor(CE_WEIGHTS, dtype=dtype))
    x = logits.detach().clone().to(dtype).requires_grad_(True)
    out = x * 1.0                         # the model's output is no leaf: the script writes into it in place
    msks, lbl_msk = msk.long(), lbl.long()
    ch = [seg_loss(out[:, c, ...], msks[:, c, ...]) for c in range(5)]
    bldg_mask = (lbl_msk > 0)
    for c in range(5):
        out[:, c, ...] = torch.mul(out[:, c, ...], bldg_mask)
    loss5 = ce_loss(out, lbl_msk)
    loss = sum(w * l for w, l in zip(CHANNEL_WEIGHTS, ch)) + loss5 * CE_SCALE
    with torch.no_grad():
        dice_sc = 1 - L.soft_dice_loss(torch.sigmoid(out[:, 0, ...]), msks[:, 0, ...])
    loss.backward()
    np_dtype = np.float32 if dtype == torch.float32 else np.float64
    return {"loss": np.asarray(loss.item(), dtype=np_dtype), "channel": np.array([l.item() for l in ch], dtype=np_dtype),
            "ce": np.asarray(loss5.item(), dtype=np_dtype), "dice": np.asarray(dice_sc.item(), dtype=np_dtype),
            "grad": x.grad.numpy().astype(np_dtype)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", default=os.environ.get("DAHITRA_REFERENCE"), help="the reference tree (holds xBD_code/losses.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "xbd_unet_loss.npz"))
    args = ap.parse_args()
    if not args.reference or not os.path.exists(os.path.join(args.reference, "xBD_code", "losses.py")):
        sys.exit("no xBD_code/losses.py under --reference / $DAHITRA_REFERENCE (%r)" % args.reference)
    spec = importlib.util.spec_from_file_location("_reference_xbd_losses", os.path.join(args.reference, "xBD_code", "losses.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)
    torch.set_num_threads(1)              # one summation order for the float32 sums, whatever the machine

    data = {"torch_version": np.array(torch.__version__)}
    for name, seed in (("zero", 21), ("damage", 22)):
        logits, msk = inputs(seed)
        lbl = torch.zeros(SHAPE, dtype=torch.uint8) if name == "zero" else damage_label(msk)
        data.update({name + "_logits": logits.numpy(), name + "_msk": msk.numpy(), name + "_lbl": lbl.numpy()})
        res = {}
        for p, dtype in ((32, torch.float32), (64, torch.float64)):
            res[p] = evaluate(L, logits, msk, lbl, dtype)
            data.update({"%s_%s%d" % (name, k, p): v for k, v in res[p].items()})
        rel = lambda k: float(np.max(np.abs(res[32][k].astype(np.float64) - res[64][k]) / np.abs(res[64][k])))
        g64 = res[64]["grad"]
        print("%s: float32 against float64: loss %.3e, channel %.3e, ce %.3e, dice %.3e (relative); gradient %.3e of its maximum %.3e"
              % (name, rel("loss"), rel("channel"), rel("ce"), rel("dice"),
                 float(np.abs(res[32]["grad"].astype(np.float64) - g64).max() / np.abs(g64).max()), float(np.abs(g64).max())))
    for v in data.values():
        assert v.dtype != object
    np.savez_compressed(args.out, **data)
    print("%s: %d arrays, %d bytes" % (args.out, len(data), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
