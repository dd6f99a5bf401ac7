#!/usr/bin/env python
"""Write tests/golden/xbd_adapt_loss.npz FROM THE REFERENCE's xBD_code/losses.py (needs the reference tree; no GPU): the loss of
xBD_code/train_adapt.py:332-342 on two small seeded cases, for tests/test_xbd_adapt_cpu.py and tests/test_xbd_adapt_gpu.py to hold
dahitra_amd's restatement and kernels to.  losses.py is loaded by path (it imports numpy and torch only), as
tools/make_unet_loss_golden.py does.  The composition is the script's: ComboLoss({'dice': 1, 'focal': 8}) on each of the four
channels, loss_seg = 0.1 l0 + 0.8 l1 + 2 l2 + 8 l3, then the in-place msks[:, 0] = 1 - msks[:, 0] on the long masks,
lbl_msk = argmax(msks, dim=1), loss_cls = nn.CrossEntropyLoss(weight=[0.1, 0.5, 1.5, 1.5])(out, lbl_msk) * 5 on the RAW logits, and
loss = loss_seg + loss_cls.  Everything is evaluated in float32 AND in float64 on the CPU: the distance between the two is the
yardstick the GPU tests measure the kernels with.

Cases (2 x 4 x 15 x 17, H * W odd), logits with +25 and -25 patches so that both clamps of FocalLoss2d are hit:
    train    TrainData's masks: m1, m2, m3 cut from one label byte (4 merged into 3), m0 their union
    val      ValData-style masks: m0 drawn on its own, so it is set on pixels without a damage plane (the label is 0 there: all
             four of (1 - m0, m1, m2, m3) are 0 and the first wins) and clear on pixels with one (0 again: 1 - m0 comes first)

    python tools/make_adapt_loss_golden.py [--reference DIR]       # DIR defaults to $DAHITRA_REFERENCE

Arrays per case <name>: <name>_logits fp32, <name>_msk uint8, <name>_lbl uint8 (the label the script derived) and, for p in
(32, 64): <name>_loss<p>, <name>_channel<p> [4], <name>_ce<p>, <name>_grad<p> (d loss / d logits)."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (2, 15, 17)
CHANNEL_WEIGHTS = (0.1, 0.8, 2, 8)                   # train_adapt.py:336
CE_WEIGHTS = (0.1, 0.5, 1.5, 1.5)                    # ... :320
CE_SCALE = 5                                         # ... :340


def inputs(seed, val):
    B, H, W = SHAPE
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, 4, H, W, generator=g) * 3
    logits[0, 1, :3] = 25.0              # the sigmoid saturates: both clamps of FocalLoss2d are hit
    logits[1, 2, :3] = -25.0
    logits[1, 0, 5:7] = 25.0
    lab = torch.randint(0, 5, (B, H, W), generator=g)
    msk = torch.zeros(B, 4, H, W, dtype=torch.uint8)
    msk[:, 1] = (lab == 1).to(torch.uint8)
    msk[:, 2] = (lab == 2).to(torch.uint8)
    msk[:, 3] = ((lab == 3) | (lab == 4)).to(torch.uint8)
    if val:
        msk[:, 0] = (torch.rand(B, H, W, generator=g) > 0.4).to(torch.uint8)          # the pre-disaster mask, on its own
    else:
        msk[:, 0] = msk[:, 1:].amax(1)
    return logits, msk


def evaluate(L, logits, msk, dtype):
    seg_loss = L.ComboLoss({'dice': 1, 'focal': 8}, per_image=False)
    ce_loss = torch.nn.CrossEntropyLoss(weight=torch.tensor(CE_WEIGHTS, dtype=dtype))
    x = logits.detach().clone().to(dtype).requires_grad_(True)
    out = x * 1.0
    msks = msk.long()
    loss0 = seg_loss(out[:, 0, ...], msks[:, 0, ...])
    loss1 = seg_loss(out[:, 1, ...], msks[:, 1, ...])
    loss2 = seg_loss(out[:, 2, ...], msks[:, 2, ...])
    loss3 = seg_loss(out[:, 3, ...], msks[:, 3, ...])
    loss_seg = 0.1 * loss0 + 0.8 * loss1 + 2 * loss2 + 8 * loss3
    msks[:, 0, ...] = 1 - msks[:, 0, ...]
    lbl_msk = torch.argmax(msks, dim=1)
    ce = ce_loss(out, lbl_msk)
    loss_cls = ce * CE_SCALE
    loss = loss_seg + loss_cls
    loss.backward()
    np_dtype = np.float32 if dtype == torch.float32 else np.float64
    return {"loss": np.asarray(loss.item(), dtype=np_dtype),
            "channel": np.array([l.item() for l in (loss0, loss1, loss2, loss3)], dtype=np_dtype),
            "ce": np.asarray(ce.item(), dtype=np_dtype), "grad": x.grad.numpy().astype(np_dtype)}, lbl_msk.numpy().astype(np.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", default=os.environ.get("DAHITRA_REFERENCE"), help="the reference tree (holds xBD_code/losses.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "xbd_adapt_loss.npz"))
    args = ap.parse_args()
    if not args.reference or not os.path.exists(os.path.join(args.reference, "xBD_code", "losses.py")):
        sys.exit("no xBD_code/losses.py under --reference / $DAHITRA_REFERENCE (%r)" % args.reference)
    spec = importlib.util.spec_from_file_location("_reference_xbd_losses", os.path.join(args.reference, "xBD_code", "losses.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)
    torch.set_num_threads(1)              # one summation order for the float32 sums, whatever the machine

    data = {"torch_version": np.array(torch.__version__)}
    for name, seed in (("train", 31), ("val", 32)):
        logits, msk = inputs(seed, name == "val")
        data.update({name + "_logits": logits.numpy(), name + "_msk": msk.numpy()})
        res = {}
        for p, dtype in ((32, torch.float32), (64, torch.float64)):
            res[p], lbl = evaluate(L, logits, msk, dtype)
            data.update({"%s_%s%d" % (name, k, p): v for k, v in res[p].items()})
        data[name + "_lbl"] = lbl
        rel = lambda k: float(np.max(np.abs(res[32][k].astype(np.float64) - res[64][k]) / np.abs(res[64][k])))
        g64 = res[64]["grad"]
        print("%s: float32 against float64: loss %.3e, channel %.3e, ce %.3e (relative); gradient %.3e of its maximum %.3e; "
              "labels %s" % (name, rel("loss"), rel("channel"), rel("ce"),
                             float(np.abs(res[32]["grad"].astype(np.float64) - g64).max() / np.abs(g64).max()),
                             float(np.abs(g64).max()), np.bincount(lbl.reshape(-1), minlength=4).tolist()))
    for v in data.values():
        assert v.dtype != object
    np.savez_compressed(args.out, **data)
    print("%s: %d arrays, %d bytes" % (args.out, len(data), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
