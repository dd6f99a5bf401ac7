#!/usr/bin/env python3
"""Time of the Lovasz hinge (csrc/xbd_seg_losses.hip, ops.xbd_lovasz: loss AND gradient in one call) at the xBD step's sizes:

    python tools/lovasz_bench.py [--reps 10] [--rounds 7] [--window-ms 30]

    shapes     16 x 1 x 256 x 256, 16 x 5 x 256 x 256, 1 x 5 x 1024 x 1024, per_image 0 and 1, uint8 targets
    lovasz_us  one ops.xbd_lovasz call (mode 'hinge'): every launch from the keys to the finalize
    copy_us    a device copy_ of the bytes the call must touch at the least: the logits read and the gradient written (fp32 each)
               and the targets read
    torch_us   the same loss AND its gradient written with torch ops on the device: per segment 1 - x (2 t - 1),
               torch.sort(descending=True), a gather of the labels, cumsum, the differences of 1 - I / U, relu and dot, then
               autograd's backward -- what the reference's ten lines do under PyTorch-ROCm (nothing ignored: the masks hold 0 / 1)
    combo_us   for scale: ops.combo_loss_fwd + ops.combo_loss_bwd on the same tensors, the loss of the recorded xBD step

A timed window is `reps` calls or more -- as many as last `window-ms` -- between two device events, after a warm-up; `rounds`
windows per operation, the operations alternating; median, min and max are printed.  The two losses are compared before
anything is timed.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dahitra_amd import ops  # noqa: E402

SHAPES = ((16, 1, 256, 256), (16, 5, 256, 256), (1, 5, 1024, 1024))


def torch_lovasz(x, t, per_image):
    """sum over the channels of lovasz_hinge (mean over the images with per_image), and d / dx, in torch ops"""
    x = x.detach().requires_grad_(True)
    B, C = x.shape[:2]
    total = 0
    for c in range(C):
        groups = [(x[b, c].reshape(-1), t[b, c].reshape(-1)) for b in range(B)] if per_image else [(x[:, c].reshape(-1), t[:, c].reshape(-1))]
        for xs, ts in groups:
            lab = ts.float()
            errors = 1. - xs * (2. * lab - 1.)
            errors_sorted, perm = torch.sort(errors, dim=0, descending=True)
            gt = lab[perm]
            gts = gt.sum()
            jac = 1. - (gts - gt.cumsum(0)) / (gts + (1 - gt).cumsum(0))
            jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
            total = total + torch.dot(torch.relu(errors_sorted), jac) / len(groups)
    total.backward()
    return total.detach(), x.grad


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps                          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10, help="least calls per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=30.0, help="least length of a timed window (more calls are added)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lovasz_bench: no GPU; a time is measured on the MI355X or not at all")
    dev = "cuda"
    rows = {}
    for shape in SHAPES:
        g = torch.Generator(device=dev).manual_seed(7)
        x = torch.randn(shape, generator=g, device=dev) * 3
        t = (torch.rand(shape, generator=g, device=dev) < 0.3).to(torch.uint8)
        tf = t.float()
        ones = torch.ones(shape[1], device=dev)
        src = torch.empty(2 * x.numel() * 4 + t.numel(), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        for per_image in (0, 1):
            def combo():
                _, _, sums = ops.combo_loss_fwd(x, tf, ones, 1.0, 8.0)
                ops.combo_loss_bwd(x, tf, sums, ones, None, 1.0, 8.0)
            ops_ = {"lovasz": lambda: ops.xbd_lovasz(x, t, "hinge", bool(per_image), None),
                    "copy": lambda: dst.copy_(src),
                    "torch": lambda: torch_lovasz(x, t, bool(per_image)),
                    "combo": combo}
            for fn in ops_.values():                                # warm-up
                for _ in range(2):
                    fn()
            torch.cuda.synchronize()
            ours, _, dx = ops.xbd_lovasz(x, t, "hinge", bool(per_image), None)
            theirs, dxt = torch_lovasz(x, t, bool(per_image))
            reps = {k: max(args.reps, int(args.window_ms * 1e3 / max(window(fn, args.reps), 1e-3)) + 1) for k, fn in ops_.items()}
            tm = {k: [] for k in ops_}
            for _ in range(args.rounds):
                for k, fn in ops_.items():
                    tm[k].append(window(fn, reps[k]))
            stat = lambda k: {"median": round(statistics.median(tm[k]), 1), "min": round(min(tm[k]), 1), "max": round(max(tm[k]), 1)}
            lv, cp, to, co = stat("lovasz"), stat("copy"), stat("torch"), stat("combo")
            rows["%s per_image=%d" % ("x".join(map(str, shape)), per_image)] = {
                "elements": x.numel(), "bytes_touched": src.numel(), "calls_per_window": reps, "lovasz_us": lv, "copy_us": cp,
                "torch_us": to, "combo_us": co, "lovasz_over_copy": round(lv["median"] / cp["median"], 2),
                "torch_over_lovasz": round(to["median"] / lv["median"], 2), "lovasz_over_combo": round(lv["median"] / co["median"], 2),
                "loss": float(ours), "torch_loss": float(theirs),
                "torch_grad_off_by": float((dxt - dx).abs().max() / dx.abs().max())}
    print(json.dumps({"rounds": args.rounds, "window_ms": args.window_ms, "device": torch.cuda.get_device_name(0),
                      "what": "us per call between two device events; lovasz and torch: loss and gradient; combo: dice + focal "
                              "forward and backward; torch_grad_off_by: the torch gradient's distance from the kernel's, as a "
                              "share of the largest element", "shapes": rows}))


if __name__ == "__main__":
    main()
