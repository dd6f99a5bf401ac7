#!/usr/bin/env python3
"""What the step of xBD_code/train_unettransformer.py costs beside train.py's, on one MI355X in one call.  A report, not a gate.

1. The loss launches on one batch (`--batch` x 5 x `--size` x `--size` logits, the loader's uint8 masks), alternating over `--rounds`:

    unet_lbl      xbd_unet_loss_fwd + xbd_unet_loss_bwd, labels='lbl_msk' (three launches; the masks are read as bytes)
    unet_damage   the same with labels='damage' (the label derived in the kernel, no label plane read)
    parent        what GraphedXbdStep._loss_and_grad records: msk.float(), combo_loss_fwd, combo_loss_bwd (four launches)
    parent_float  combo_loss_fwd + combo_loss_bwd on masks that are float already (train.py's own loader hands over such masks)

2. Pairs/s of the recorded steps on the xBD net without decoder position (`--dtype`, batch and size as above): GraphedXbdUnetStep
   (both label modes) against GraphedXbdStep fed the same uint8 masks; `--steps` replays per window, alternating over `--rounds`.

    python tools/unet_step_rate.py [--batch 16] [--size 256] [--dtype bf16] [--rounds 7] [--window-ms 200] [--steps 30] [--no-step]

Device events around the windows after a warm-up; medians.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dahitra_amd import ops  # noqa: E402
from dahitra_amd.models import xbd  # noqa: E402


def window(f, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)                                  # ms


def spread(v, digits=2):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32", "bf16x3"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=200.0, help="least length of a timed window of loss launches")
    ap.add_argument("--steps", type=int, default=30, help="replays per timed window of a recorded step")
    ap.add_argument("--no-step", action="store_true", help="time the loss launches only")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("unet_step_rate: no GPU; a time is measured on the MI355X or not at all")
    dev, B, S = "cuda", args.batch, args.size
    g = torch.Generator().manual_seed(args.seed)
    logits = (torch.randn(B, 5, S, S, generator=g) * 3).to(dev)
    r = torch.rand(B, S, S, generator=g)
    lab = torch.where(r < 0.85, torch.zeros_like(r), 1 + torch.floor((r - 0.85) / 0.15 * 4).clamp_(max=3)).long()
    msk = torch.stack([(lab > 0)] + [(lab == c) for c in range(1, 5)], 1).to(torch.uint8).to(dev)
    lbl = torch.zeros(B, S, S, dtype=torch.uint8, device=dev)
    msk_f = msk.float()
    w_unet, w_parent = xbd.unet_weights_dev(dev), xbd.channel_weights_dev(dev)
    one = torch.ones(1, dtype=torch.float32, device=dev)

    def unet(labels):
        def f():
            _, _, sums = ops.xbd_unet_loss_fwd(logits, msk, lbl, labels, w_unet, 1.0, 8.0, 8.0)
            ops.xbd_unet_loss_bwd(logits, msk, lbl, labels, sums, w_unet, None, 1.0, 8.0, 8.0)
        return f

    def parent(masks):
        def f():
            ms = masks.float().contiguous()                   # a new tensor for bytes, the same tensor for floats
            _, _, sums = ops.combo_loss_fwd(logits, ms, w_parent, 1.0, 8.0)
            ops.combo_loss_bwd(logits, ms, sums, w_parent, one, 1.0, 8.0)
        return f

    variants = {"unet_lbl": unet("lbl_msk"), "unet_damage": unet("damage"), "parent": parent(msk), "parent_float": parent(msk_f)}
    reps = {}
    for name, f in variants.items():                         # warm-up, then as many repetitions as fill a window
        window(f, 10)
        reps[name] = max(10, int(args.window_ms / max(window(f, 50) / 50, 1e-3)) + 1)
    t = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, f in variants.items():
            t[name].append(window(f, reps[name]) * 1e3 / reps[name])
    us = {name: spread(v) for name, v in t.items()}
    px = B * S * S
    out = {"batch": B, "size": S, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "loss": {"what": "us per batch for the loss and its gradient; parent includes the uint8-to-float conversion of the masks",
                    "us": us, "bytes_unet_lbl": px * (2 * 25 + 2 + 20), "bytes_parent": px * (5 + 20 + 2 * 40 + 20),
                    "unet_lbl_over_parent": round(us["unet_lbl"]["median"] / us["parent"]["median"], 3),
                    "unet_lbl_over_parent_float": round(us["unet_lbl"]["median"] / us["parent_float"]["median"], 3)}}

    if not args.no_step:
        from dahitra_amd.graph import GraphedXbdStep, GraphedXbdUnetStep
        x6 = torch.randn(B, 6, S, S, generator=g).clamp_(-1, 1).to(dev)

        def build(kind):
            torch.manual_seed(args.seed)
            net = xbd.BASE_Transformer_UNet(with_decoder_pos=None, compute_dtype=args.dtype).to(dev).train()
            opt = xbd.AdamW(net.parameters(), lr=1e-4, weight_decay=1e-6, capturable=True)
            if kind == "parent":
                return GraphedXbdStep(net, opt, x6, msk)
            return GraphedXbdUnetStep(net, opt, x6, msk, lbl, labels=kind)
        steps = {kind: build(kind) for kind in ("parent", "lbl_msk", "damage")}
        for s in steps.values():
            window(s, 5)
        rate = {kind: [] for kind in steps}
        for _ in range(args.rounds):
            for kind, s in steps.items():
                rate[kind].append(B * args.steps / (window(s, args.steps) * 1e-3))
        pairs = {kind: spread(v, 1) for kind, v in rate.items()}
        out["step"] = {"what": "image pairs/s of the recorded step, replayed on its static inputs; parent = GraphedXbdStep with the "
                               "same uint8 masks (train.py's weights, clip_grad_norm_)", "net": "xbd_unet_transformer_nodecpos",
                       "dtype": args.dtype, "steps_per_window": args.steps, "pairs_per_s": pairs,
                       "ms_per_step": {k: round(B / v["median"] * 1e3, 3) for k, v in pairs.items()},
                       "lbl_msk_over_parent": round(pairs["lbl_msk"]["median"] / pairs["parent"]["median"], 4),
                       "damage_over_parent": round(pairs["damage"]["median"] / pairs["parent"]["median"], 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
