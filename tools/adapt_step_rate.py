#!/usr/bin/env python3
"""What the step of xBD_code/train_adapt.py costs on one MI355X, at the script's own shape (`--batch` 1 x 1024 x 1024), in one call.
A report, not a gate.

1. The loss launches on one batch (`--batch` x 4 x `--size` x `--size` logits, the loader's uint8 masks), alternating over `--rounds`:

    adapt         xbd_adapt_loss_fwd + xbd_adapt_loss_bwd (three launches; the masks are read as bytes, the label derived in place)
    unet_damage   xbd_unet_loss_fwd + _bwd, labels='damage', on the five-channel counterpart of the same batch, for scale

2. The batch launch (GpuXbdPipeline.make_adapt_batch from `--sources` resident tiles, whole-tile crop; and ops.xbd_adapt_batch alone,
   without the index upload) against a device-to-device copy of exactly its output bytes (24 + 4 + 1 per pixel), the floor of any
   kernel that writes them.

3. Pairs/s of the recorded steps (`--dtype`): GraphedXbdAdaptStep on the four-output net with decoder position -- the script's net --
   and, beside it for scale, GraphedXbdStep on the five-output net at the same shape, in the same process; `--steps` replays per
   window, alternating over `--rounds`.

    python tools/adapt_step_rate.py [--batch 1] [--size 1024] [--dtype bf16] [--rounds 7] [--window-ms 200] [--steps 20] [--no-step]

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


def timed(variants, rounds, window_ms):
    """us per call of every variant: warm-up, as many repetitions as fill a window, `rounds` windows each, alternating"""
    reps = {}
    for name, f in variants.items():
        window(f, 10)
        reps[name] = max(10, int(window_ms / max(window(f, 50) / 50, 1e-3)) + 1)
    t = {name: [] for name in variants}
    for _ in range(rounds):
        for name, f in variants.items():
            t[name].append(window(f, reps[name]) * 1e3 / reps[name])
    return {name: spread(v) for name, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32", "bf16x3"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=200.0, help="least length of a timed window of launches")
    ap.add_argument("--steps", type=int, default=20, help="replays per timed window of a recorded step")
    ap.add_argument("--sources", type=int, default=4, help="resident tiles of the pipeline the batch launch reads")
    ap.add_argument("--no-step", action="store_true", help="time the loss and batch launches only")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adapt_step_rate: no GPU; a time is measured on the MI355X or not at all")
    dev, B, S = "cuda", args.batch, args.size
    g = torch.Generator().manual_seed(args.seed)
    r = torch.rand(B, S, S, generator=g)
    lab = torch.where(r < 0.85, torch.zeros_like(r), 1 + torch.floor((r - 0.85) / 0.15 * 4).clamp_(max=3)).long()
    m1, m2, m3 = lab == 1, lab == 2, (lab == 3) | (lab == 4)
    msk4 = torch.stack([m1 | m2 | m3, m1, m2, m3], 1).to(torch.uint8).to(dev)
    msk5 = torch.stack([(lab > 0)] + [(lab == c) for c in range(1, 5)], 1).to(torch.uint8).to(dev)
    logits5 = (torch.randn(B, 5, S, S, generator=g) * 3).to(dev)
    logits4 = logits5[:, :4].contiguous()
    w_adapt, w_unet = xbd.adapt_weights_dev(dev), xbd.unet_weights_dev(dev)

    def adapt():
        _, _, sums = ops.xbd_adapt_loss_fwd(logits4, msk4, w_adapt, 1.0, 8.0, 5.0)
        ops.xbd_adapt_loss_bwd(logits4, msk4, sums, w_adapt, None, 1.0, 8.0, 5.0)

    def unet_damage():
        _, _, sums = ops.xbd_unet_loss_fwd(logits5, msk5, None, "damage", w_unet, 1.0, 8.0, 8.0)
        ops.xbd_unet_loss_bwd(logits5, msk5, None, "damage", sums, w_unet, None, 1.0, 8.0, 8.0)

    px = B * S * S
    us = timed({"adapt": adapt, "unet_damage": unet_damage}, args.rounds, args.window_ms)
    out = {"batch": B, "size": S, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "loss": {"what": "us per batch for the loss and its gradient (three launches)", "us": us,
                    "bytes_adapt": px * (2 * 20 + 16), "GBps_adapt": round(px * (2 * 20 + 16) / us["adapt"]["median"] * 1e-3, 1)}}

    from dahitra_amd.datasets.xbd_pipeline import GpuXbdPipeline
    n = max(args.sources, 1)
    u8 = lambda *shape, hi=256: torch.randint(0, hi, shape, dtype=torch.uint8, generator=g).to(dev)
    pipe = GpuXbdPipeline(u8(n, S, S, 3), u8(n, S, S, 3), u8(n, S, S), u8(n, S, S, hi=5))
    indices = [i % n for i in range(B)]
    first = pipe.make_adapt_batch(indices, S)
    src = torch.empty(px * 29, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    idx = torch.as_tensor(indices, dtype=torch.int32).to(dev)
    launch = lambda: ops.xbd_adapt_batch(pipe.pre, pipe.post, pipe.pre_mask, pipe.post_label, idx, None, S, True)
    us = timed({"batch": lambda: pipe.make_adapt_batch(indices, S), "launch": launch, "copy": lambda: dst.copy_(src)}, args.rounds,
               args.window_ms)
    out["loader"] = {"what": "us per batch: make_adapt_batch (index upload, allocation and ONE launch), the launch alone on a resident "
                             "index tensor (with its three allocations), and a device copy of its 29 output bytes per pixel",
                     "us": us, "bytes_written": px * 29, "bytes_read": px * 8,
                     "batch_over_copy": round(us["batch"]["median"] / us["copy"]["median"], 3),
                     "launch_over_copy": round(us["launch"]["median"] / us["copy"]["median"], 3),
                     "msk_shape": list(first['msk'].shape)}

    if not args.no_step:
        from dahitra_amd.graph import GraphedXbdAdaptStep, GraphedXbdStep
        x6 = torch.randn(B, 6, S, S, generator=g).clamp_(-1, 1).to(dev)
        pos = 'learned' if S == 1024 else None

        def build(kind):
            torch.manual_seed(args.seed)
            net = xbd.BASE_Transformer_UNet(output_nc=4 if kind == "adapt" else 5, with_decoder_pos=pos,
                                            compute_dtype=args.dtype).to(dev).train()
            if kind == "adapt":
                opt = xbd.AdamW(net.parameters(), lr=1e-4, weight_decay=1e-7, capturable=True)
                return GraphedXbdAdaptStep(net, opt, x6, msk4)
            opt = xbd.AdamW(net.parameters(), lr=1e-4, weight_decay=1e-6, capturable=True)
            return GraphedXbdStep(net, opt, x6, msk5)
        steps = {kind: build(kind) for kind in ("adapt", "xbd_step")}
        for s in steps.values():
            window(s, 5)
        rate = {kind: [] for kind in steps}
        for _ in range(args.rounds):
            for kind, s in steps.items():
                rate[kind].append(B * args.steps / (window(s, args.steps) * 1e-3))
        pairs = {kind: spread(v, 1) for kind, v in rate.items()}
        out["step"] = {"what": "image pairs/s of the recorded step, replayed on its static inputs; xbd_step = GraphedXbdStep (train.py: "
                               "five outputs, five ComboLoss terms, clip) at the same shape, for scale",
                       "nets": ["xbd_unet_transformer_c4" + ("" if pos else "_nodecpos"), "xbd_unet_transformer" + ("" if pos else "_nodecpos")],
                       "dtype": args.dtype, "steps_per_window": args.steps, "pairs_per_s": pairs,
                       "ms_per_step": {k: round(B / v["median"] * 1e3, 3) for k, v in pairs.items()},
                       "adapt_over_xbd_step": round(pairs["adapt"]["median"] / pairs["xbd_step"]["median"], 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
