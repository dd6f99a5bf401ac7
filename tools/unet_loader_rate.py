#!/usr/bin/env python3
"""Time of the device loader with xBD_code/train_unettransformer.py's geometry (dh_xbd_augment_warp_u8): a batch of `--batch` crops
of `--size` from `--sources` sources of `--source-size`, the rows drawn by a seeded draw_unet_params -- the script's own
distribution: 95 % rot90, 50 % vflip, 40 % rotate / scale, 10 % shift.  In the same call, alternating over `--rounds`:

    warp        the kernel alone on `--sets` drawn batches in turn (tables on the device, outputs given)
    make_unet   make_unet_batch(dilate=0) as a user calls it: rows checked, tables written and copied, outputs allocated
    parent      train.py's kernel (dh_xbd_augment_u8) on draw_train_params rows at the same batch and crop
    copy        a device copy_ of as many bytes as a batch's outputs (fp32 images and uint8 masks)

    python tools/unet_loader_rate.py [--batch 16] [--size 256] [--source-size 1024] [--sources 16] [--rounds 7] [--window-ms 300]

Device events around windows of `--window-ms` or more after a warm-up; medians.  Prints one JSON line."""
import argparse
import json
import os
import random
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dahitra_amd import ops  # noqa: E402
from dahitra_amd.datasets import xbd_pipeline as X  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--source-size", type=int, default=1024)
    ap.add_argument("--sources", type=int, default=16)
    ap.add_argument("--sets", type=int, default=8, help="drawn batches the kernel windows cycle through")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=300.0, help="least length of a timed window")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("unet_loader_rate: no GPU; a time is measured on the MI355X or not at all")
    dev, n, S, HW = "cuda", args.batch, args.size, args.source_size
    g = torch.Generator().manual_seed(args.seed)
    u8 = lambda *shape, hi=256: torch.randint(0, hi, shape, dtype=torch.uint8, generator=g).to(dev)
    pipe = X.GpuXbdPipeline(u8(args.sources, HW, HW, 3), u8(args.sources, HW, HW, 3), u8(args.sources, HW, HW),
                            u8(args.sources, HW, HW, hi=5))
    rng = random.Random(args.seed)
    sets, host_sets, old_sets, ops_drawn = [], [], [], {"rot": 0, "vflip": 0, "shift": 0, "warp": 0}
    for _ in range(args.sets):
        ind = [rng.randrange(args.sources) for _ in range(n)]
        rows = [X.draw_unet_params(rng, HW, HW, S)[0] for _ in range(n)]
        for r in rows:
            ops_drawn["rot"] += r["rot"] > 0
            ops_drawn["vflip"] += r["vflip"]
            ops_drawn["shift"] += r["shift"] is not None
            ops_drawn["warp"] += r["warp"] is not None
        tab = X.unet_warp_table(rows, S)
        sets.append((torch.tensor(ind, dtype=torch.int32, device=dev), torch.from_numpy(X.unet_param_rows(rows)).to(dev),
                     torch.from_numpy(tab).to(dev) if tab is not None else None))
        host_sets.append((ind, rows))
        old = X.check_params([X.draw_train_params(rng, HW, HW, S)[0] for _ in range(n)], HW, HW, S)
        coef = X.coef_table(old, S)
        old_sets.append((sets[-1][0], old.to(dev), coef.to(dev) if coef is not None else None))
    img = torch.empty(n, 6, S, S, dtype=torch.float32, device=dev)
    msk = torch.empty(n, 5, S, S, dtype=torch.uint8, device=dev)
    src_img, src_msk = torch.randn_like(img), torch.ones_like(msk)

    def warp(k):
        idx, p, tab = sets[k % args.sets]
        ops.xbd_augment_warp(pipe.pre, pipe.post, pipe.post_label, idx, p, tab, S, out_img=img, out_msk=msk)

    def make_unet(k):
        ind, rows = host_sets[k % args.sets]
        pipe.make_unet_batch(ind, S, rows, dilate=0)

    def parent(k):
        idx, p, coef = old_sets[k % args.sets]
        ops._call("dh_xbd_augment_u8", ops.P(pipe.pre), ops.P(pipe.post), ops.P(None), ops.P(pipe.post_label), ops.P(idx), ops.P(p),
                  ops.P(coef), n, HW, HW, S, 0, ops.P(img), ops.P(msk), ops.P(None), ops.S())

    def copy(k):
        img.copy_(src_img)
        msk.copy_(src_msk)

    variants = {"warp": warp, "make_unet": make_unet, "parent": parent, "copy": copy}

    def window(f, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for k in range(reps):
            f(k)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)                                  # ms

    reps = {}
    for name, f in variants.items():                             # warm-up, then as many repetitions as fill a window
        window(f, 3 * args.sets)
        reps[name] = max(10, int(args.window_ms / max(window(f, 50) / 50, 1e-3)) + 1)
    t = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, f in variants.items():
            t[name].append(window(f, reps[name]) * 1e3 / reps[name])
    us = {name: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for name, v in t.items()}
    out_bytes = img.numel() * 4 + msk.numel()
    print(json.dumps({"batch": n, "size": S, "source_size": HW, "sources": args.sources, "sets": args.sets, "rounds": args.rounds,
                      "window_ms": args.window_ms, "device": torch.cuda.get_device_name(0),
                      "drawn_fraction": {k: round(v / (n * args.sets), 3) for k, v in ops_drawn.items()},
                      "what": "us per batch; copy: two device copies of a batch's output bytes (read + written)",
                      "output_bytes": out_bytes, "us": us,
                      "warp_over_copy": round(us["warp"]["median"] / us["copy"]["median"], 2),
                      "warp_over_parent": round(us["warp"]["median"] / us["parent"]["median"], 2),
                      "warp_output_GBs": round(out_bytes / us["warp"]["median"] / 1e3, 1)}))


if __name__ == "__main__":
    main()
