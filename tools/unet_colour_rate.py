#!/usr/bin/env python3
"""Time of the colour stage of the xBD loader (dh_xbd_unet_colour_u8: two launches) on a batch of `--batch` crops of `--size`.
In the same call, alternating over `--rounds`:

    colour_1      the two launches with ONE job (a change_hsv: what a batch that drew anything usually holds)
    colour_max    the two launches with 2 x batch jobs of the costliest mix: change_hsv on every image, then blur, contrast,
                  saturation and gauss_noise in turn
    copy_1 / copy_max   a device copy_ of the bytes those launches touch (3 float32 planes a job, read and written)
    warp          dh_xbd_augment_warp_u8 on the same batch (rows of a seeded draw_unet_params)
    make_plain / make_colour_1   make_unet_batch(dilate=0) without colour and with the one job, as a user calls it: the host time
                  the argument adds (checks, job table, its copy to the device) is their difference minus colour_1

and, from one epoch of `--epoch-samples` samples drawn with draw_unet_colour (the script's own distribution, gauss_noise
included), the number of batches that hold a job and the mean time the colour stage adds per batch: each batch's jobs are timed
on the device and averaged over ALL batches of the epoch.

    python tools/unet_colour_rate.py [--batch 16] [--size 256] [--source-size 1024] [--sources 16] [--rounds 7] [--window-ms 300]

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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=300.0, help="least length of a timed window")
    ap.add_argument("--epoch-samples", type=int, default=9168, help="samples of the epoch whose mean added time is reported")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("unet_colour_rate: no GPU; a time is measured on the MI355X or not at all")
    dev, n, S, HW = "cuda", args.batch, args.size, args.source_size
    g = torch.Generator().manual_seed(args.seed)
    u8 = lambda *shape, hi=256: torch.randint(0, hi, shape, dtype=torch.uint8, generator=g).to(dev)
    pipe = X.GpuXbdPipeline(u8(args.sources, HW, HW, 3), u8(args.sources, HW, HW, 3), u8(args.sources, HW, HW),
                            u8(args.sources, HW, HW, hi=5))
    rng, np_rng = random.Random(args.seed), np.random.RandomState(args.seed)
    ind = [rng.randrange(args.sources) for _ in range(n)]
    rows = [X.draw_unet_params(rng, HW, HW, S)[0] for _ in range(n)]
    tab = X.unet_warp_table(rows, S)
    idx = torch.tensor(ind, dtype=torch.int32, device=dev)
    par = torch.from_numpy(X.unet_param_rows(rows)).to(dev)
    tab = torch.from_numpy(tab).to(dev) if tab is not None else None
    img = torch.empty(n, 6, S, S, dtype=torch.float32, device=dev)
    msk = torch.empty(n, 5, S, S, dtype=torch.uint8, device=dev)
    ops.xbd_augment_warp(pipe.pre, pipe.post, pipe.post_label, idx, par, tab, S, out_img=img, out_msk=msk)
    start = img.clone()

    one = [None] * n
    one[n // 2] = {"hsv": (1, 5, -5, 5), "pre": None, "post": None}
    block = [("blur", None), ("contrast", 1.0999), ("saturation", 0.9), ("gauss_noise", None)]
    most = []
    for k in range(n):
        entry = {"hsv": (1 + k % 2, 5, -5, 5)}
        for i, im in enumerate(("pre", "post")):
            op, value = block[(2 * k + i) % 4]
            entry[im] = (op, X.draw_unet_noise(np_rng, S) if op == "gauss_noise" else value)
        most.append(entry)

    def device_jobs(colour):
        jobs, noise = X.unet_colour_jobs(X.check_unet_colour(colour, S), S)
        jobs = torch.from_numpy(jobs).to(dev)
        return jobs, (torch.from_numpy(noise).to(dev) if noise is not None else None), \
            torch.empty(ops.xbd_unet_colour_ws_bytes(len(jobs), S), dtype=torch.uint8, device=dev)

    sets = {"colour_1": device_jobs(one), "colour_max": device_jobs(most)}
    planes = {name: torch.empty(len(s[0]), 3, S, S, dtype=torch.float32, device=dev) for name, s in sets.items()}

    def colour(name):
        jobs, noise, ws = sets[name]

        def run(k):
            ops.xbd_unet_colour(img, jobs, noise, ws=ws)      # in place, again and again: the bytes drift, the work does not
        return run

    def copy(name):
        dst, src = planes[name], torch.randn_like(planes[name])
        return lambda k: dst.copy_(src)

    variants = {"colour_1": colour("colour_1"), "colour_max": colour("colour_max"), "copy_1": copy("colour_1"),
                "copy_max": copy("colour_max"),
                "warp": lambda k: ops.xbd_augment_warp(pipe.pre, pipe.post, pipe.post_label, idx, par, tab, S, out_img=img, out_msk=msk),
                "make_plain": lambda k: pipe.make_unet_batch(ind, S, rows, dilate=0),
                "make_colour_1": lambda k: pipe.make_unet_batch(ind, S, rows, dilate=0, colour=one)}

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
        window(f, 20)
        reps[name] = max(10, int(args.window_ms / max(window(f, 50) / 50, 1e-3)) + 1)
    t = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, f in variants.items():
            t[name].append(window(f, reps[name]) * 1e3 / reps[name])
    us = {name: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for name, v in t.items()}

    # one epoch of the script's distribution: the jobs of every batch that drew any, timed on the device
    erng, enp = random.Random(args.seed + 1), np.random.RandomState(args.seed + 1)
    batches, with_jobs, n_jobs, added_ms, applied = 0, 0, 0, 0.0, {}
    for s in range(0, args.epoch_samples, n):
        m = min(n, args.epoch_samples - s)
        cols = [X.draw_unet_colour(erng, HW, HW, S, enp)[1] for _ in range(m)]
        for c in cols:
            for name in X.unet_colour_names(c):
                applied[name.rsplit("_", 1)[0]] = applied.get(name.rsplit("_", 1)[0], 0) + 1
        batches += 1
        jobs, noise = X.unet_colour_jobs(cols, S)
        if jobs is None:
            continue
        with_jobs += 1
        n_jobs += len(jobs)
        sets["epoch"] = device_jobs(cols + [None] * (n - m))
        f = colour("epoch")
        window(f, 5)
        added_ms += window(f, 200) / 200
    img.copy_(start)
    med = lambda name: us[name]["median"]
    print(json.dumps({"batch": n, "size": S, "source_size": HW, "rounds": args.rounds, "window_ms": args.window_ms,
                      "device": torch.cuda.get_device_name(0),
                      "what": "us per batch; copy: a device copy of 3 float32 planes a job (read + written)",
                      "jobs": {name: len(s[0]) for name, s in sets.items() if name != "epoch"}, "us": us,
                      "colour_1_over_copy": round(med("colour_1") / med("copy_1"), 2),
                      "colour_max_over_copy": round(med("colour_max") / med("copy_max"), 2),
                      "colour_1_over_warp": round(med("colour_1") / med("warp"), 2),
                      "colour_max_over_warp": round(med("colour_max") / med("warp"), 2),
                      "host_added_us": round(med("make_colour_1") - med("make_plain") - med("colour_1"), 2),
                      "epoch": {"samples": args.epoch_samples, "batches": batches, "batches_with_jobs": with_jobs, "jobs": n_jobs,
                                "applied": applied, "mean_added_us_per_batch": round(added_ms * 1e3 / batches, 3),
                                "mean_us_of_a_batch_with_jobs": round(added_ms * 1e3 / max(with_jobs, 1), 2)}}))


if __name__ == "__main__":
    main()
