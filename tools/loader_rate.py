#!/usr/bin/env python3
"""Rate of the device loader (datasets/gpu_pipeline.py) without and with the Gaussian blur, same process, same data: batch 32 of
256 x 256 windows from 256 x 256 random-noise sources, random flips and radii.  HIP events around 50 repetitions after 10
warm-ups, the two variants alternating over a few rounds (median reported).  Two figures per variant: `make_batch` (what a training loop
pays per batch: the parameter tables' host-to-device copies, the output allocations, the kernel) and the kernel alone
(dh_augment_pairs_u8 / dh_augment_pairs_blur_u8 on tables already on the device).

    python tools/loader_rate.py [--batch 32] [--size 256] [--sources 64] [--rounds 5]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dahitra_amd import ops  # noqa: E402
from dahitra_amd.datasets.gpu_pipeline import GpuPairPipeline, blur_table  # noqa: E402

WARMUP, REPS = 10, 50


def timed(fn):
    """microseconds per call: events around REPS calls after WARMUP calls"""
    for _ in range(WARMUP):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--sources", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loader_rate: needs the GPU (no rate is reported without one)")
    n, sz, S = args.batch, args.size, args.sources
    g = torch.Generator().manual_seed(1)
    a = torch.randint(0, 256, (S, sz, sz, 3), generator=g, dtype=torch.uint8).cuda()
    b = torch.randint(0, 256, (S, sz, sz, 3), generator=g, dtype=torch.uint8).cuda()
    lab = (torch.rand(S, sz, sz, generator=g) > 0.9).to(torch.uint8).cuda()
    pipe = GpuPairPipeline(a, b, lab)
    ind = torch.randperm(S, generator=g)[:n].tolist() if S >= n else torch.randint(0, S, (n,), generator=g).tolist()
    flips = (torch.rand(n, 2, generator=g) > 0.5).int()
    radii = torch.rand(n, generator=g).tolist()

    dev = a.device
    idx = torch.tensor(ind, dtype=torch.int32, device=dev)
    params = torch.zeros(n, 4, dtype=torch.int32)
    params[:, 2:] = flips
    params, table = params.to(dev), blur_table(radii).to(dev)
    oa = torch.empty(n, 3, sz, sz, dtype=torch.float32, device=dev)
    ob, ol = torch.empty_like(oa), torch.empty(n, 1, sz, sz, dtype=torch.uint8, device=dev)

    def kernel(blur):
        extra = (ops.P(table),) if blur else ()
        ops._call("dh_augment_pairs_blur_u8" if blur else "dh_augment_pairs_u8", ops.P(a), ops.P(b), ops.P(lab), ops.P(idx),
                  ops.P(params), *extra, n, sz, sz, sz, sz, ops.P(oa), ops.P(ob), ops.P(ol), ops.S())

    variants = {"make_batch plain": lambda: pipe.make_batch(ind, sz, flips),
                "make_batch blur": lambda: pipe.make_batch(ind, sz, flips, blur=radii),
                "kernel plain": lambda: kernel(False),
                "kernel blur": lambda: kernel(True)}
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    for k in variants:
        print("%-17s %8.1f us per batch of %d  (min %.1f)  %9.0f pairs/s" % (k, med[k], n, min(times[k]), n / med[k] * 1e6))
    print("blur / plain: make_batch %.2fx, kernel %.2fx" % (med["make_batch blur"] / med["make_batch plain"],
                                                           med["kernel blur"] / med["kernel plain"]))
    out_bytes = 2 * n * 3 * sz * sz * 4 + n * sz * sz
    in_bytes = 2 * n * sz * sz * 3 + n * sz * sz
    print("bytes per batch: %.1f MB in + %.1f MB out; kernel plain %.2f TB/s, kernel blur %.2f TB/s"
          % (in_bytes / 1e6, out_bytes / 1e6, (in_bytes + out_bytes) / med["kernel plain"] / 1e6,
             (in_bytes + out_bytes) / med["kernel blur"] / 1e6))


if __name__ == "__main__":
    main()
