#!/usr/bin/env python3
"""Rate of the device loader (datasets/gpu_pipeline.py) without and with the Gaussian blur, same process, same data: batch 32 of
256 x 256 windows from 256 x 256 random-noise sources, random flips and radii.  HIP events around 50 repetitions after 10
warm-ups, the two variants alternating over a few rounds (median reported).  Two figures per variant: `make_batch` (what a training loop
pays per batch: the parameter tables' host-to-device copies, the output allocations, the kernel) and the kernel alone
(dh_augment_pairs_u8 / dh_augment_pairs_blur_u8 on tables already on the device).

    python tools/loader_rate.py [--batch 32] [--size 256] [--sources 64] [--rounds 5]

--xbd measures the xBD loader instead (datasets/xbd_pipeline.py, dh_xbd_augment_u8): batches of `--size` crops from sources of
the same size, in three variants -- no sample resized, every sample resized with a box at the mean of the reference's offsets
(top = left = 100: the worst case, every byte goes through both passes with real coefficients), and val mode.

    python tools/loader_rate.py --xbd --batch 4 --size 1024 --sources 8

--jitter FRACTION adds a fourth variant to --xbd: the plain rows with ColorJitter (dh_xbd_augment_jitter_u8) on that fraction of
the samples, spread evenly over the 50 batches of a measurement (the reference jitters 9 %: --jitter 0.09; 1 jitters every
sample, 0 none).  A batch without a jittered sample goes through dh_xbd_augment_u8, as it does in the loader.
"""
import argparse
import ctypes
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


def main_xbd(args):
    from dahitra_amd.datasets.xbd_pipeline import GpuXbdPipeline, check_params, coef_table
    n, sz, S = args.batch, args.size, args.sources
    g = torch.Generator().manual_seed(1)
    pre = torch.randint(0, 256, (S, sz, sz, 3), generator=g, dtype=torch.uint8).cuda()
    post = torch.randint(0, 256, (S, sz, sz, 3), generator=g, dtype=torch.uint8).cuda()
    pmask = ((torch.rand(S, sz, sz, generator=g) > 0.9) * 255).to(torch.uint8).cuda()
    label = torch.randint(0, 5, (S, sz, sz), generator=g, dtype=torch.uint8).cuda()
    pipe = GpuXbdPipeline(pre, post, pmask, label)
    ind = torch.randint(0, S, (n,), generator=g).tolist()
    flips = (torch.rand(n, 2, generator=g) > 0.5).int().tolist()
    off = min(100, sz // 4)
    rows = {"plain": [[0, 0, hf, vf, 0, 0, 0, sz, sz] for hf, vf in flips],
            "resized": [[0, 0, hf, vf, 1, off, off, sz - off, sz - off] for hf, vf in flips]}
    rows["val"] = [[0, 0, 0, 0, 0, 0, 0, sz, sz]] * n

    dev = pre.device
    idx = torch.tensor(ind, dtype=torch.int32, device=dev)
    img = torch.empty(n, 6, sz, sz, dtype=torch.float32, device=dev)
    msk = torch.empty(n, 5, sz, sz, dtype=torch.uint8, device=dev)
    lbl = torch.empty(n, sz, sz, dtype=torch.uint8, device=dev)
    tables = {}
    for k, r in rows.items():
        p = check_params(r, sz, sz, sz)
        c = coef_table(p, sz)
        tables[k] = (p.to(dev), c.to(dev) if c is not None else None)

    def kernel(k):
        p, c = tables[k]
        val = k == "val"
        ops._call("dh_xbd_augment_u8", ops.P(pre), ops.P(post), ops.P(pmask if val else None), ops.P(label), ops.P(idx), ops.P(p),
                  ops.P(c), n, sz, sz, sz, int(val), ops.P(img), ops.P(msk), ops.P(lbl if val else None), ops.S())

    variants = {}
    for k in rows:
        variants["make_batch " + k] = lambda k=k: pipe.make_batch(ind, sz, rows[k], train=k != "val")
        variants["kernel " + k] = lambda k=k: kernel(k)
    if args.jitter is not None:
        from dahitra_amd.datasets.xbd_pipeline import draw_jitter_params, jitter_table, jitter_workspace_bytes
        if not 0 <= args.jitter <= 1:
            raise SystemExit("loader_rate: --jitter takes a fraction in [0, 1]")
        gj = torch.Generator().manual_seed(2)
        # sample j of the REPS batches is jittered where the running count j * fraction steps: evenly spread, exact in total
        flag = [int((j + 1) * args.jitter + 1e-9) > int(j * args.jitter + 1e-9) for j in range(n * REPS)]
        lists = [[(draw_jitter_params(gj), draw_jitter_params(gj)) if flag[b * n + k] else None for k in range(n)]
                 for b in range(REPS)]
        tabs = [jitter_table(l) for l in lists]
        need = jitter_workspace_bytes(n, sz)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        calls = {"make_batch": 0, "kernel": 0}

        def make_batch_jitter():
            b = calls["make_batch"] % REPS
            calls["make_batch"] += 1
            pipe.make_batch(ind, sz, rows["plain"], jitter=lists[b])

        def kernel_jitter():
            b = calls["kernel"] % REPS
            calls["kernel"] += 1
            if tabs[b] is None:
                return kernel("plain")
            p, c = tables["plain"]
            ops._call("dh_xbd_augment_jitter_u8", ops.P(pre), ops.P(post), ops.P(None), ops.P(label), ops.P(idx), ops.P(p), ops.P(c),
                      ctypes.c_void_p(tabs[b].ctypes.data), n, sz, sz, sz, 0, ops.P(img), ops.P(msk), ops.P(None), ops.P(ws), need,
                      ops.S())

        variants["make_batch jitter"], variants["kernel jitter"] = make_batch_jitter, kernel_jitter
        print("jitter: %d of the %d samples of %d batches, %d batches with one" % (sum(flag), n * REPS, REPS,
                                                                                  sum(t is not None for t in tabs)))
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    for k in variants:
        print("%-19s %8.1f us per batch of %d  (min %.1f)  %9.0f samples/s" % (k, med[k], n, min(times[k]), n / med[k] * 1e6))
    # bytes the kernel has to move: the source pixels inside the box (6 + 1 bytes, + 1 in val mode) and the outputs
    out_b = n * sz * sz * (6 * 4 + 5)
    for k in rows:
        side = sz - off if k == "resized" else sz
        in_b = n * side * side * (8 if k == "val" else 7)
        tot = in_b + out_b + (n * sz * sz if k == "val" else 0)
        print("kernel %-8s %.1f MB in + %.1f MB out: %.2f TB/s" % (k, in_b / 1e6, (tot - in_b) / 1e6, tot / med["kernel " + k] / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--xbd", action="store_true", help="the xBD loader (datasets/xbd_pipeline.py) instead of the pair loader")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--sources", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--jitter", type=float, default=None, metavar="FRACTION",
                    help="with --xbd: also measure ColorJitter on this fraction of the samples (the reference: 0.09)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loader_rate: needs the GPU (no rate is reported without one)")
    if args.xbd:
        return main_xbd(args)
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
