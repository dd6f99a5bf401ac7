#!/usr/bin/env python3
"""Time of one xBD prediction (models/xbd.predict_tta: pack, eval-mode forward at batch 4, merge) at the reference's size:

    python tools/predict_bench.py [--size 1024] [--reps 20] [--dtype fp32]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/predict_bench.py --profile      # per-kernel times, a run of its own

The recorded step and the eager path alternate; each repetition is timed between two device events (copy of the pair into the
step's static sources included for the recorded step).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dahitra_amd.models import xbd  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--dtype", default=None, help="compute_dtype of the net (default: the net's own default)")
    ap.add_argument("--profile", action="store_true", help="10 replays and 10 eager calls after warm-up, nothing timed")
    args = ap.parse_args()
    torch.manual_seed(0)
    net = xbd.BASE_Transformer_UNet(with_decoder_pos=None, compute_dtype=args.dtype).cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(1)
    S = args.size
    pairs = [tuple(torch.randint(0, 256, (1, S, S, 3), dtype=torch.uint8, device="cuda", generator=g) for _ in range(2))
             for _ in range(2)]
    graphed = lambda p: xbd.predict_tta(net, *p)
    eager = lambda p: xbd.predict_tta(net, *p, graph=False)
    for _ in range(3):                                   # warm-up of both paths (records the step)
        for p in pairs:
            same = torch.equal(graphed(p), eager(p))
    torch.cuda.synchronize()
    if args.profile:
        for i in range(10):
            graphed(pairs[i & 1])
        torch.cuda.synchronize()
        for i in range(10):
            eager(pairs[i & 1])
        torch.cuda.synchronize()
        return
    tg, te = [], []
    for i in range(args.reps):
        tg.append(timed(lambda: graphed(pairs[i & 1])))
        te.append(timed(lambda: eager(pairs[i & 1])))
    row = lambda t: {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3),
                     "pairs_per_s": round(1e3 / statistics.median(t), 1)}
    print(json.dumps({"size": S, "reps": args.reps, "graph_equals_eager": same, "recorded": row(tg), "eager": row(te)}))


if __name__ == "__main__":
    main()
