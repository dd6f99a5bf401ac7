#!/usr/bin/env python3
"""Time of the two kernels of csrc/xbd_visual.hip (ops.xbd_damage_map, ops.xbd_vis_grid) at the reference's tile:

    python tools/visual_bench.py [--n 1] [--size 1024] [--chain 100] [--replays 20]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/visual_bench.py --profile KERNEL [--loc none]
                                                                          # per-kernel time, a run of its own per variant

No host work is inside a timed window: each variant is recorded once as a graph of `chain` launches (arguments checked and
thresholds converted at record time), and `replays` replays of it are timed between two device events, several rounds, the
variants alternating -- 2000 launches, 5 ms or more, per figure.  The figure is the time per launch in such a chain: kernel
time plus the gap to the next kernel node.  The kernel time alone comes from the trace.  Bytes are the algorithmic ones: the map
reads 5 and writes 1 byte per pixel, the grid reads 12 and writes 12.  `grid_dword_stores` is the grid with its output 4 bytes off
a 16-byte address: the same loads, dword stores.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dahitra_amd import ops  # noqa: E402

KERNELS = ("map", "grid", "grid_dword_stores")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--chain", type=int, default=100, help="launches per recorded graph")
    ap.add_argument("--replays", type=int, default=20, help="replays per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--loc", default="script", choices=("none", "script"))
    ap.add_argument("--profile", default=None, choices=KERNELS, help="220 eager launches of one variant and nothing else, nothing timed")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("visual_bench: no GPU; a time is measured on the MI355X or not at all")
    N, S = args.n, args.size
    loc = None if args.loc == "none" else ops.XBD_LOC_THR
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda hi, *shape: torch.randint(0, hi, shape, dtype=torch.uint8, device="cuda", generator=g)
    pre, post, gt, msk = rnd(256, N, S, S, 3), rnd(256, N, S, S, 3), rnd(5, N, S, S), rnd(256, N, S, S, 5)
    cls = torch.empty(N, S, S, dtype=torch.uint8, device="cuda")
    grid = torch.empty(N, S, 4 * S, 3, dtype=torch.uint8, device="cuda")
    grid4 = torch.empty(grid.numel() + 16, dtype=torch.uint8, device="cuda")[4:4 + grid.numel()].view(grid.shape)
    run = {"map": lambda: ops.xbd_damage_map(msk, loc, out=cls),
           "grid": lambda: ops.xbd_vis_grid(pre, post, gt, msk, loc, out=grid),
           "grid_dword_stores": lambda: ops.xbd_vis_grid(pre, post, gt, msk, loc, out=grid4)}
    if args.profile:                                          # this variant alone, so the trace's statistics are its own
        for _ in range(220):
            run[args.profile]()
        torch.cuda.synchronize()
        return
    for fn in run.values():                                   # warm-up: code objects loaded
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    same = torch.equal(grid, grid4)
    graphs = {}
    for k, fn in run.items():
        graphs[k] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[k]):
            for _ in range(args.chain):
                fn()
        graphs[k].replay()
    torch.cuda.synchronize()

    def timed(gr):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.replays):
            gr.replay()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / (args.replays * args.chain)          # us per launch

    t = {k: [] for k in run}
    for _ in range(args.rounds):
        for k in run:
            t[k].append(timed(graphs[k]))
    px = N * S * S
    nbytes = {"map": 6 * px, "grid": 24 * px, "grid_dword_stores": 24 * px}
    row = lambda k: {"median_us": round(statistics.median(t[k]), 2), "min_us": round(min(t[k]), 2), "max_us": round(max(t[k]), 2),
                     "MB": round(nbytes[k] / 1e6, 1)}
    print(json.dumps(dict({"n": N, "size": S, "chain": args.chain, "replays": args.replays, "rounds": args.rounds, "loc": args.loc,
                           "what": "us per launch in a recorded chain (kernel + gap between nodes)", "stores_agree": same,
                           "device": torch.cuda.get_device_name(0)}, **{k: row(k) for k in run})))


if __name__ == "__main__":
    main()
