#!/usr/bin/env python3
"""Whole-tile change maps (models/tiles.predict_tile, csrc/cd_tile.hip) on one 1024 x 1024 pair: tiles per second through the
recorded step for three plans, the stitch kernel alone, and the parent's only way to a tile's predictions for comparison.

    python tools/cd_tile_bench.py [--net newUNetTrans] [--dtype bf16] [--tiles 20] [--rounds 5] [--chain 20] [--replays 10]

Plans, all with 256-pixel windows: B = stride 256, no flips, mean (16 views); S = stride 128, no flips, triangle (49 views);
F = stride 128, four flips, triangle (196 views).  Per plan, medians (min - max) over `rounds`, each after a warm-up round:
  tile_ms       predict_tile(graph=True), `tiles` calls between two host clock readings that end in a device synchronise
  stitch_us     us per launch of dh_cd_tile_stitch alone: a recorded chain of `chain` launches, `replays` replays between two
                device events.  The chain walks FOUR logits buffers in turn (4 x 103 MB at plan F does not fit the 256 MiB
                Infinity Cache), so GB/s -- P C h w 4 bytes read plus (4 C + 1) H W written, over that time -- is an HBM rate
                wherever 4 P C h w 4 bytes exceed the cache, and says so where they do not.
  parent_ms     plan B only: the sixteen `make_batch([0], 256, patch=i)` + eager forward + argmax_mask of the code before this
                feature, same process, same box, host clock ending in a synchronise.  (Its patch 0 is the window at (256, 256)
                again, as the reference executes it; the work is the same sixteen forwards.)
Prints one JSON line."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dahitra_amd import ops  # noqa: E402
from dahitra_amd.datasets.gpu_pipeline import GpuPairPipeline  # noqa: E402
from dahitra_amd.graph import tile_chunk  # noqa: E402
from dahitra_amd.models.losses import argmax_mask  # noqa: E402
from dahitra_amd.models.networks import define_G  # noqa: E402
from dahitra_amd.models.tiles import predict_tile  # noqa: E402
from dahitra_amd.tiles import TilePlan  # noqa: E402

CACHE_BYTES = 256 << 20


def stats(ts, digits):
    return {"median": round(statistics.median(ts), digits), "min": round(min(ts), digits), "max": round(max(ts), digits)}


def host_timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", default="newUNetTrans")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--tiles", type=int, default=20, help="tiles per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chain", type=int, default=20, help="stitch launches per recorded graph")
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--chunk", type=int, nargs="*", default=[], help="also time plans S and F at these views per forward")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cd_tile_bench: no GPU; a time is measured on the MI355X or not at all")
    S = args.size
    g = torch.Generator(device="cuda").manual_seed(1)
    img = lambda: torch.randint(0, 256, (1, S, S, 3), device="cuda", generator=g, dtype=torch.uint8)
    pipe = GpuPairPipeline(img(), img(), (torch.rand(1, S, S, device="cuda", generator=g) > 0.9).to(torch.uint8))
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):                        # define_G prints; this tool prints one JSON line
        net = define_G(types.SimpleNamespace(net_G=args.net, compute_dtype=args.dtype), gpu_ids=[0])
    net.eval()
    plans = {"B": TilePlan(S, S, (256, 256), (256, 256), (0,), "mean"),
             "S": TilePlan(S, S, (256, 256), (128, 128), (0,), "triangle"),
             "F": TilePlan(S, S, (256, 256), (128, 128), (0, 1, 2, 3), "triangle")}
    result = {"net": args.net, "dtype": args.dtype, "size": S, "tiles": args.tiles, "rounds": args.rounds, "chain": args.chain,
              "replays": args.replays, "device": torch.cuda.get_device_name(0), "plans": {}}

    def parent():
        for patch in range(16):
            batch = pipe.make_batch([0], 256, patch=patch)
            with torch.no_grad():
                argmax_mask(net(batch['A'], batch['B']))

    for name, plan in plans.items():
        mask, logits = predict_tile(net, pipe, 0, plan)                     # records the step
        C = logits.shape[0]
        tile = [host_timed(lambda: predict_tile(net, pipe, 0, plan), args.tiles) for _ in range(args.rounds + 1)][1:]
        bufs = [torch.randn(plan.P, C, plan.h, plan.w, device="cuda", generator=g) for _ in range(4)]
        out_l, out_m = torch.empty_like(logits), torch.empty_like(mask)
        for b in bufs:
            ops.cd_tile_stitch(b, plan, out_logits=out_l, out_mask=out_m)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for i in range(args.chain):
                ops.cd_tile_stitch(bufs[i % 4], plan, out_logits=out_l, out_mask=out_m)
        stitch = []
        for _ in range(args.rounds + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.replays):
                graph.replay()
            e1.record()
            torch.cuda.synchronize()
            stitch.append(e0.elapsed_time(e1) * 1e3 / (args.replays * args.chain))
        read = plan.P * C * plan.h * plan.w * 4
        nbytes = read + (4 * C + 1) * S * S
        t, k = stats(tile, 3), stats(stitch[1:], 2)
        row = {"views": plan.P, "chunk": tile_chunk(plan.P), "tile_ms": t,
               "tiles_per_s": round(1e3 / t["median"], 2), "views_per_s": round(plan.P * 1e3 / t["median"], 1), "stitch_us": k,
               "stitch_MB": round(nbytes / 1e6, 1), "stitch_GBps": round(nbytes / k["median"] / 1e3, 0),
               "stitch_reads_exceed_cache": 4 * read > CACHE_BYTES, "mask_ones": int(mask.sum())}
        if name == "B":
            p = stats([host_timed(parent, max(args.tiles // 4, 2)) for _ in range(args.rounds + 1)][1:], 3)
            row["parent_ms"] = p
            row["parent_tiles_per_s"] = round(1e3 / p["median"], 2)
            row["ratio"] = round(p["median"] / t["median"], 2)
        for chunk in args.chunk:
            if name != "B" and plan.P % chunk == 0:
                predict_tile(net, pipe, 0, plan, chunk=chunk)
                c = stats([host_timed(lambda: predict_tile(net, pipe, 0, plan, chunk=chunk), args.tiles)
                           for _ in range(args.rounds + 1)][1:], 3)
                row["tile_ms_chunk_%d" % chunk] = c
        result["plans"][name] = row
        del bufs
    print(json.dumps(result))


if __name__ == "__main__":
    main()
