#!/usr/bin/env python3
"""Time of the xBD mask morphology (csrc/xbd_morph.hip) on a synthetic 1024 x 1024 footprint, for two inputs:

    buildings   14 x 14 squares on a pitch of 40 (12 % set) with 0.5 % of the pixels flipped: pin-holes and specks
    noisy       random pixels at density 0.5 (the complement has tens of thousands of components)

and five operations: dilate k = 5 (one launch), opening k = 3 (two), fill_holes (nine), clean_footprint(open=3, close=3,
fill=True) (thirteen) and xbd_msk_dilate k = 5 on [4, 5, S, S] training masks (one).

    python tools/morph_bench.py [--size 1024] [--chain 20] [--replays 10] [--rounds 7] [--window-ms 100]

No host work is inside a timed window: an operation is recorded `chain` times into one graph per input (arguments checked at
record time, every buffer given), and `replays` replays of it or more -- as many as make a window of `window-ms` -- are timed
between two device events, several rounds, the operations alternating.  `us` is the time per operation in such a chain.
Two baselines are measured in the same run: `host_ms`, the path the operation replaces -- the map copied to the host, the scipy.ndimage call, the result copied back (a
host clock, median of `rounds`) -- and `copy_us`, a device copy_ of the operation's input to a buffer of its output's size
(as many bytes read and written as the operation's own input and output; its intermediate traffic is on top), timed in a
chain like the operation; `x_copy` = us / copy_us.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dahitra_amd import ops  # noqa: E402
from dahitra_amd.models import xbd  # noqa: E402


def inputs(S, seed=1):
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[:S, :S]
    b = ((y % 40 < 14) & (x % 40 < 14))
    b ^= rng.random_sample((S, S)) < 0.005
    return {"buildings": b.astype(np.uint8), "noisy": (rng.random_sample((S, S)) < 0.5).astype(np.uint8)}


def labels_of(S, seed=2):
    """[4, S, S] labels 0 .. 4: rectangles of random classes over 12 % of the tile"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[:S, :S]
    cls = rng.randint(1, 5, size=(4, S // 40 + 1, S // 40 + 1))
    on = (y % 40 < 14) & (x % 40 < 14)
    return (on[None] * cls[:, y // 40, x // 40]).astype(np.uint8)


def host_ops():
    from scipy import ndimage
    sq = lambda k: np.ones((k, k), dtype=bool)
    er = lambda a, k: ndimage.binary_erosion(a, structure=sq(k), border_value=1)
    di = lambda a, k: ndimage.binary_dilation(a, structure=sq(k))
    op = lambda a, k: di(er(a, k), k)
    cl = lambda a, k: er(di(a, k), k)

    def msk(m):
        d = [np.stack([di(m[n, c], 5) for n in range(m.shape[0])]) for c in range(1, 5)]
        m2, m3, m4 = d[1], d[2] & ~d[1], d[3] & ~d[1] & ~d[2]
        m1 = d[0] & ~(d[1] | d[2] | d[3])
        return np.stack([m1 | m2 | m3 | m4, m1, m2, m3, m4], axis=1)

    one = lambda f: (lambda a: f(a[0] != 0)[None])
    return {"dilate5": one(lambda a: di(a, 5)), "opening3": one(lambda a: op(a, 3)), "fill_holes": one(ndimage.binary_fill_holes),
            "clean_3_3_fill": one(lambda a: ndimage.binary_fill_holes(cl(op(a, 3), 3))), "msk_dilate5": lambda m: msk(m != 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--chain", type=int, default=20, help="operations per recorded graph")
    ap.add_argument("--replays", type=int, default=10, help="replays per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=100.0, help="least length of a timed window (more replays are added)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("morph_bench: no GPU; a time is measured on the MI355X or not at all")
    S, dev = args.size, "cuda"
    maps = {k: torch.from_numpy(v[None]).to(dev) for k, v in inputs(S).items()}
    msk = torch.from_numpy(np.ascontiguousarray(np.stack([(labels_of(S) == c) for c in range(5)], axis=1), dtype=np.uint8)).to(dev)
    msk[:, 0] = msk[:, 1:].amax(dim=1)
    out = torch.empty(1, S, S, dtype=torch.uint8, device=dev)
    tmp = torch.empty(1, S, S, dtype=torch.uint8, device=dev)
    msk_out = torch.empty_like(msk)
    need = ops.xbd_fill_holes_ws_bytes(1, S, S)
    ws = torch.empty(need + 2 * S * S, dtype=torch.uint8, device=dev)

    def opening3(a):
        ops.xbd_morph(a, "erode", 3, out=tmp)
        return ops.xbd_morph(tmp, "dilate", 3, out=out)

    device_ops = {"dilate5": lambda a: ops.xbd_morph(a, "dilate", 5, out=out), "opening3": opening3,
                  "fill_holes": lambda a: ops.xbd_fill_holes(a, 4, out=out, ws=ws[:need]),
                  "clean_3_3_fill": lambda a: xbd.clean_footprint(a, open=3, close=3, fill=True, out=out, ws=ws),
                  "msk_dilate5": lambda m: ops.xbd_msk_dilate(m, 5, out=msk_out)}
    launches = {"dilate5": 1, "opening3": 2, "fill_holes": 9, "clean_3_3_fill": 13, "msk_dilate5": 1}
    cases = [(name, k) for name in device_ops if name != "msk_dilate5" for k in maps] + [("msk_dilate5", "masks")]
    arg = lambda k: msk if k == "masks" else maps[k]
    res_of = lambda k: msk_out if k == "masks" else out
    try:
        host = host_ops()
    except ImportError:
        host = None
    host_ms, agree, graphs = {}, {}, {}
    for name, k in cases:                                     # warm-up, the result checked against the host path, the graph
        a = arg(k)
        for _ in range(3):
            device_ops[name](a)
        torch.cuda.synchronize()
        if host is not None:
            ts = []
            for _ in range(max(3, args.rounds // 2)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                back = torch.from_numpy(host[name](a.cpu().numpy()).astype(np.uint8)).to(dev)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            host_ms[name, k] = round(statistics.median(ts), 2)
            agree[name, k] = bool(torch.equal(back, res_of(k)))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(args.chain):
                device_ops[name](a)
        g.replay()
        graphs[name, k] = g
        if ("copy", k) in graphs:
            continue
        c = torch.cuda.CUDAGraph()
        dst = res_of(k)
        with torch.cuda.graph(c):
            for _ in range(args.chain):
                dst.copy_(a)
        c.replay()
        graphs["copy", k] = c
    torch.cuda.synchronize()

    def window(g, replays):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(replays):
            g.replay()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)                                  # ms

    # a timed window lasts --window-ms or more: a window of a millisecond measures the clock as much as the kernel
    replays = {k: max(args.replays, int(args.window_ms / max(window(g, args.replays) / args.replays, 1e-3)) + 1) for k, g in graphs.items()}

    def timed(k):
        return window(graphs[k], replays[k]) * 1e3 / (replays[k] * args.chain)          # us per operation

    t = {k: [] for k in graphs}
    for _ in range(args.rounds):
        for k in graphs:
            t[k].append(timed(k))
    row = lambda k: {"median": round(statistics.median(t[k]), 1), "min": round(min(t[k]), 1), "max": round(max(t[k]), 1)}
    table = {}
    for name, k in cases:
        us, cp = row((name, k)), row(("copy", k))
        table["%s/%s" % (name, k)] = {"launches": launches[name], "us": us, "copy_us": cp,
                                      "x_copy": round(us["median"] / cp["median"], 2),
                                      "host_ms": host_ms.get((name, k)), "host_agrees": agree.get((name, k)),
                                      "x_host": round(host_ms[name, k] * 1e3 / us["median"], 1) if host is not None else None}
    print(json.dumps({"size": S, "chain": args.chain, "window_ms": args.window_ms, "rounds": args.rounds,
                      "what": "us per operation in a recorded chain (kernels + gaps between nodes); host_ms: copy out, scipy.ndimage, copy back",
                      "device": torch.cuda.get_device_name(0), "set_fraction": {k: round(float(v.float().mean()), 4) for k, v in maps.items()},
                      "ops": table}))


if __name__ == "__main__":
    main()
