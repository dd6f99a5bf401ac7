#!/usr/bin/env python3
"""Time of the building step (csrc/xbd_buildings.hip: ops.xbd_cc_label + xbd_cc_stats + xbd_cc_vote + xbd_cc_paint) on one
1024 x 1024 image, for three inputs whose union-find work differs as much as it can:

    noise       random pixels at density 0.59 (8-connectivity: a few large components and thousands of small ones)
    serpentine  ONE component whose path runs through every other row (the longest chains a 1024 x 1024 image can hold)
    squares     a grid of 5 x 5 squares with 1-pixel gaps (29241 components, none crosses more than two tiles)

    python tools/buildings_bench.py [--size 1024] [--chain 20] [--replays 10] [--rounds 7] [--cap 32768]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/buildings_bench.py --profile INPUT
                                                                          # per-kernel time, a run of its own per input

No host work is inside a timed window: the four calls are recorded `chain` times into one graph per input and stage (arguments
checked at record time), and `replays` replays of it are timed between two device events, several rounds, the inputs
alternating.  `label_us` is the labelling alone (six launches), `all_us` label + stats + vote + paint (ten launches), per
sequence in such a chain.  If scipy can be imported, `host_ms` is what the step costs without these kernels: the map copied to
the host, scipy.ndimage.label, np.bincount votes per building and class, the painted map copied back.

The `match` record times the matching of two label maps (ops.xbd_cc_match, five launches) for three pairs of predicted / true
buildings: `match_us` the same way, in a chain of its own with both label maps already on the device, `building_match_ms` the
whole models/xbd.building_match (both labellings, statistics, votes, the match, the two counts read and the small tables
copied; a host clock around the call, which ends in those copies, median of `rounds`), and `host_ms` the route without the
kernel, timed once: both label maps copied to the host, np.unique over the pairs a * (cap + 1) + b, the definition on arrays.
Prints one JSON line."""
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


def inputs(S, seed=1):
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[:S, :S]
    serp = np.zeros((S, S), dtype=np.uint8)
    serp[0::2] = 1
    serp[1::4, S - 1] = 1
    serp[3::4, 0] = 1
    if S % 2 == 0:
        serp[S - 1] = 0
    return {"noise": (rng.random_sample((S, S)) < 0.59).astype(np.uint8), "serpentine": serp,
            "squares": ((y % 6 < 5) & (x % 6 < 5)).astype(np.uint8)}


def host_path(key_dev, vote_dev, conn8=True):
    """the same result without the kernels: copy, scipy.ndimage.label, bincount votes, paint, copy back"""
    from scipy import ndimage
    key, vote = key_dev.cpu().numpy()[0], vote_dev.cpu().numpy()[0]
    labels, k = ndimage.label(key, structure=np.ones((3, 3), dtype=int) if conn8 else None)
    hist = np.bincount(labels.ravel() * 5 + np.minimum(vote.ravel(), 4), minlength=(k + 1) * 5).reshape(k + 1, 5)
    cls = np.where(hist[:, 1:].max(1) > 0, 1 + hist[:, 1:].argmax(1), 0).astype(np.uint8)
    cls[0] = 0
    return torch.from_numpy(cls[labels][None]).to(key_dev.device), k


def host_match(la_dev, lb_dev, cap, num=1, den=2):
    """ops.xbd_cc_match's two outputs without the kernel: both label maps copied back, np.unique over the pairs"""
    a, b = la_dev.cpu().numpy()[0].astype(np.int64).ravel(), lb_dev.cpu().numpy()[0].astype(np.int64).ravel()
    a, b = np.where((a >= 1) & (a <= cap), a, 0), np.where((b >= 1) & (b <= cap), b, 0)
    area_a, area_b = np.bincount(a, minlength=cap + 1), np.bincount(b, minlength=cap + 1)
    pairs, cnt = np.unique(a * (cap + 1) + b, return_counts=True)
    pa, pb = pairs // (cap + 1), pairs % (cap + 1)
    sel = (pa >= 1) & (pb >= 1) & (2 * cnt > area_a[pa])
    m = np.zeros((cap, 5), dtype=np.int64)
    m[:, 0] = area_a[1:]
    m[pa[sel] - 1, 1], m[pa[sel] - 1, 2], m[pa[sel] - 1, 3] = pb[sel], cnt[sel], area_b[pb[sel]]
    ok = (m[:, 1] > 0) & (m[:, 2] * den > num * (m[:, 0] + m[:, 3] - m[:, 2]))
    m[:, 4] = np.where(ok, m[:, 1], 0)
    mb = np.zeros(cap, dtype=np.int32)
    mb[m[ok, 4] - 1] = np.flatnonzero(ok) + 1
    return m.astype(np.int32)[None], mb[None]


def shifted(t):
    """one column to the right, column 0 cleared"""
    out = torch.zeros_like(t)
    out[:, :, 1:] = t[:, :, :-1]
    return out


def match_record(args, keys, vote, timed):
    from dahitra_amd.models import xbd
    S, cap, dev = args.size, args.cap, vote.device
    pairs = {"squares_shifted": (keys["squares"], shifted(keys["squares"])), "noise_squares": (keys["noise"], keys["squares"]),
             "serpentine_squares": (keys["serpentine"], keys["squares"])}
    match_a = torch.empty(1, cap, ops.XBD_CC_MATCH_COLS, dtype=torch.int32, device=dev)
    match_b = torch.empty(1, cap, dtype=torch.int32, device=dev)
    ws = torch.empty(ops.xbd_cc_match_ws_bytes(1, cap, cap), dtype=torch.uint8, device=dev)
    labels, graphs, matched, host_ms, agree, whole_ms = {}, {}, {}, {}, {}, {}
    for k, (pred, gt) in pairs.items():
        la, lb = ops.xbd_cc_label(pred, 8, False)[0], ops.xbd_cc_label(gt, 8, False)[0]
        labels[k] = (la, lb)
        for _ in range(3):
            ops.xbd_cc_match(la, lb, cap, cap, (1, 2), out=(match_a, match_b), ws=ws)
        torch.cuda.synchronize()
        matched[k] = int((match_b != 0).sum())
        t0 = time.perf_counter()
        want = host_match(la, lb, cap)
        host_ms[k] = round((time.perf_counter() - t0) * 1e3, 2)
        agree[k] = bool(np.array_equal(match_a.cpu().numpy(), want[0]) and np.array_equal(match_b.cpu().numpy(), want[1]))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(args.chain):
                ops.xbd_cc_match(la, lb, cap, cap, (1, 2), out=(match_a, match_b), ws=ws)
        g.replay()
        graphs[k] = g
    torch.cuda.synchronize()
    t = {k: [] for k in graphs}
    for _ in range(args.rounds):
        for k in graphs:
            t[k].append(timed(graphs[k]))
    yy, xx = torch.meshgrid(torch.arange(S, device=dev), torch.arange(S, device=dev), indexing="ij")
    blocks = (1 + (yy // 48 + xx // 48) % 4).to(torch.uint8)[None]        # classes 1 .. 4 in 48 x 48 blocks: no square is cut
    for k, (pred, gt) in pairs.items():                       # the whole building_match: class maps on both sides
        pm, gm = pred * vote, gt * blocks
        ts = []
        for i in range(args.rounds + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = xbd.building_match(pm, gm, (1, 2), 8, cap)
            torch.cuda.synchronize()
            if i >= 2:
                ts.append((time.perf_counter() - t0) * 1e3)
        whole_ms[k] = {"median": round(statistics.median(ts), 2), "min": round(min(ts), 2), "max": round(max(ts), 2),
                       "loc": r.loc.tolist()}
    row = lambda k: {"median": round(statistics.median(t[k]), 1), "min": round(min(t[k]), 1), "max": round(max(t[k]), 1)}
    return {"what": "match_us: us per xbd_cc_match in a recorded chain; building_match_ms: host clock around the whole call",
            "matched": matched, "match_us": {k: row(k) for k in pairs}, "building_match_ms": whole_ms, "host_ms": host_ms,
            "host_agrees": agree}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--chain", type=int, default=20, help="sequences per recorded graph")
    ap.add_argument("--replays", type=int, default=10, help="replays per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--cap", type=int, default=32768, help="table rows")
    ap.add_argument("--profile", default=None, choices=("noise", "serpentine", "squares"),
                    help="100 eager sequences on one input and nothing else, nothing timed")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("buildings_bench: no GPU; a time is measured on the MI355X or not at all")
    S, cap = args.size, args.cap
    dev = "cuda"
    keys = {k: torch.from_numpy(v[None]).to(dev) for k, v in inputs(S).items()}
    vote = torch.from_numpy(np.random.RandomState(2).randint(1, 5, size=(1, S, S)).astype(np.uint8)).to(dev)
    labels = torch.empty(1, S, S, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(ops.xbd_cc_ws_bytes(1, S, S), dtype=torch.uint8, device=dev)
    table = torch.empty(1, cap, ops.XBD_CC_COLS, dtype=torch.int32, device=dev)
    cls = torch.empty(1, cap, dtype=torch.uint8, device=dev)
    out = torch.empty(1, S, S, dtype=torch.uint8, device=dev)

    def label(key):
        ops.xbd_cc_label(key, 8, False, out=(labels, count), ws=ws)

    def whole(key):
        label(key)
        ops.xbd_cc_stats(labels, vote, cap, out=table)
        ops.xbd_cc_vote(table, 0, "damage", out=cls)
        ops.xbd_cc_paint(labels, cls, out=out)

    if args.profile:                                          # this input alone, so the trace's statistics are its own
        for _ in range(100):
            whole(keys[args.profile])
        torch.cuda.synchronize()
        return
    components, host_ms, agree = {}, {}, {}
    for k, key in keys.items():                               # warm-up, and the result checked against the host path
        for _ in range(3):
            whole(key)
        torch.cuda.synchronize()
        components[k] = int(count[0])
        try:
            t0 = time.perf_counter()
            painted, n = host_path(key, vote)
            torch.cuda.synchronize()
            host_ms[k] = round((time.perf_counter() - t0) * 1e3, 2)
            agree[k] = bool(n == components[k] and n <= cap and torch.equal(painted, out))
        except ImportError:
            host_ms = agree = None
            break
    graphs = {}
    for stage, fn in (("label", label), ("all", whole)):
        for k, key in keys.items():
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(args.chain):
                    fn(key)
            g.replay()
            graphs[stage, k] = g
    torch.cuda.synchronize()

    def timed(g):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.replays):
            g.replay()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / (args.replays * args.chain)          # us per sequence

    t = {k: [] for k in graphs}
    for _ in range(args.rounds):
        for k in graphs:
            t[k].append(timed(graphs[k]))
    row = lambda k: {"median": round(statistics.median(t[k]), 1), "min": round(min(t[k]), 1), "max": round(max(t[k]), 1)}
    res = {"size": S, "cap": cap, "chain": args.chain, "replays": args.replays, "rounds": args.rounds,
           "what": "us per sequence in a recorded chain (kernels + gaps between nodes)", "device": torch.cuda.get_device_name(0),
           "components": components, "label_us": {k: row(("label", k)) for k in keys}, "all_us": {k: row(("all", k)) for k in keys},
           "host_ms": host_ms, "host_agrees": agree}
    med = [res["all_us"][k]["median"] for k in keys]
    res["spread_all"] = round(max(med) / min(med), 2)
    res["match"] = match_record(args, keys, vote, timed)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
