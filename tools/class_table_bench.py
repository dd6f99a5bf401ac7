#!/usr/bin/env python3
"""Time of the xBD class table (csrc/xbd_classes.hip, ops.xbd_class_table) on resident stacks of 1024 x 1024 labels, 64 files
(64 MiB, inside the 256 MiB Infinity Cache) and 2799 files (the xBD `train` folder, 2.7 GiB, from HBM):

    python tools/class_table_bench.py [--files 64 2799] [--size 1024] [--reps 20] [--rounds 7] [--window-ms 50]

    table_us   one ops.xbd_class_table call into a given buffer: the memset node and the launch
    copy_us    a device copy_ of the same bytes to a second buffer, on the same box in the same run: it reads what the table
               reads and writes as much again
    host_ms    the path the call replaces: the stack copied to the host and np.bincount per file (a host clock; once for a
               stack above 1 GiB, the median of three otherwise)

A timed window is `reps` calls or more -- as many as last `window-ms` -- between two device events, after a warm-up; `rounds`
windows per operation, the two operations alternating; median, min and max are printed.  The table is compared with the host
path's before anything is timed.  The labels are synthetic: buildings of random classes 1 .. 4 on a pitch of 40 pixels, 12 % of a
tile, as many distinct tiles as fit 64 and repeated on the device beyond that.  Prints one JSON line."""
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


def tiles(k, S, seed=2):
    """[k, S, S] labels 0 .. 4: 14 x 14 rectangles of random classes on a pitch of 40; every fifth tile holds no building"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[:S, :S]
    on = (y % 40 < 14) & (x % 40 < 14)
    cls = rng.randint(1, 5, size=(k, S // 40 + 1, S // 40 + 1))
    lab = (on[None] * cls[:, y // 40, x // 40]).astype(np.uint8)
    lab[::5] = 0
    return lab


def host_table(stack):
    host = stack.cpu().numpy()
    out = np.zeros((host.shape[0], 6), dtype=np.int64)
    for f in range(host.shape[0]):
        b = np.bincount(host[f].reshape(-1), minlength=256)
        out[f, :5], out[f, 5] = b[:5], b[5:].sum()
    return out


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps                          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, nargs="+", default=[64, 2799])
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20, help="least calls per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=50.0, help="least length of a timed window (more calls are added)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("class_table_bench: no GPU; a time is measured on the MI355X or not at all")
    S, dev = args.size, "cuda"
    base = torch.from_numpy(tiles(min(64, max(args.files)), S)).to(dev)
    rows = {}
    for n in args.files:
        stack = base[torch.arange(n, device=dev) % base.shape[0]].contiguous()
        out = torch.empty(n, 6, dtype=torch.int32, device=dev)
        dst = torch.empty_like(stack)
        nbytes = stack.numel()
        ops_ = {"table": lambda: ops.xbd_class_table(stack, out=out), "copy": lambda: dst.copy_(stack)}
        host_ms = []
        for _ in range(1 if nbytes > (1 << 30) else 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            want = host_table(stack)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        for fn in ops_.values():                                # warm-up
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        agrees = bool(np.array_equal(out.cpu().numpy(), want))
        reps = {k: max(args.reps, int(args.window_ms * 1e3 / max(window(fn, args.reps), 1e-3)) + 1) for k, fn in ops_.items()}
        t = {k: [] for k in ops_}
        for _ in range(args.rounds):
            for k, fn in ops_.items():
                t[k].append(window(fn, reps[k]))
        stat = lambda k: {"median": round(statistics.median(t[k]), 1), "min": round(min(t[k]), 1), "max": round(max(t[k]), 1)}
        tb, cp, hm = stat("table"), stat("copy"), statistics.median(host_ms)
        rows[str(n)] = {"bytes": nbytes, "calls_per_window": reps, "table_us": tb, "copy_us": cp,
                        "table_read_GBps": round(nbytes / tb["median"] / 1e3, 1),
                        "copy_read_plus_write_GBps": round(2 * nbytes / cp["median"] / 1e3, 1),
                        "table_over_copy": round(tb["median"] / cp["median"], 3), "host_ms": round(hm, 1),
                        "host_over_table": round(hm * 1e3 / tb["median"], 1), "host_agrees": agrees}
        stack = dst = None                                      # the next stack takes their place
    print(json.dumps({"size": S, "rounds": args.rounds, "window_ms": args.window_ms, "device": torch.cuda.get_device_name(0),
                      "what": "us per call between two device events; host_ms: stack copied to the host + np.bincount per file",
                      "files": rows}))


if __name__ == "__main__":
    main()
