#!/usr/bin/env python3
"""Time of the xBD ensemble prediction (csrc/xbd_ensemble.hip, models/xbd.predict_ensemble) for one 1024 x 1024 pair, for
M in {1, 2, 4} snapshots and V in {4, 8} views:

    step     the graphed predict_ensemble: one pack, M eval-mode forwards at batch V, one merge, replayed (ms per pair)
    pack     ops.xbd_tta_pack_views alone                 6 B read + 24 V B written per pixel
    merge    ops.xbd_tta_merge_multi alone                20 M V B read + 5 B written per pixel
    host     the route a user has without it: the same pack, M eval forwards, every model's sigmoids copied to the host, the
             script's un-flips (and un-transposes), its numpy stack and mean(axis=0), uint8 (a host clock, ms per pair)

    python tools/ensemble_bench.py [--size 1024] [--models 1 2 4] [--views 4 8] [--chain 20] [--replays 5] [--rounds 7] [--window-ms 100]

No host work is inside a timed device window: pack and merge are recorded `chain` times into one graph each, and as many replays
as make a window of `window-ms` are timed between two device events, several rounds, the cases alternating.  Beside each of the
two kernels stands `copy_us`, a device copy_ that moves the same number of bytes (a buffer of half the kernel's read + written
bytes, read once and written once), timed the same way in the same process; `x_copy` = us / copy_us.  A case whose forward does
not fit is reported with its error and the run goes on.  Prints one JSON line."""
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
from dahitra_amd.graph import GraphedXbdEnsembleStep  # noqa: E402
from dahitra_amd.models import xbd  # noqa: E402


def unview(s, v):
    """the script's un-flip of one [5, H, W] map, and for v >= 4 the un-transpose before it"""
    if v >= 4:
        s = s.swapaxes(-1, -2)
    if v & 1:
        s = s[:, ::-1, :]
    if v & 2:
        s = s[:, :, ::-1]
    return s


def host_route(nets, pre, post, V):
    inp = ops.xbd_tta_pack_views(pre, post, "bgr", V)
    pred = []
    with torch.no_grad():
        for net in nets:
            msk = torch.sigmoid(net(inp).float()).cpu().numpy()
            for v in range(V):
                pred.append(unview(msk[v], v))
    return (np.asarray(pred).mean(axis=0) * 255).astype('uint8').transpose(1, 2, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--models", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--views", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--chain", type=int, default=20, help="kernels per recorded graph")
    ap.add_argument("--replays", type=int, default=5, help="least replays per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=100.0, help="least length of a timed window (more replays are added)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_bench: no GPU; a time is measured on the MI355X or not at all")
    S, dev = args.size, "cuda"
    rng = np.random.RandomState(1)
    pre, post = (torch.from_numpy(rng.randint(0, 256, (1, S, S, 3)).astype(np.uint8)).to(dev) for _ in range(2))
    nets = []
    for m in range(max(args.models)):
        torch.manual_seed(m)
        nets.append(xbd.BASE_Transformer_UNet(input_nc=3, output_nc=5, token_len=4, resnet_stages_num=4, with_pos='learned',
                                              with_decoder_pos=None, enc_depth=1, dec_depth=8).to(dev).eval())

    def window(g, replays):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(replays):
            g.replay()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)                                  # ms

    def chained(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(args.chain):
                fn()
        g.replay()
        torch.cuda.synchronize()
        return g

    graphs, per, bytes_of, errors, host_ms, agree = {}, {}, {}, {}, {}, {}
    keep = []

    def copy_graph(nbytes):
        """a copy_ that reads nbytes / 2 and writes nbytes / 2"""
        key = ("copy", nbytes)
        if key not in graphs:
            src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev).random_(0, 256)
            dst = torch.empty_like(src)
            keep.extend((src, dst))
            graphs[key], per[key] = chained(lambda: dst.copy_(src)), args.chain
        return key

    for V in args.views:
        inp = ops.xbd_tta_pack_views(pre, post, "bgr", V)
        keep.append(inp)
        key = ("pack", V)
        graphs[key], per[key] = chained(lambda inp=inp, V=V: ops.xbd_tta_pack_views(pre, post, "bgr", V, out=inp)), args.chain
        bytes_of[key] = S * S * (6 + 24 * V)
        copy_graph(bytes_of[key])
        for M in args.models:
            logits = [torch.randn(V, 5, S, S, device=dev) * 3 for _ in range(M)]
            out = torch.empty(1, S, S, 5, dtype=torch.uint8, device=dev)
            keep.extend(logits + [out])
            key = ("merge", M, V)
            graphs[key] = chained(lambda logits=logits, out=out, V=V: ops.xbd_tta_merge_multi(logits, V, out=out))
            per[key] = args.chain
            bytes_of[key] = S * S * (20 * M * V + 5)
            copy_graph(bytes_of[key])
            try:
                step = GraphedXbdEnsembleStep(nets[:M], pre, post, "bgr", V)
                graphs["step", M, V], per["step", M, V] = step.graph, 1
                keep.append(step)
                ts = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    back = host_route(nets[:M], pre, post, V)
                    ts.append((time.perf_counter() - t0) * 1e3)
                host_ms[M, V] = round(statistics.median(ts), 1)
                got = step.step()[0].cpu().numpy()
                agree[M, V] = round(float((got == back).mean()), 6)          # the device expf is not numpy's: a few bytes may differ
            except (RuntimeError, torch.cuda.OutOfMemoryError) as e:
                errors["%dx%d" % (M, V)] = str(e).splitlines()[0][:200]
    torch.cuda.synchronize()
    replays = {k: max(args.replays, int(args.window_ms / max(window(g, args.replays) / args.replays, 1e-3)) + 1) for k, g in graphs.items()}
    t = {k: [] for k in graphs}
    for _ in range(args.rounds):
        for k, g in graphs.items():
            t[k].append(window(g, replays[k]) * 1e3 / (replays[k] * per[k]))          # us per operation
    row = lambda k: {"median": round(statistics.median(t[k]), 1), "min": round(min(t[k]), 1), "max": round(max(t[k]), 1)}
    table = {}
    for k in graphs:
        if k[0] == "copy":
            continue
        name = "%s/%s" % (k[0], "x".join(str(v) for v in k[1:]))
        if k[0] == "step":
            us = row(k)
            table[name] = {"ms": round(us["median"] / 1e3, 3), "ms_min": round(us["min"] / 1e3, 3), "ms_max": round(us["max"] / 1e3, 3),
                           "host_ms": host_ms.get(k[1:]), "host_equal_bytes": agree.get(k[1:]),
                           "x_host": round(host_ms[k[1:]] * 1e3 / us["median"], 2) if k[1:] in host_ms else None}
        else:
            us, cp = row(k), row(("copy", bytes_of[k]))
            table[name] = {"us": us, "MB": round(bytes_of[k] / 1e6, 1), "TB_s": round(bytes_of[k] / us["median"] / 1e6, 2),
                           "copy_us": cp, "copy_TB_s": round(bytes_of[k] / cp["median"] / 1e6, 2),
                           "x_copy": round(us["median"] / cp["median"], 2)}
    print(json.dumps({"size": S, "chain": args.chain, "window_ms": args.window_ms, "rounds": args.rounds,
                      "what": "step: ms per pair, graph replay; pack / merge: us per kernel in a recorded chain, bytes read + written; "
                              "copy: a copy_ moving the same bytes; host_ms: forwards, sigmoids to the host, numpy stack and mean",
                      "device": torch.cuda.get_device_name(0), "errors": errors, "ops": table}))


if __name__ == "__main__":
    main()
