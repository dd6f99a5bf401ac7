#!/usr/bin/env python3
"""Time of the CD evaluator's picture (csrc/cd_visual.hip, ops.cd_eval_vis, CDEvaluator.vis_picture) at batch 8, 256 x 256 and
1024 x 1024, two classes, next to the way the picture is made without the kernel:

    python tools/cd_visual_bench.py [--n 8] [--sizes 256 1024] [--chain 100] [--replays 20] [--rounds 7]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/cd_visual_bench.py --profile 256
                                                                          # per-kernel time, 220 eager launches and nothing else

Per size, medians (min - max) over `rounds`, each after warm-ups:
  kernel        us per launch of a recorded chain of `chain` launches, `replays` replays between two device events (kernel plus
                the gap to the next node; no host work in the window).  Bytes are the algorithmic ones: per image pixel 12 + 12 of
                A and B, 4 C of the logits and 8 of the label read, 12 written -- 52 at C = 2.
  picture_host  ms of CDEvaluator.vis_picture() plus the copy of the uint8 picture to the host, between two device events
                around work that ends in the blocking copy
  jpeg          ms of PIL's default JPEG save of that array to a file (host clock)
  host_recipe   ms of the reference's recipe on the same batch (host clock, ends synchronised): A, B, logits and L copied to the
                host, de_norm and make_numpy_grid four times, concatenate, clip, * 255 to uint8 -- the array the JPEG is made of
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dahitra_amd import ops, utils  # noqa: E402


def batch_of(N, S, C, seed):
    """images with structure at 16 pixels plus a little noise (pure noise would be the JPEG encoder's worst case), in [-1, 1]"""
    g = torch.Generator(device="cuda").manual_seed(seed)

    def image():
        coarse = torch.rand(N, 3, max(S // 16, 1), max(S // 16, 1), device="cuda", generator=g) * 2 - 1
        fine = torch.nn.functional.interpolate(coarse, size=(S, S), mode="bilinear", align_corners=False)
        return (fine + 0.05 * torch.randn(N, 3, S, S, device="cuda", generator=g)).clamp_(-1, 1).contiguous()
    a, b = image(), image()
    logits = torch.randn(N, C, S, S, device="cuda", generator=g)
    lab = (torch.rand(N, 1, S, S, device="cuda", generator=g) > 0.9).to(torch.int64)
    return a, b, logits, lab


def host_recipe(a, b, logits, lab):
    """models/evaluator.py:118-128 of the reference with the tensors starting on the device, and the bytes imsave stores"""
    vis_input = utils.make_numpy_grid(utils.de_norm(a.cpu()))
    vis_input2 = utils.make_numpy_grid(utils.de_norm(b.cpu()))
    vis_pred = utils.make_numpy_grid(torch.argmax(logits.cpu(), dim=1, keepdim=True) * 255)
    vis_gt = utils.make_numpy_grid(lab.cpu())
    vis = np.clip(np.concatenate([vis_input, vis_input2, vis_pred, vis_gt], axis=0), a_min=0.0, a_max=1.0)
    return (vis * 255).astype(np.uint8)


def stats(ts, digits):
    return {"median": round(statistics.median(ts), digits), "min": round(min(ts), digits), "max": round(max(ts), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--chain", type=int, default=100, help="launches per recorded graph")
    ap.add_argument("--replays", type=int, default=20, help="replays per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--profile", type=int, default=None, metavar="SIZE", help="220 eager launches at SIZE and nothing else, nothing timed")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cd_visual_bench: no GPU; a time is measured on the MI355X or not at all")
    N, C = args.n, args.classes
    if args.profile:
        a, b, logits, lab = batch_of(N, args.profile, C, 1)
        out = torch.empty(ops.cd_vis_shape(N, args.profile, args.profile), dtype=torch.uint8, device="cuda")
        for _ in range(220):
            ops.cd_eval_vis(a, b, logits, lab, out=out)
        torch.cuda.synchronize()
        return
    from PIL import Image
    from dahitra_amd.models.evaluator import CDEvaluator
    ev = CDEvaluator(types.SimpleNamespace(net_G="base_transformer_pos_s4", compute_dtype="fp32", gpu_ids=[0], n_class=C, checkpoint_dir=None),
                     [])
    result = {"n": N, "classes": C, "chain": args.chain, "replays": args.replays, "rounds": args.rounds,
              "device": torch.cuda.get_device_name(0), "sizes": {}}
    tmp = tempfile.mkdtemp(prefix="cd_visual_bench_")
    for S in args.sizes:
        a, b, logits, lab = batch_of(N, S, C, S)
        out = torch.empty(ops.cd_vis_shape(N, S, S), dtype=torch.uint8, device="cuda")
        for _ in range(20):                                       # warm-up: code object loaded
            ops.cd_eval_vis(a, b, logits, lab, out=out)
        torch.cuda.synchronize()
        same = bool(np.array_equal(out.cpu().numpy(), host_recipe(a, b, logits, lab)))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(args.chain):
                ops.cd_eval_vis(a, b, logits, lab, out=out)
        graph.replay()
        torch.cuda.synchronize()
        ev.batch, ev.G_pred = {"A": a, "B": b, "L": lab}, logits
        kernel, picture, jpeg, recipe = [], [], [], []
        for rnd in range(args.rounds + 1):                        # round 0 warms every path up and is dropped
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.replays):
                graph.replay()
            e1.record()
            torch.cuda.synchronize()
            kernel.append(e0.elapsed_time(e1) * 1e3 / (args.replays * args.chain))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            host = ev.vis_picture().cpu().numpy()
            e1.record()
            torch.cuda.synchronize()
            picture.append(e0.elapsed_time(e1))
            t0 = time.perf_counter()
            Image.fromarray(host).save(os.path.join(tmp, "eval_%d.jpg" % S), format="jpeg")
            jpeg.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_recipe(a, b, logits, lab)
            recipe.append((time.perf_counter() - t0) * 1e3)
        px = N * S * S
        nbytes = (24 + 4 * C + 8 + 12) * px
        k = stats(kernel[1:], 2)
        result["sizes"][str(S)] = {
            "equal_to_host_recipe": same, "picture_shape": list(out.shape), "kernel_MB": round(nbytes / 1e6, 1),
            "kernel_us": k, "kernel_GBps": round(nbytes / k["median"] / 1e3, 0),
            "picture_host_ms": stats(picture[1:], 3), "jpeg_ms": stats(jpeg[1:], 2), "host_recipe_ms": stats(recipe[1:], 2),
            "jpeg_file_bytes": os.path.getsize(os.path.join(tmp, "eval_%d.jpg" % S))}
        os.remove(os.path.join(tmp, "eval_%d.jpg" % S))
    os.rmdir(tmp)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
