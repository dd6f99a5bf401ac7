"""Change maps of whole tiles from nets of fixed input size: windowed inference, stitched on the device.

newUNetTrans runs at 256 x 256 only and the BiT nets are trained there; LEVIR and xBD tiles are 1024 x 1024.  The reference's
answer is eval_cd.py:49-55 -- sixteen CDEvaluators, one per `patch` index, each reloading the checkpoint and scoring its own
256-pixel window; sixteen score lines, no assembled map (demo.py:72-81 has the unfold into patches commented out).  Here a
tiles.TilePlan names the windows of a tile (any stride up to the window, optionally several flips per window), one launch cuts
them, the eval-mode forward runs over them and one launch blends the logits back (ops.cd_tile_stitch), recorded as one HIP
graph per (net, pipeline, plan) unless graph=False.

    pipe = GpuPairPipeline.from_dataset_root(root, split='test')                   # 1024 x 1024 pairs on the device
    plan = TilePlan(1024, 1024, window=(256, 256), stride=(128, 128), flips=(0, 3), weight='triangle')
    mask, logits = predict_tile(net, pipe, 0, plan)                                # uint8 [1024, 1024], float32 [C, 1024, 1024]
    names = predict_tiles(net, pipe, out_dir)                                      # one 0 / 255 PNG per pair
    scores = evaluate_tiles(net, pipe, plan)                                       # cm2score of the stitched maps
    sixteen = evaluate_tiles(net, pipe, TilePlan.eval_cd(1024, 1024))              # what eval_cd.py's sixteen evaluators log

The flip codes of a plan are those of models/xbd.py's 4-flip prediction (bit 0: rows reversed, bit 1: columns reversed)."""
import os

import torch

from ..graph import GraphedTileStep, TileBuffers, tile_chunk
from ..misc.imutils import save_image
from ..tiles import TilePlan
from .evaluator import cm2score


def default_plan(pipe):
    """non-overlapping 256-pixel windows, no flips"""
    _, H, W, _ = pipe.a.shape
    return TilePlan(H, W, window=(256, 256), stride=(256, 256), flips=(0,), weight="mean")


class _Runner:
    """one tile pass per call, recorded (GraphedTileStep) or eager (TileBuffers.run, the very launches the graph records)"""

    def __init__(self, net, pipe, plan, graph, confusion=None, chunk=None):
        net.eval()
        if graph:
            self.step = GraphedTileStep(net, pipe, plan, confusion=confusion, chunk=chunk)
            self.buf = self.step.buf
        else:
            self.step, self.buf = None, TileBuffers(net, pipe, plan, confusion, chunk)
        self.net = net

    def __call__(self, index):
        if self.step is not None:
            return self.step.step(index)
        if self.net.training:
            raise RuntimeError("dahitra_amd: a tile pass is the eval-mode forward; call net.eval()")
        self.buf.aim(index)
        return self.buf.run()


def _runner(net, pipe, plan, graph, chunk):
    """the recorded step of (net, pipe, plan, chunk), kept on the net until forget_tile_steps(): recording costs seconds, a
    replay microseconds"""
    if not graph:
        return _Runner(net, pipe, plan, False, chunk=chunk)
    cache = net.__dict__.setdefault("_tile_steps", {})
    key = (id(pipe), plan, tile_chunk(plan.P) if chunk is None else int(chunk))          # the default chunk is not a second key
    r = cache.get(key)
    if r is None or r.buf.pipe is not pipe or r.step._generation != net._arena.generation:
        r = cache[key] = _Runner(net, pipe, plan, True, chunk=key[2])
    return r


def forget_tile_steps(net, pipe=None):
    """Drop the recorded steps predict_tile / predict_tiles keep on `net` -- all of them, or those of `pipe` -- with their static
    buffers (the cut views and the per-view logits: about 300 MB for a 196-view plan of 256-pixel windows) and their reference
    to the pipeline.  The next call records again.  Returns how many were dropped."""
    cache = net.__dict__.get("_tile_steps", {})
    drop = [k for k, r in cache.items() if pipe is None or r.buf.pipe is pipe]
    for k in drop:
        del cache[k]
    return len(drop)


def predict_tile(net, pipe, index, plan, graph=True, chunk=None):
    """(mask uint8 [H, W], logits float32 [C, H, W]) of source pair `index` of `pipe` (a GpuPairPipeline of H x W pairs) under
    the stitchable `plan`, on the device.  graph=True replays the recorded step of (net, pipe, plan), recording it on first
    use; graph=False makes the same launches eagerly; both give the same bytes.  chunk: views per forward (a divisor of plan.P;
    default the largest up to 16).  The tensors returned are the caller's own (copies of the step's static buffers).  The
    recorded step stays on the net, with its buffers and the pipeline, until forget_tile_steps(net)."""
    plan._need_stitchable("predict_tile")
    mask, logits = _runner(net, pipe, plan, graph, chunk)(index)
    return mask.clone(), logits.clone()


def prediction_name(name):
    """the file name basic_model.CDEvaluator._save_predictions gives the prediction of input `name`"""
    name = name.replace('.jpg', '.png')
    return name if "." in os.path.basename(name) else name + ".png"


def predict_tiles(net, pipe, out_dir, plan=None, graph=True, chunk=None):
    """one binary PNG (0 / 255) per pair of `pipe` in `out_dir`, the stitched class map >= 1, named as
    basic_model.CDEvaluator._save_predictions names its files.  plan: default_plan(pipe) unless given.  Returns the names."""
    plan = default_plan(pipe) if plan is None else plan
    plan._need_stitchable("predict_tiles")
    os.makedirs(out_dir, exist_ok=True)
    run = _runner(net, pipe, plan, graph, chunk)
    written = []
    for i in range(len(pipe)):
        mask, _ = run(i)
        name = prediction_name(pipe.names[i])
        save_image(((mask >= 1).to(torch.uint8) * 255).cpu().numpy(), os.path.join(out_dir, name))
        written.append(name)
    return written


def evaluate_tiles(net, pipe, plan, graph=True, chunk=None, want_counts=False):
    """Scores over every pair of `pipe`.  Stitchable plan: ONE dict, evaluator.cm2score of the confusion of the stitched maps
    against the label tiles.  TilePlan.eval_cd plan: a LIST of sixteen dicts in patch order, what the sixteen evaluators of
    the reference's eval_cd.py:49-55 log (entry 0 repeats entry 5 and the window at (0, 0) is in none: TilePlan.eval_cd).  The
    counts stay on the device until one read at the end.  want_counts: also return the int64 count matrices ([C, C] or
    [16, C, C]) as a numpy array."""
    n_class = _n_class(net, pipe, plan)
    shape = (n_class, n_class) if plan.stitchable else (plan.P, n_class, n_class)
    confusion = torch.zeros(shape, dtype=torch.int64, device=pipe.a.device)
    run = _Runner(net, pipe, plan, graph, confusion=confusion, chunk=chunk)
    for i in range(len(pipe)):
        run(i)
    cm = confusion.cpu().numpy()
    scores = cm2score(cm) if plan.stitchable else [cm2score(m) for m in cm]
    return (scores, cm) if want_counts else scores


def _n_class(net, pipe, plan):
    """the class count of the net's answer, which sizes the confusion buffer before the step exists: one eager forward of ONE
    view, the window at the first pair's corner"""
    from ..datasets.gpu_pipeline import GpuPairPipeline
    net.eval()
    h, w = plan.h, plan.w
    corner = GpuPairPipeline(pipe.a[:1, :h, :w], pipe.b[:1, :h, :w], pipe.l[:1, :h, :w])
    v = corner.window_batch(0, TilePlan(h, w, window=(h, w), stride=(h, w)))
    with torch.no_grad():
        return int(net(v['A'], v['B']).shape[1])
