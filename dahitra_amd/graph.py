"""One train step as ONE HIP graph: ~500 (BiT) to ~2000 (newUNetTrans) kernel launches recorded once and
replayed per step, so the host cost of a step drops from milliseconds of Python/ctypes to a single
hipGraphLaunch (MI355X guidance: capture launch-bound inner loops in hipGraphs, not a tracing compiler).

    step = GraphedTrainStep(net, opt, a, b, lab)      # opt = dahitra_amd.optim.AdamW(..., capturable=True)
    loss = step(a, b, lab)                            # device scalar, same semantics as the eager step

Recorded: forward, zero_grad, focal loss, backward (at engine level, no autograd graph) and (single process) the AdamW
kernel.  With
torch.distributed the step is TWO graphs around the exchange:
    graph 1: forward, loss and the first part of the backward -- BiT nets: down to and including resnet.layer3, so that
             every gradient from layer3 to the end of the flat arena (~77 % of its bytes for base_transformer_pos_s4) is
             final; newUNetTrans / the xBD model: head, top-down path and the three transformer levels (the 5 MB behind the
             trunk in the arena);
    all-reduce of that arena tail, ASYNC (RCCL's stream) ..........  } concurrently
    graph 2: the rest of the backward (BiT: layer2 / layer1 / stem;  }
             newUNetTrans / xBD: the whole ResNet trunk)             }
    all-reduce of the arena head, wait for both, then the update: AdamW with 1/world folded into its grad_scale, or for the
    xBD step the mean over ranks, clip_grad_norm_ over the complete arena and the hand-rolled AdamW (train.py:373-374).
DAHITRA_OVERLAP=auto (default) takes this form only where the all-reduce it hides is modelled longer than the form costs
(parallel.split_offset: world size and tail bytes; 1 forces it, 0 / DAHITRA_NO_OVERLAP=1 gives one graph, then one all-reduce and
the update).  The warm-up steps torch needs before capture are
undone (parameters, BN buffers and optimizer state are restored), so the first graphed step is step 1.

How launches become a graph is written once, `_Recorded._capture`, for the train steps (GraphedTrainStep and the three xBD steps
that derive from it) and for the recorded evaluation steps (`_RecordedEval`).  A train step is its hooks: `_forward_split`,
`_loss_and_grad`, `_eager_body` and `_update`, the class attributes INPUTS and ENGINE_LEVEL, and `max_norm`."""
import torch
import torch.distributed as dist

from . import ops, parallel
from .models import losses


class _Recorded:
    """How launches become a HIP graph, for train and evaluation steps alike.  A subclass says what the warm-up disturbs
    (`_snapshot` -> saved, `_restore(saved)`) and sets the nets' mode; `stale()` tells whether a replay is still safe."""

    def _capture(self, nets, device, warm, bodies, warmup):
        """`warmup` times `warm()` eagerly on a side stream, the state put back, then bodies[0]() captured into self.graph and --
        the overlapped train step -- bodies[1]() into self.graph2, which shares its pool.  Returns what the bodies returned
        (their static outputs)."""
        self._nets = list(nets)
        saved = self._snapshot()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(warmup):
                warm()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self._restore(saved)
        # A captured graph holds RAW pointers: the shared scratch workspace, the weight-gradient plan's slabs and
        # job table, the packed-weight buffers.  ops.pin_captured_buffers() makes every buffer the capture touched
        # immutable for the life of the process (a later, larger eager call allocates a NEW buffer instead of
        # freeing the one the graph still reads and writes).
        # The capture runs on a stream of our own that inherits the warm-up stream's scratch workspace (ops.workspace is keyed
        # by stream): sized by the warm-up, allocated outside the graph's private pool, and no entry of a dead stream remains.
        # (kept for the life of the step: released, PyTorch's stream pool could hand its handle to a later torch.cuda.Stream(),
        # whose eager launches would then look up -- and scribble over -- the workspace the recorded graph reads and writes)
        cs = self._capture_stream = torch.cuda.Stream()
        ops.rekey_workspace(device, s, cs)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=cs):
            outs = [bodies[0]()]
        if len(bodies) > 1:
            self.graph2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph2, pool=self.graph.pool(), stream=cs):
                outs.append(bodies[1]())
        self._pinned = [ops.pin_captured_buffers(net) for net in self._nets]
        self._generations = [net._arena.generation for net in self._nets]
        torch.cuda.synchronize()
        return outs

    @property
    def _generation(self):
        """the arena generation of the (first) net at the capture"""
        return self._generations[0]

    def stale(self):
        """whether a net's parameter arena was rebuilt after the capture"""
        return any(net._arena.generation != g for net, g in zip(self._nets, self._generations))


class GraphedTrainStep(_Recorded):
    CHECK_EVERY = 64          # replays between two read-backs of the persistent-BatchNorm error words
    INPUTS = ("a", "b", "lab")          # the static inputs this step holds, in call order
    ENGINE_LEVEL = True       # the one-graph form records `_engine_pass` (no autograd graph); False: it records `_eager_body`
    max_norm = None           # clip_grad_norm_ before the update (the xBD step of train.py)

    def __init__(self, net, opt, a, b, lab, warmup=3, confusion=None):
        """confusion: an int64 [n_class, n_class] device tensor; the recorded step then also counts arg-max(logits) against
        the labels into it (dh_confusion_matrix, one more kernel inside the graph: the running metric of the reference's
        trainer without any per-step launch or host read)"""
        self._build(net, opt, (a, b, lab), warmup, confusion)

    def _build(self, net, opt, inputs, warmup, confusion=None):
        """hold `inputs` (one per name of INPUTS; None: not held), warm up, record; the state is what it was before"""
        if not getattr(opt, "capturable", False):
            raise ValueError("GraphedTrainStep needs dahitra_amd.optim.AdamW(..., capturable=True)")
        dev = inputs[0].device
        self.net, self.opt = net, opt
        self.confusion = confusion
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        # the mean over the ranks for an update that cannot fold 1 / world into the optimizer's grad_scale (the xBD steps)
        self._inv_world = torch.tensor([1.0 / self.world], device=dev) if self.world > 1 else None
        self.exchange = parallel.exchange_enabled()      # gradient all-reduce + AdamW after the replay
        self.split_off = None                            # arena offset where the overlapped (two-graph) form splits
        self.persist_bn_launches = None                  # (graph 1, graph 2) counts of the overlapped form
        for name, t in zip(self.INPUTS, inputs):
            setattr(self, name, t.clone() if t is not None else None)
        net._ensure_arena(dev)
        counts = []

        def counted(body):          # the persistent BatchNorm launches a capture records
            def run():
                n0 = ops.BN_PERSIST_LAUNCHES
                out = body()
                counts.append(ops.BN_PERSIST_LAUNCHES - n0)
                return out
            return run
        if self.exchange and self._can_split():
            def warm():          # the same launches the two captures make (the split backward has its own reduce tables)
                self._split_first()
                self._second()
                self._update()
            self.loss = self._capture([net], dev, warm, [counted(self._split_first), counted(self._second)], warmup)[0]
            # graph 2 replays beside RCCL's kernels and must hold none
            self.persist_bn_launches = tuple(counts)
            if self.persist_bn_launches[1]:
                raise RuntimeError("dahitra_amd: %d persistent BatchNorm launches were recorded into the graph that overlaps the "
                                   "gradient all-reduce" % self.persist_bn_launches[1])
        else:
            self.loss = self._capture([net], dev, lambda: self._body(include_opt=True),
                                      [lambda: self._body(include_opt=not self.exchange)], warmup)[0]
        self._calls = 0
        ops.bn_persist_check(dev)         # the warm-up steps and the capture left no barrier timeout behind

    def _snapshot(self):
        """parameters, BatchNorm buffers, the confusion matrix and the optimizer's state"""
        tensors = [self.net._arena.flat] + list(self.net.buffers()) + ([self.confusion] if self.confusion is not None else [])
        return tensors, [t.clone() for t in tensors], self.opt.snapshot_flat_state(self.net)

    def _restore(self, saved):
        tensors, clones, opt_state = saved
        for t, t0 in zip(tensors, clones):
            t.copy_(t0)
        self.opt.restore_flat_state(self.net, opt_state)     # the optimizer keeps what it carried (e.g. a resumed checkpoint)

    def _copy_inputs(self, *inputs):
        """one per name of INPUTS; None, or an input the step does not hold, leaves what is held"""
        if len(inputs) != len(self.INPUTS):
            raise TypeError("%s is called with (%s) or with nothing" % (type(self).__name__, ", ".join(self.INPUTS)))
        for name, t in zip(self.INPUTS, inputs):
            held = getattr(self, name)
            if held is not None and t is not None:
                held.copy_(t, non_blocking=True)

    def _eager_body(self, include_opt):
        logits = self.net(self.a, self.b)
        self.logits = logits.detach()          # static output buffer of the graph: valid after every replay
        self.opt.zero_grad()
        loss = losses.focal_loss(logits, self.lab)
        loss.backward()
        self._count(self.logits)
        if include_opt:
            self.opt.step()
        return loss.detach()

    def _engine_pass(self, backward):
        """forward, loss, zero_grad and `backward(dloss/dlogits, saved)` at engine level (no autograd graph): the same kernels
        as `_eager_body` minus what autograd adds around them -- the fill of the upstream gradient 1.0, the pass that scales
        dloss/dlogits by it and the copies at its boundary (34 MB per step at batch 32)"""
        net = self.net
        logits = self._forward_split()
        bwd = net._engine.take_backward()
        self.logits = logits
        loss, dl = self._loss_and_grad(logits)
        self._count(logits)
        net._arena.grad.zero_()
        backward(dl, bwd)
        net._bind_grad_views()           # the optimizer skips parameters without a .grad, as torch does
        return loss

    def _body(self, include_opt):
        """the one-graph step: `_engine_pass` with the whole backward for an ENGINE_LEVEL class, the autograd step
        `_eager_body` otherwise"""
        if not self.ENGINE_LEVEL:
            return self._eager_body(include_opt)
        loss = self._engine_pass(self.net._engine.backward)
        if include_opt:
            self.opt.step()
        return loss

    def _forward_split(self):
        return self.net._run_forward(self.a, self.b, need_grad=True)

    def _loss_and_grad(self, logits):
        """(loss, dloss/dlogits) at engine level (no autograd graph): focal loss of the BiT / DAHiTra trainers"""
        tgt = self.lab[:, 0] if self.lab.dim() == logits.dim() else self.lab
        return ops.focal_loss(logits, tgt.to(torch.int64).contiguous(), want_grad=True)

    def _count(self, logits):
        if self.confusion is not None:
            tgt = self.lab[:, 0] if self.lab.dim() == logits.dim() else self.lab
            ops.confusion_matrix(logits, tgt.to(torch.int64).contiguous(), self.confusion)

    # ---- overlapped form ------------------------------------------------------------------------------
    def _can_split(self):
        """the net's backward has a split point and every gradient the second graph writes (bit: stem, layer1, layer2; unet /
        xbd: the whole trunk) lies below the first offset of what the first graph completes: the arena tail [split, end) is
        final after the first graph.  Keys below the split that the first graph writes (positional embeddings are registered
        first) just ride with the second all-reduce."""
        self.split_off = parallel.split_offset(self.net, self.world)
        return self.split_off is not None

    def _split_first(self):
        """graph 1: forward, loss and the first part of the backward (every class, ENGINE_LEVEL or not)"""
        return self._engine_pass(self.net._engine.backward_first)

    def _second(self):
        """graph 2 (layer2 / layer1 / stem backward) replays WHILE the all-reduce of the arena tail runs on RCCL's stream: its
        BatchNorm backward must not be the persistent one-launch form, whose device-wide barrier needs every CU"""
        with ops.no_persist_bn():
            self.net._engine.backward_second()

    def _replay_overlapped(self):
        _, grad = self.net.flat_params()
        self.graph.replay()
        w1 = dist.all_reduce(grad[self.split_off:], op=dist.ReduceOp.SUM, async_op=True)      # waits for graph 1 only
        self.graph2.replay()                                                                  # ... while this runs
        w2 = dist.all_reduce(grad[:self.split_off], op=dist.ReduceOp.SUM, async_op=True)
        w1.wait()
        w2.wait()
        self._update()

    def _update(self):
        """world > 1, after the all-reduces have landed: the (eager) parameter update"""
        self.opt.step()

    def __call__(self, *inputs):
        if self.stale():
            raise RuntimeError("dahitra_amd: the net's parameter arena was rebuilt (moved to another device / "
                               "parameters replaced) after this step was captured; build a new %s" % type(self).__name__)
        if inputs and inputs[0] is not None:
            self._copy_inputs(*inputs)
        self._calls += 1
        if self._calls in (2, 8) or self._calls % self.CHECK_EVERY == 0:
            # the persistent BatchNorm backward's device-wide barrier: a timeout (bit 0) or a non-finite sum (bit 1) of any
            # replay since the last check raises here (one 4-byte read-back per sync block: a host sync, hence not per step)
            ops.bn_persist_check(self.a.device)
        self.opt.sync_hyper(1.0 / self.world)
        if self.split_off is not None:
            self._replay_overlapped()
            return self.loss
        self.graph.replay()
        if self.exchange:      # the exchange step and the update run eagerly after the replayed forward / backward
            parallel.allreduce_net_grads_(self.net)
            self._update()
        return self.loss


class _RecordedEval(_Recorded):
    """What the recorded evaluation steps below share: how an eval-mode body becomes one HIP graph (`_record`) and what a replay
    refuses (`_guard`).  A subclass holds its static buffers, its `_body`, its input copy and its shape check."""
    _word = "evaluation"                                  # "... after this <word> step was captured"
    _whose, _eval_call = "the net's", "net.eval()"

    def _record(self, nets, device, body, accumulators=(), warmup=2):
        """net.eval() on every net, `warmup` eager bodies on a side stream, then `body()` captured into self.graph; returns what
        the captured body returned (its static output).  accumulators: the tensors the body adds to (None entries are skipped);
        they are as they were before, since neither the warm-up nor the capture is part of any count."""
        for net in nets:
            net.eval()
            net._ensure_arena(device)
        self._accumulators = [t for t in accumulators if t is not None]
        return self._capture(nets, device, body, [body], warmup)[0]

    def _snapshot(self):
        return [t.clone() for t in self._accumulators]

    def _restore(self, saved):
        for t, t0 in zip(self._accumulators, saved):
            t.copy_(t0)

    def _guard(self):
        """what every replay refuses: a rebuilt arena (the graph holds the old one's addresses) and a net in train mode"""
        name = type(self).__name__
        if self.stale():
            raise RuntimeError("dahitra_amd: %s parameter arena was rebuilt after this %s step was captured; build a new %s"
                               % (self._whose, self._word, name))
        if any(net.training for net in self._nets):
            raise RuntimeError("dahitra_amd: %s replays the eval-mode forward; call %s (a train-mode forward in between re-packs "
                               "the weights for training)" % (name, self._eval_call))


class GraphedEvalStep(_RecordedEval):
    """The evaluation forward (models/evaluator.py:156-164: net.eval(), no gradient state) as ONE HIP graph: the eval-mode weight
    re-pack (every BatchNorm folded into its convolution), the forward and -- with `confusion` -- the arg-max + confusion-matrix
    count against the labels (one kernel, no host read).  ~130 (BiT) / ~200 (DAHiTra) launches per batch become one
    hipGraphLaunch: the eager evaluation forward of DAHiTra proper is bound by its launches from Python.

        step = GraphedEvalStep(net, a, b, lab, confusion)      # net.eval() is called here
        logits = step(a, b, lab)                                # static shapes; the caller runs other shapes eagerly

    The parameters are read when the graph replays, so a checkpoint loaded into `net` afterwards is what the next replay scores."""

    def __init__(self, net, a, b, lab=None, confusion=None, warmup=2):
        self.net, self.confusion = net, confusion
        self.a, self.b = a.clone(), b.clone()
        self.lab = lab.clone() if lab is not None else None
        if confusion is not None and lab is None:
            raise ValueError("GraphedEvalStep: a confusion matrix needs the labels")
        self.logits = self._record([net], a.device, self._body, (confusion,), warmup)

    def _body(self):
        with torch.no_grad():
            logits = self.net(self.a, self.b)
        if self.confusion is not None:
            tgt = self.lab[:, 0] if self.lab.dim() == logits.dim() else self.lab
            ops.confusion_matrix(logits.detach().float().contiguous(), tgt.to(torch.int64).contiguous(), self.confusion)
        return logits

    def __call__(self, a=None, b=None, lab=None):
        self._guard()
        if a is not None:
            self.a.copy_(a, non_blocking=True)
            self.b.copy_(b, non_blocking=True)
            if lab is not None and self.lab is not None:
                self.lab.copy_(lab, non_blocking=True)
        self.graph.replay()
        return self.logits


def tile_chunk(P, cap=16):
    """the default number of views per forward of a tile: the largest divisor of P up to `cap` (16 of 16 views, 7 of 49, 14 of
    196; measured on newUNetTrans in bf16: 7 views per forward deliver 9.4 k views/s, 14 deliver 15.4 k, 16 deliver 17.8 k --
    larger chunks are not measured, pass `chunk` to try them)"""
    return max(c for c in range(1, min(P, cap) + 1) if P % c == 0)


class TileBuffers:
    """The static tensors of one tile's pass: the index of the source pair (device int32), the P cut views, the net's
    [P, C, h, w] answers and what comes out of them.  GraphedTileStep records `run()`; models.tiles runs the same method eagerly,
    so both paths make the same launches."""

    def __init__(self, net, pipe, plan, confusion=None, chunk=None):
        dev = pipe.a.device
        S, H, W, _ = pipe.a.shape
        if (plan.H, plan.W) != (H, W):
            raise ValueError("tile step: the plan is for %dx%d tiles, the pipeline holds %dx%d" % (plan.H, plan.W, H, W))
        P, h, w = plan.P, plan.h, plan.w
        chunk = tile_chunk(P) if chunk is None else int(chunk)
        if chunk < 1 or P % chunk:
            raise ValueError("tile step: chunk %d does not divide the %d views of %r" % (chunk, P, plan))
        self.net, self.pipe, self.plan, self.chunk, self.confusion = net, pipe, plan, chunk, confusion
        self.index = torch.zeros(1, dtype=torch.int32, device=dev)
        self.views = {'A': torch.empty(P, 3, h, w, dtype=torch.float32, device=dev),
                      'B': torch.empty(P, 3, h, w, dtype=torch.float32, device=dev),
                      'L': torch.empty(P, 1, h, w, dtype=torch.uint8, device=dev)}
        self.view_logits = self.mask = self.logits = None          # allocated by the first run(), which learns C from the net

    def _allocate(self, C):
        dev, plan = self.index.device, self.plan
        want = (C, C) if plan.stitchable else (plan.P, C, C)
        cf = self.confusion
        if cf is not None and (tuple(cf.shape) != want or cf.dtype != torch.int64 or cf.device != dev or not cf.is_contiguous()):
            raise ValueError("tile step: confusion %s %s is not a contiguous int64 %s on %s for %r"
                             % (tuple(cf.shape), cf.dtype, list(want), dev, plan))
        if not plan.stitchable and cf is None:
            raise ValueError("tile step: %r only counts per view; give it a confusion buffer [%d, C, C]" % (plan, plan.P))
        self.view_logits = torch.empty(plan.P, C, plan.h, plan.w, dtype=torch.float32, device=dev)
        if plan.stitchable:
            self.mask = torch.empty(plan.H, plan.W, dtype=torch.uint8, device=dev)
            self.logits = torch.empty(C, plan.H, plan.W, dtype=torch.float32, device=dev)

    def aim(self, index):
        """name the source pair of the next run (range-checked here, on the host; one fill launch, no read)"""
        if not 0 <= int(index) < len(self.pipe):
            raise ValueError("tile step: pair %d of %d" % (index, len(self.pipe)))
        self.index.fill_(int(index))

    def run(self):
        """cut the views of the pair `index` names, the eval-mode forward in chunks, then the stitch or the per-view counts"""
        plan, v = self.plan, self.views
        self.pipe.window_batch(self.index, plan, out=v)
        with torch.no_grad():
            for s in range(0, plan.P, self.chunk):
                y = self.net(v['A'][s:s + self.chunk], v['B'][s:s + self.chunk])
                if self.view_logits is None:
                    self._allocate(y.shape[1])
                want = (self.chunk,) + tuple(self.view_logits.shape[1:])
                if tuple(y.shape) != want:                     # copy_ would broadcast a smaller answer over the chunk
                    raise ValueError("tile step: the net answered %s to %d views, the step holds %s" % (tuple(y.shape), self.chunk, list(want)))
                self.view_logits[s:s + self.chunk].copy_(y)
        if plan.stitchable:
            if self.confusion is None:
                ops.cd_tile_stitch(self.view_logits, plan, out_logits=self.logits, out_mask=self.mask)
            else:
                ops.cd_tile_stitch(self.view_logits, plan, out_logits=self.logits, out_mask=self.mask, label=self.pipe.l,
                                   counts=self.confusion, label_index=self.index)
        else:
            ops.cd_view_counts(self.view_logits, v['L'], self.confusion)
        return self.mask, self.logits


class GraphedTileStep(_RecordedEval):
    """The change map of one whole tile as ONE HIP graph: dh_augment_pairs_u8 cuts the P views of `plan` (tiles.TilePlan) from
    the pair a static device index names, the eval-mode forward runs over them in chunks of `chunk` views (back to back, into
    one [P, C, h, w] buffer), and dh_cd_tile_stitch blends the answers into the [H, W] class map and [C, H, W] logits -- or, for
    a TilePlan.eval_cd plan, dh_cd_view_counts counts the sixteen views against their own labels.  A tile is 16 to 196 eager
    forwards otherwise, each bound by its launches from Python.

        step = GraphedTileStep(net, pipe, plan)               # net.eval() is called here
        mask, logits = step.step(index)                       # the static tensors, valid until the next replay

    confusion: int64 [C, C] (stitchable plan: the stitched map against the tile's own label plane, accumulated) or [P, C, C]
    (eval_cd plan, required).  chunk: views per forward, a divisor of P (default: the largest up to 16).  Another tile is another
    value of the device index, not another recording.  The parameters are read when the graph replays."""
    _word = "tile"

    def __init__(self, net, pipe, plan, confusion=None, chunk=None, warmup=2):
        self.net = net
        self.buf = TileBuffers(net, pipe, plan, confusion, chunk)
        self._record([net], pipe.a.device, self.buf.run, (confusion,), warmup)

    def step(self, index):
        self._guard()
        self.buf.aim(index)
        self.graph.replay()
        return self.buf.mask, self.buf.logits

    __call__ = step


class _RecordedXbdBatch(_RecordedEval):
    """The static batch of the two validation steps: imgs, channel 0 of msk and lbl_msk, checked and copied by every call"""
    classes = 4          # damage classes: a four-dimensional msk has classes + 1 channels

    def _hold(self, imgs, msk, lbl_msk):
        self._check(imgs, msk, lbl_msk, tuple(imgs.shape))
        self.imgs = imgs.clone()
        self.msk0 = self._plane0(msk).to(torch.uint8).contiguous().clone()
        self.lbl = lbl_msk.to(torch.uint8).contiguous().clone()

    @staticmethod
    def _plane0(msk):
        return msk[:, 0] if msk.dim() == 4 else msk

    def _check(self, imgs, msk, lbl_msk, want):
        """`want`: the [B, 6, H, W] the step holds.  Every tensor must have exactly its shape: copy_ would broadcast a [1, ...]
        batch over the static buffer and score one image B times."""
        name = type(self).__name__
        B, _, H, W = want
        if imgs.dim() != 4 or imgs.shape[1] != 6 or tuple(imgs.shape) != tuple(want):
            raise ValueError("%s: imgs %s, the step holds [%d, 6, %d, %d]" % (name, tuple(imgs.shape), B, H, W))
        C = self.classes + 1
        if tuple(msk.shape) not in ((B, C, H, W), (B, H, W)):
            raise ValueError("%s: msk %s is neither [%d, %d, %d, %d] nor its channel 0" % (name, tuple(msk.shape), B, C, H, W))
        if tuple(lbl_msk.shape) != (B, H, W):
            raise ValueError("%s: lbl_msk %s, the step holds [%d, %d, %d]" % (name, tuple(lbl_msk.shape), B, H, W))

    def __call__(self, imgs=None, msk=None, lbl_msk=None):
        self._guard()
        if imgs is not None:
            if msk is None or lbl_msk is None:
                raise ValueError("%s: a batch is imgs, msk and lbl_msk" % type(self).__name__)
            self._check(imgs, msk, lbl_msk, tuple(self.imgs.shape))
            self.imgs.copy_(imgs, non_blocking=True)
            self.msk0.copy_(self._plane0(msk), non_blocking=True)
            self.lbl.copy_(lbl_msk, non_blocking=True)
        self.graph.replay()
        return self.logits


class GraphedXbdEvalStep(_RecordedXbdBatch):
    """One validation batch of the xBD loop (xBD_code/train.py:259-279) as ONE HIP graph: the eval-mode weight re-pack, the
    forward of the 6-channel model and dh_xbd_val_count on its logits -- sigmoid, threshold, arg-max and the tp / fn / fp and
    dice counts, no host read.

        step = GraphedXbdEvalStep(net, imgs, msk, lbl_msk, class_counts)      # net.eval() is called here
        logits = step(imgs, msk, lbl_msk)          # class_counts accumulated; step.image_counts [B, 3] holds the batch's rows

    msk is the loader's [B, 5, H, W] mask or its channel 0 ([B, H, W]); only channel 0 is kept.  The shapes are static and
    CHECKED: a batch of another shape (the ragged last one of an epoch) raises ValueError and goes through the eager path
    (models/xbd.validate does that); nothing is broadcast.  The parameters are read when the graph replays.
    classes: the damage classes, 4 (default) or 3 -- the four-output net of xBD_code/train_adapt.py, whose pass
    (lines 262-280) counts three: msk is then [B, 4, H, W] and class_counts [3, 3] (ops.xbd_val_count's `classes`)."""

    def __init__(self, net, imgs, msk, lbl_msk, class_counts, thr=0.3, select='reference', warmup=2, classes=4):
        if classes not in ops.XBD_VAL_CLASSES:
            raise ValueError("GraphedXbdEvalStep: classes %r is not one of %s" % (classes, list(ops.XBD_VAL_CLASSES)))
        self.classes = classes
        self.net, self.class_counts, self.thr, self.select = net, class_counts, float(thr), select
        self._hold(imgs, msk, lbl_msk)
        self.image_counts = torch.zeros(imgs.shape[0], 3, dtype=torch.int64, device=imgs.device)
        self.logits = self._record([net], imgs.device, self._body, (class_counts,), warmup)

    def _body(self):
        with torch.no_grad():
            logits = self.net(self.imgs)
        logits = logits.float()
        ops.xbd_val_count(logits, self.msk0, self.lbl, self.image_counts, self.class_counts, self.thr, self.select, self.classes)
        return logits


class GraphedXbdSweepStep(_RecordedXbdBatch):
    """GraphedXbdEvalStep for a whole grid of localisation thresholds: the eval-mode weight re-pack, the forward and
    dh_xbd_val_sweep on its logits as ONE HIP graph -- the batch's histograms over (threshold bin, damage arg-max, truth), from
    which models/xbd.sweep_counts gives the counts of every threshold of the grid; no host read.

        step = GraphedXbdSweepStep(net, imgs, msk, lbl_msk, class_hist, thresholds)      # net.eval() is called here
        logits = step(imgs, msk, lbl_msk)      # class_hist [T + 1, 4, 5] accumulated; step.image_hist [B, T + 1, 4, 2]: the batch's

    thresholds: 1 .. ops.XBD_SWEEP_MAX floats, ascending inside (0, 1); the graph's kernel node holds them by value.  Shapes are
    static and CHECKED as GraphedXbdEvalStep checks them: another shape raises ValueError, nothing is broadcast.  The parameters
    are read when the graph replays."""
    _word = "sweep"

    def __init__(self, net, imgs, msk, lbl_msk, class_hist, thresholds, select='reference', warmup=2):
        self.net, self.class_hist, self.select = net, class_hist, select
        self.thresholds = ops.xbd_sweep_thresholds(thresholds, "GraphedXbdSweepStep")
        self._hold(imgs, msk, lbl_msk)
        self.image_hist = torch.zeros(imgs.shape[0], self.thresholds.size + 1, 4, 2, dtype=torch.int64, device=imgs.device)
        self.logits = self._record([net], imgs.device, self._body, (class_hist,), warmup)

    def _body(self):
        with torch.no_grad():
            logits = self.net(self.imgs)
        logits = logits.float()
        ops.xbd_val_sweep(logits, self.msk0, self.lbl, self.image_hist, self.class_hist, self.thresholds, self.select)
        return logits


class _RecordedXbdPair(_RecordedEval):
    """The static pre / post pair of the two prediction steps and their [N, H, W, 5] answer: checked and copied by every call"""

    def _hold(self, pre_u8, post_u8):
        self.pre, self.post = pre_u8.clone(), post_u8.clone()
        N, H, W, _ = pre_u8.shape
        self.out = torch.empty(N, H, W, 5, dtype=torch.uint8, device=pre_u8.device)

    def _check(self, pre_u8, post_u8):
        want = tuple(self.pre.shape)
        for name, t in (("pre_u8", pre_u8), ("post_u8", post_u8)):
            if not torch.is_tensor(t) or tuple(t.shape) != want or t.dtype != torch.uint8 or t.device != self.pre.device:
                raise ValueError("%s: %s %s %s, the step holds uint8 %s on %s" % (
                    type(self).__name__, name, tuple(getattr(t, "shape", ())), getattr(t, "dtype", type(t)), list(want), self.pre.device))

    def step(self, pre_u8=None, post_u8=None):
        self._guard()
        if pre_u8 is not None or post_u8 is not None:
            self._check(pre_u8, post_u8)
            self.pre.copy_(pre_u8, non_blocking=True)
            self.post.copy_(post_u8, non_blocking=True)
        self.graph.replay()
        return self.out

    __call__ = step


class GraphedXbdPredictStep(_RecordedXbdPair):
    """The prediction of one batch of pre / post pairs (xBD_code/predict_test_cls.py:62-94) as ONE HIP graph:
    dh_xbd_tta_pack_u8 (the four flips of the normalised 6-channel image), the eval-mode forward at batch 4N and
    dh_xbd_tta_merge_u8 (sigmoid, un-flip, float32 mean, uint8), no host read.

        step = GraphedXbdPredictStep(net, pre_u8, post_u8)      # net.eval() is called here
        msk = step(pre_u8, post_u8)                             # the static [N, H, W, 5] uint8 tensor, valid until the next replay

    pre_u8, post_u8 [N, H, W, 3] uint8 on the device.  order: 'bgr' (default, the script as executed) or 'rgb', see
    ops.xbd_tta_pack.  The shapes are static and CHECKED: a pair of another shape raises ValueError, nothing is broadcast.  The
    parameters are read when the graph replays."""
    _word = "prediction"

    def __init__(self, net, pre_u8, post_u8, order='bgr', warmup=2):
        self.net, self.order = net, order
        self.inp = ops.xbd_tta_pack(pre_u8, post_u8, order)          # validates the pair; the static input of the forward
        self._hold(pre_u8, post_u8)
        self.logits = self._record([net], pre_u8.device, self._body, warmup=warmup)

    def _body(self):
        ops.xbd_tta_pack(self.pre, self.post, self.order, out=self.inp)
        with torch.no_grad():
            logits = self.net(self.inp)
        logits = logits.float().contiguous()
        ops.xbd_tta_merge(logits, out=self.out)
        return logits


class GraphedXbdEnsembleStep(_RecordedXbdPair):
    """GraphedXbdPredictStep for a list of snapshots and 4 or 8 views (xBD_code/predict_test_cls.py:38-55, 81-91) as ONE HIP
    graph: dh_xbd_tta_pack_views_u8 once, the eval-mode forward of every net at batch views * N on that one static input, and
    dh_xbd_tta_merge_multi_u8 (sigmoid, un-view, the float32 mean over models and views in the script's order, uint8).

        step = GraphedXbdEnsembleStep([net_a, net_b], pre_u8, post_u8, views=8)      # net.eval() is called on each
        msk = step(pre_u8, post_u8)                             # the static [N, H, W, 5] uint8 tensor, valid until the next replay

    All nets are on the device of pre_u8; the same net may appear twice (the script's behaviour for a repeated snapshot).  The
    shapes are static and CHECKED: a pair of another shape raises ValueError, nothing is broadcast.  The parameters are read
    when the graph replays."""
    _word = "ensemble"
    _whose, _eval_call = "a net's", "net.eval() on every net"

    def __init__(self, nets, pre_u8, post_u8, order='bgr', views=4, warmup=2):
        if not isinstance(nets, (list, tuple)) or not 1 <= len(nets) <= ops.XBD_TTA_MAX_MODELS:
            raise ValueError("GraphedXbdEnsembleStep: nets is not a list of 1 .. %d models" % ops.XBD_TTA_MAX_MODELS)
        self.nets, self.order, self.views = list(nets), order, views
        self.inp = ops.xbd_tta_pack_views(pre_u8, post_u8, order, views)      # validates the pair; the static input of the forwards
        for net in self.nets:
            if next(net.parameters()).device != pre_u8.device:
                raise ValueError("GraphedXbdEnsembleStep: a net is on %s, the pair on %s" % (next(net.parameters()).device, pre_u8.device))
        self._hold(pre_u8, post_u8)
        self.logits = self._record(self.nets, pre_u8.device, self._body, warmup=warmup)

    def _body(self):
        ops.xbd_tta_pack_views(self.pre, self.post, self.order, self.views, out=self.inp)
        logits = []
        with torch.no_grad():
            for net in self.nets:
                logits.append(net(self.inp).float().contiguous())
        ops.xbd_tta_merge_multi(logits, self.views, out=self.out)
        return logits


class GraphedXbdStep(GraphedTrainStep):
    """The xBD step (xBD_code/train.py:331-374) as one HIP graph: forward of the 6-channel model, the five weighted
    ComboLoss terms, backward, clip_grad_norm_(0.999) and the hand-rolled AdamW.

        step = GraphedXbdStep(net, xbd.AdamW(net.parameters(), lr=1e-4, weight_decay=1e-6, capturable=True), imgs, msks)
        loss = step(imgs, msks)"""
    INPUTS = ("a", "lab")          # imgs, msks
    ENGINE_LEVEL = False           # the one-graph form records the autograd step, clip_grad_norm_ included

    def __init__(self, net, opt, imgs, msks, max_norm=0.999, warmup=3):
        self.max_norm = max_norm
        self._build(net, opt, (imgs, msks), warmup)

    def _eager_body(self, include_opt):
        from .models import xbd
        self.net.zero_grad()
        logits = self.net(self.a)
        self.logits = logits.detach()
        loss = xbd.xbd_loss(logits, self.lab)
        loss.backward()
        if include_opt:
            xbd.clip_grad_norm_(self.net.parameters(), self.max_norm)
            self.opt.step()
        return loss.detach()

    def _forward_split(self):
        x = self.a
        return self.net._run_forward(x[:, :3], x[:, 3:], need_grad=True)

    def _loss_and_grad(self, logits):
        """the five weighted ComboLoss terms and their gradient at engine level (xBD_code/train.py:348-353)"""
        from .models import xbd
        w = xbd.channel_weights_dev(logits.device)
        lo, ms = logits.float().contiguous(), self.lab.float().contiguous()
        loss, _, sums = ops.combo_loss_fwd(lo, ms, w, 1.0, 8.0)
        one = self._one if getattr(self, "_one", None) is not None else torch.ones(1, dtype=torch.float32, device=lo.device)
        self._one = one
        return loss, ops.combo_loss_bwd(lo, ms, sums, w, one, 1.0, 8.0)

    def _update(self):
        """mean over the ranks, clip_grad_norm_(max_norm) over the WHOLE (now complete) arena where the step clips, then the
        hand-rolled AdamW: the clip needs the total norm, so it cannot start before both all-reduces have landed
        (train.py:373-374)"""
        from .models import xbd
        if self._inv_world is not None:
            _, grad = self.net.flat_params()
            ops.scale_into(grad, self._inv_world, grad)
        if self.max_norm is not None:
            xbd.clip_grad_norm_(self.net.parameters(), self.max_norm)
        self.opt.step()


class _GraphedXbdScriptStep(GraphedXbdStep):
    """What the recorded steps of the two training scripts share: the check of imgs / msks (/ lbl_msk), the loss weights made
    before the capture, `parts`, and the script's loss at engine level.  A subclass names its row of ops._XBD_LOSS_FORMS in
    `_form` and gives `_eager_step(update)` -> (logits, loss, parts)."""
    ENGINE_LEVEL = True
    _form = None
    lbl = labels = None                   # what the loss pair takes where the form has no lbl

    def _build_script(self, what, net, opt, imgs, msks, lbl_msk, weights_dev, ce_scale, warmup):
        channels = ops._XBD_LOSS_FORMS[self._form][0]
        a = ops._Args(what, cpu_error=True)
        B, _, H, W = a.tensor("imgs", imgs, torch.float32, lambda t: t.dim() == 4 and t.shape[1] == 6 and t.numel() > 0,
                              "[B, 6, H, W], not empty").shape
        a.tensor("msks", msks, torch.uint8, (B, channels, H, W), "[%d, %d, %d, %d] like imgs" % (B, channels, H, W))
        if lbl_msk is not None:
            a.tensor("lbl_msk", lbl_msk, torch.uint8, (B, H, W), "[%d, %d, %d] like imgs" % (B, H, W))
        a.placed()
        self.parts, self._ce_scale = None, ce_scale
        self._w = weights_dev(imgs.device)        # made here: no host-to-device copy inside the capture
        self._build(net, opt, (imgs, msks, lbl_msk), warmup)          # one per name of INPUTS: a step without "lbl" holds two

    def _eager_body(self, include_opt):
        self.logits, loss, self.parts = self._eager_step(include_opt)
        return loss

    def _loss_and_grad(self, logits):
        """the script's loss and its gradient at engine level: two launches forward, one backward, the masks read as bytes"""
        lo, label = logits.float().contiguous(), (self.lbl, self.labels)
        loss, self.parts, sums = ops._xbd_loss_fwd(self._form, lo, self.lab, *label, self._w, 1.0, 8.0, self._ce_scale)
        return loss, ops._xbd_loss_bwd(self._form, lo, self.lab, *label, sums, self._w, None, 1.0, 8.0, self._ce_scale)


class GraphedXbdUnetStep(_GraphedXbdScriptStep):
    """The step of xBD_code/train_unettransformer.py:436-481, the script that trains DAHiTra proper, as one HIP graph: forward of
    the 6-channel model, its loss (models/xbd.unet_loss: five ComboLoss terms weighted 0.1, 0.1, 0.6, 0.3, 1 plus 8 * the
    class-weighted cross-entropy of the masked logits) at engine level, backward, NO gradient clip (commented out at line 480)
    and the hand-rolled AdamW.  msks are the loader's uint8 bytes and stay bytes: the loss kernels read them as they lie.

        step = GraphedXbdUnetStep(net, xbd.AdamW(net.parameters(), lr=1e-4, weight_decay=1e-6, capturable=True), imgs, msks, lbl_msk)
        loss = step(imgs, msks, lbl_msk)          # step.parts: the static [8] tensor of ops.XBD_UNET_PARTS, valid after every replay

    labels: 'lbl_msk' (the script as executed; lbl_msk uint8 [B, H, W] is needed) or 'damage' (the label is derived from msks in
    the kernel; lbl_msk is neither kept nor copied).  A scheduler's learning rate reaches the replay through opt.sync_hyper, as in
    the parent.  ValueError for a label mode, dtype or shape that does not fit, before anything is recorded."""
    INPUTS = ("a", "lab", "lbl")          # imgs, msks, lbl_msk (lbl is None under labels='damage')
    _form = "unet"
    max_norm = None                       # the script does not clip

    def __init__(self, net, opt, imgs, msks, lbl_msk=None, labels='lbl_msk', warmup=3):
        from .models import xbd
        what = "GraphedXbdUnetStep"
        if labels not in ops.XBD_UNET_LABELS:
            raise ValueError("%s: labels %r is not one of %s" % (what, labels, sorted(ops.XBD_UNET_LABELS)))
        if labels == 'lbl_msk' and lbl_msk is None:
            raise ValueError("%s: labels='lbl_msk' reads lbl_msk, which is None" % what)
        self.labels = labels
        self._build_script(what, net, opt, imgs, msks, lbl_msk if labels == 'lbl_msk' else None, xbd.unet_weights_dev,
                           xbd.UNET_CE_SCALE, warmup)

    def __call__(self, imgs=None, msks=None, lbl_msk=None):
        return super().__call__(imgs, msks, lbl_msk)

    def _eager_step(self, update):
        from .models import xbd
        return xbd.unet_eager_step(self.net, self.opt, self.a, self.lab, self.lbl, self.labels, update=update)


class GraphedXbdAdaptStep(_GraphedXbdScriptStep):
    """The step of xBD_code/train_adapt.py:326-347, the Ida-BD adaptation of the FOUR-output DAHiTra, as one HIP graph: forward of
    the 6-channel model, its loss (models/xbd.adapt_loss: four ComboLoss terms weighted 0.1, 0.8, 2, 8 plus 5 * the class-weighted
    cross-entropy of the raw logits) at engine level, backward, clip_grad_norm_(0.999) (line 346) and the hand-rolled AdamW.
    msks are the loader's uint8 bytes [B, 4, H, W] (GpuXbdPipeline.make_adapt_batch) and stay bytes.

        step = GraphedXbdAdaptStep(net, xbd.AdamW(net.parameters(), lr=1e-4, weight_decay=1e-7, capturable=True), imgs, msks)
        loss = step(imgs, msks)          # step.parts: the static [6] tensor of ops.XBD_ADAPT_PARTS, valid after every replay

    step() without arguments replays on the inputs the step holds.  With torch.distributed the parent's forms apply: the mean over
    the ranks, then the clip over the complete arena, then the update.  A scheduler's learning rate reaches the replay through
    opt.sync_hyper, as in the parent.  ValueError for a dtype or shape that does not fit, before anything is recorded."""
    INPUTS = ("a", "lab")          # imgs, msks
    _form = "adapt"

    def __init__(self, net, opt, imgs, msks, max_norm=0.999, warmup=3):
        from .models import xbd
        self.max_norm = max_norm
        self._build_script("GraphedXbdAdaptStep", net, opt, imgs, msks, None, xbd.adapt_weights_dev, xbd.ADAPT_CE_SCALE, warmup)

    def __call__(self, imgs=None, msks=None):
        return super().__call__(imgs, msks)

    def _body(self, include_opt):
        """the one-graph step: the engine-level pass, then (single process) the clip and the update"""
        loss = self._engine_pass(self.net._engine.backward)
        if include_opt:
            self._update()
        return loss

    def _eager_step(self, update):
        from .models import xbd
        return xbd.adapt_eager_step(self.net, self.opt, self.a, self.lab, self.max_norm, update=update)
