"""Whole-tile change maps on the MI355X: dh_cd_tile_stitch and dh_cd_view_counts (csrc/cd_tile.hip) through ops against the numpy
restatement (tests/_cd_tile_cases.py), bit for bit; then GpuPairPipeline.window_batch, graph.GraphedTileStep and
models/tiles.predict_tile / predict_tiles / evaluate_tiles on mosaics of the four shipped LEVIR pairs."""
import os
import types

import numpy as np
import pytest
import torch

import _cd_tile_cases as T
import cdnet_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAME = "base_transformer_pos_s4"
SENTINEL = 0xA5
ALIGNED = (2, 32, 48, (16, 16), (8, 8), (0, 1, 2, 3), "triangle")          # x_align 4, cover up to 2 x 2 x 4: the quad form, small


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def offset_view(a, offset_bytes):
    """a device copy of `a` that starts `offset_bytes` into a larger buffer of sentinel bytes"""
    buf = torch.full((a.nbytes + 64,), SENTINEL, dtype=torch.uint8, device=DEV)
    view = buf[offset_bytes:offset_bytes + a.nbytes].view(torch.from_numpy(a).dtype).view(a.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return view


@pytest.fixture(scope="module")
def cases():
    """per shape: the plan, random logits and the restatement's (out, mask), computed once and left unchanged"""
    out = {}
    for name, case in dict(T.SHAPES, aligned=ALIGNED).items():
        plan = T.make_plan(case)
        lg = T.random_logits(plan, case[0], seed=len(name))
        want = T.stitch(lg, plan)[0]
        out[name] = (plan, lg, want, T.first_max(want))
    return out


# ---- 1. the stitch kernel against the restatement, bit for bit -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd", "identity", "maxc", "big", "loop"])
def test_stitch_equals_the_restatement_bit_for_bit(cases, name):
    from dahitra_amd import ops
    plan, lg, want, want_mask = cases[name]
    assert plan.P == {"odd": 64, "identity": 6, "maxc": 64, "big": 196, "loop": 80}[name]
    mask, out = ops.cd_tile_stitch(dev(lg), plan)
    assert out.shape == want.shape and out.dtype == torch.float32 and mask.shape == want_mask.shape and mask.dtype == torch.uint8
    assert np.array_equal(bits(out), bits(want))
    assert np.array_equal(mask.cpu().numpy(), want_mask)
    if name == "identity":
        for iy in range(plan.ny):
            for ix in range(plan.nx):
                got = out[:, 32 * iy:32 * iy + 32, 32 * ix:32 * ix + 32]
                assert np.array_equal(bits(got), bits(lg[iy * plan.nx + ix])), "output bits are the input bits"
    if name == "loop":
        assert plan.x_align() == 4 and plan.H * plan.W // 4 > 2048 * 256, "the quad form's grid-stride loop takes a second pass"
    if name == "big":
        # one element into a larger buffer: the pixel-by-pixel form, whose 4096 workgroups' worth of pixels go through the
        # grid-stride loop of 2048
        mask1, out1 = ops.cd_tile_stitch(offset_view(lg, 4), plan)
        assert torch.equal(mask1, mask) and np.array_equal(bits(out1), bits(want))


# ---- 2. planted ties and NaNs --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd", "maxc", "aligned"])
def test_planted_ties_and_nans_give_argmax_nchws_class(cases, name):
    from dahitra_amd import ops
    plan, lg, _, _ = cases[name]
    lg = T.plant(lg, plan, seed=21)
    want = T.stitch(lg, plan)[0]
    top = np.nanmax(np.where(np.isnan(want), -np.inf, want), axis=0)
    assert ((want == top).sum(axis=0) > 1).mean() > 0.1 and np.isnan(want).any(axis=0).mean() > 0.01, "ties and NaNs decide many pixels"
    mask, out = ops.cd_tile_stitch(dev(lg), plan)
    assert np.array_equal(bits(out), bits(want)) and np.array_equal(mask.cpu().numpy(), T.first_max(want))
    assert torch.equal(mask.to(torch.int64), ops.argmax_nchw(out[None].contiguous())[0]), "mask == argmax(out) everywhere"


# ---- 3. unaligned base pointers ------------------------------------------------------------------------------------------------
def test_unaligned_pointers_give_the_aligned_result(cases):
    from dahitra_amd import ops
    plan, lg, want, want_mask = cases["aligned"]
    assert plan.x_align() == 4
    dlg = dev(lg)
    assert dlg.data_ptr() % 16 == 0
    C = lg.shape[1]
    shifted = offset_view(lg, 4)
    assert shifted.data_ptr() % 16 == 4
    mask, out = ops.cd_tile_stitch(shifted, plan)
    assert np.array_equal(bits(out), bits(want)) and np.array_equal(mask.cpu().numpy(), want_mask)
    for off_out, off_mask in ((4, 0), (0, 1), (8, 2)):
        o = offset_view(np.zeros((C, plan.H, plan.W), dtype=np.float32), off_out)
        m = offset_view(np.zeros((plan.H, plan.W), dtype=np.uint8), off_mask)
        ops.cd_tile_stitch(dlg, plan, out_logits=o, out_mask=m)
        assert np.array_equal(bits(o), bits(want)) and np.array_equal(m.cpu().numpy(), want_mask), (off_out, off_mask)
    lab = np.random.RandomState(3).randint(0, C, (plan.H, plan.W)).astype(np.uint8)
    counts = torch.zeros(C, C, dtype=torch.int64, device=DEV)
    ops.cd_tile_stitch(dlg, plan, label=offset_view(lab, 1), counts=counts)
    assert np.array_equal(counts.cpu().numpy(), T.confusion(lab, want_mask, C))


# ---- 4. given output buffers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd", "aligned"])
def test_every_byte_of_given_buffers_is_written(cases, name):
    from dahitra_amd import ops
    plan, lg, want, want_mask = cases[name]
    o = torch.full(want.shape, SENTINEL, dtype=torch.uint8, device=DEV).repeat_interleave(4, dim=-1).view(torch.float32)
    m = torch.full(want_mask.shape, SENTINEL, dtype=torch.uint8, device=DEV)
    assert o.shape == want.shape and bool((o.view(torch.int32) == -0x5A5A5A5B).all())
    got_m, got_o = ops.cd_tile_stitch(dev(lg), plan, out_logits=o, out_mask=m)
    assert got_m is m and got_o is o
    assert np.array_equal(bits(o), bits(want)) and np.array_equal(m.cpu().numpy(), want_mask)
    assert not (bits(want) == 0xA5A5A5A5).any() and not (want_mask == SENTINEL).any()


# ---- 5. counts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd", "maxc", "aligned"])
def test_counts_are_the_confusion_of_the_returned_mask(cases, name):
    from dahitra_amd import ops
    plan, lg, want, want_mask = cases[name]
    C = lg.shape[1]
    lab = np.random.RandomState(5).randint(0, C, (plan.H, plan.W)).astype(np.uint8)
    counts = torch.zeros(C, C, dtype=torch.int64, device=DEV)
    mask, _ = ops.cd_tile_stitch(dev(lg), plan, label=dev(lab), counts=counts)
    one = counts.cpu().numpy().copy()
    assert np.array_equal(one, T.confusion(lab, mask.cpu().numpy(), C)) and one.sum() == plan.H * plan.W
    assert np.array_equal(mask.cpu().numpy(), want_mask)
    ops.cd_tile_stitch(dev(lg), plan, label=dev(lab), counts=counts)
    assert np.array_equal(counts.cpu().numpy(), 2 * one), "a second call accumulates"
    # the label plane a device index names
    stack = np.stack([np.zeros_like(lab), lab])
    counts.zero_()
    ops.cd_tile_stitch(dev(lg), plan, label=dev(stack), counts=counts, label_index=torch.tensor([1], dtype=torch.int32, device=DEV))
    assert np.array_equal(counts.cpu().numpy(), one)


# ---- 6. refused arguments ------------------------------------------------------------------------------------------------------
def test_refused_arguments_raise_and_launch_nothing(cases):
    from dahitra_amd import _lib, ops
    from dahitra_amd.tiles import TilePlan
    plan, lg, want, want_mask = cases["aligned"]
    C, H, W, P, h, w = 2, plan.H, plan.W, plan.P, plan.h, plan.w
    dlg = dev(lg)
    o = torch.full((C, H, W), 7.5, device=DEV)
    m = torch.full((H, W), SENTINEL, dtype=torch.uint8, device=DEV)
    lab = torch.zeros(H, W, dtype=torch.uint8, device=DEV)
    counts = torch.zeros(C, C, dtype=torch.int64, device=DEV)
    good = dict(logits=dlg, plan=plan, out_logits=o, out_mask=m, label=lab, counts=counts)
    wide = torch.zeros(P, C, h, 2 * w, device=DEV)
    for kw in (dict(logits=dlg[0]), dict(logits=dlg.double()), dict(logits=dlg[:-1]), dict(logits=wide[..., ::2]),
               dict(logits=torch.zeros(P, 9, h, w, device=DEV)), dict(logits=dlg[:, :, :8]), dict(out_logits=o[:1]),
               dict(out_logits=o.double()), dict(out_logits=o.cpu()), dict(out_mask=m[:4]), dict(out_mask=m.int()),
               dict(out_mask=m.cpu()), dict(label=lab.long()), dict(label=lab[:4]), dict(label=None), dict(counts=None),
               dict(counts=counts.int()), dict(counts=counts[:1]), dict(counts=counts.cpu()), dict(label_index=torch.zeros(2, dtype=torch.int32, device=DEV)),
               dict(label=None, counts=None, label_index=torch.zeros(1, dtype=torch.int32, device=DEV)),
               dict(plan=TilePlan.eval_cd(1024, 1024)), dict(plan=T.make_plan(T.ODD))):
        with pytest.raises(ValueError):
            ops.cd_tile_stitch(**dict(good, **kw))
    with pytest.raises(_lib.HipLibraryError):
        ops.cd_tile_stitch(dlg.cpu(), plan)
    vl = torch.zeros(3, 2, 8, 8, device=DEV)
    vlab = torch.zeros(3, 8, 8, dtype=torch.uint8, device=DEV)
    vc = torch.zeros(3, 2, 2, dtype=torch.int64, device=DEV)
    for kw in (dict(logits=vl[0]), dict(logits=vl.half()), dict(labels=vlab.long()), dict(labels=vlab[:2]), dict(labels=vlab.cpu()),
               dict(counts=vc[:2]), dict(counts=vc.int()), dict(counts=vc.cpu()), dict(logits=torch.zeros(3, 9, 8, 8, device=DEV)),
               dict(logits=torch.zeros(3, 2, 8, 16, device=DEV)[..., ::2])):
        with pytest.raises(ValueError):
            ops.cd_view_counts(**dict(dict(logits=vl, labels=vlab, counts=vc), **kw))
    with pytest.raises(_lib.HipLibraryError):
        ops.cd_view_counts(vl.cpu(), vlab.cpu(), vc.cpu())
    # what the library itself refuses
    L, S = _lib.lib(), ops.S
    t = ops.tile_tables(plan, dlg.device)
    ptr = lambda x: ops._vp(x.data_ptr()) if x is not None else ops._vp(0)
    order = ("logits", "P", "C", "h", "w", "ys", "ny", "xs", "nx", "flips", "nf", "wy", "wx", "rows", "cols", "x_align", "H", "W",
             "out", "mask", "label", "label_index", "counts")
    base = dict(logits=ptr(dlg), P=P, C=C, h=h, w=w, ys=ptr(t["ys"]), ny=plan.ny, xs=ptr(t["xs"]), nx=plan.nx, flips=ptr(t["flips"]),
                nf=plan.nf, wy=ptr(t["wy"]), wx=ptr(t["wx"]), rows=ptr(t["rows"]), cols=ptr(t["cols"]), x_align=4, H=H, W=W,
                out=ptr(o), mask=ptr(m), label=ptr(lab), label_index=ptr(None), counts=ptr(counts))
    for change in (dict(logits=ptr(None)), dict(ys=ptr(None)), dict(xs=ptr(None)), dict(flips=ptr(None)), dict(wy=ptr(None)),
                   dict(wx=ptr(None)), dict(rows=ptr(None)), dict(cols=ptr(None)), dict(mask=ptr(None)), dict(label=ptr(None)),
                   dict(counts=ptr(None)), dict(label=ptr(None), counts=ptr(None), label_index=ptr(lab)), dict(C=0), dict(C=9),
                   dict(h=0), dict(w=W + 1), dict(h=H + 1), dict(H=1 << 16, W=1 << 15), dict(P=P + 1), dict(P=0), dict(nf=0),
                   dict(nf=5), dict(ny=0), dict(nx=-1), dict(x_align=2), dict(x_align=0)):
        args = dict(base, **change)
        assert L.dh_cd_tile_stitch(*[args[k] for k in order], S()) != 0, change
        assert L.dh_last_error().decode().startswith("cd_tile_stitch"), (change, L.dh_last_error())
    vbase = dict(logits=ptr(vl), labels=ptr(vlab), P=3, C=2, h=8, w=8, counts=ptr(vc))
    vorder = ("logits", "labels", "P", "C", "h", "w", "counts")
    for change in (dict(logits=ptr(None)), dict(labels=ptr(None)), dict(counts=ptr(None)), dict(P=0), dict(P=65536), dict(C=0),
                   dict(C=9), dict(h=0), dict(w=-1), dict(h=1 << 16, w=1 << 15)):
        args = dict(vbase, **change)
        assert L.dh_cd_view_counts(*[args[k] for k in vorder], S()) != 0, change
        assert L.dh_last_error().decode().startswith("cd_view_counts"), (change, L.dh_last_error())
    torch.cuda.synchronize()
    assert bool((o == 7.5).all()) and bool((m == SENTINEL).all()) and int(counts.sum()) == 0 and int(vc.sum()) == 0
    ops.cd_tile_stitch(**good)                                                     # the good call does write
    assert np.array_equal(bits(o), bits(want)) and np.array_equal(m.cpu().numpy(), want_mask) and int(counts.sum()) == H * W


# ---- 7. per-view counts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,C,h,w", [(3, 2, 8, 8), (16, 5, 256, 256), (2, 8, 5, 7)])
def test_view_counts_equal_confusion_matrix_per_view(P, C, h, w):
    from dahitra_amd import ops
    rng = np.random.RandomState(P * C)
    lg = rng.randint(-3, 4, (P, C, h, w)).astype(np.float32)                    # small integers: ties decide many pixels
    lab = rng.randint(0, C, (P, h, w)).astype(np.uint8)
    dlg, dlab = dev(lg), dev(lab)
    counts = torch.zeros(P, C, C, dtype=torch.int64, device=DEV)
    ops.cd_view_counts(dlg, dlab, counts)
    want = torch.zeros(P, C, C, dtype=torch.int64, device=DEV)
    for p in range(P):
        ops.confusion_matrix(dlg[p:p + 1], dlab[p:p + 1].to(torch.int64), want[p])
    assert torch.equal(counts, want) and int(counts.sum()) == P * h * w
    assert all(np.array_equal(counts[p].cpu().numpy(), T.confusion(lab[p], T.first_max(lg[p]), C)) for p in range(min(P, 3)))
    ops.cd_view_counts(dlg, dlab[:, None].contiguous(), counts)                    # labels as [P, 1, h, w]; accumulated
    assert torch.equal(counts, 2 * want)


# ---- 8. model level, stitchable plans ----------------------------------------------------------------------------------------------
ORDERS = ((0, 1, 2, 3), (3, 0, 2, 1), (2, 3, 1, 0))          # three 512 x 512 tiles: 2 x 2 mosaics of the four pairs


def make_net(name):
    from dahitra_amd.models.networks import define_G
    net = define_G(types.SimpleNamespace(net_G=name, compute_dtype="fp32"), gpu_ids=[0])
    net.load_state_dict(O.large_margin_state(name))
    net.eval()
    return net


@pytest.fixture(scope="module")
def world():
    from dahitra_amd.datasets.gpu_pipeline import GpuPairPipeline
    from dahitra_amd.tiles import TilePlan
    A, B, L, names = T.levir_pairs()
    tiles = [tuple(T.mosaic(x, o, 2) for x in (A, B, L)) for o in ORDERS]
    pipe = GpuPairPipeline(*(dev(np.stack([t[i] for t in tiles])) for i in range(3)), names=["tile_a.png", "tile_b.jpg", "tile_c"])
    pairs = GpuPairPipeline(dev(A), dev(B), dev(L), names=names)
    plan_a = TilePlan(512, 512, (256, 256), (128, 128), (0, 3), "triangle")
    plan_b = TilePlan(512, 512, (256, 256), (256, 256), (0,), "mean")
    assert plan_a.P == 18 and plan_b.P == 4
    return types.SimpleNamespace(net=make_net(NAME), pipe=pipe, pairs=pairs, plan_a=plan_a, plan_b=plan_b, labels=[t[2] for t in tiles])


def restated(net, pipe, plan, index):
    """the restatement applied to the logits of an eager net(A, B) on the cut views"""
    v = pipe.window_batch(index, plan)
    with torch.no_grad():
        lg = net(v['A'], v['B']).float().cpu().numpy()
    out = T.stitch(lg, plan)[0]
    return out, T.first_max(out)


@pytest.fixture(scope="module")
def answers(world):
    """per plan: (graph mask, graph logits, eager mask, eager logits) of tile 0 on the host, computed once"""
    from dahitra_amd.models.tiles import predict_tile
    out = {}
    for key in ("a", "b"):
        plan = getattr(world, "plan_" + key)
        got = predict_tile(world.net, world.pipe, 0, plan, graph=True) + predict_tile(world.net, world.pipe, 0, plan, graph=False)
        out[key] = tuple(t.cpu().numpy() for t in got)
    return out


@pytest.mark.parametrize("key", ["a", "b"])
def test_predict_tile_graph_and_eager_equal_the_restatement(world, answers, key):
    plan = getattr(world, "plan_" + key)
    gm, gl, em, el = answers[key]
    assert gm.shape == (512, 512) and gm.dtype == np.uint8 and gl.shape == (2, 512, 512) and gl.dtype == np.float32
    assert np.array_equal(gm, em) and np.array_equal(bits(gl), bits(el)), "graph and eager paths give the same bytes"
    want, want_mask = restated(world.net, world.pipe, plan, 0)
    assert np.array_equal(bits(gl), bits(want)) and np.array_equal(gm, want_mask)
    assert 0 < int(gm.sum()) < gm.size, "a degenerate mask cannot pass"


def test_plans_differ_and_plan_b_is_the_existing_path_in_place(world, answers):
    from dahitra_amd import ops
    from dahitra_amd.models.tiles import evaluate_tiles
    assert (answers["a"][0] != answers["b"][0]).any(), "overlap, flips and the triangle change at least one pixel"
    mask_b = answers["b"][0]
    counts = torch.zeros(2, 2, dtype=torch.int64, device=DEV)
    for k, src in enumerate(ORDERS[0]):
        batch = world.pairs.make_batch([src], 256)                              # the whole 256-pixel pair: the existing path
        with torch.no_grad():
            lg = world.net(batch['A'], batch['B']).float().contiguous()
        m = ops.confusion_matrix(lg, batch['L'][:, 0].to(torch.int64).contiguous(), counts, want_mask=True)
        iy, ix = divmod(k, 2)
        assert np.array_equal(mask_b[256 * iy:256 * iy + 256, 256 * ix:256 * ix + 256], m[0].cpu().numpy().astype(np.uint8)), k
    from dahitra_amd.datasets.gpu_pipeline import GpuPairPipeline
    first = GpuPairPipeline(world.pipe.a[:1], world.pipe.b[:1], world.pipe.l[:1])          # tile 0 alone
    scores, cm = evaluate_tiles(world.net, first, world.plan_b, want_counts=True)
    assert np.array_equal(cm, counts.cpu().numpy()) and cm.sum() == 512 * 512
    assert np.array_equal(cm, T.confusion(world.labels[0], mask_b, 2))
    from dahitra_amd.models.evaluator import cm2score
    assert scores == cm2score(cm) and 0 < scores["mf1"] <= 1


def test_one_recorded_step_follows_its_device_index(world):
    from dahitra_amd.graph import GraphedTileStep
    step = GraphedTileStep(world.net, world.pipe, world.plan_a)
    graph = step.graph
    seen = []
    for index in (1, 2, 1):
        mask, logits = step.step(index)                                            # the step's static tensors
        want, want_mask = restated(world.net, world.pipe, world.plan_a, index)
        assert step.graph is graph and mask is step.buf.mask and logits is step.buf.logits
        assert np.array_equal(bits(logits), bits(want)) and np.array_equal(mask.cpu().numpy(), want_mask), index
        seen.append(mask.cpu().numpy().copy())
    assert np.array_equal(seen[0], seen[2]) and (seen[0] != seen[1]).any()
    for bad in (-1, 3):
        with pytest.raises(ValueError):
            step.step(bad)
    world.net.train()
    with pytest.raises(RuntimeError, match="eval-mode forward"):
        step.step(0)
    world.net.eval()
    with pytest.raises(ValueError):
        GraphedTileStep(world.net, world.pipe, world.plan_a, chunk=4)              # 4 does not divide 18
    with pytest.raises(ValueError):
        GraphedTileStep(world.net, world.pipe, world.plan_a, confusion=torch.zeros(3, 2, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        GraphedTileStep(world.net, world.pairs, world.plan_a)                      # 256-pixel pairs under a 512 plan


def test_chunks_of_two_and_four_give_the_same_bytes(world, answers):
    from dahitra_amd.models.tiles import predict_tile
    m2, l2 = predict_tile(world.net, world.pipe, 0, world.plan_b, chunk=2)
    m4, l4 = predict_tile(world.net, world.pipe, 0, world.plan_b, chunk=4)
    assert torch.equal(m2, m4) and np.array_equal(bits(l2), bits(l4))
    assert np.array_equal(m4.cpu().numpy(), answers["b"][0])


def test_newunettrans_gets_a_whole_tile(world):
    """the net that runs at 256 x 256 only"""
    from dahitra_amd.models.tiles import predict_tile
    net = make_net("newUNetTrans")
    mask, logits = predict_tile(net, world.pipe, 0, world.plan_b)
    want, want_mask = restated(net, world.pipe, world.plan_b, 0)
    assert np.array_equal(bits(logits), bits(want)) and np.array_equal(mask.cpu().numpy(), want_mask)
    assert 0 < int(mask.sum()) < mask.numel()


# ---- 9. model level, eval_cd plan -------------------------------------------------------------------------------------------------
def test_evaluate_tiles_eval_cd_is_the_sixteen_patch_evaluation(world):
    from dahitra_amd import ops
    from dahitra_amd.datasets.gpu_pipeline import GpuPairPipeline
    from dahitra_amd.models.evaluator import cm2score
    from dahitra_amd.models.tiles import evaluate_tiles
    from dahitra_amd.tiles import TilePlan
    A, B, L, _ = T.levir_pairs()
    order = [(5 * r + 3 * c) % 4 for r in range(4) for c in range(4)]
    tile = [T.mosaic(x, order, 4) for x in (A, B, L)]
    tile[2] = tile[2].copy()
    tile[2][:256, :256] = 1                                                        # the (0, 0) window: every pixel labelled 1
    assert all(int(L[i].sum()) < 256 * 256 for i in range(4))
    pipe = GpuPairPipeline(*(dev(x[None]) for x in tile))
    scores, cm = evaluate_tiles(world.net, pipe, TilePlan.eval_cd(1024, 1024), want_counts=True)
    assert isinstance(scores, list) and len(scores) == 16 and cm.shape == (16, 2, 2) and cm.dtype == np.int64
    for patch in range(16):                                                        # the parent's path, patch by patch
        batch = pipe.make_batch([0], 256, patch=patch)
        with torch.no_grad():
            lg = world.net(batch['A'], batch['B']).float().contiguous()
        counts = torch.zeros(2, 2, dtype=torch.int64, device=DEV)
        ops.confusion_matrix(lg, batch['L'][:, 0].to(torch.int64).contiguous(), counts)
        assert np.array_equal(cm[patch], counts.cpu().numpy()), patch
        assert scores[patch] == cm2score(cm[patch])
    assert np.array_equal(cm[0], cm[5]) and scores[0] == scores[5], "patch 0 repeats patch 5"
    assert (cm.sum(axis=(1, 2)) == 256 * 256).all()
    assert (cm[:, 1].sum(axis=1) < 256 * 256).all(), "the all-ones labels of the (0, 0) window are in no entry"
    eager = evaluate_tiles(world.net, pipe, TilePlan.eval_cd(1024, 1024), graph=False, want_counts=True)[1]
    assert np.array_equal(eager, cm)


# ---- 10. predict_tiles ------------------------------------------------------------------------------------------------------------
def test_predict_tiles_writes_one_png_per_pair(world, tmp_path):
    from PIL import Image
    from dahitra_amd.models.tiles import predict_tile, predict_tiles
    names = predict_tiles(world.net, world.pipe, str(tmp_path / "pred"))
    assert names == ["tile_a.png", "tile_b.png", "tile_c.png"] and sorted(os.listdir(str(tmp_path / "pred"))) == names
    for i, n in enumerate(names):
        mask, _ = predict_tile(world.net, world.pipe, i, world.plan_b)           # the default plan: 256-pixel windows, no overlap
        img = Image.open(str(tmp_path / "pred" / n))
        assert img.size == (512, 512) and np.array_equal(np.asarray(img), mask.cpu().numpy() * 255), n
    ev = types.SimpleNamespace(net_G=world.net, pred_dir=str(tmp_path / "ev"), eval=world.net.eval)
    from dahitra_amd.models.basic_model import CDEvaluator
    assert CDEvaluator.predict_tiles(ev, world.pipe, plan=world.plan_a) == names
    a = np.asarray(Image.open(str(tmp_path / "ev" / "tile_b.png")))
    assert np.array_equal(a, predict_tile(world.net, world.pipe, 1, world.plan_a)[0].cpu().numpy() * 255)


def test_recorded_steps_are_kept_once_and_can_be_dropped(world):
    from dahitra_amd.models.tiles import forget_tile_steps, predict_tile
    forget_tile_steps(world.net)
    m0, _ = predict_tile(world.net, world.pipe, 0, world.plan_b)
    m1, _ = predict_tile(world.net, world.pipe, 1, world.plan_b, chunk=4)          # the default chunk of four views: the same step
    predict_tile(world.net, world.pipe, 0, world.plan_b, chunk=2)
    assert forget_tile_steps(world.net, world.pairs) == 0, "steps of another pipeline only"
    assert forget_tile_steps(world.net, world.pipe) == 2 and forget_tile_steps(world.net) == 0
    again, _ = predict_tile(world.net, world.pipe, 0, world.plan_b)               # recorded anew, the same bytes
    assert torch.equal(again, m0) and not torch.equal(m0, m1)


def test_recorded_step_leaves_its_counts_alone_and_refuses_a_rebuilt_arena(world):
    """(last in the file: it replaces a parameter of the shared net)"""
    from dahitra_amd.graph import GraphedTileStep, TileBuffers
    prefill = torch.tensor([[11, 22], [33, 44]], dtype=torch.int64, device=DEV)
    conf = prefill.clone()
    step = GraphedTileStep(world.net, world.pipe, world.plan_b, confusion=conf)
    assert torch.equal(conf, prefill), "warm-up and capture leave the counts as they were"
    eager = prefill.clone()
    buf = TileBuffers(world.net, world.pipe, world.plan_b, eager)
    for index in (0, 2):                                                           # two replays against two eager bodies
        mask, logits = step.step(index)
        buf.aim(index)
        buf.run()
        assert torch.equal(mask, buf.mask) and np.array_equal(bits(logits), bits(buf.logits)) and torch.equal(conf, eager), index
    assert int(conf.sum()) == int(prefill.sum()) + 2 * 512 * 512
    p = next(world.net.parameters())
    p.data = p.data.clone()
    world.net._ensure_arena(p.device)
    with pytest.raises(RuntimeError, match="rebuilt"):
        step.step(0)
    assert torch.equal(conf, eager)
