"""What the evaluation-side and loader-side wrappers of dahitra_amd.ops refuse, and the epoch loop of models/xbd.validate /
validate_sweep, without a GPU.  A table tries one bad argument at a time on every tensor argument of every wrapper (`out` and `ws` included) and asserts
the exception type, that the message names the function and the argument, and that no kernel entry of the library was reached.
The order in which two simultaneous faults are reported is deliberately not pinned."""
import types

import numpy as np
import pytest
import torch

from dahitra_amd import _lib, ops
from dahitra_amd.models import xbd
from dahitra_amd.tiles import TilePlan

U8, I32, I64, F32 = torch.uint8, torch.int32, torch.int64, torch.float32
OTHER = {U8: F32, F32: torch.float64, I32: I64, I64: I32}
WS_BYTES = 4096          # what the stand-in library answers to every *_ws_bytes query
CAP = 4
CROP = 8                 # the loaders' window: it fits the sources at either size
JITTER_TILES = 3         # what the stand-in library answers to dh_xbd_augment_jitter_tiles


class SizesOnly:
    """stands in for the library: the host-side workspace size queries answer, any other use is a failure"""

    def __getattr__(self, name):
        if name.endswith("_ws_bytes"):
            def size(*args):
                args[-1]._obj.value = WS_BYTES
                return 0
            return size
        if name == "dh_xbd_augment_jitter_tiles":
            return lambda S: JITTER_TILES
        raise AssertionError("the library was touched: %s" % name)


class Reached(Exception):
    """the wrapper accepted its arguments and went on to its C entry"""


@pytest.fixture
def no_library(monkeypatch):
    def entry(name, *args):
        raise Reached(name)
    monkeypatch.setattr(_lib, "lib", lambda: SizesOnly())
    monkeypatch.setattr(ops, "_call", entry)
    monkeypatch.setattr(ops, "S", lambda: None)


def z(dtype, *shape):
    return torch.zeros(*shape, dtype=dtype)


def plan(alt):
    return TilePlan(32, 64 if alt else 48, (16, 16), (8, 8), (0, 1), "triangle")


# every wrapper: (the arguments by the name its messages use, first the one the others must agree with; how to call it).
# alt=True gives every argument at another size (N 3 for 2, 8 x 12 for 8 x 8, one more class): one of them among the others disagrees.
def dims(alt):
    return (3, 8, 12) if alt else (2, 8, 8)


def tta_pack(alt):
    N, H, W = dims(alt)
    return {"pre_u8": z(U8, N, H, W, 3), "post_u8": z(U8, N, H, W, 3), "out": z(F32, 4 * N, 6, H, W)}


def tta_merge(alt):
    N, H, W = dims(alt)
    return {"logits": z(F32, 4 * N, 5, H, W), "out": z(U8, N, H, W, 5)}


def tta_pack_views(alt):
    N, H, W = dims(alt)
    return {"pre_u8": z(U8, N, H, W, 3), "post_u8": z(U8, N, H, W, 3), "out": z(F32, 8 * N, 6, H, W)}


def tta_merge_multi(alt):
    N, H, W = dims(alt)
    return {"logits_list[0]": z(F32, 8 * N, 5, H, W), "logits_list[1]": z(F32, 8 * N, 5, H, W), "out": z(U8, N, H, W, 5)}


def damage_map(alt):
    N, H, W = dims(alt)
    return {"msk_u8": z(U8, N, H, W, 5), "out": z(U8, N, H, W)}


def vis_grid(alt):
    N, H, W = dims(alt)
    return {"msk_u8": z(U8, N, H, W, 5), "pre_u8": z(U8, N, H, W, 3), "post_u8": z(U8, N, H, W, 3), "gt_u8": z(U8, N, H, W),
            "out": z(U8, N, H, 4 * W, 3)}


def cc_label(alt):
    N, H, W = dims(alt)
    return {"key_u8": z(U8, N, H, W), "out[0]": z(I32, N, H, W), "out[1]": z(I32, N), "ws": z(U8, WS_BYTES)}


def cc_stats(alt):
    N, H, W = dims(alt)
    return {"labels": z(I32, N, H, W), "vote_u8": z(U8, N, H, W), "out": z(I32, N, CAP, ops.XBD_CC_COLS)}


def cc_vote(alt):
    N = dims(alt)[0]
    return {"table": z(I32, N, CAP, ops.XBD_CC_COLS), "out": z(U8, N, CAP)}


def cc_paint(alt):
    N, H, W = dims(alt)
    return {"labels": z(I32, N, H, W), "cls_u8": z(U8, N, CAP), "out": z(U8, N, H, W)}


def cc_match(alt):
    N, H, W = dims(alt)
    return {"labels_a": z(I32, N, H, W), "labels_b": z(I32, N, H, W), "out[0]": z(I32, N, CAP, ops.XBD_CC_MATCH_COLS),
            "out[1]": z(I32, N, CAP + 1), "ws": z(U8, WS_BYTES)}


def morph(alt):
    N, H, W = dims(alt)
    return {"map_u8": z(U8, N, H, W), "out": z(U8, N, H, W)}


def msk_dilate(alt):
    N, H, W = dims(alt)
    return {"msk_u8": z(U8, N, 5, H, W), "out": z(U8, N, 5, H, W)}


def fill_holes(alt):
    N, H, W = dims(alt)
    return {"map_u8": z(U8, N, H, W), "out": z(U8, N, H, W), "ws": z(U8, WS_BYTES)}


def eval_vis(alt):
    N, H, W = dims(alt)
    return {"a": z(F32, N, 3, H, W), "b": z(F32, N, 3, H, W), "logits": z(F32, N, 2, H, W), "label": z(I64, N, H, W),
            "out": z(U8, *ops.cd_vis_shape(N, H, W))}


def tile_stitch(alt):
    p, C = plan(alt), 3 if alt else 2
    return {"logits": z(F32, p.P, C, p.h, p.w), "out_logits": z(F32, C, p.H, p.W), "out_mask": z(U8, p.H, p.W),
            "label": z(U8, 2, p.H, p.W), "counts": z(I64, C, C), "label_index": z(I32, 2 if alt else 1)}


def view_counts(alt):
    P, h, w = dims(alt)
    C = 3 if alt else 2
    return {"logits": z(F32, P, C, h, w), "labels": z(U8, P, h, w), "counts": z(I64, P, C, C)}


# the loaders: the resident sources at dims(alt), and a batch of 3 (alt: 4) samples, which idx sets
def xbd_sources(alt):
    n, H, W = dims(alt)
    return {"pre_u8": z(U8, n, H, W, 3), "post_u8": z(U8, n, H, W, 3), "pre_mask_u8": z(U8, n, H, W), "post_label_u8": z(U8, n, H, W)}


def augment(alt):
    N = 4 if alt else 3
    return {**xbd_sources(alt), "idx": z(I32, N), "params": z(I32, N, 9), "coef": z(I32, N, 2, CROP, 4),
            "out_img": z(F32, N, 6, CROP, CROP), "out_msk": z(U8, N, 5, CROP, CROP), "out_lbl": z(U8, N, CROP, CROP)}


def pairs(alt):
    n, H, W = dims(alt)
    N = 4 if alt else 3
    return {"a_u8": z(U8, n, H, W, 3), "b_u8": z(U8, n, H, W, 3), "l_u8": z(U8, n, H, W), "idx": z(I32, N), "params": z(I32, N, 4),
            "blur": z(I32, N, 2), "out_a": z(F32, N, 3, 4, 6), "out_b": z(F32, N, 3, 4, 6), "out_l": z(U8, N, 1, 4, 6)}


def augment_warp(alt):
    n, H, W = dims(alt)
    N = 4 if alt else 3
    return {"pre_u8": z(U8, n, H, W, 3), "post_u8": z(U8, n, H, W, 3), "label_u8": z(U8, n, H, W), "idx": z(I32, N),
            "params": z(I32, N, ops.XBD_WARP_PARAM_WORDS), "tab": z(I32, N, 4, CROP), "out_img": z(F32, N, 6, CROP, CROP),
            "out_msk": z(U8, N, 5, CROP, CROP)}


def unet_colour(alt):
    N, S = (4, 12) if alt else (3, 8)
    return {"img": z(F32, N, 6, S, S), "jobs": z(I32, 3 if alt else 2, ops.XBD_COLOUR_JOB_WORDS), "noise": z(U8, 1, S, S, 3),
            "ws": z(U8, WS_BYTES)}


def adapt_batch(alt):
    N = 4 if alt else 3
    return {**xbd_sources(alt), "idx": z(I32, N), "origins": z(I32, N, 2)}


def class_table(alt):
    n, H, W = dims(alt)
    return {"labels_u8": z(U8, n, H, W), "out": z(I32, n, len(ops.XBD_CLASS_COLUMNS))}


def call_augment(a, **more):
    return ops.xbd_augment(a["pre_u8"], a["post_u8"], a["pre_mask_u8"], a["post_label_u8"], a["idx"], a["params"], a["coef"], CROP,
                           out_img=a["out_img"], out_msk=a["out_msk"], out_lbl=a["out_lbl"], **more)


WRAPPERS = {
    "xbd_tta_pack": (tta_pack, lambda a: ops.xbd_tta_pack(a["pre_u8"], a["post_u8"], "bgr", out=a["out"])),
    "xbd_tta_merge": (tta_merge, lambda a: ops.xbd_tta_merge(a["logits"], out=a["out"])),
    "xbd_tta_pack_views": (tta_pack_views, lambda a: ops.xbd_tta_pack_views(a["pre_u8"], a["post_u8"], "rgb", 8, out=a["out"])),
    "xbd_tta_merge_multi": (tta_merge_multi,
                            lambda a: ops.xbd_tta_merge_multi([a["logits_list[0]"], a["logits_list[1]"]], 8, out=a["out"])),
    "xbd_damage_map": (damage_map, lambda a: ops.xbd_damage_map(a["msk_u8"], ops.XBD_LOC_THR, out=a["out"])),
    "xbd_vis_grid": (vis_grid, lambda a: ops.xbd_vis_grid(a["pre_u8"], a["post_u8"], a["gt_u8"], a["msk_u8"], out=a["out"])),
    "xbd_cc_label": (cc_label, lambda a: ops.xbd_cc_label(a["key_u8"], 8, True, out=(a["out[0]"], a["out[1]"]), ws=a["ws"])),
    "xbd_cc_stats": (cc_stats, lambda a: ops.xbd_cc_stats(a["labels"], a["vote_u8"], CAP, out=a["out"])),
    "xbd_cc_vote": (cc_vote, lambda a: ops.xbd_cc_vote(a["table"], 0, "all", out=a["out"])),
    "xbd_cc_paint": (cc_paint, lambda a: ops.xbd_cc_paint(a["labels"], a["cls_u8"], out=a["out"])),
    "xbd_cc_match": (cc_match, lambda a: ops.xbd_cc_match(a["labels_a"], a["labels_b"], CAP, CAP + 1, (2, 3),
                                                          out=(a["out[0]"], a["out[1]"]), ws=a["ws"])),
    "xbd_morph": (morph, lambda a: ops.xbd_morph(a["map_u8"], "erode", 3, out=a["out"])),
    "xbd_msk_dilate": (msk_dilate, lambda a: ops.xbd_msk_dilate(a["msk_u8"], 5, out=a["out"])),
    "xbd_fill_holes": (fill_holes, lambda a: ops.xbd_fill_holes(a["map_u8"], 8, out=a["out"], ws=a["ws"])),
    "cd_eval_vis": (eval_vis, lambda a: ops.cd_eval_vis(a["a"], a["b"], a["logits"], a["label"], out=a["out"])),
    "cd_tile_stitch": (tile_stitch, lambda a: ops.cd_tile_stitch(a["logits"], plan(False), a["out_logits"], a["out_mask"], a["label"],
                                                                 a["counts"], a["label_index"])),
    "cd_view_counts": (view_counts, lambda a: ops.cd_view_counts(a["logits"], a["labels"], a["counts"])),
    "xbd_augment": (augment, lambda a: call_augment(a, train=False)),                      # (validation mode writes out_lbl)
    "augment_pairs": (pairs, lambda a: ops.augment_pairs(a["a_u8"], a["b_u8"], a["l_u8"], a["idx"], a["params"], 4, 6, a["blur"],
                                                         out_a=a["out_a"], out_b=a["out_b"], out_l=a["out_l"])),
    "xbd_augment_warp": (augment_warp, lambda a: ops.xbd_augment_warp(a["pre_u8"], a["post_u8"], a["label_u8"], a["idx"], a["params"],
                                                                      a["tab"], CROP, out_img=a["out_img"], out_msk=a["out_msk"])),
    "xbd_unet_colour": (unet_colour, lambda a: ops.xbd_unet_colour(a["img"], a["jobs"], a["noise"], ws=a["ws"])),
    "xbd_adapt_batch": (adapt_batch, lambda a: ops.xbd_adapt_batch(a["pre_u8"], a["post_u8"], a["pre_mask_u8"], a["post_label_u8"],
                                                                   a["idx"], a["origins"], CROP)),
    "xbd_class_table": (class_table, lambda a: ops.xbd_class_table(a["labels_u8"], out=a["out"])),
}
# the others refuse a CPU tensor with ValueError
HIP_ERROR_ON_CPU = ("cd_eval_vis", "cd_tile_stitch", "cd_view_counts", "xbd_class_table")


def strided(t):
    """a view [..., ::2] with t's shape and dtype"""
    return torch.zeros(tuple(t.shape[:-1]) + (2 * t.shape[-1],), dtype=t.dtype)[..., ::2]


def bad_arguments():
    cases = []
    for fn, (make, _) in WRAPPERS.items():
        names = list(make(False))
        for i, name in enumerate(names):
            kinds = ["non-tensor", "dtype", "strided"]
            if name != "ws":                              # a workspace is a count of bytes: any shape of enough bytes will do
                kinds += ["rank"] + (["disagrees"] if i else [])
            else:
                kinds += ["short"]
            if name == "label_index":                     # one element: of any rank, and never strided
                kinds = ["non-tensor", "dtype", "disagrees"]
            if (fn, name) == ("xbd_unet_colour", "jobs"):  # any number of jobs: no other argument has a say in it
                kinds.remove("disagrees")
            cases += [(fn, name, kind) for kind in kinds]
    return cases


@pytest.mark.parametrize("fn,name,kind", bad_arguments(), ids=lambda v: v)
def test_one_bad_argument_is_a_value_error_that_names_it(no_library, monkeypatch, fn, name, kind):
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    make, call = WRAPPERS[fn]
    args = make(False)
    call_ok = dict(args)
    good = args[name]
    args[name] = {"non-tensor": lambda: np.zeros(tuple(good.shape), dtype=np.uint8), "dtype": lambda: good.to(OTHER[good.dtype]),
                  "rank": lambda: good[None], "disagrees": lambda: make(True)[name], "strided": lambda: strided(good),
                  "short": lambda: good[:8]}[kind]()
    if torch.is_tensor(args[name]):
        assert (kind == "strided") != args[name].is_contiguous()
        assert kind in ("dtype", "strided") or tuple(args[name].shape) != tuple(good.shape)
    with pytest.raises(ValueError) as e:
        call(args)
    assert type(e.value) is ValueError and fn in str(e.value) and name in str(e.value), str(e.value)
    with pytest.raises(Reached, match="dh_" + fn):          # the case's other arguments are good: alone they reach the entry
        call(call_ok)


@pytest.mark.parametrize("fn", list(WRAPPERS))
def test_cpu_tensors_are_refused_before_the_library_is_touched(no_library, fn):
    make, call = WRAPPERS[fn]
    args = make(False)
    with pytest.raises((ValueError, _lib.HipLibraryError)) as e:
        call(args)
    assert fn in str(e.value), str(e.value)
    if fn in HIP_ERROR_ON_CPU:
        assert type(e.value) is _lib.HipLibraryError
    else:
        assert type(e.value) is ValueError and next(iter(args)) in str(e.value), str(e.value)


def test_xbd_augment_checks_its_jitter_table_and_workspace(no_library, monkeypatch):
    """the two arguments of xbd_augment's ColorJitter form, which the table's row does not take"""
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    args = augment(False)
    table = np.zeros((3, 2, ops.XBD_JITTER_WORDS), dtype=np.int32)
    need = ops.xbd_augment_jitter_ws_bytes(3, CROP)
    assert need == 3 * 2 * (ops.XBD_JITTER_WORDS + JITTER_TILES) * 4
    ws = z(U8, need)
    for bad in (torch.from_numpy(table), table.astype(np.int64), table[:2], table[None], np.asfortranarray(table),
                np.zeros((3, 2, 2 * ops.XBD_JITTER_WORDS), dtype=np.int32)[..., ::2], table.tolist()):
        with pytest.raises(ValueError, match="xbd_augment: jitter"):
            call_augment(args, jitter=bad, ws=ws)
    with pytest.raises(ValueError, match="xbd_augment: jitter"):                            # a validation batch is not jittered
        call_augment(args, jitter=table, ws=ws, train=False)
    for bad in (np.zeros(need, dtype=np.uint8), ws.to(F32), strided(ws), ws[:need - 1]):
        with pytest.raises(ValueError, match="xbd_augment: ws"):
            call_augment(args, jitter=table, ws=bad)
    for fits in (ws, z(U8, need + 1), None):
        with pytest.raises(Reached, match="dh_xbd_augment_jitter_u8"):
            call_augment(args, jitter=table, ws=fits)
    with pytest.raises(Reached, match="dh_xbd_augment_u8"):                                 # no table: the plain entry
        call_augment(args, ws=ws)


# ---- the epoch loop of validate and validate_sweep -----------------------------------------------------------------
ROW = np.array([7, 5, 3], dtype=np.int64)
HIST_ROW = np.arange(1, 25, dtype=np.int64).reshape(3, 4, 2)             # T = 2 thresholds: [T + 1, 4, 2]
CLASS_STEP = np.arange(1, 13, dtype=np.int64).reshape(4, 3)
HIST_STEP = np.arange(1, 61, dtype=np.int64).reshape(3, 4, 5)
THR = [0.2, 0.5]


class Zeros(torch.nn.Module):
    def forward(self, x):
        return torch.zeros(x.shape[0], 5, 8, 8)


def epoch(sizes):
    for B in sizes:
        yield {"img": torch.zeros(B, 6, 8, 8), "msk": torch.zeros(B, 5, 8, 8, dtype=U8), "lbl_msk": torch.zeros(B, 8, 8, dtype=U8)}


@pytest.fixture
def stand_ins(no_library, monkeypatch):
    """ops.xbd_val_count / ops.xbd_val_sweep replaced: image i of the epoch (from 1) gets ROW * i or HIST_ROW * i, and every batch
    of B images adds B * CLASS_STEP or B * HIST_STEP to the class accumulator"""
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    seen = types.SimpleNamespace(images=0, batches=[])

    def stand_in(row, step):
        def op(logits, msk, lbl, image_rows, class_acc, *rest):
            B = logits.shape[0]
            assert tuple(logits.shape) == (B, 5, 8, 8) and logits.dtype == F32 and image_rows.shape[0] == B and msk.shape[0] == B
            for i in range(B):
                seen.images += 1
                image_rows[i] = torch.from_numpy(row * seen.images)
            class_acc += torch.from_numpy(step * B)
            seen.batches.append(B)
        return op
    monkeypatch.setattr(ops, "xbd_val_count", stand_in(ROW, CLASS_STEP))
    monkeypatch.setattr(ops, "xbd_val_sweep", stand_in(HIST_ROW, HIST_STEP))
    return seen


SIZES = [3] * 22 + [2]          # 68 images: past the 64 rows the buffer starts with, and a ragged last batch
INDEX = np.arange(1, 69, dtype=np.int64)


def test_validate_keeps_every_row_in_order_past_the_first_buffer(stand_ins, capsys):
    model = Zeros()
    sc, parts, ic, cc = xbd.validate(model, epoch(SIZES), graph=False, want_counts=True)
    assert stand_ins.batches == SIZES and ic.shape == (68, 3) and ic.dtype == np.int64
    assert np.array_equal(ic, INDEX[:, None] * ROW[None, :])
    assert np.array_equal(cc, 68 * CLASS_STEP)
    want = xbd.val_score(ic, cc)[0]
    assert sc == want and "Val Score: %s, Dice: " % want in capsys.readouterr().out
    # a second epoch on the same model starts its class counts from zero
    assert np.array_equal(xbd.validate(model, epoch([2, 1]), graph=False, want_counts=True)[3], 3 * CLASS_STEP)
    assert isinstance(xbd.validate(model, epoch([2]), graph=False), float)


def test_validate_sweep_keeps_every_row_in_order_past_the_first_buffer(stand_ins, capsys):
    model = Zeros()
    sweep = xbd.validate_sweep(model, epoch(SIZES), THR, graph=False)
    assert stand_ins.batches == SIZES and isinstance(sweep, xbd.XbdSweep)
    assert sweep.image_hist.shape == (68, 3, 4, 2) and sweep.image_hist.dtype == np.int64
    assert np.array_equal(sweep.image_hist, INDEX[:, None, None, None] * HIST_ROW[None])
    assert np.array_equal(sweep.class_hist, 68 * HIST_STEP)
    out = capsys.readouterr().out
    assert out.count("Val Score: ") == 2 and "thr 0.2: Val Score: %s, Dice: " % sweep.scores[0] in out
    assert np.array_equal(xbd.validate_sweep(model, epoch([2, 1]), THR, graph=False).class_hist, 3 * HIST_STEP)


def test_an_epoch_without_batches_is_refused(stand_ins):
    with pytest.raises(ValueError, match="validate: no batches"):
        xbd.validate(Zeros(), epoch([]), graph=False)
    with pytest.raises(ValueError, match="validate_sweep: no batches"):
        xbd.validate_sweep(Zeros(), epoch([]), THR, graph=False)
    assert stand_ins.images == 0


def test_cpu_batches_are_refused(no_library):
    for run in (lambda: xbd.validate(Zeros(), epoch([2]), graph=False), lambda: xbd.validate_sweep(Zeros(), epoch([2]), THR, graph=False)):
        with pytest.raises(_lib.HipLibraryError, match="xBD validation runs on MI355X only"):
            run()
