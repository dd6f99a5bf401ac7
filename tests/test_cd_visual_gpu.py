"""The CD evaluator's picture on the MI355X: dh_cd_eval_vis_u8 (csrc/cd_visual.hip) through ops.cd_eval_vis against the numpy
restatement of the reference's models/evaluator.py:118-131 (tests/_cd_visual_cases.py), then CDEvaluator.vis_picture and the
eval_<batch_id>.jpg files of eval_models on the golden LEVIR pairs.  Every comparison is on bytes."""
import os
import types

import numpy as np
import pytest
import torch

import _cd_visual_cases as V
import cdnet_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
NAME = "base_transformer_pos_s4"
SENTINEL = 0xA5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def offset_view(a, offset=1, whole=False):
    """a device copy of the array `a` that starts `offset` bytes into a larger buffer of sentinel bytes (whole: and that buffer)"""
    buf = torch.full((a.nbytes + 32,), SENTINEL, dtype=torch.uint8, device=DEV)
    view = buf[offset:offset + a.nbytes].view(torch.from_numpy(a).dtype).view(a.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return (view, buf) if whole else view


@pytest.fixture(scope="module")
def cases():
    """inputs and the restatement's picture per shape, computed once and left unchanged"""
    out = {}
    for shape in V.SHAPES:
        args = V.inputs(*shape)
        out[shape] = (args, V.picture(*args))
    return out


@pytest.mark.parametrize("shape", V.SHAPES)
def test_kernel_is_byte_equal_to_the_restatement(cases, shape):
    from dahitra_amd import ops
    (a, b, logits, label), want = cases[shape]
    N, C, H, W = shape
    da, db, dlg, dlab = (dev(t) for t in (a, b, logits, label))
    assert ops.cd_vis_shape(N, H, W) == want.shape
    out = torch.full(want.shape, SENTINEL, dtype=torch.uint8, device=DEV)          # every byte of a given buffer is written
    got = ops.cd_eval_vis(da, db, dlg, dlab, out=out)
    assert got is out and np.array_equal(got.cpu().numpy(), want)
    fresh = ops.cd_eval_vis(da, db, dlg, dlab[:, 0].contiguous())                  # the label as [N, H, W]
    assert fresh.shape == want.shape and fresh.dtype == torch.uint8 and torch.equal(fresh, out)


@pytest.mark.parametrize("shape", [(3, 2, 16, 12), (9, 2, 16, 16), (1, 2, 5, 7)])
def test_unaligned_pointers_give_the_aligned_result(cases, shape):
    """out 1 byte into a larger buffer goes pixel by pixel, 4 bytes in keeps the dword stores; a source 4 bytes off its
    16-byte address goes pixel by pixel too; nothing outside the output is written"""
    from dahitra_amd import ops
    (a, b, logits, label), want = cases[shape]
    aligned = [dev(t) for t in (a, b, logits, label)]
    assert all(t.data_ptr() % 16 == 0 for t in aligned)
    for offset in (1, 4):
        out, whole = offset_view(np.full(want.shape, SENTINEL, dtype=np.uint8), offset, whole=True)
        assert out.data_ptr() % 16 == offset
        ops.cd_eval_vis(*aligned, out=out)
        assert np.array_equal(out.cpu().numpy(), want), offset
        rest = torch.cat([whole[:offset], whole[offset + want.size:]])
        assert bool((rest == SENTINEL).all()), "nothing outside the output is written"
    for which in range(4):
        args = list(aligned)
        args[which] = offset_view((a, b, logits, label)[which], 8 if which == 3 else 4)
        assert args[which].data_ptr() % 16 != 0
        assert np.array_equal(ops.cd_eval_vis(*args).cpu().numpy(), want), which


def test_planted_ties_give_argmax_masks_class():
    from dahitra_amd import ops
    from dahitra_amd.models.losses import argmax_mask
    for shape in ((8, 5, 8, 8), (2, 2, 256, 256), (3, 2, 16, 12)):
        N, C, H, W = shape
        a, b, logits, label = V.inputs(*shape)
        top = logits.max(axis=1, keepdims=True)
        assert ((logits == top).sum(axis=1) > 1).mean() > 0.1, "ties decide many pixels"
        dlg = dev(logits)
        mask = argmax_mask(dlg)
        assert np.array_equal(mask.cpu().numpy(), V.first_max(logits))
        pic = ops.cd_eval_vis(dev(a), dev(b), dlg, dev(label))
        rows, cols = V.grid_dims(N)
        band = pic.view(4, rows, H, cols, W, 3)[2].permute(0, 2, 1, 3, 4).reshape(rows * cols, H, W, 3)[:N]
        white = (mask >= 1).to(torch.uint8) * 255
        assert torch.equal(band, white[..., None].expand(-1, -1, -1, 3))
        assert 0 < int((mask >= 1).sum()) < mask.numel()


@pytest.mark.parametrize("H,W", V.PINNED_HW)
def test_pinned_byte_values(H, W):
    from dahitra_amd import ops
    args = V.pinned_inputs(H, W)
    got = ops.cd_eval_vis(*(dev(t) for t in args)).cpu().numpy()
    V.check_pinned(got, H, W)
    assert np.array_equal(got, V.picture(*args))


def test_refused_arguments_raise_and_launch_nothing():
    from dahitra_amd import _lib, ops
    a = torch.zeros(2, 3, 8, 8, device=DEV)
    lg = torch.zeros(2, 2, 8, 8, device=DEV)
    lab = torch.zeros(2, 1, 8, 8, dtype=torch.int64, device=DEV)
    out = torch.full((32, 16, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    good = dict(a=a, b=a, logits=lg, label=lab, out=out)
    wide = torch.zeros(2, 3, 8, 16, device=DEV)
    for kw in (dict(a=a[0]), dict(a=a.double()), dict(b=a[:1]), dict(b=wide[..., ::2]), dict(logits=lg[:, :, :4]),
               dict(logits=lg.half()), dict(label=lab.int()), dict(label=lab[:, :, :4]), dict(label=lab.cpu()), dict(a=a.cpu()),
               dict(out=out.cpu()), dict(out=out[:16]), dict(out=out.float()),
               dict(out=torch.zeros(32, 16, 4, dtype=torch.uint8, device=DEV)[..., :3])):
        with pytest.raises(ValueError):
            ops.cd_eval_vis(**dict(good, **kw))
    with pytest.raises(_lib.HipLibraryError):
        ops.cd_eval_vis(a.cpu(), a.cpu(), lg.cpu(), lab.cpu())
    # what the library itself refuses
    L, P, S = _lib.lib(), ops.P, ops.S
    base = dict(A=P(a), B=P(a), logits=P(lg), label=P(lab), N=2, C=2, H=8, W=8, out=P(out))
    order = ("A", "B", "logits", "label", "N", "C", "H", "W", "out")
    for change in (dict(N=0), dict(N=-1), dict(C=0), dict(H=0), dict(W=0), dict(H=1 << 16, W=1 << 15), dict(A=P(None)),
                   dict(B=P(None)), dict(logits=P(None)), dict(label=P(None)), dict(out=P(None)),
                   dict(N=1 << 20, H=1 << 15, W=1 << 15)):
        args = dict(base, **change)
        assert L.dh_cd_eval_vis_u8(*[args[k] for k in order], S()) != 0, change
        assert L.dh_last_error().decode().startswith("cd_eval_vis"), (change, L.dh_last_error())
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    ops.cd_eval_vis(**good)                                                        # the good call does write: x = 0 is byte 127
    assert bool((out[:16] == 127).all()) and bool((out[16:] == 0).all())


# ---- evaluator -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def levir(tmp_path_factory):
    """a checkpoint in the reference's format; the data are the four shipped LEVIR pairs (tests/golden/levir)"""
    ck = tmp_path_factory.mktemp("cdvis")
    torch.save({"epoch_id": 0, "best_val_acc": 0.1, "best_epoch_id": 0, "model_G_state_dict": O.large_margin_state(NAME)},
               ck / "best_ckpt.pt")
    return ck


def run_evaluator(ck, vis_dir, batch_size=2, **kw):
    """eval_models over the four pairs, batch 2 at 256 -> scores, and per batch (vis_picture, A, B, G_pred, L) on the host"""
    from torch.utils.data import DataLoader
    from dahitra_amd.datasets.CD_dataset import CDDataset
    from dahitra_amd.models.evaluator import CDEvaluator
    os.makedirs(vis_dir, exist_ok=True)
    args = types.SimpleNamespace(gpu_ids=[0], n_class=2, net_G=NAME, compute_dtype="fp32", vis_dir=str(vis_dir),
                                 checkpoint_dir=str(ck), **kw)
    data = CDDataset(root_dir=os.path.join(G, "levir"), img_size=256, split="train", is_train=False, label_transform="norm")
    loader = DataLoader(data, batch_size=batch_size, shuffle=False, num_workers=0)
    ev = CDEvaluator(args=args, dataloader=loader)
    seen = []
    save = ev._save_vis

    def recording():
        seen.append((ev.batch_id, ev.vis_picture().cpu().numpy(), ev.batch["A"].cpu().numpy(), ev.batch["B"].cpu().numpy(),
                     ev.G_pred.detach().float().cpu().numpy(), ev.batch["L"].long().cpu().numpy()))
        save()
    ev._save_vis = recording
    return ev, ev.eval_models(), seen


def test_evaluator_writes_nothing_without_save_vis(levir, tmp_path):
    ev, scores, seen = run_evaluator(levir, tmp_path / "vis")
    assert not ev.save_vis and seen == [] and os.listdir(str(tmp_path / "vis")) == []
    assert int(ev.confusion.sum()) == 4 * 256 * 256


def test_evaluator_writes_the_references_pictures(levir, tmp_path):
    from PIL import Image
    import io
    plain = run_evaluator(levir, tmp_path / "plain")[1]
    runs = {}
    for graph in (True, False):
        vis = tmp_path / ("graph" if graph else "eager")
        ev, scores, seen = run_evaluator(levir, vis, save_vis=True, hip_graph=graph)
        assert ev.save_vis and (ev._graph is not None) == graph
        assert scores == plain, "the pictures change no score"
        assert sorted(os.listdir(str(vis))) == ["eval_0.jpg", "eval_1.jpg"] and [s[0] for s in seen] == [0, 1]
        for i, pic, a, b, pred, lab in seen:
            assert pic.shape == (4 * 256, 2 * 256, 3) and pic.dtype == np.uint8
            assert np.array_equal(pic, V.picture(a, b, pred, lab)), (graph, i)
            assert 0 < int((pic[2 * 256:3 * 256] == 255).sum()) < pic[:256].size, "a degenerate prediction cannot pass"
            buf = io.BytesIO()
            Image.fromarray(pic).save(buf, format='jpeg')
            img = Image.open(str(vis / ("eval_%d.jpg" % i)))
            assert img.mode == "RGB" and img.size == (2 * 256, 4 * 256)
            assert np.array_equal(np.asarray(img), np.asarray(Image.open(io.BytesIO(buf.getvalue())))), (graph, i)
        runs[graph] = [s[1] for s in seen]
    assert all(np.array_equal(g, e) for g, e in zip(runs[True], runs[False])), "graph and eager paths paint the same bytes"
    assert not np.array_equal(runs[True][0], runs[True][1])


def test_ragged_last_batch_gets_its_picture(levir, tmp_path):
    """batch 3 over four pairs: the recorded step paints eval_0.jpg with three tiles, the eager forward of the last pair eval_1.jpg"""
    from PIL import Image
    ev, scores, seen = run_evaluator(levir, tmp_path / "vis", batch_size=3, save_vis=True)
    assert ev._graph is not None and [s[1].shape for s in seen] == [(4 * 256, 3 * 256, 3), (4 * 256, 256, 3)]
    for i, pic, a, b, pred, lab in seen:
        assert np.array_equal(pic, V.picture(a, b, pred, lab)), i
        assert Image.open(str(tmp_path / "vis" / ("eval_%d.jpg" % i))).size == (pic.shape[1], pic.shape[0])
    assert sorted(os.listdir(str(tmp_path / "vis"))) == ["eval_0.jpg", "eval_1.jpg"]
