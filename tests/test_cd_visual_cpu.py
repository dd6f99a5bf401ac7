"""The numpy restatement of the CD evaluator's picture (tests/_cd_visual_cases.py) against a per-pixel loop, against what
matplotlib and PIL really write, and on the pinned byte values.  No GPU."""
import io

import numpy as np
import pytest

import _cd_visual_cases as V


def test_restatement_equals_the_per_pixel_form():
    for shape in V.SMALL:
        a, b, logits, label = V.inputs(*shape)
        N, C, H, W = shape
        rows, cols = V.grid_dims(N)
        got = V.picture(a, b, logits, label)
        assert got.shape == (4 * rows * H, cols * W, 3) and got.dtype == np.uint8
        assert np.array_equal(got, V.picture_slow(a, b, logits, label)), shape
        assert np.array_equal(got, V.picture(a, b, logits, label[:, 0])), "the label as [N, H, W]"
        # the inputs can tell a wrong rule from the right one: values outside [-1, 1], ties, every kind of label
        assert (np.abs(a) > 1).any() and set(np.unique(label).tolist()) <= set(V.LABELS)
        top = logits.max(axis=1, keepdims=True)
        assert ((logits == top).sum(axis=1) > 1).mean() > 0.1
    assert V.grid_dims(1) == (1, 1) and V.grid_dims(8) == (1, 8) and V.grid_dims(9) == (2, 8) and V.grid_dims(17) == (3, 8)
    # the empty tiles of the second row are black in all four bands
    a, b, logits, label = V.inputs(9, 2, 3, 4)
    pic = V.picture(np.full_like(a, 2), np.full_like(b, 1), logits, np.ones_like(label)).reshape(4, 2, 3, 8 * 4, 3)
    assert (pic[:, 1, :, 4:] == 0).all() and (pic[(0, 1, 3), 1, :, :4] == 255).all()


def test_restatement_is_what_matplotlib_and_pil_write():
    pytest.importorskip("matplotlib")
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from PIL import Image
    for shape in ((3, 2, 16, 12), (9, 2, 8, 8)):
        args = V.inputs(*shape)
        vis, want = V.float_picture(*args), V.picture(*args)
        buf = io.BytesIO()
        plt.imsave(buf, vis, format='png')
        rgba = np.asarray(Image.open(io.BytesIO(buf.getvalue())))
        assert rgba.shape == want.shape[:2] + (4,) and (rgba[..., 3] == 255).all()
        assert np.array_equal(rgba[..., :3], want), shape
        ref, ours = io.BytesIO(), io.BytesIO()
        plt.imsave(ref, vis, format='jpg')
        Image.fromarray(want).save(ours, format='jpeg')
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(ref.getvalue())).convert("RGB")),
                              np.asarray(Image.open(io.BytesIO(ours.getvalue())))), shape
        assert len(ref.getvalue()) == len(ours.getvalue())


def test_pinned_byte_values():
    for H, W in V.PINNED_HW:
        args = V.pinned_inputs(H, W)
        V.check_pinned(V.picture(*args), H, W)
        V.check_pinned(V.picture_slow(*args), H, W)
    # the kernel's arithmetic: the float32 product truncates as the float64 product does at fl(k / 255) and both its
    # neighbours, k = 1 .. 255.  Both products increase with t, so these are the only float32 t at which they could part.
    t = V.boundary_t().ravel()
    assert np.array_equal(np.floor((t * V.F32(255)).astype(V.F32)), np.floor(t.astype(np.float64) * 255))
    # x * 0.5 is exact, so a fused multiply-add (float64 sum, rounded once) gives de_norm's float32
    x = np.concatenate([g for g in V.pinned_x().values()])
    assert np.array_equal((x.astype(np.float64) * 0.5 + 0.5).astype(V.F32), (x * V.F32(0.5) + V.F32(0.5)).astype(V.F32))


def test_arguments_are_checked_before_any_launch():
    import ctypes
    import torch
    from dahitra_amd import _lib, ops
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert _lib.prototypes()["dh_cd_eval_vis_u8"] == (i, [vp, vp, vp, vp, i, i, i, i, vp, vp])
    assert ops.cd_vis_shape(1, 5, 7) == (20, 7, 3) and ops.cd_vis_shape(9, 16, 16) == (128, 128, 3)
    a = torch.zeros(2, 3, 8, 8)
    lg = torch.zeros(2, 2, 8, 8)
    lab = torch.zeros(2, 1, 8, 8, dtype=torch.int64)
    for args, name in (((a[0], a, lg, lab), "a"), ((a.double(), a, lg, lab), "a"), ((a[:, :2], a, lg, lab), "a"),
                       ((a, a[:1], lg, lab), "b"), ((a, a.half(), lg, lab), "b"), ((a, a, lg[:, :, :4], lab), "logits"),
                       ((a, a, lg[0], lab), "logits"), ((a, a, lg, lab.int()), "label"), ((a, a, lg, lab[:, :, :4]), "label"),
                       ((a, a, lg, lab[:, 0, 0]), "label"), ((None, a, lg, lab), "a")):
        with pytest.raises(ValueError, match=name):
            ops.cd_eval_vis(*args)
    for out in (torch.zeros(32, 16, 3), torch.zeros(32, 16, 4, dtype=torch.uint8), torch.zeros(16, 16, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="out"):
            ops.cd_eval_vis(a, a, lg, lab, out=out)
    with pytest.raises(_lib.HipLibraryError):               # well-formed, on the CPU: there is no CPU path
        ops.cd_eval_vis(a, a, lg, lab)
    with pytest.raises(_lib.HipLibraryError):
        ops.cd_eval_vis(a, a, lg, lab[:, 0], out=torch.zeros(32, 16, 3, dtype=torch.uint8))
