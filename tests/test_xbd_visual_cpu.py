"""The numpy restatement of the xBD damage map and visual grid (tests/_xbd_visual_cases.py) against a per-pixel form, against
numpy's argmax and the BGR picture built on float64 zeros (what xBD_code/visualize_results.py:206-220 arrives at), and the parts of the interface that need no GPU."""
import ctypes

import numpy as np
import pytest
import torch

import _xbd_visual_cases as V


@pytest.fixture(scope="module")
def cases():
    return [(V.masks(*s, seed=V.seed_of(*s)),) + V.pictures(*s, seed=V.seed_of(*s)) for s in V.SMALL]


def test_inputs_can_tell_a_wrong_rule_from_the_right_one(cases):
    for msk, _, _, gt in cases:
        c = V.input_conditions(msk)
        print(c)
        assert set(np.unique(msk).tolist()) == set(V.ALPHABET)
        assert c["classes"] == [1, 2, 3, 4], "every class occurs"
        assert c["tie_share"] >= 0.10, "ties for the maximum decide many pixels"
        assert c["clause1"] > 0 and c["clause2_alone"] > 0 and c["clause3_alone"] > 0 and c["dropped"] > 0
        assert c["clause3_alone_classes"] == [4], "what clause 2 does not cover of clause 3 is class 4"
        assert sorted(np.unique(gt).tolist()) == [0, 1, 2, 3, 4]
        # each loc of the tests gives another map
        maps = [V.damage_map(msk, loc) for loc in V.LOCS]
        assert not any(np.array_equal(maps[i], maps[j]) for i in range(3) for j in range(i))


def test_restatement_equals_the_per_pixel_form(cases):
    for msk, pre, post, gt in cases:
        for loc in V.LOCS:
            assert np.array_equal(V.damage_map(msk, loc), V.damage_map_slow(msk, loc)), loc
        for loc in (None, V.SCRIPT_THR):
            got = V.vis_grid(pre, post, gt, msk, loc)
            assert got.shape == msk.shape[:2] + (4 * msk.shape[2], 3) and got.dtype == np.uint8
            assert np.array_equal(got, V.vis_grid_slow(pre, post, gt, msk, loc)), loc
    # a label outside the table
    msk, pre, post, gt = (a[:, :5, :7] for a in cases[0])
    gt = gt.copy()
    gt[0, 1, 2], gt[0, 4, 6] = 5, 255
    got = V.vis_grid(pre, post, gt, msk)
    assert np.array_equal(got, V.vis_grid_slow(pre, post, gt, msk))
    assert tuple(got[0, 1, 14 + 2]) == tuple(got[0, 4, 14 + 6]) == V.MAGENTA and int((got[0, :, 14:21] == V.MAGENTA).all(-1).sum()) == 2


def test_restatement_equals_numpys_argmax_and_the_bgr_picture_on_float64_zeros(cases):
    t0, t1, t2 = V.SCRIPT_THR
    bgr = np.array([V.COLOURS[c][::-1] for c in range(5)], dtype=np.uint8)        # the RGB table seen in cv2's channel order
    assert bgr.tolist() == [[0, 0, 0], [0, 255, 0], [0, 255, 255], [0, 127, 255], [0, 0, 255]]
    for msks, pres, posts, gts in cases:
        for msk, pre, post, gt in zip(msks, pres, posts, gts):
            H, W = gt.shape
            dmg = msk[..., 1:].argmax(axis=2) + 1
            assert np.array_equal(V.damage_map(msk), dmg)
            p = msk[..., 0] / 255
            assert p.dtype == np.float64
            keep = np.zeros((H, W), dtype=bool)
            keep[p > t0] = True
            keep[(p > t1) & np.isin(dmg, (2, 3))] = True
            keep[(p > t2) & (dmg != 1)] = True
            ruled = np.where(keep, dmg, 0)
            assert np.array_equal(V.damage_map(msk, V.SCRIPT_THR), ruled)
            # the picture the way the script's array comes about: float64 zeros, the images in BGR, a table lookup per panel,
            # then a saturating cast that leaves integral values in 0 .. 255 unchanged
            for out, loc in ((dmg, None), (ruled, V.SCRIPT_THR)):
                grid = np.zeros((H, 4 * W, 3))
                for k, panel in enumerate((pre[..., ::-1], post[..., ::-1], bgr[gt], bgr[out])):
                    grid[:, k * W:(k + 1) * W] = panel
                assert grid.dtype == np.float64 and np.array_equal(grid, np.rint(grid)) and 0 <= grid.min() and grid.max() <= 255
                assert np.array_equal(V.vis_grid(pre, post, gt, msk, loc)[..., ::-1], grid.astype(np.uint8))


def test_loc_bounds_are_the_float64_comparison_on_every_byte():
    from dahitra_amd import ops
    assert ops.XBD_LOC_THR == V.SCRIPT_THR
    assert ops.xbd_loc_bounds(None) == (0, 0, 0, 0)
    assert ops.xbd_loc_bounds(V.SCRIPT_THR) == (1, 97, 34, 36)
    assert ops.xbd_loc_bounds(0.2) == (1, 52, 52, 52), "ceil(0.2 * 255) = 51, but 51 / 255 > 0.2 is false"
    assert ops.xbd_loc_bounds(1.0) == (1, 256, 256, 256)
    assert ops.xbd_loc_bounds(-0.5) == (1, 0, 0, 0)
    assert ops.xbd_loc_bounds([0.0, np.float32(0.5), 254 / 255]) == (1, 1, 128, 255)
    for one in (np.float64(0.2), np.array(0.2), torch.tensor(0.2, dtype=torch.float64), np.array([0.2, 0.2, 0.2]), 1):
        assert ops.xbd_loc_bounds(one) == ((1, 52, 52, 52) if not isinstance(one, int) else (1, 256, 256, 256)), one
    p = np.arange(256) / 255
    rs = np.random.RandomState(5)
    ts = np.concatenate([rs.uniform(-0.1, 1.1, 700), p[rs.randint(0, 256, 300)]])          # on the grid of bytes too
    for t in ts.tolist():
        use, b0, b1, b2 = ops.xbd_loc_bounds(t)
        assert use == 1 and b0 == b1 == b2 and 0 <= b0 <= 256
        assert np.array_equal(np.arange(256) >= b0, p > t), t
    for bad in (float("nan"), float("inf"), -float("inf"), (0.1, float("nan"), 0.2), (0.1, 0.2), (0.1, 0.2, 0.3, 0.4), "abc", ()):
        with pytest.raises(ValueError):
            ops.xbd_loc_bounds(bad)


def test_visual_name_is_the_scripts_with_its_missing_underscore():
    from dahitra_amd.models import xbd
    assert xbd.visual_name("x_pre_disaster.png") == "TUNet_x_visdisaster.png"
    assert xbd.visual_name("x_pre_disaster_part1.png") == "TUNet_x_visdisaster.png"
    assert xbd.visual_name("guatemala-volcano_00000003_pre_disaster.png", model_str="m") == "m_guatemala-volcano_00000003_visdisaster.png"


def test_header_declares_both_entry_points():
    from dahitra_amd import _lib
    p = _lib.prototypes()
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert p["dh_xbd_damage_map_u8"] == (i, [vp, i, i, i, i, i, i, i, vp, vp])      # msk, N, H, W, use_loc, b0, b1, b2, out, stream
    assert p["dh_xbd_vis_grid_u8"] == (i, [vp, vp, vp, vp, i, i, i, i, i, i, i, vp, vp])


def test_arguments_are_checked_before_any_launch():
    from dahitra_amd import _lib, ops
    from dahitra_amd.models import xbd
    msk = torch.zeros(1, 8, 8, 5, dtype=torch.uint8)
    img = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    gt = torch.zeros(1, 8, 8, dtype=torch.uint8)
    for bad, name in ((msk[0], "msk_u8"), (msk.float(), "msk_u8"), (img, "msk_u8"), (None, "msk_u8"), (msk, "msk_u8")):      # the last: CPU
        with pytest.raises(ValueError, match=name):
            ops.xbd_damage_map(bad)
        with pytest.raises(ValueError, match=name):
            ops.xbd_vis_grid(img, img, gt, bad)
    # shapes that do not agree, a wrong dtype or rank of the other arguments: named, whatever device they are on
    for args, name in (((img[:, :4], img, gt, msk), "pre_u8"), ((img, img[:, :, :4], gt, msk), "post_u8"),
                       ((img, img, gt[:, :4], msk), "gt_u8"), ((img, img, img, msk), "gt_u8"), ((img, img.int(), gt, msk), "post_u8"),
                       ((gt, img, gt, msk), "pre_u8"), ((img, img, gt.long(), msk), "gt_u8")):
        with pytest.raises(ValueError, match=name):
            ops.xbd_vis_grid(*args)
    with pytest.raises(ValueError, match="out"):
        ops.xbd_vis_grid(img, img, gt, msk, out=torch.zeros(1, 8, 8 * 4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="out"):
        ops.xbd_damage_map(msk, out=torch.zeros(1, 8, 8, 1, dtype=torch.uint8))
    with pytest.raises(ValueError, match="out"):
        ops.xbd_damage_map(msk, out=torch.zeros(1, 8, 8))
    for loc in (float("nan"), (0.1, float("inf"), 0.2), (0.1, 0.2)):
        with pytest.raises(ValueError, match="loc"):
            ops.xbd_damage_map(msk, loc=loc)
        with pytest.raises(ValueError, match="loc"):
            ops.xbd_vis_grid(img, img, gt, msk, loc=loc)
    # CPU tensors at the model level
    with pytest.raises(_lib.HipLibraryError):
        xbd.damage_map(msk)
    with pytest.raises(_lib.HipLibraryError):
        xbd.visual_grid(torch.nn.Identity(), img, img, gt)
    with pytest.raises(_lib.HipLibraryError):
        xbd.visualize_dir(torch.nn.Linear(1, 1), "a", "b", "c")
