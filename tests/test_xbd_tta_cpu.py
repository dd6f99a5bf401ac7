"""The numpy restatement of the xBD predictor's 4-flip merge (tests/_xbd_tta_cases.py) against the literal expressions of
xBD_code/predict_test_cls.py:69-94, and the parts of the prediction interface that need no GPU."""
import ctypes

import numpy as np
import pytest
import torch

import _xbd_tta_cases as T


def unflipped(seed=3, shape=(5, 37, 41)):
    """four float32 sigmoid maps, each seen through the script's own un-flip view"""
    s = T.sigmoid32(np.random.RandomState(seed).randn(4, *shape) * 3)
    return s[0], s[1][:, ::-1, :], s[2][:, :, ::-1], s[3][:, ::-1, ::-1]


def test_sequential_sum_is_numpys_mean_over_the_stack_and_the_pairwise_sum_is_not():
    u = unflipped()
    want = np.asarray([u[0], u[1], u[2], u[3]]).mean(axis=0)
    assert want.dtype == np.float32
    got = T.mean32(*u)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    pairwise = ((u[0] + u[1]) + (u[2] + u[3])) / np.float32(4)
    differ = int((pairwise.view(np.uint32) != want.view(np.uint32)).sum())
    print("pairwise sum: %d of %d means differ in their bits" % (differ, want.size))
    assert differ > 0, "the order of the four additions matters"
    # merge() is that mean, times 255, truncated, channels last -- on the flips T.flip names
    logits = T.random_logits(1, 37, 41, seed=4)
    s = T.sigmoid32(logits)
    lit = (np.asarray([s[0], s[1][:, ::-1, :], s[2][:, :, ::-1], s[3][:, ::-1, ::-1]]).mean(axis=0) * 255).astype('uint8')
    assert np.array_equal(T.merge(logits)[0], lit.transpose(1, 2, 0))


def test_pack_is_the_in_place_normalisation_on_every_byte_and_the_scripts_flips():
    pre = np.arange(256, dtype=np.uint8).reshape(1, 4, 64, 1).repeat(3, axis=3)
    post = pre[:, ::-1].copy()
    got = T.pack(pre, post, "rgb")
    x = np.concatenate([pre[0], post[0]], axis=2).astype('float32')       # preprocess_inputs as written
    x /= 127
    x -= 1
    lit = np.asarray([x, x[::-1, ...], x[:, ::-1, ...], x[::-1, ::-1, ...]], dtype='float').transpose((0, 3, 1, 2)).astype(np.float32)
    assert got.shape == (4, 6, 4, 64) and np.array_equal(got.view(np.uint32), lit.view(np.uint32))
    assert len(np.unique(got[0, 0])) == 256
    # the kernel's expression, (float)v / 127.f - 1.f, on all 256 values
    v = np.arange(256, dtype=np.float32)
    assert np.array_equal(got[0, 0].reshape(-1), v / np.float32(127) - np.float32(1))
    # 'bgr' reverses each image's triple and nothing else
    a, b = T.sources(2, 5, 7, seed=1)
    rgb, bgr = T.pack(a, b, "rgb"), T.pack(a, b, "bgr")
    assert np.array_equal(bgr, rgb[:, [2, 1, 0, 5, 4, 3]]) and not np.array_equal(bgr, rgb)
    assert np.array_equal(rgb[4 + 3, 4], (b[1, ::-1, ::-1, 1].astype(np.float32) / np.float32(127)) - np.float32(1))


def test_three_level_logits_meet_their_conditions():
    for N, H, W in ((1, 37, 41), (2, 40, 40)):
        out = T.check_three_level(T.three_level(N, H, W, seed=N * 100 + H))
        assert set(np.unique(out).tolist()) == set(T.BYTES), "every byte of the nine occurs"
    logits, L = T.equivariant(37, 41, seed=9)
    out = T.check_three_level(logits)
    assert set(np.unique(out).tolist()) == {0, 127, 255}
    assert np.array_equal(out[0], np.trunc(T.sigmoid32(L) * np.float32(255)).astype(np.uint8).transpose(1, 2, 0))


def test_random_logits_leave_few_bytes_undecided():
    logits = T.random_logits(1, 37, 41, seed=5)
    share = T.check_against_merge64(T.merge(logits), T.merge64(logits))
    print("undecided bytes: %.3f %%" % (100 * share))


def test_predict_names_are_the_scripts_with_its_doubled_extension():
    from dahitra_amd.models import xbd
    f = "guatemala-volcano_00000003_pre_disaster.png"
    assert xbd.predict_names(f) == ("guatemala-volcano_00000003_pre_disaster_full.png.png.npy",
                                    "guatemala-volcano_00000003_pre_disaster_part1.png.png",
                                    "guatemala-volcano_00000003_pre_disaster_part2.png.png")


def test_header_declares_both_entry_points():
    from dahitra_amd import _lib
    p = _lib.prototypes()
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert p["dh_xbd_tta_pack_u8"] == (i, [vp, vp, i, i, i, i, vp, vp])          # pre, post, N, H, W, bgr, inp, stream
    assert p["dh_xbd_tta_merge_u8"] == (i, [vp, i, i, i, vp, vp])                # logits, N, H, W, out, stream


def test_cpu_tensors_and_ensembles_are_refused():
    from dahitra_amd import _lib, ops
    from dahitra_amd.models import xbd
    pre = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(_lib.HipLibraryError):
        xbd.predict_tta(torch.nn.Identity(), pre, pre)
    with pytest.raises(NotImplementedError):
        xbd.predict_tta([torch.nn.Identity(), torch.nn.Identity()], pre, pre)
    with pytest.raises(ValueError):
        xbd.predict_tta(torch.nn.Identity(), pre, pre, order="grb")
    with pytest.raises(ValueError):
        ops.xbd_tta_pack(pre, pre)
    with pytest.raises(ValueError):
        ops.xbd_tta_merge(torch.zeros(4, 5, 8, 8))
