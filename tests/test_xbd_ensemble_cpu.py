"""The numpy restatement of the xBD predictor for several snapshots and 4 or 8 views (tests/_xbd_ensemble_cases.py): the views
are the symmetries of the square, the restatement contains the 4-flip one and is numpy's mean over the script's stack, the
conditions under which the GPU comparisons may be exact or banded hold -- and the parts of the interface that need no GPU."""
import ctypes

import numpy as np
import pytest
import torch

import _xbd_ensemble_cases as E
import _xbd_tta_cases as T


def test_the_eight_views_are_the_symmetries_of_the_square():
    x = np.random.RandomState(1).randint(0, 256, (3, 7, 7)).astype(np.float32)
    assert E.asymmetric(x)
    views = [E.view(x, v) for v in range(8)]
    for a in range(8):
        for b in range(a + 1, 8):
            assert not np.array_equal(views[a], views[b]), (a, b)
    for k in (1, 3):
        r = np.rot90(x, k, axes=(-2, -1))
        assert sum(np.array_equal(r, w) for w in views) == 1, "rot90 by %d quarter turns is one of the views" % k
    assert np.array_equal(views[4], x.swapaxes(-1, -2)) and np.array_equal(views[7], x[:, ::-1, ::-1].swapaxes(-1, -2))
    for v in range(8):
        assert np.array_equal(E.unview(views[v], v), x), v
        assert np.array_equal(E.view(x, v)[1, 2, 5], T.flip(x, v & 3)[1, 5, 2] if v >= 4 else T.flip(x, v)[1, 2, 5])
    # not square: the four flips only
    y = np.arange(2 * 5 * 9, dtype=np.float32).reshape(2, 5, 9)
    for v in range(4):
        assert np.array_equal(E.unview(E.view(y, v), v), y)


def test_the_restatement_contains_the_four_flip_one():
    pre, post = T.sources(2, 9, 13, seed=2)
    for order in ("bgr", "rgb"):
        assert np.array_equal(E.pack_views(pre, post, order, 4).view(np.uint32), T.pack(pre, post, order).view(np.uint32))
    pre, post = T.sources(2, 11, 11, seed=3)
    p8, p4 = E.pack_views(pre, post, "bgr", 8), T.pack(pre, post, "bgr")
    assert p8.shape == (16, 6, 11, 11)
    for n in range(2):
        for k in range(4):
            assert np.array_equal(p8[8 * n + k], p4[4 * n + k]) and np.array_equal(p8[8 * n + 4 + k], p4[4 * n + k].swapaxes(1, 2))
    for N, H, W, seed in ((1, 37, 41, 4), (2, 40, 40, 5)):
        logits = T.random_logits(N, H, W, seed)
        assert np.array_equal(E.merge_multi([logits], 4), T.merge(logits))
        assert np.array_equal(E.merge_multi64([logits], 4), T.merge64(logits))
    with pytest.raises(AssertionError):
        E.pack_views(*T.sources(1, 8, 12, seed=6), V=8)


@pytest.mark.parametrize("M,V", [(1, 8), (2, 4), (3, 4), (2, 8), (3, 8), (4, 8), (8, 4)])
def test_sequential_sum_and_true_division_are_numpys_mean_over_the_stack(M, V):
    """M V in {8, 12, 16, 24, 32}: bit for bit; at 12 and 24 a multiplication by the reciprocal is something else"""
    K = M * V
    assert K in (8, 12, 16, 24, 32)
    s_list = [T.sigmoid32(l) for l in E.random_multi(M, V, 1, 24, seed=K)]
    pred = E.stack(s_list, V, 0)
    assert len(pred) == K
    want = np.asarray(pred).mean(axis=0)
    assert want.dtype == np.float32
    got = E.mean32(pred)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    t = pred[0]
    for u in pred[1:]:
        t = t + u
    recip = t * (np.float32(1) / np.float32(K))
    differ = int((recip.view(np.uint32) != want.view(np.uint32)).sum())
    print("M V = %d: multiplying by the reciprocal changes %d of %d means" % (K, differ, want.size))
    assert (differ > 0) == (K in (12, 24))
    # merge_multi is that mean, times 255, truncated, channels last
    logits = E.random_multi(M, V, 1, 24, seed=K)
    assert np.array_equal(E.merge_multi(logits, V)[0], (want * 255).astype('uint8').transpose(1, 2, 0))


@pytest.mark.parametrize("M,V", [(1, 4)] + list(E.EXACT_MV))
def test_three_level_logits_meet_their_conditions(M, V):
    for N, S in ((1, 33), (2, 12)):
        out = E.check_three_level_multi(E.three_level_multi(M, V, N, S, seed=M * 100 + V * 10 + S), V)
        assert out.shape == (N, S, S, 5) and len(np.unique(out)) > 8
    logits, L = E.equivariant_multi(M, V, 33, seed=9)
    out = E.check_three_level_multi(logits, V)
    assert set(np.unique(out).tolist()) == {0, 127, 255}
    assert np.array_equal(out[0], np.trunc(T.sigmoid32(L) * np.float32(255)).astype(np.uint8).transpose(1, 2, 0))
    if M > 1:
        logits, region = E.one_hot_models(M, V, 33, seed=10)
        out = E.check_three_level_multi(logits, V)
        assert (out == 255 // M).all()


def test_a_count_that_is_no_power_of_two_is_refused_for_exact_tests():
    with pytest.raises(AssertionError):
        E.check_three_level_multi(E.three_level_multi(3, 8, 1, 8, seed=1), 8)


@pytest.mark.parametrize("M,V,S,N,seed", E.RANDOM_CASES)
def test_random_logits_leave_few_bytes_undecided(M, V, S, N, seed):
    logits = E.random_multi(M, V, N, S, seed)
    v = E.merge_multi64(logits, V)
    got = E.merge_multi(logits, V)
    share = T.check_against_merge64(got, v)
    m32 = np.stack([(E.mean32(E.stack([T.sigmoid32(l) for l in logits], V, n)) * np.float32(255)).transpose(1, 2, 0) for n in range(N)])
    print("M V = %d, %d x %d: undecided bytes %.3f %%, float32 value at most %.1e of a byte from the float64 one"
          % (M * V, S, S, 100 * share, float(np.abs(m32 - v).max())))
    assert np.abs(m32 - v).max() < T.BAND / 10


def test_header_declares_both_entry_points():
    from dahitra_amd import _lib
    p = _lib.prototypes()
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert p["dh_xbd_tta_pack_views_u8"] == (i, [vp, vp, i, i, i, i, i, vp, vp])       # pre, post, N, H, W, bgr, V, inp, stream
    assert p["dh_xbd_tta_merge_multi_u8"] == (i, [vp, i, i, i, i, i, vp, vp])          # table, M, V, N, H, W, out, stream


class Untouchable:
    """stands in for the library: any use is a failure"""

    def __getattr__(self, name):
        raise AssertionError("the library was touched: %s" % name)


@pytest.fixture
def no_library(monkeypatch):
    from dahitra_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: Untouchable())


def test_refusals_happen_before_the_library_is_touched(no_library):
    from dahitra_amd import _lib, ops
    from dahitra_amd.models import xbd
    net = torch.nn.Identity()
    pre = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    wide = torch.zeros(1, 8, 12, 3, dtype=torch.uint8)
    with pytest.raises(_lib.HipLibraryError):
        xbd.predict_ensemble([net, net], pre, pre)
    with pytest.raises(_lib.HipLibraryError):
        xbd.predict_ensemble([net], pre, pre, views=8, graph=False)
    for models in ([], (), [net] * 9, net, None):
        with pytest.raises(ValueError):
            xbd.predict_ensemble(models, pre, pre)
    for views in (0, 2, 6, 16, "8", True, None):
        with pytest.raises(ValueError):
            xbd.predict_ensemble([net], pre, pre, views=views)
    with pytest.raises(ValueError):
        xbd.predict_ensemble([net], pre, pre, order="grb")
    # CPU tensors, then what the two ops refuse about their arguments (a meta tensor claims the device without one)
    with pytest.raises((ValueError, _lib.HipLibraryError)):
        ops.xbd_tta_pack_views(pre, pre)
    with pytest.raises((ValueError, _lib.HipLibraryError)):
        ops.xbd_tta_merge_multi([torch.zeros(4, 5, 8, 8)])
    for lst in ([], [torch.zeros(4, 5, 8, 8)] * 9, torch.zeros(4, 5, 8, 8)):
        with pytest.raises(ValueError):
            ops.xbd_tta_merge_multi(lst)
    for views in (0, 2, 16, True):
        with pytest.raises(ValueError):
            ops.xbd_tta_pack_views(pre, pre, views=views)
        with pytest.raises(ValueError):
            ops.xbd_tta_merge_multi([torch.zeros(16, 5, 8, 8)], views=views)
    with pytest.raises(ValueError):
        ops.xbd_tta_pack_views(wide, wide, views=8)
    with pytest.raises(ValueError):
        ops.xbd_tta_merge_multi([torch.zeros(8, 5, 8, 12)], views=8)
    with pytest.raises(ValueError):
        ops.xbd_tta_pack_views(pre, wide)
    with pytest.raises(ValueError):
        ops.xbd_tta_merge_multi([torch.zeros(4, 5, 8, 8), torch.zeros(4, 5, 8, 12)])
    with pytest.raises(ValueError):
        ops.xbd_tta_merge_multi([torch.zeros(12, 5, 8, 8)], views=8)               # no multiple of 8


def test_predict_ensemble_refuses_mismatched_pairs_before_the_library_is_touched(no_library, monkeypatch):
    """tensors that say they are on the device (is_cuda is patched: no GPU here) reach the shape checks"""
    from dahitra_amd.models import xbd
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    net = torch.nn.Identity()
    pre = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    wide = torch.zeros(1, 8, 12, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="one shape"):
        xbd.predict_ensemble([net], pre, wide)
    with pytest.raises(ValueError, match="square"):
        xbd.predict_ensemble([net, net], wide, wide, views=8)
    from dahitra_amd import ops
    with pytest.raises(ValueError, match="square"):
        ops.xbd_tta_pack_views(wide, wide, views=8)
    with pytest.raises(ValueError, match="square"):
        ops.xbd_tta_merge_multi([torch.zeros(8, 5, 8, 12)], views=8)
    with pytest.raises(ValueError, match="like pre_u8"):
        ops.xbd_tta_pack_views(pre, wide)
    with pytest.raises(ValueError, match="like logits_list"):
        ops.xbd_tta_merge_multi([torch.zeros(4, 5, 8, 8), torch.zeros(4, 5, 8, 12)])
    with pytest.raises(ValueError, match="float32"):
        ops.xbd_tta_merge_multi([torch.zeros(4, 5, 8, 8), torch.zeros(4, 5, 8, 8, dtype=torch.float64)])
    with pytest.raises(ValueError, match="not contiguous"):
        ops.xbd_tta_merge_multi([torch.zeros(4, 5, 8, 8), torch.zeros(4, 5, 8, 16)[..., ::2]])
