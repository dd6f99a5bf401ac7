"""ColorJitter of the xBD device loader on the MI355X (dh_xbd_augment_jitter_u8, csrc/augment_xbd.hip): byte for byte what
TrainData.__getitem__ (xBD_code/train.py:99-183) computes with Pillow -- window, flips, crop(box).resize(BILINEAR), the ImageEnhance
chain in the drawn order on pre and post, the mask channels, preprocess_inputs.  Every comparison is exact: uint32 views of the
float32 images, bytes of the masks.  tests/test_xbd_jitter_cpu.py shows that a fused multiply-add in the blend fails on these
very images and factors."""
import ctypes
import random

import numpy as np
import pytest
import torch

import _xbd_jitter_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def src():
    s = C.sources()
    for a in s:
        a.setflags(write=False)
    return s


def dev_tables(src, idx, rows, S):
    from dahitra_amd.datasets.xbd_pipeline import check_params, coef_table
    _, H, W, _ = src[0].shape
    p = check_params(rows, H, W, S)
    coef = coef_table(p, S)
    return (tuple(torch.from_numpy(np.array(a)).to(DEV) for a in src), torch.tensor(idx, dtype=torch.int32, device=DEV), p.to(DEV),
            coef.to(DEV) if coef is not None else None)


def outputs(n, S):
    """pre-filled with NaN / 255: an element the kernel does not write shows"""
    return (torch.full((n, 6, S, S), float("nan"), dtype=torch.float32, device=DEV),
            torch.full((n, 5, S, S), 255, dtype=torch.uint8, device=DEV))


def call_plain(src, idx, rows, S):
    from dahitra_amd import ops
    (pre, post, _, label), tidx, p, coef = dev_tables(src, idx, rows, S)
    img, msk = outputs(len(idx), S)
    ops._call("dh_xbd_augment_u8", ops.P(pre), ops.P(post), ops.P(None), ops.P(label), ops.P(tidx), ops.P(p), ops.P(coef), len(idx),
              C.H, C.W, S, 0, ops.P(img), ops.P(msk), ops.P(None), ops.S())
    torch.cuda.synchronize()
    return img.cpu().numpy(), msk.cpu().numpy()


def call_jitter(src, idx, rows, S, jitter):
    from dahitra_amd import ops
    from dahitra_amd.datasets.xbd_pipeline import jitter_table, jitter_workspace_bytes
    (pre, post, _, label), tidx, p, coef = dev_tables(src, idx, rows, S)
    n = len(idx)
    img, msk = outputs(n, S)
    table = jitter_table(jitter)
    need = jitter_workspace_bytes(n, S)
    tiles = -(-S // 64) * -(-S // 32)
    assert need == n * 2 * (8 + tiles) * 4
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)               # no fill is assumed
    ops._call("dh_xbd_augment_jitter_u8", ops.P(pre), ops.P(post), ops.P(None), ops.P(label), ops.P(tidx), ops.P(p), ops.P(coef),
              ctypes.c_void_p(table.ctypes.data), n, C.H, C.W, S, 0, ops.P(img), ops.P(msk), ops.P(None), ops.P(ws), need, ops.S())
    torch.cuda.synchronize()
    return img.cpu().numpy(), msk.cpu().numpy()


def assert_equals_host(src, idx, rows, S, jitter, img, msk):
    for n, (i, row, jit) in enumerate(zip(idx, rows, jitter)):
        wimg, wmsk = C.host_sample(src, i, row, S, jit)
        bad = np.argwhere(img[n].view(np.uint32) != wimg.view(np.uint32))
        assert bad.size == 0, ("img", S, n, row, jit, len(bad), bad[:4].tolist())
        bad = np.argwhere(msk[n] != wmsk)
        assert bad.size == 0, ("msk", S, n, row, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("S", [64, 70])
def test_c_abi_equals_the_pillow_chain(src, S):
    """S = 64: two tiles of 64 x 32, the mean spans workgroups.  S = 70: partial tiles in both directions (2 x 3 workgroups, the
    last 6 columns and 6 rows wide) and the scalar stores (70 % 4 = 2).  All six effective orders with hue at every position,
    other parameters for pre and post, rows without and with the box and with both flips, the pinned factors on contrast and
    on saturation, bright (clips at 255), dark (reaches 0) and plain sources."""
    from dahitra_amd.datasets.xbd_pipeline import jitter_reference_u8
    rows, cases = C.rows_for(S), C.jitter_cases()
    img, msk = call_jitter(src, C.IDX, rows, S, cases)
    assert_equals_host(src, C.IDX, rows, S, cases, img, msk)
    plain = call_plain(src, C.IDX, rows, S)
    assert np.array_equal(msk, plain[1])                                        # the labels are not touched
    for n in range(len(rows)):
        assert not np.array_equal(img[n, :3], plain[0][n, :3]) and not np.array_equal(img[n, 3:], plain[0][n, 3:])
    # the numpy statement of the arithmetic says the same as Pillow on these windows (what the kernel was written from), and
    # the clip acts inside the chain: at 255 on both images of the bright samples, at 0 on both of the dark ones (a later
    # operation may move such a byte again, so the final image need not hold it)
    for i, row, case in zip(C.IDX, rows, cases):
        win = C.host_windows(src, i, row, S)
        for im in (0, 1):
            assert np.array_equal(jitter_reference_u8(win[im], *case[im]), C.pil_jitter(win[im], *case[im]))
            hit = C.clips(win[im], *case[im])
            assert hit[255] or i != 0, (i, im, case[im])
            assert hit[0] or i != 1, (i, im, case[im])


def test_c_abi_contrast_mean_of_the_clipped_image(src):
    """brightness 1.2 in front of contrast on the bright source: the mean is the clipped image's"""
    rows = [[3, 1, 0, 0, 0, 0, 0, 64, 64], [3, 1, 0, 0, 0, 0, 0, 64, 64]]
    jit = [(([0, 1, 3, 2], (1.2, 0.8, 1.0)), ([1, 0, 3, 2], (1.2, 0.8, 1.0)))] * 2
    img, msk = call_jitter(src, [0, 0], rows, 64, jit)
    assert_equals_host(src, [0, 0], rows, 64, jit, img, msk)
    pre = C.host_windows(src, 0, rows[0], 64)[0]
    assert not np.array_equal(C.pil_jitter(pre, [0, 1], (1.2, 0.8, 1.0)), C.pil_jitter(pre, [1, 0], (1.2, 0.8, 1.0)))


@pytest.mark.parametrize("S", [32, 37])
def test_wrapper_gives_the_raw_entrys_bytes(S):
    """ops.xbd_augment with a jitter table against dh_xbd_augment_jitter_u8 on the same arguments, into fresh outputs and into
    sentinel-filled ones.  40 x 48 sources; S = 32 takes the vector stores, S = 37 the scalar ones; a repeated index, a sample
    with both flips and ColorJitter, one with the box"""
    from dahitra_amd import ops
    from dahitra_amd.datasets.xbd_pipeline import jitter_table
    small = C.sources(seed=13, h=40, w=48)
    idx = [2, 0, 2]
    rows = [[48 - S, 40 - S, 0, 0, 0, 0, 0, S, S], [2, 1, 1, 1, 0, 0, 0, S, S], [0, 3, 0, 1, 1, 4, 6, S - 7, S - 10]]
    jitter = [None, (([0, 3, 2, 1], (1.1, 0.9, 1.2)), ([1, 0, 2, 3], (0.85, C.PINNED[1], 0.8))), None]
    table = jitter_table(jitter)
    (pre, post, pmask, label), tidx, p, coef = dev_tables(small, idx, rows, S)
    assert coef is not None
    need = ops.xbd_augment_jitter_ws_bytes(3, S)
    want_img, want_msk = outputs(3, S)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    ops._call("dh_xbd_augment_jitter_u8", ops.P(pre), ops.P(post), ops.P(None), ops.P(label), ops.P(tidx), ops.P(p), ops.P(coef),
              ctypes.c_void_p(table.ctypes.data), 3, 40, 48, S, 0, ops.P(want_img), ops.P(want_msk), ops.P(None), ops.P(ws), need, ops.S())
    torch.cuda.synchronize()
    want_img, want_msk = want_img.cpu().numpy(), want_msk.cpu().numpy()
    assert_equals_host(small, idx, rows, S, jitter, want_img, want_msk)

    def same_bytes(got):
        torch.cuda.synchronize()
        assert np.array_equal(got[0].cpu().numpy().view(np.int32), want_img.view(np.int32))
        assert np.array_equal(got[1].cpu().numpy(), want_msk)

    fresh = ops.xbd_augment(pre, post, pmask, label, tidx, p, coef, S, True, table)
    same_bytes(fresh)
    assert fresh[2] is None
    out = outputs(3, S) + (torch.full((3, S, S), 255, dtype=torch.uint8, device=DEV),)
    given = ops.xbd_augment(pre, post, pmask, label, tidx, p, coef, S, True, table, out_img=out[0], out_msk=out[1], out_lbl=out[2],
                            ws=torch.full((need + 4,), 0xFF, dtype=torch.uint8, device=DEV))
    assert all(g is o for g, o in zip(given, out))
    same_bytes(given)
    assert bool((out[2] == 255).all()), "train mode does not write out_lbl"
    plain = ops.xbd_augment(pre, post, pmask, label, tidx, p, coef, S, True)[0].cpu().numpy()
    assert [np.array_equal(plain[n], want_img[n]) for n in range(3)] == [True, False, True]


def make_pipe(src):
    from dahitra_amd.datasets.xbd_pipeline import GpuXbdPipeline
    return GpuXbdPipeline(*(torch.from_numpy(np.array(a)).to(DEV) for a in src), files=["s%d" % i for i in range(len(src[0]))])


def test_mixed_batch_leaves_the_other_samples_alone(src):
    rows, cases = C.rows_for(64), C.jitter_cases()
    mixed = [cases[0], None, None, cases[3], None, cases[5]]
    plain = call_plain(src, C.IDX, rows, 64)
    img, msk = call_jitter(src, C.IDX, rows, 64, mixed)
    assert_equals_host(src, C.IDX, rows, 64, mixed, img, msk)
    for n, jit in enumerate(mixed):
        same = np.array_equal(img[n].view(np.uint32), plain[0][n].view(np.uint32))
        assert same == (jit is None), n
    assert np.array_equal(msk, plain[1])
    # through the loader: the same bytes; no jitter at all is the plain entry's batch
    pipe = make_pipe(src)
    got = pipe.make_batch(C.IDX, 64, rows, jitter=mixed)
    assert np.array_equal(got["img"].cpu().numpy().view(np.uint32), img.view(np.uint32)) and np.array_equal(got["msk"].cpu().numpy(), msk)
    assert got["lbl_msk"].shape == (6, 64, 64) and not got["lbl_msk"].any()
    for none in (None, [None] * 6):
        got = pipe.make_batch(C.IDX, 64, rows, jitter=none)
        assert np.array_equal(got["img"].cpu().numpy().view(np.uint32), plain[0].view(np.uint32))
        assert np.array_equal(got["msk"].cpu().numpy(), plain[1])
    assert pipe._jitter_ws is not None
    # one enabled image of a pair: the jitter table has a row per image
    from dahitra_amd.datasets.xbd_pipeline import jitter_table
    assert jitter_table(mixed)[1].tolist() == [[0] * 8] * 2


EPOCH_SEED = 3          # an epoch of three samples whose second draws ColorJitter (asserted where it is used)


def test_seeded_epoch_equals_the_host_chain():
    """crop 208 in 240 x 232 sources, as the loader's own epoch test: 7 x 4 tiles with ragged edges"""
    from dahitra_amd.datasets.xbd_pipeline import draw_jitter_params, draw_train_params
    src = C.sources(seed=12, h=240, w=232)
    pipe = make_pipe(src)

    def epoch(jitter_seed):
        g = None if jitter_seed is None else torch.Generator().manual_seed(jitter_seed)
        return list(pipe.batches(2, 208, train=True, rng=random.Random(EPOCH_SEED), jitter_gen=g))

    one, two, other, plain = epoch(7), epoch(7), epoch(8), epoch(None)
    # the epoch is: shuffle, then per sample draw_train_params and, if it says so, draw_jitter_params for pre, then post
    rng, g = random.Random(EPOCH_SEED), torch.Generator().manual_seed(7)
    order = [0, 1, 2]
    rng.shuffle(order)
    rows, jitter = [], []
    for _ in order:
        row, flag = draw_train_params(rng, 240, 232, 208)
        rows.append(row)
        jitter.append((draw_jitter_params(g), draw_jitter_params(g)) if flag else None)
    assert any(j is not None for j in jitter) and any(j is None for j in jitter)
    assert [b["fn"] for b in one] == [["s%d" % i for i in order[:2]], ["s%d" % order[2]]]
    flat = lambda ep, key: [b[key][n].cpu().numpy() for b in ep for n in range(b[key].shape[0])]
    for n, (i, row, jit) in enumerate(zip(order, rows, jitter)):
        wimg, wmsk = C.host_sample(src, i, row, 208, jit)
        assert np.array_equal(flat(one, "img")[n].view(np.uint32), wimg.view(np.uint32)), (n, row, jit)
        assert np.array_equal(flat(one, "msk")[n], wmsk)
        assert np.array_equal(flat(two, "img")[n].view(np.uint32), wimg.view(np.uint32))
        assert np.array_equal(flat(plain, "msk")[n], wmsk)
        pimg = C.host_sample(src, i, row, 208, None)[0]
        assert np.array_equal(flat(plain, "img")[n].view(np.uint32), pimg.view(np.uint32))
        assert np.array_equal(flat(other, "img")[n], wimg) == (jit is None)      # other jitter draws, the same Python draws


def test_c_abi_refuses_bad_arguments_and_launches_nothing(src):
    from dahitra_amd import _lib, ops
    from dahitra_amd.datasets.xbd_pipeline import jitter_table, jitter_workspace_bytes
    rows, idx = C.rows_for(64)[:2], [0, 1]
    (pre, post, _, label), tidx, p, coef = dev_tables(src, idx, rows, 64)
    img, msk = outputs(2, 64)
    good = jitter_table([C.jitter_cases()[0], None])
    need = jitter_workspace_bytes(2, 64)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)

    def call(table=good, ws=ws, ws_bytes=need, S=64, H=C.H, W=C.W):
        ops._call("dh_xbd_augment_jitter_u8", ops.P(pre), ops.P(post), ops.P(None), ops.P(label), ops.P(tidx), ops.P(p), ops.P(coef),
                  ctypes.c_void_p(table.ctypes.data if table is not None else 0), 2, H, W, S, 0, ops.P(img), ops.P(msk), ops.P(None),
                  ops.P(ws), ws_bytes, ops.S())

    def edited(word, value, row=0):
        t = good.copy()
        t[0, row, word] = value
        return t

    nan_bits, inf_bits = int(np.float32("nan").view(np.int32)), int(np.float32("inf").view(np.int32))
    bad = [(dict(table=None), "NULL"), (dict(ws=None), "NULL"),
           (dict(table=edited(1, 3)), "operation"), (dict(table=edited(3, -1)), "operation"), (dict(table=edited(2, good[0, 0, 1])), "twice"),
           (dict(table=edited(0, 2, row=1)), "enabled"),
           (dict(table=edited(5, nan_bits)), "finite"), (dict(table=edited(6, inf_bits)), "finite"),
           (dict(ws_bytes=need - 1), "workspace"), (dict(ws_bytes=0), "workspace"),
           # 4097 x 4097 x 255 + half of it does not fit the 32-bit sum; the workspace size is wrong too, so nothing can start
           (dict(S=4097, H=5000, W=5000, ws_bytes=0), "32-bit sum"),
           (dict(S=81), "bad sizes")]
    for kwargs, word in bad:
        with pytest.raises(_lib.HipLibraryError, match=word):
            call(**kwargs)
    torch.cuda.synchronize()
    assert bool(torch.isnan(img).all()) and bool((msk == 255).all())            # nothing was launched
    assert [_lib.lib().dh_xbd_augment_jitter_tiles(s) for s in (0, 64, 70, 1024, 4096, 4097)] == [0, 2, 6, 512, 8192, 0]
    call()                                                                      # and the good call does run
    torch.cuda.synchronize()
    assert not bool(torch.isnan(img).any()) and int(msk.max()) == 1
