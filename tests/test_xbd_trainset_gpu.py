"""The xBD training set on the MI355X: the class table of the resident labels (csrc/xbd_classes.hip, ops.xbd_class_table,
GpuXbdPipeline.class_table / file_classes), epochs over an index list (`indices`, `drop_last` of batches / unet_batches,
`indices` of models/xbd.unet_val_batches) and unet_trainset / trainset end to end.  Everything is integer or a byte-exact
loader: every comparison is exact.  The table's reference is numpy's bincount per file (tests/_xbd_trainset_cases.table_np, held
against the scripts' `c in msk1` in test_xbd_trainset_cpu.py), computed once per shape and shared.  The largest table input is
2 MB; the validation loader's fixed crop at (512, 512) needs two 514 x 514 sources, 1.6 MB a stack."""
import functools
import random

import numpy as np
import pytest
import torch

import _xbd_trainset_cases as C
import _xbd_unet_cases as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                  # a copy: the shared cases are read-only


def filled_table(n):
    """an output buffer whose every byte is 0xAA"""
    return torch.full((n, 6), -0x55555556, dtype=torch.int32, device=DEV)


def same_batch(a, b):
    return (a['fn'] == b['fn'] and torch.equal(a['msk'], b['msk']) and torch.equal(a['lbl_msk'], b['lbl_msk'])
            and a['img'].shape == b['img'].shape and torch.equal(a['img'].view(torch.int32), b['img'].view(torch.int32)))


@functools.lru_cache(maxsize=None)
def pipe(n, H, W):
    from dahitra_amd.datasets.xbd_pipeline import GpuXbdPipeline
    return GpuXbdPipeline(*(dev(a) for a in U.sources(n, H, W)))


@functools.lru_cache(maxsize=None)
def known_pipe(H=40, W=52):
    from dahitra_amd.datasets.xbd_pipeline import GpuXbdPipeline
    return GpuXbdPipeline(*(dev(a) for a in C.known_sources(H, W)), files=C.file_names(len(C.KNOWN_CLASSES), (1, 5)))


# train.py's loader draws a resized_crop box of up to 200 pixels off the crop (draw_train_params): its epochs need a crop above 200
TRAIN_PY_SIDE, TRAIN_PY_CROP = 208, 204


def test_the_chunk_is_the_one_the_shapes_were_placed_around():
    from dahitra_amd import _lib, ops
    assert _lib.lib().dh_xbd_class_table_chunk() == C.CHUNK and C.CHUNK % 16 == 0
    assert {(3, C.CHUNK - 1), (2, C.CHUNK), (2, C.CHUNK + 1), (2, 2 * C.CHUNK + 33)} <= set(C.SHAPES)
    assert len(ops.XBD_CLASS_COLUMNS) == 6


@pytest.mark.parametrize("n,hw", C.SHAPES)
def test_the_table_equals_bincount_per_file(n, hw):
    from dahitra_amd import ops
    assert (0xAA * 0x01010101) - (1 << 32) == -0x55555556
    for name, (labels, want) in C.label_cases(n, hw).items():
        d = dev(labels)
        keep = d.clone()
        out = filled_table(n)
        assert ops.xbd_class_table(d, out=out) is out
        got = out.cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, want), (name, got.tolist(), want.tolist())
        again = ops.xbd_class_table(d)                                   # a fresh buffer: the same bits
        assert again.dtype == torch.int32 and again.shape == (n, 6) and torch.equal(again, out), name
        assert torch.equal(d, keep), name                               # the input is not written


def test_a_slice_with_an_unaligned_base_pointer():
    from dahitra_amd import ops
    stack = np.random.RandomState(5).randint(0, 7, size=(4, 1, 17)).astype(np.uint8)
    d = dev(stack)
    part = d[1:]
    assert part.is_contiguous() and part.data_ptr() % 16 == 1 and d.data_ptr() % 16 == 0
    assert np.array_equal(ops.xbd_class_table(part, out=filled_table(3)).cpu().numpy(), C.table_np(stack[1:]))
    # ... and at every offset of a 16-byte piece, around one chunk, where head, body and tail all exist
    hw = C.CHUNK + 21
    flat = np.random.RandomState(6).randint(0, 256, size=16 + 2 * hw).astype(np.uint8)
    dflat = dev(flat)
    for off in range(16):
        view = dflat[off:off + 2 * hw].view(2, 1, hw)
        assert view.data_ptr() % 16 == off
        got = ops.xbd_class_table(view, out=filled_table(2)).cpu().numpy()
        assert np.array_equal(got, C.table_np(flat[off:off + 2 * hw].reshape(2, hw))), off


def test_the_table_refuses_what_it_cannot_read():
    from dahitra_amd import _lib, ops
    good = dev(np.zeros((2, 3, 5), dtype=np.uint8))
    out = filled_table(2)
    keep = out.clone()
    # the C entry: non-zero, dh_last_error set, nothing written
    for args in ((ops.P(None), 2, 15, ops.P(out)), (ops.P(good), 2, 15, ops.P(None)), (ops.P(good), 0, 15, ops.P(out)),
                 (ops.P(good), -1, 15, ops.P(out)), (ops.P(good), 2, 0, ops.P(out)), (ops.P(good), 2, -4, ops.P(out)),
                 (ops.P(good), 2, 2 ** 31, ops.P(out))):
        assert _lib.lib().dh_xbd_class_table_u8(*args, ops.S()) != 0
        assert _lib.lib().dh_last_error().decode().startswith("xbd_class_table")
        with pytest.raises(_lib.HipLibraryError, match="xbd_class_table"):
            ops._call("dh_xbd_class_table_u8", *args, ops.S())
    torch.cuda.synchronize()
    assert torch.equal(out, keep)
    # the wrapper, before any launch
    with pytest.raises(_lib.HipLibraryError, match="xbd_class_table"):
        ops.xbd_class_table(torch.zeros(2, 3, 5, dtype=torch.uint8))
    huge = torch.zeros(1, dtype=torch.uint8, device=DEV).expand(1, 1 << 16, 1 << 15)            # H * W = 2^31, one byte of storage
    for bad in (good.to(torch.int32), good.to(torch.int8), good.transpose(1, 2), good[:, :, ::2], good[:0], good[0], huge,
                torch.zeros(2, 0, 5, dtype=torch.uint8, device=DEV), good.cpu().numpy()):
        with pytest.raises(ValueError, match="xbd_class_table"):
            ops.xbd_class_table(bad)
    for bad_out in (torch.zeros(2, 6, dtype=torch.int64, device=DEV), torch.zeros(3, 6, dtype=torch.int32, device=DEV),
                    torch.zeros(2, 6, dtype=torch.int32), torch.zeros(2, 12, dtype=torch.int32, device=DEV)[:, ::2]):
        with pytest.raises(ValueError, match="xbd_class_table"):
            ops.xbd_class_table(good, out=bad_out)
    assert np.array_equal(ops.xbd_class_table(good).cpu().numpy(), [[15, 0, 0, 0, 0, 0]] * 2)


def test_class_table_and_file_classes_of_a_pipeline(monkeypatch):
    from dahitra_amd import ops
    from dahitra_amd.datasets.xbd_pipeline import GpuXbdPipeline
    src = U.sources(3, 40, 52)
    p = GpuXbdPipeline(*(dev(a) for a in src))                              # a fresh one: nothing cached
    table = p.class_table()
    assert table.dtype == np.int64 and table.shape == (3, 6) and np.array_equal(table, C.table_np(src[3]))
    fc = p.file_classes()
    assert fc.dtype == np.bool_ and fc.shape == (3, 4)
    assert np.array_equal(fc, [[c in src[3][k] for c in range(1, 5)] for k in range(3)])
    # the second call is the kept array: no launch
    monkeypatch.setattr(ops, "xbd_class_table", lambda *a, **k: pytest.fail("class_table launched again"))
    assert p.class_table() is table and np.array_equal(p.file_classes(), fc)
    with pytest.raises(ValueError):
        table[0, 0] = 1                                                     # read-only: it is the cache


INDICES = [2, 2, 0, 1, 2]


@pytest.mark.parametrize("drop_last", [False, True])
def test_unet_batches_over_an_index_list(drop_last):
    from dahitra_amd.datasets.xbd_pipeline import draw_unet_params
    S, H, W = 37, 40, 52
    p = pipe(3, H, W)
    given = list(INDICES)
    got = list(p.unet_batches(4, S, random.Random(11), indices=given, drop_last=drop_last))
    assert given == INDICES                                                 # a copy is shuffled
    assert len(got) == (len(INDICES) // 4 if drop_last else len(INDICES) // 4 + 1)
    assert [b['img'].shape[0] for b in got] == ([4] if drop_last else [4, 1])
    rng = random.Random(11)
    order = list(INDICES)
    rng.shuffle(order)
    for s, b in zip(range(0, len(order), 4), got):
        ind = order[s:s + 4]
        want = p.make_unet_batch(ind, S, [draw_unet_params(rng, H, W, S)[0] for _ in ind])
        assert same_batch(b, want) and b['fn'] == [p.files[i] for i in ind]
    fns = sorted(f for b in got for f in b['fn'])
    if not drop_last:
        assert fns == sorted(p.files[i] for i in INDICES)
    else:
        assert fns == sorted(p.files[i] for i in order[:4])


@pytest.mark.parametrize("drop_last", [False, True])
def test_batches_over_an_index_list(drop_last):
    from dahitra_amd.datasets.xbd_pipeline import draw_train_params
    S, H, W = TRAIN_PY_CROP, TRAIN_PY_SIDE, TRAIN_PY_SIDE
    p = pipe(3, H, W)
    got = list(p.batches(4, S, train=True, rng=random.Random(12), indices=tuple(INDICES), drop_last=drop_last))
    assert [b['img'].shape[0] for b in got] == ([4] if drop_last else [4, 1])
    rng = random.Random(12)
    order = list(INDICES)
    rng.shuffle(order)
    for s, b in zip(range(0, len(order), 4), got):
        ind = order[s:s + 4]
        want = p.make_batch(ind, S, [draw_train_params(rng, H, W, S)[0] for _ in ind], train=True)
        assert same_batch(b, want) and b['fn'] == [p.files[i] for i in ind]
    if not drop_last:
        assert sorted(f for b in got for f in b['fn']) == sorted(p.files[i] for i in INDICES)


def test_no_indices_is_every_sample_once():
    S, H, W = 37, 40, 52
    p, t = pipe(3, H, W), pipe(3, TRAIN_PY_SIDE, TRAIN_PY_SIDE)
    for epoch in (lambda **kw: p.unet_batches(2, S, random.Random(3), **kw),
                  lambda **kw: t.batches(2, TRAIN_PY_CROP, rng=random.Random(3), **kw)):
        a, b, c = list(epoch()), list(epoch(indices=range(3))), list(epoch(indices=None, drop_last=False))
        assert len(a) == len(b) == len(c) == 2 and all(same_batch(x, y) and same_batch(x, z) for x, y, z in zip(a, b, c))
    # ... and the generators leave equally seeded streams at the same place
    r1, r2 = random.Random(4), random.Random(4)
    list(p.unet_batches(2, S, r1))
    list(p.unet_batches(2, S, r2, indices=[0, 1, 2]))
    assert r1.getstate() == r2.getstate()


def test_validation_over_an_index_list():
    from dahitra_amd.models import xbd
    q = pipe(3, 40, 40)
    val = [2, 0]
    got = list(q.batches(1, 40, train=False, indices=val))
    assert len(got) == 2 and all(same_batch(b, q.make_batch([i], 40, None, train=False)) for b, i in zip(got, val))
    assert [b['fn'] for b in got] == [[q.files[2]], [q.files[0]]]
    got = list(q.batches(2, 40, train=False, indices=[1, 1, 0], drop_last=True))
    assert len(got) == 1 and same_batch(got[0], q.make_batch([1, 1], 40, None, train=False))
    # the script's ValData crops at (512, 512)
    big = pipe(2, 514, 514)
    val = [1, 0, 1]
    got = list(xbd.unet_val_batches(big, 2, 2, indices=val))
    row = [512, 512, 0, 0, 0, 0, 0, 2, 2]
    assert len(got) == 2 and same_batch(got[0], big.make_batch([1, 0], 2, [row, row], train=False))
    assert same_batch(got[1], big.make_batch([1], 2, [row], train=False))
    every = list(xbd.unet_val_batches(big, 2, 2))
    assert len(every) == 1 and same_batch(every[0], big.make_batch([0, 1], 2, [row, row], train=False))


def test_epochs_refuse_an_empty_list_and_an_index_outside():
    from dahitra_amd.models import xbd
    S, H, W = 37, 40, 52
    p = pipe(3, H, W)
    sq = pipe(3, 40, 40)
    for bad in ([], [3], [0, -1], [0, 1, 2, 3]):
        for epoch in (lambda: p.unet_batches(2, S, random.Random(0), indices=bad), lambda: p.batches(2, S, rng=random.Random(0), indices=bad),
                      lambda: sq.batches(2, 40, train=False, indices=bad), lambda: xbd.unet_val_batches(p, 2, 2, indices=bad)):
            with pytest.raises(ValueError, match="indices"):
                next(iter(epoch()))
    # nothing was drawn on the way to the refusal
    rng = random.Random(9)
    with pytest.raises(ValueError, match="indices"):
        next(p.unet_batches(2, S, rng, indices=[7]))
    assert rng.getstate() == random.Random(9).getstate()


def test_the_unet_scripts_trainset_end_to_end():
    from dahitra_amd.datasets import xbd_pipeline as X
    p = known_pipe()
    label = C.known_sources()[3]
    fc = np.array([[c in label[k] for c in range(1, 5)] for k in range(len(label))])
    assert np.array_equal(p.file_classes(), fc)
    train, val = p.unet_trainset(seed=0)
    train0, val0 = X.split_indices(12, 0.1, 0)
    assert np.array_equal(val, val0) and np.array_equal(train, X.unet_train_indices(fc, train0))
    assert np.array_equal(train, C.script_unet_train_indices(fc, train0)) and len(train) > len(train0)
    S, bs = 37, 4
    got = list(p.unet_batches(bs, S, random.Random(321), indices=train, drop_last=True))
    assert len(got) == len(train) // bs and all(b['img'].shape == (bs, 6, S, S) for b in got)
    shown = sorted(f for b in got for f in b['fn'])
    order = [int(i) for i in train]
    random.Random(321).shuffle(order)
    assert shown == sorted(p.files[i] for i in order[:len(got) * bs])
    # the held-out files are never trained on
    assert len(val) == 2 and not {p.files[int(i)] for i in val} & set(shown)


def test_the_train_scripts_trainset_end_to_end(capsys):
    from dahitra_amd.datasets import xbd_pipeline as X
    p = known_pipe(TRAIN_PY_SIDE, TRAIN_PY_SIDE)
    fc = p.file_classes()
    train, val, rng = p.trainset(seed=0)
    line = capsys.readouterr().out.split()
    train0, val0 = X.split_indices(12, 0.1, 0)
    want = C.script_train_indices(p.files, list(fc), train0, random.Random(321))
    assert np.array_equal(val, val0) and np.array_equal(train, want[0])
    assert [int(v) for v in line] == [want[1], want[2], len(train), len(val)]
    # the returned rng goes on where the script's stands: one draw per index of train_idxs0
    fresh = random.Random(321)
    for _ in range(len(train0)):
        fresh.random()
    assert rng.getstate() == fresh.getstate()
    given = random.Random(5)
    assert p.trainset(seed=0, rng=given)[2] is given
    # an epoch over it, the ragged batch dropped
    got = list(p.batches(4, TRAIN_PY_CROP, train=True, rng=rng, indices=train, drop_last=True))
    assert len(got) == len(train) // 4 and all(b['img'].shape[0] == 4 for b in got)
