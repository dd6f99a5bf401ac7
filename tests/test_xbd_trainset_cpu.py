"""The xBD training set on the host (datasets/xbd_pipeline): split_indices against scikit-learn's train_test_split -- a committed
fixture written from it (tools/make_xbd_split_golden.py), and sklearn itself where it imports --, the two oversampled index
lists against the scripts' loops (tests/_xbd_trainset_cases.py), and the numpy restatement of the class table against the
scripts' own test `c in msk1` on every case the GPU test gives the kernel.  No GPU."""
import hashlib
import json
import os
import random

import numpy as np
import pytest

import _xbd_trainset_cases as C
from dahitra_amd.datasets import xbd_pipeline as X

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "xbd_split.json")
NS = (2, 3, 4, 9, 10, 11, 19, 20, 21, 30, 31, 100, 2799, 9168)
TEST_SIZES = (0.1, 0.15)
SEEDS = (0, 10, 321)


def digest(idxs):
    return hashlib.sha256(np.asarray(idxs).astype("<i8").tobytes()).hexdigest()


def test_split_indices_equals_the_sklearn_fixture():
    cases = json.load(open(GOLDEN))["cases"]
    assert sorted((c["n"], c["test_size"], c["seed"]) for c in cases) == sorted((n, t, s) for n in NS for t in TEST_SIZES for s in SEEDS)
    full = 0
    for c in cases:
        train, val = X.split_indices(c["n"], c["test_size"], c["seed"])
        assert train.dtype == np.int64 and val.dtype == np.int64 and (len(train), len(val)) == (c["n_train"], c["n_val"]), c
        assert sorted(train.tolist() + val.tolist()) == list(range(c["n"]))
        if "train" in c:
            assert train.tolist() == c["train"] and val.tolist() == c["val"], (c["n"], c["test_size"], c["seed"])
            full += 1
        else:
            assert (digest(train), digest(val)) == (c["train_sha256"], c["val_sha256"]), (c["n"], c["test_size"], c["seed"])
    assert full == 12 * 6 and len(cases) - full == 2 * 6
    # the defaults are the scripts': test_size 0.1, seed 0
    a, b = X.split_indices(100)
    c = next(c for c in cases if (c["n"], c["test_size"], c["seed"]) == (100, 0.1, 0))
    assert a.tolist() == c["train"] and b.tolist() == c["val"]


def test_split_indices_equals_sklearn_where_it_imports():
    model_selection = pytest.importorskip("sklearn.model_selection")
    for n in NS:
        for t in TEST_SIZES:
            for s in SEEDS:
                want = model_selection.train_test_split(np.arange(n), test_size=t, random_state=s)
                got = X.split_indices(n, t, s)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (n, t, s)


def test_split_indices_refuses_what_sklearn_refuses():
    for bad in (dict(n=1), dict(n=0), dict(n=-3), dict(n=10, test_size=0.0), dict(n=10, test_size=1.0), dict(n=10, test_size=-0.1),
                dict(n=10, test_size=0.95), dict(n=2.0), dict(n=True)):
        with pytest.raises(ValueError, match="split_indices"):
            X.split_indices(**bad)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_unet_train_indices_equals_the_scripts_loop(seed):
    n = 40
    fc = C.class_rows(n, seed)
    assert all(any((fc[k] == np.array(kind, dtype=bool)).all() for k in range(n)) for kind in C.KINDS)
    idxs0, _ = X.split_indices(n, 0.1, seed)
    want = C.script_unet_train_indices(fc, idxs0)
    got = X.unet_train_indices(fc, idxs0)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    counts = np.bincount(got, minlength=n)
    assert set(counts[idxs0]) == {1, 2, 3} and not counts[np.setdiff1d(np.arange(n), idxs0)].any()
    # the order of train_idxs0 is kept: dropping the repeats gives it back
    assert [i for k, i in enumerate(got.tolist()) if k == 0 or got[k - 1] != i] == idxs0.tolist()


AOI_PLACES = ((), (0,), (17,), (39,), (0, 17, 39), tuple(range(0, 40, 3)))


@pytest.mark.parametrize("aoi_at", AOI_PLACES)
def test_train_indices_equals_the_scripts_loop(aoi_at):
    n, seed = 40, 4
    fc = C.class_rows(n, seed)
    files = C.file_names(n, aoi_at)
    assert [k for k, f in enumerate(files) if 'AOI' in f] == list(aoi_at)
    idxs0, _ = X.split_indices(n, 0.1, seed)
    for given in (files, None):
        # without `files` the rows are the files': the script's loop on names of which none holds 'AOI'
        names = files if given is not None else C.file_names(n, ())
        want = C.script_train_indices(names, list(fc), idxs0, random.Random(seed + 321))
        rng = random.Random(seed + 321)
        got = X.train_indices(fc, idxs0, rng, given)
        assert got[0].dtype == np.int64 and np.array_equal(got[0], want[0]) and got[1:] == want[1:], (aoi_at, given is None)
        assert got[1] + got[2] == len(got[0])
        # one draw per index of train_idxs0, with or without damage
        fresh = random.Random(seed + 321)
        for _ in range(len(idxs0)):
            fresh.random()
        assert rng.getstate() == fresh.getstate()
    if aoi_at and aoi_at[0] < n - 1:
        # the quirk is visible: behind the first 'AOI' path the script reads another file's row (behind the last file is none)
        shifted = X.train_indices(fc, idxs0, random.Random(seed + 321), files)[0]
        meant = X.train_indices(fc, idxs0, random.Random(seed + 321))[0]
        assert not np.array_equal(shifted, meant)
    # a file without a building is dropped, one with damage can appear twice, none more often
    meant = X.train_indices(fc, idxs0, random.Random(seed + 321))[0]
    counts = np.bincount(meant, minlength=n)
    assert not counts[~fc.any(axis=1)].any() and set(counts[idxs0]) == {0, 1, 2}
    assert not (counts[fc.any(axis=1) & ~fc[:, 1:].any(axis=1)] > 1).any()


def test_index_lists_refuse_what_does_not_fit():
    fc = C.class_rows(8, 0)
    for call in (lambda: X.unet_train_indices(fc.astype(np.uint8), [0]), lambda: X.unet_train_indices(fc[:, :3], [0]),
                 lambda: X.unet_train_indices(fc, [8]), lambda: X.unet_train_indices(fc, [-1]),
                 lambda: X.train_indices(fc, [8], random.Random(0)), lambda: X.train_indices(fc, [0], random.Random(0), ["a"] * 7),
                 lambda: X.epoch_order(3, []), lambda: X.epoch_order(3, [0, 3]), lambda: X.epoch_order(3, [-1])):
        with pytest.raises(ValueError):
            call()
    assert X.epoch_order(3, None) == [0, 1, 2] and X.epoch_order(3, np.array([2, 2, 0])) == [2, 2, 0]
    assert X.epoch_order(3, range(3)) == [0, 1, 2]


@pytest.mark.parametrize("n,hw", C.SHAPES)
def test_the_numpy_table_agrees_with_the_scripts_membership_test(n, hw):
    for name, (labels, table) in C.label_cases(n, hw).items():
        assert table.shape == (n, 6) and (table.sum(axis=1) == hw).all() and (table >= 0).all(), name
        for f in range(n):
            msk1 = labels[f]
            fl = np.zeros((4,), dtype=bool)
            for c in range(1, 5):
                fl[c - 1] = c in msk1
            assert ((table[f, 1:5] > 0) == fl).all(), (name, f)
            assert table[f, 0] == (msk1 == 0).sum() and table[f, 5] == (msk1 > 4).sum(), (name, f)


def test_known_sources_hold_the_classes_they_name():
    label = C.known_sources()[3]
    table = C.table_np(label)
    assert [tuple(c for c in range(1, 5) if table[k, c]) for k in range(len(label))] == list(C.KNOWN_CLASSES)
    assert not table[:, 5].any()
    fc = table[:, 1:5] > 0
    train, val = X.split_indices(len(label), 0.1, 0)
    # the end-to-end GPU test oversamples: some training file repeats twice and some three times
    counts = np.bincount(X.unet_train_indices(fc, train), minlength=len(label))
    assert {1, 2, 3} <= set(counts.tolist())
