"""The epoch bodies of the device loaders, without a GPU: GpuXbdPipeline.batches / adapt_batches / unet_batches,
GpuPairPipeline.batches and GpuPairLoader.  Pipelines whose make_*batch only record their arguments run every entry point from
fixed seeds; what they record -- the indices, the drawn rows, the jitter, origins or colours of every batch -- and the state each
generator is left in are compared with a plain restatement of the loop written out here.  A draw taken in another order, or one
more or fewer, changes which augmentation a seed produces: these tests pin the streams."""
import collections
import random

import numpy as np
import pytest
import torch

from dahitra_amd.datasets.gpu_pipeline import GpuPairLoader, GpuPairPipeline
from dahitra_amd.datasets.xbd_pipeline import (GpuXbdPipeline, draw_jitter_params, draw_train_params, draw_unet_colour,
                                               draw_unet_params, unet_colour_names)

N_SRC, H, W = 7, 300, 320
REPEATING = [5, 0, 5, 3, 3, 6, 1, 5, 0, 2, 6]          # 11 samples: batches of 4 leave a ragged tail of 3


class RecordingXbd(GpuXbdPipeline):
    """the three xBD epochs over host tensors; make_*batch record what they are handed"""

    def __init__(self, n=N_SRC, h=H, w=W):
        self.pre = torch.zeros(n, h, w, 3, dtype=torch.uint8)
        self.files = ["f%d" % i for i in range(n)]
        self.unet_skipped, self.unet_applied = collections.Counter(), collections.Counter()
        self.calls = []

    def make_batch(self, indices, crop, params=None, train=True, jitter=None, dilate=0):
        self.calls.append((list(indices), crop, params, train, jitter, dilate))
        return len(self.calls)

    def make_adapt_batch(self, indices, crop, origins=None, train=True):
        self.calls.append((list(indices), crop, origins, train))
        return len(self.calls)

    def make_unet_batch(self, indices, crop, rows, dilate=5, colour=None):
        self.calls.append((list(indices), crop, rows, dilate, colour))
        return len(self.calls)


class RecordingPairs(GpuPairPipeline):
    def __init__(self, n):
        self.n, self.calls = n, []

    def __len__(self):
        return self.n

    def make_batch(self, indices, img_size, flips=None, patch=None, blur=None):
        self.calls.append((list(indices), img_size, None if flips is None else torch.as_tensor(flips).tolist(), patch, blur))
        return len(self.calls)


def same(a, b):
    """equality through lists, tuples, dicts and numpy arrays"""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def np_state_equal(a, b):
    return same(list(a.get_state()), list(b.get_state()))


def chunks(order, batch_size, drop_last):
    out = [order[s:s + batch_size] for s in range(0, len(order), batch_size)]
    return [c for c in out if not (drop_last and len(c) < batch_size)]


def epoch_list(n, indices, train, rng):
    order = list(range(n)) if indices is None else [int(i) for i in indices]
    if train:
        rng.shuffle(order)
    return order


# ---- the restatements: each script's loop as the loaders ran it before they shared one ---------------------------------
def restated_batches(batch_size, crop, train, rng, gen, dilate, indices, drop_last, h=H, w=W, n=N_SRC):
    want = []
    for ind in chunks(epoch_list(n, indices, train, rng), batch_size, drop_last):
        if not train:
            want.append((ind, crop, None, False, None, 0))
            continue
        params, jitter = [], []
        for _ in ind:
            row, flag = draw_train_params(rng, h, w, crop)
            params.append(row)
            pair = None
            if flag and gen is not None:
                pre = draw_jitter_params(gen)
                pair = (pre, draw_jitter_params(gen))
            jitter.append(pair)
        want.append((ind, crop, params, True, jitter if gen is not None else None, dilate))
    return want


def restated_adapt(batch_size, crop, train, rng, indices, drop_last, h=H, w=W, n=N_SRC):
    want = []
    for ind in chunks(epoch_list(n, indices, train, rng), batch_size, drop_last):
        origins = None
        if train:
            origins = []
            for _ in ind:
                x0 = rng.randint(0, w - crop)
                y0 = rng.randint(0, h - crop)
                origins.append((x0, y0))
        want.append((ind, crop, origins, train))
    return want


def restated_unet(batch_size, crop, rng, dilate, colour, np_rng, indices, drop_last):
    want, skipped_all, applied_all = [], collections.Counter(), collections.Counter()
    for ind in chunks(epoch_list(N_SRC, indices, True, rng), batch_size, drop_last):
        rows, colours = [], []
        for _ in ind:
            if colour:
                row, col, skipped = draw_unet_colour(rng, H, W, crop, np_rng)
                colours.append(col)
                applied_all.update(unet_colour_names(col))
            else:
                row, skipped = draw_unet_params(rng, H, W, crop)
            rows.append(row)
            skipped_all.update(skipped)
        want.append((ind, crop, rows, dilate, colours if colour else None))
    return want, skipped_all, applied_all


def restated_pairs(S, batch_size, img_size, train, gen, patch, drop_last, blur, rank=0, world=1):
    order = torch.randperm(S, generator=gen).tolist() if train else list(range(S))
    per = S // world
    want = []
    for ind in chunks(order[rank * per:(rank + 1) * per], batch_size, drop_last):
        flips = (torch.rand(len(ind), 2, generator=gen) > 0.5).int().tolist() if train else None
        radii = torch.rand(len(ind), generator=gen).tolist() if train and blur else None
        want.append((ind, img_size, flips, patch, radii))
    return want


EPOCHS = [dict(indices=None, drop_last=False), dict(indices=REPEATING, drop_last=False), dict(indices=REPEATING, drop_last=True),
          dict(indices=np.array(REPEATING), drop_last=True), dict(indices=None, drop_last=True)]
EPOCH_IDS = ["all", "repeating", "repeating-drop_last", "array-drop_last", "all-drop_last"]


# ---- GpuXbdPipeline.batches ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epoch", EPOCHS, ids=EPOCH_IDS)
@pytest.mark.parametrize("with_jitter", [False, True])
def test_batches_train_draws_as_the_restated_loop(epoch, with_jitter):
    pipe = RecordingXbd()
    jittered = 0
    for seed in (0, 1, 2, 3):                          # two epochs from one pair of generators, then other seeds
        rng, twin = random.Random(seed), random.Random(seed)
        gen = torch.Generator().manual_seed(seed + 50) if with_jitter else None
        gen_twin = torch.Generator().manual_seed(seed + 50) if with_jitter else None
        before = torch.get_rng_state()
        for _ in range(2):
            pipe.calls = []
            got = list(pipe.batches(4, 256, True, rng, gen, 5, **epoch))
            want = restated_batches(4, 256, True, twin, gen_twin, 5, **epoch)
            assert got == list(range(1, len(want) + 1)) and same(pipe.calls, want)
            assert rng.getstate() == twin.getstate()
            assert gen is None or torch.equal(gen.get_state(), gen_twin.get_state())
            jittered += sum(j is not None for c in want if c[4] is not None for j in c[4])
        assert torch.equal(torch.get_rng_state(), before), "nothing is drawn from torch's global generator"
    n = 11 if epoch["indices"] is not None else N_SRC
    assert len(want) == (n // 4 if epoch["drop_last"] else -(-n // 4))
    assert bool(jittered) == with_jitter, "the seeds reach the ColorJitter draws, and only with a generator"


@pytest.mark.parametrize("epoch", EPOCHS, ids=EPOCH_IDS)
def test_batches_validation_takes_the_order_given_and_draws_nothing(epoch):
    pipe = RecordingXbd(N_SRC, 64, 64)
    rng, gen = random.Random(3), torch.Generator().manual_seed(3)
    state, gen_state = rng.getstate(), gen.get_state()
    list(pipe.batches(4, 64, False, rng, gen, **epoch))
    want = restated_batches(4, 64, False, None, None, 0, h=64, w=64, **epoch)
    assert same(pipe.calls, want) and rng.getstate() == state and torch.equal(gen.get_state(), gen_state)
    order = list(range(N_SRC)) if epoch["indices"] is None else REPEATING
    assert [i for c in pipe.calls for i in c[0]] == order[:len(order) // 4 * 4 if epoch["drop_last"] else None]
    pipe.calls = []
    list(pipe.batches(4, 64, False, **epoch))            # and needs no generator at all
    assert same(pipe.calls, want)


# ---- GpuXbdPipeline.adapt_batches ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("epoch", EPOCHS, ids=EPOCH_IDS)
@pytest.mark.parametrize("crop", [256, 300])
def test_adapt_batches_train_draws_as_the_restated_loop(epoch, crop):
    pipe = RecordingXbd()
    rng, twin = random.Random(9), random.Random(9)
    for _ in range(2):
        pipe.calls = []
        list(pipe.adapt_batches(4, crop, True, rng, **epoch))
        want = restated_adapt(4, crop, True, twin, **epoch)
        assert same(pipe.calls, want) and rng.getstate() == twin.getstate()
    assert any(o != (0, 0) for c in want for o in c[2])


@pytest.mark.parametrize("epoch", EPOCHS, ids=EPOCH_IDS)
def test_adapt_batches_validation_takes_the_order_given_and_draws_nothing(epoch):
    pipe = RecordingXbd(N_SRC, 64, 64)
    rng = random.Random(3)
    state = rng.getstate()
    list(pipe.adapt_batches(4, 64, False, rng, **epoch))
    want = restated_adapt(4, 64, False, None, h=64, w=64, **epoch)
    assert same(pipe.calls, want) and rng.getstate() == state and all(c[2] is None for c in pipe.calls)
    pipe.calls = []
    list(pipe.adapt_batches(4, 64, False, **epoch))
    assert same(pipe.calls, want)


# ---- GpuXbdPipeline.unet_batches ----------------------------------------------------------------------------------------
LONG = [i % N_SRC for i in range(403)]                   # long enough to reach the rare colour draws
UNET_SEED = 5                                            # the first seed whose second epoch over LONG draws a gauss_noise


@pytest.mark.parametrize("epoch", EPOCHS + [dict(indices=LONG, drop_last=True)], ids=EPOCH_IDS + ["long"])
@pytest.mark.parametrize("colour,noise", [(False, False), (True, False), (True, True)])
def test_unet_batches_draw_as_the_restated_loop(epoch, colour, noise):
    pipe = RecordingXbd()
    rng, twin = random.Random(UNET_SEED), random.Random(UNET_SEED)
    np_rng, np_twin = (np.random.RandomState(4), np.random.RandomState(4)) if noise else (None, None)
    pipe.unet_skipped["left over"] = pipe.unet_applied["left over"] = 1          # reset when the iteration starts
    for _ in range(2):
        pipe.calls = []
        list(pipe.unet_batches(4, 8, rng, 3, colour, np_rng, **epoch))
        want, skipped, applied = restated_unet(4, 8, twin, 3, colour, np_twin, **epoch)
        assert same(pipe.calls, want) and rng.getstate() == twin.getstate()
        assert not noise or np_state_equal(np_rng, np_twin)
        assert pipe.unet_skipped == skipped and pipe.unet_applied == applied
    if epoch["indices"] is LONG:
        assert sum(skipped.values()) > 0 and (sum(applied.values()) > 0) == colour
        drew_noise = any(col[im] is not None and col[im][0] == "gauss_noise" for c in want if colour for col in c[4]
                         for im in ("pre", "post"))
        assert drew_noise == noise, "the seed reaches gauss_noise, which draws from np_rng"


# ---- GpuPairPipeline.batches and GpuPairLoader ------------------------------------------------------------------------------
@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("train,blur", [(True, False), (True, True), (False, False), (False, True)])
def test_pair_batches_draw_as_the_restated_loop(train, blur, drop_last):
    pipe = RecordingPairs(11)
    gen, twin = torch.Generator().manual_seed(21), torch.Generator().manual_seed(21)
    before = torch.get_rng_state()
    for patch in (None, 5):
        pipe.calls = []
        got = list(pipe.batches(4, 256, train, gen, patch, drop_last, blur))
        want = restated_pairs(11, 4, 256, train, twin, patch, drop_last, blur)
        assert got == list(range(1, len(want) + 1)) and same(pipe.calls, want)
        assert torch.equal(gen.get_state(), twin.get_state()) and len(want) == (2 if drop_last else 3)
    assert torch.equal(torch.get_rng_state(), before)
    if not train:
        assert torch.equal(gen.get_state(), torch.Generator().manual_seed(21).get_state()), "a validation epoch draws nothing"
        assert [i for c in pipe.calls for i in c[0]] == list(range(8 if drop_last else 11))


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("train,blur", [(True, False), (True, True), (False, True)])
def test_pair_loader_draws_as_the_restated_loop_on_every_rank(train, blur, drop_last, world):
    seen = []
    for rank in range(world):
        pipe = RecordingPairs(11)
        gen, twin = torch.Generator().manual_seed(21), torch.Generator().manual_seed(21)
        loader = GpuPairLoader(pipe, 2, 256, train, gen, drop_last, rank, world, blur)
        for _ in range(2):                               # every epoch draws a fresh permutation
            pipe.calls = []
            got = list(loader)
            want = restated_pairs(11, 2, 256, train, twin, None, drop_last or world > 1, blur, rank, world)
            assert got == list(range(1, len(want) + 1)) and same(pipe.calls, want) and len(want) == len(loader)
            assert torch.equal(gen.get_state(), twin.get_state())
        seen.append([i for c in pipe.calls for i in c[0]])
    if world == 2:
        assert len(seen[0]) == len(seen[1]) == 4 and not set(seen[0]) & set(seen[1]), "equal, disjoint shards of one permutation"
        if not train:
            assert seen == [[0, 1, 2, 3], [5, 6, 7, 8]]
