"""tiles.TilePlan and the numpy restatement of dh_cd_tile_stitch (tests/_cd_tile_cases.py), without a GPU: the plan's origins,
view order, rows and refusals; the eval_cd plan against the reference's formula (and its own CDDataAugmentation where the reference tree is present);
the properties of the restatement that make it an oracle, and the mutants those properties must catch."""
import numpy as np
import pytest

import _cd_tile_cases as T
from _xbd_tta_cases import flip
from dahitra_amd.tiles import TilePlan, axis_cover, axis_origins


# ---- plan ----------------------------------------------------------------------------------------------------------------
def test_origins_exact_stride_clamped_last_window_and_whole_tile():
    assert axis_origins(1024, 256, 256) == [0, 256, 512, 768]
    assert axis_origins(1024, 256, 128) == [0, 128, 256, 384, 512, 640, 768]
    assert axis_origins(19, 8, 5) == [0, 5, 10, 11], "the last window is clamped to the edge"
    assert axis_origins(23, 8, 6) == [0, 6, 12, 15]
    assert axis_origins(256, 256, 256) == [0] and axis_origins(256, 256, 7) == [0]
    p = TilePlan(19, 23, (8, 8), (5, 6), (0, 1, 2, 3), "triangle")
    assert (p.ys, p.xs, p.ny, p.nx, p.nf, p.P) == ([0, 5, 10, 11], [0, 6, 12, 15], 4, 4, 4, 64)
    assert TilePlan(256, 256).P == 1 and TilePlan(1024, 1024).P == 16
    assert TilePlan(1024, 1024, stride=(128, 128)).P == 49 and TilePlan(1024, 1024, stride=(128, 128), flips=(0, 1, 2, 3)).P == 196


def test_view_order_and_params_rows():
    p = TilePlan(19, 23, (8, 8), (5, 6), (0, 3, 1), "mean")
    rows = p.params()
    assert rows.dtype == np.int32 and rows.shape == (p.P, 4)
    for iy in range(p.ny):
        for ix in range(p.nx):
            for f, k in enumerate(p.flips):
                # (x0, y0, hflip, vflip): hflip reverses the columns (bit 1), vflip the rows (bit 0)
                assert rows[(iy * p.nx + ix) * p.nf + f].tolist() == [p.xs[ix], p.ys[iy], (k >> 1) & 1, k & 1]
    # the rows cut what flip() of the xBD tests makes of the crop (dh_augment_pairs_u8's indexing, restated)
    img = np.arange(19 * 23).reshape(19, 23)
    for (x0, y0, hf, vf), (_, k) in zip(rows, [(o, k) for o in p.origins() for k in p.flips]):
        yy = y0 + (7 - np.arange(8) if vf else np.arange(8))
        xx = x0 + (7 - np.arange(8) if hf else np.arange(8))
        assert np.array_equal(img[np.ix_(yy, xx)], flip(img[y0:y0 + 8, x0:x0 + 8], k))


def test_cover_tables_name_exactly_the_windows_over_a_position():
    for size, win, stride in ((19, 8, 5), (23, 8, 6), (1024, 256, 128), (1024, 256, 256), (64, 32, 8), (9, 9, 3), (40, 16, 5)):
        o = axis_origins(size, win, stride)
        cov = axis_cover(size, win, o)
        assert cov.shape == (size, 2) and cov.dtype == np.int32
        for t in range(size):
            want = [i for i, v in enumerate(o) if v <= t < v + win]
            assert want and list(range(cov[t, 0], cov[t, 0] + cov[t, 1])) == want, (size, win, stride, t)
    assert axis_cover(19, 8, [0, 5, 10, 11])[:, 1].max() == 3, "cover goes up to three once the last window is clamped"
    assert axis_cover(64, 32, axis_origins(64, 32, 8))[:, 1].max() == 4


def test_weights_and_alignment():
    wy, wx = TilePlan(19, 23, (8, 6), (5, 6), weight="triangle").weights()
    assert wy.dtype == np.float32 and wy.tolist() == [1, 2, 3, 4, 4, 3, 2, 1] and wx.tolist() == [1, 2, 3, 3, 2, 1]
    wy, wx = TilePlan(19, 23, (8, 6), (5, 6)).weights()
    assert wy.tolist() == [1] * 8 and wx.tolist() == [1] * 6
    wy, wx = TilePlan(1024, 1024, stride=(128, 128), weight="triangle").weights()
    g = wy.astype(np.float64)[:, None] * wx.astype(np.float64)[None, :]
    assert g.max() == 128 * 128 and np.array_equal((wy[:, None] * wx[None, :]).astype(np.float64), g), "every product is exact"
    assert TilePlan(1024, 1024, stride=(128, 128)).x_align() == 4 and TilePlan(19, 23, (8, 8), (5, 6)).x_align() == 1
    assert TilePlan(64, 64, (32, 32), (32, 30)).x_align() == 1, "an x origin of 30"


@pytest.mark.parametrize("kw", [dict(window=(300, 256)), dict(window=(256, 300)), dict(stride=(0, 256)), dict(stride=(256, -1)),
                                dict(stride=(257, 256)), dict(stride=(256, 300)), dict(flips=(4,)), dict(flips=(-1,)),
                                dict(flips=(0, 0)), dict(flips=(1, 2, 1)), dict(flips=()), dict(weight="gauss"),
                                dict(window=(0, 256))])
def test_plan_refusals(kw):
    with pytest.raises(ValueError):
        TilePlan(256, 256, **dict(dict(window=(256, 256), stride=(256, 256)), **kw))


def test_plans_are_values():
    a, b = TilePlan(1024, 1024, stride=(128, 128)), TilePlan(1024, 1024, stride=(128, 128))
    assert a == b and hash(a) == hash(b) and a != TilePlan(1024, 1024) and len({a, b, TilePlan.eval_cd(1024, 1024)}) == 2


# ---- eval_cd plan --------------------------------------------------------------------------------------------------------
def test_eval_cd_plan_is_the_references_sixteen_views_as_executed():
    p = TilePlan.eval_cd(1024, 1024)
    assert (p.P, p.nf, p.flips, p.h, p.w) == (16, 1, (0,), 256, 256) and not p.stitchable
    rows = p.params()
    for patch in range(16):          # datasets/data_utils.py:65-68: `if patch:` is false for patch 0
        x0, y0 = (256 * (patch // 4), 256 * (patch % 4)) if patch else (256, 256)
        assert rows[patch].tolist() == [x0, y0, 0, 0]
    assert rows[0].tolist() == rows[5].tolist() == [256, 256, 0, 0], "view 0 repeats view 5"
    assert [0, 0] not in rows[:, :2].tolist(), "the window at (0, 0) is never evaluated"
    assert len({tuple(r) for r in rows[:, :2].tolist()}) == 15
    for bad in (dict(H=1024, W=512), dict(H=1024, W=1000, size=256), dict(H=768, W=1024), dict(H=1024, W=1024, size=512)):
        with pytest.raises(ValueError):
            TilePlan.eval_cd(**bad)
    for call in (p.cover, p.x_align):
        with pytest.raises(ValueError):
            call()


@pytest.fixture
def reference_augmentation():
    """the reference's own CDDataAugmentation, through oracle/ref_import.load_data() (datasets/data_utils.py with the five
    torchvision.transforms.functional primitives it calls supplied; every decision of the crop is the reference's code).  The
    module names the import registers (the reference's `models`, the third-party stand-ins) are taken out again afterwards, so
    that no later test sees them."""
    import sys
    import ref_import
    before = set(sys.modules)
    yield ref_import.load_data()[1].CDDataAugmentation
    for k in set(sys.modules) - before:
        if k.split(".")[0] in ("models", "torchvision", "timm", "segmentation_models_pytorch", "cv2", "sklearn"):
            del sys.modules[k]


def _no_reference():
    import ref_import
    return not ref_import.available()


@pytest.mark.skipif(_no_reference(), reason="the reference tree is not on this machine")
def test_eval_cd_plan_equals_the_references_crops(reference_augmentation):
    aug = reference_augmentation
    yy, xx = np.meshgrid(np.arange(1024), np.arange(1024), indexing="ij")
    img = np.stack([yy % 256, xx % 256, (yy // 256) * 4 + xx // 256], axis=2).astype(np.uint8)      # pixels encode their coordinates
    lab = ((yy // 256) * 4 + xx // 256).astype(np.uint8)
    rows = TilePlan.eval_cd(1024, 1024).params()
    for patch in range(16):
        imgs, labels = aug(img_size=256).transform([img], [lab], to_tensor=False, patch=patch)
        x0, y0 = rows[patch, :2]
        assert np.array_equal(np.asarray(imgs[0]), img[y0:y0 + 256, x0:x0 + 256])
        assert np.array_equal(np.asarray(labels[0]), lab[y0:y0 + 256, x0:x0 + 256])


# ---- the restatement -----------------------------------------------------------------------------------------------------
SMALL = [T.ODD, (3, 17, 40, (8, 16), (3, 5), (2, 1), "mean"), (2, 24, 24, (8, 8), (8, 8), (3,), "triangle"),
         (2, 16, 20, (16, 8), (16, 4), (0, 3), "triangle")]


def test_identity_moves_the_input_bits_into_place():
    plan = T.make_plan(T.IDENTITY)
    lg = T.random_logits(plan, 5, 1)
    out, ws = T.stitch(lg, plan)
    assert np.array_equal(ws, np.ones_like(ws))
    for iy in range(plan.ny):
        for ix in range(plan.nx):
            got = out[:, 32 * iy:32 * iy + 32, 32 * ix:32 * ix + 32]
            assert np.array_equal(got.view(np.uint32), lg[iy * plan.nx + ix].view(np.uint32))


@pytest.mark.parametrize("case", SMALL)
def test_equivariant_views_return_the_field_exactly(case):
    plan = T.make_plan(case)
    F = T.field(case[0], plan.H, plan.W, seed=3)
    T.check_exact(F, plan)
    out, _ = T.stitch(T.views_of(F, plan), plan)
    assert np.array_equal(out, F), "a wrong un-flip or a wrong origin cannot return F"
    assert np.array_equal(T.first_max(out), np.argmax(F, axis=0))          # (no ties survive: argmax's first maximum either way)


@pytest.mark.parametrize("case", SMALL)
def test_vectorised_and_literal_statements_agree_bit_for_bit(case):
    plan = T.make_plan(case)
    lg = T.random_logits(plan, case[0], 5)
    out, _ = T.stitch(lg, plan)
    assert np.array_equal(out.view(np.uint32), T.stitch_literal(lg, plan).view(np.uint32))


@pytest.mark.parametrize("case", SMALL + [T.IDENTITY])
def test_agrees_with_float64_within_the_rounding_of_cover_additions(case):
    """float32: each product g * v is rounded once (u = 2^-24 relative), each of the n = cover additions once, the division
    once; ws is a sum of small integers and exact.  So |out32 - out64| <= (n + 2) u / (1 - (n + 2) u) * sum(g |v|) / sum(g)."""
    plan = T.make_plan(case)
    lg = T.random_logits(plan, case[0], 7)
    out, ws = T.stitch(lg, plan)
    want, cover, mag, ws64 = T.stitch64(lg, plan)
    assert np.array_equal(ws.astype(np.float64), ws64), "ws is exact"
    n = cover + 2
    bound = n * 2.0 ** -24 / (1 - n * 2.0 ** -24) * mag
    err = np.abs(out.astype(np.float64) - want)
    assert (err <= bound[None]).all(), float((err / bound[None]).max())
    over = lambda size, win, origins: max(sum(1 for o in origins if o <= t < o + win) for t in range(size))
    assert cover.max() == over(plan.H, plan.h, plan.ys) * over(plan.W, plan.w, plan.xs) * plan.nf


def test_relabelled_flips_give_the_same_bits():
    """the content of every view as it lies in the tile, stored under another flip code: same (g, v) sequence per pixel"""
    plan = T.make_plan(T.ODD)
    lg = T.random_logits(plan, 2, 11)
    wy, wx = np.arange(1, 9, dtype=np.float32), np.arange(8, 0, -1, dtype=np.float32) * 2          # asymmetric profiles
    want, _ = T.stitch(lg, plan, wy, wx)
    for flips in ((3, 2, 1, 0), (1, 0, 3, 2), (2, 3, 0, 1)):
        lg2, plan2 = T.relabel(lg, plan, flips)
        assert np.array_equal(T.stitch(lg2, plan2, wy, wx)[0].view(np.uint32), want.view(np.uint32)), flips


# ---- mutants: each wrong restatement is caught by one of the properties above ------------------------------------------------
def test_mutant_with_swapped_flips_fails_the_exact_field_property():
    plan = T.make_plan(T.ODD)
    F = T.field(2, plan.H, plan.W, seed=3)
    assert not np.array_equal(T.stitch(T.views_of(F, plan), plan, mutate="flips")[0], F)
    one = T.make_plan((2, 24, 24, (8, 8), (8, 8), (1,), "mean"))          # a single flip code, no overlap: still caught
    F = T.field(2, 24, 24, seed=4)
    assert np.array_equal(T.stitch(T.views_of(F, one), one)[0], F)
    assert not np.array_equal(T.stitch(T.views_of(F, one), one, mutate="flips")[0], F)


def test_mutant_with_the_weight_at_the_flipped_coordinate_fails_relabelling():
    """a weighted mean of equal values is that value under ANY weights, so the exact-field property cannot see this mutant; the
    relabelling property does, under an asymmetric profile (and only there: the plan's own profiles are symmetric)"""
    plan = T.make_plan(T.ODD)
    lg = T.random_logits(plan, 2, 11)
    wy, wx = np.arange(1, 9, dtype=np.float32), np.arange(8, 0, -1, dtype=np.float32) * 2
    F = T.field(2, plan.H, plan.W, seed=3, span=1)
    T.check_exact(F, plan, wy, wx)
    assert np.array_equal(T.stitch(T.views_of(F, plan), plan, wy, wx, mutate="weight")[0], F), "invisible on the exact field"
    lg2, plan2 = T.relabel(lg, plan, (3, 2, 1, 0))
    a, b = T.stitch(lg, plan, wy, wx, mutate="weight")[0], T.stitch(lg2, plan2, wy, wx, mutate="weight")[0]
    assert not np.array_equal(a, b), "caught"
    sym = T.stitch(lg, plan, mutate="weight")[0]
    assert np.array_equal(sym.view(np.uint32), T.stitch(lg, plan)[0].view(np.uint32)), "a symmetric profile hides it"
    assert not np.array_equal(a.view(np.uint32), T.stitch_literal(lg, plan, wy, wx).view(np.uint32))


def test_mutant_with_reversed_cover_order_fails_the_literal_statement():
    """the order of the additions shows in the roundings alone: exact sums (the field property) cannot see it, the bit
    comparison with the literal statement does"""
    plan = T.make_plan(T.ODD)
    F = T.field(2, plan.H, plan.W, seed=3)
    assert np.array_equal(T.stitch(T.views_of(F, plan), plan, mutate="order")[0], F), "invisible where every sum is exact"
    lg = T.random_logits(plan, 2, 5)
    got = T.stitch(lg, plan, mutate="order")[0]
    lit = T.stitch_literal(lg, plan)
    differ = got.view(np.uint32) != lit.view(np.uint32)
    assert differ.any() and np.abs(got - lit).max() < 1e-5, "caught, and it is a matter of the last bits"
    cover = T.stitch64(lg, plan)[1]
    assert not differ[:, cover <= 2].any(), "one or two terms add up the same in either order"


def test_planted_ties_and_nans_survive_the_blend():
    plan = T.make_plan(T.ODD)
    lg = T.plant(T.random_logits(plan, 2, 13), plan, seed=14)
    out, _ = T.stitch(lg, plan)
    tie = out[0] == out[1]
    assert 0.1 < tie.mean() < 0.4 and 0.01 < np.isnan(out).any(axis=0).mean() < 0.2
    m = T.first_max(out)
    assert (m[tie] == 0).all() and (m[np.isnan(out[0])] == 0).all() and (m[np.isnan(out[1])] == 0).all()
    assert 0 < m.sum() < m.size
