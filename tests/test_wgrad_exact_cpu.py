"""CPU side of tests/test_wgrad_exact_gpu.py: every case of tests/_wgrad_exact_cases.py keeps the exactness premise (the float64
reference equals its own float32 evaluation and stays below 2^24), the launch plan grants it the row it states and the edges it
exists for (recomputed from dh_conv2d_wgrad_describe on the host), the table reaches all six kernel families and every
instantiation of conv_wgrad_kernel, and the comparator turns red on one changed pixel and on one dropped tile.  Host code only."""
import ctypes

import pytest
import torch

import _wgrad_exact_cases as E

BATCHED = (E.WS_BATCH, E.C32_BATCH)


@pytest.fixture(scope="module")
def lib():
    from dahitra_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("c", E.CASES, ids=["%s-%s" % (c.group, c.name) for c in E.CASES])
def test_reference_is_exact_in_float32(c):
    """the premise, per case: integer (BatchNorm on load: half-integer) inputs the number formats hold, a float64 reference that
    equals its float32 evaluation bit for bit, every |dW| -- and, with every product replaced by its magnitude, every partial
    sum in any order -- below 2^24 units"""
    d = E.data(c)
    unit = E.granule(c)
    x = E.effective_input(c, d)
    dy = d["dy"].double()
    for name, t in (("x", d["x"].double()), ("effective x", x), ("dy", dy)):
        assert bool((t / unit == (t / unit).round()).all()), (c.name, name)
        assert bool((t.to(E.dtype_of(c)).double() == t).all()), (c.name, name, "not exact in the case's dtype")
        if E.mma_of(c):          # the split fp32 form: the high bf16 plane holds the value, the low plane is 0
            assert bool((t.to(E.BF16).double() == t).all()), (c.name, name, "low plane not 0")
    assert float(d["x"].abs().max()) <= E.IMAX and float(dy.abs().max()) <= E.IMAX
    want = E.reference(c)
    assert tuple(want.shape) == E.dw_shape(c) and want.dtype == torch.float64
    assert torch.equal(E.reference_of(c, d, torch.float32).double(), want)
    assert bool((want / unit == (want / unit).round()).all())
    oh, ow = E.out_hw(c)
    pixels = c.N * oh * ow * (4 if c.form == "phase" else 1)
    worst = float(x.abs().max()) * float(dy.abs().max()) * pixels / unit        # sum of |product| over every pixel, in units
    assert float(want.abs().max()) / unit <= worst < E.EXACT_LIMIT, (c.name, worst)


@pytest.mark.parametrize("c", E.CASES, ids=["%s-%s" % (c.group, c.name) for c in E.CASES])
def test_plan_grants_the_stated_row_and_edges(lib, c):
    r = E.describe(lib, c)
    print("%s %s: %s ct=%d it=%d cig=%d ci_tiles=%d splitk=%d direct=%d grid=%s threads=%d lds=%d, %d tiles" % (
        c.group, c.name, E.FAMILIES[r[0]], r[1], r[2], r[3], r[4], r[5], r[6], r[7:10], r[10], r[11], E.tiles_of(c)))
    assert (r[0], r[1], r[2], r[3], r[5]) == c.row, (c.name, r)
    assert E.tiles_of(c) == c.tiles
    assert r[8] == r[5]                                         # grid y: the K slices
    assert c.edges, c.name
    for e in c.edges:
        assert E.EDGES[e](c, r), "%s: the plan no longer puts this case on its edge '%s' (row %s)" % (c.name, e, r)
    # the same layer recorded into an open batch: the stated batched row, or none where the batch refuses it
    b = E.describe(lib, c, batch=True)
    if c.batch:
        assert c.batch_row is None and b == r
    else:
        assert ((b[0], b[5]) if b[0] in BATCHED else None) == c.batch_row, (c.name, b)
    # the workspace contract: the slabs of the planned launch fit what dh_conv2d_wgrad_workspace_size grants
    oh, ow = E.out_hw(c)
    if c.form != "phase":
        ws = lib.dh_conv2d_wgrad_workspace_size(c.N, oh, ow, c.Cin, c.dy_ch or c.Cout, c.ks, E.weight_groups(c))
        assert E.weight_groups(c) * r[5] * c.ks * c.ks * (c.dy_ch or c.Cout) * c.Cin * 4 <= ws
    else:
        assert 4 * r[5] * 4 * 32 * c.Cin * 4 <= lib.dh_conv2d_wgrad_phase_workspace_size(c.N, c.H, c.W, c.Cin)


def test_table_reaches_every_family_and_every_instantiation(lib):
    """all six families, and every conv_wgrad_kernel instantiation launch_generic can reach -- (ks, stride, dilation, co tile, ci
    channels, ci wave groups, precision) -- at least once WITH a split (split-K > 1 and an uneven, carrying tile walk)"""
    rows = [(c, E.describe(lib, c)) for c in E.CASES]
    assert {r[0] for _, r in rows} == {E.W1, E.WS, E.WS_BATCH, E.C32_BATCH, E.GENERIC, E.PHASE}
    for fam in (E.W1, E.WS, E.WS_BATCH, E.C32_BATCH, E.GENERIC, E.PHASE):
        uneven = E.EDGES["chunks_uneven" if fam == E.W1 else "uneven"]       # (wgrad1x1_kernel walks 64-pixel chunks, not tiles)
        assert any(r[0] == fam and r[5] > 1 and uneven(c, r) for c, r in rows), E.FAMILIES[fam]
    got = {E.instantiation(c, r) for c, r in rows if r[0] in (E.GENERIC, E.PHASE) and r[5] > 1 and E.EDGES["uneven"](c, r)}
    want = E.reachable_instantiations()
    assert len(want) == 100
    assert got == want, "missing %s, beyond the list %s" % (sorted(want - got), sorted(got - want))
    # the wave-specialised kernel in both dilations, with BatchNorm on load and with a split input
    ws = [c for c, r in rows if r[0] == E.WS]
    assert {c.dil for c in ws} == {1, 2} and {c.form for c in ws} == {"plain", "bn", "split"}
    # every precision sees BatchNorm on load, a padded dy and the 4x4 stem form
    for p in range(4):
        mine = [c for c in E.CASES if c.prec == p and c.group == "GENERIC"]
        assert any(c.form == "bn" for c in mine) and any(c.dy_ch for c in mine) and any(c.ks == 4 for c in mine)


def test_reduce_cases_cover_both_forms_and_a_ragged_last_block(lib):
    from dahitra_amd import ops
    assert ctypes.sizeof(ops.WgradPlan._Job) == lib.dh_wgrad_reduce_job_size()
    assert lib.dh_wgrad_reduce_outputs_per_block(E.RED_I_VEC) == 128 and lib.dh_wgrad_reduce_outputs_per_block(E.RED_I_SCALAR) == 32
    assert E.RED_I_VEC % 4 == 0 and E.RED_I_SCALAR % 4 != 0 and E.RED_OSLAB > E.RED_O
    # 8 phases: below, at, above; the unrolled loop takes 32 slabs per trip while k + 24 < splitk: none, one trip, one trip + tail
    assert {7, 8, 9} <= set(E.RED_SPLITK) and {24, 25, 32, 33} <= set(E.RED_SPLITK) and max(E.RED_SPLITK) > 32 + 24
    ragged = 0
    for swap in (0, 1):
        jobs = E.reduce_jobs(9, swap)
        assert [t for t, _ in jobs] == E.RED_TAPS
        for taps, I in jobs:
            n, epb = E.RED_O * I * taps, lib.dh_wgrad_reduce_outputs_per_block(I)
            ragged += n % epb != 0
            assert n % epb != 0 or (I, taps) == (E.RED_I_SCALAR, 16)        # 5 x 6 x 16 = 480 = 15 x 32: the one full last block
    assert ragged == 7
    part, before = E.reduce_job(9, 4, E.RED_I_VEC, 0)
    assert bool(torch.isnan(part[:, :, E.RED_O:]).all()) and bool(torch.isfinite(part[:, :, :E.RED_O]).all())
    assert E.RED_MAX * (max(E.RED_SPLITK) + 1) < E.EXACT_LIMIT
    want = E.reduce_ref(part, before, True)
    assert tuple(want.shape) == (E.RED_O, E.RED_I_VEC, 4) and bool(torch.isfinite(want).all())
    assert torch.equal(want, E.reduce_ref(part, before, False) + before.double())


def _case(group, name):
    return next(c for c in E.CASES if (c.group, c.name) == (group, name))


@pytest.mark.parametrize("group,name", [("GENERIC", "k3s1d1-co32-ci32x1-bf16-tr"), ("WS", "128x64-remap"), ("PHASE", "up2-32-f32"),
                                        ("W1", "264x520-n28-generic")])
def test_comparator_fails_on_one_pixel_and_on_one_dropped_tile(group, name, capsys):
    c = _case(group, name)
    d = E.data(c)
    want = E.reference(c)
    E.exact(want.float(), want, "the reference against itself")
    # one input pixel (all its channels) one higher
    bumped = dict(d, x=d["x"].clone())
    bumped["x"][c.N - 1, c.H // 2, c.W // 2, :c.Cin] += 1
    with pytest.raises(AssertionError, match="elements differ, first at"):
        E.exact(E.reference_of(c, bumped).float(), want, "one pixel of x one higher")
    # one element of one pixel
    bumped["x"] = d["x"].clone()
    bumped["x"][0, 0, 0, 0] += 1
    with pytest.raises(AssertionError, match="elements differ"):
        E.exact(E.reference_of(c, bumped).float(), want, "one element of x one higher")
    # the last pixel tile dropped from the sum
    assert int(E.last_tile_mask(c).sum()) > 0
    with pytest.raises(AssertionError, match="elements differ"):
        E.exact(E.reference_of(c, d, drop_last_tile=True).float(), want, "the last pixel tile dropped")
    # non-finite results and wrong shapes are refused too
    nan = want.float().clone()
    nan.view(-1)[0] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        E.exact(nan, want, "a NaN")
    with pytest.raises(AssertionError):
        E.exact(want.float()[1:], want, "a missing row")
    out = capsys.readouterr().out
    assert "0 of %d elements differ" % want.numel() in out
