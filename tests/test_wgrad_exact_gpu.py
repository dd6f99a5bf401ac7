"""Every kernel family of the weight gradient (csrc/conv_wgrad.hip: W1, WS, WS_BATCH, C32_BATCH, GENERIC, PHASE), every
instantiation of conv_wgrad_kernel, the split-K tile walk at its edges and the reduce kernels, on integer data against a float64
reference: the sums are exact in fp32 in any order, so every comparison is torch.equal (tests/_wgrad_exact_cases.py: `exact`).
A dropped, doubled or misplaced pixel -- a lost tile of an uneven split, a wrong carry of the (image, ty, tx) counter, a halo
column, a ragged last tile read one row too far, a slab the reduce skips -- changes an integer and fails.

Each case runs through the public ops entry directly (its own reduce), deferred (ops.WgradPlan + run(): dh_wgrad_reduce_multi)
and, where the batch takes the layer, recorded into an open batch; each with accumulate=False over a 777.0 sentinel and
accumulate=True onto an integer fill of 3.0.  The described row of the case is printed first; tests/test_wgrad_exact_cpu.py
asserts it on the host.  No environment switch is touched: the library's A/B switches stay at their defaults."""
import pytest
import torch

import _wgrad_exact_cases as E
from _wgrad_exact_cases import BF16, F32, exact

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from dahitra_amd import ops as o
    return o


@pytest.fixture(autouse=True)
def _nothing_more_after_a_device_error():
    """a kernel fault leaves the device unusable for this process: end the session instead of launching the remaining cases on it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device error, nothing more is launched: %s" % e, returncode=3)


def show(ops, c):
    r = E.describe(ops._lib.lib(), c)
    print("%s %s: %s ct=%d it=%d cig=%d ci_tiles=%d splitk=%d direct=%d grid=%s threads=%d lds=%d, %d tiles" % (
        c.group, c.name, E.FAMILIES[r[0]], r[1], r[2], r[3], r[4], r[5], r[6], r[7:10], r[10], r[11], E.tiles_of(c)))
    assert (r[0], r[1], r[2], r[3], r[5]) == c.row, (c.name, r)
    return r


def operands(ops, c):
    """(x as the ops entry takes it, dy) on the device in the case's dtype"""
    d, dtype = E.data(c), E.dtype_of(c)
    x = d["x"].to(dtype).cuda().contiguous()
    dy = d["dy"].to(dtype).cuda().contiguous()
    if c.form == "bn":
        x = ops.BnInput(x, d["scale"].cuda(), d["shift"].cuda(), c.bn_groups)
    elif c.form == "split":
        x = ops.SplitCat(x)
    return x, dy


def start(c, accumulate):
    return torch.full(E.dw_shape(c), E.ACC_FILL if accumulate else E.SENTINEL, dtype=F32, device="cuda")


def launch(ops, c, x, dy, dw, accumulate, defer):
    if c.form == "phase":
        ops.conv_up2_wgrad(x, dy, dw, accumulate=accumulate, use_tr=E.tr_of(c))
    elif c.form == "split":
        ops.conv2d_wgrad(x, dy, dw, 3, 1, 1, accumulate=accumulate, defer=defer)
    else:
        ops.conv2d_wgrad(x, dy, dw, c.ks, c.stride, E.pad_of(c), accumulate=accumulate, groups=E.weight_groups(c), use_tr=E.tr_of(c),
                         cout_real=c.Cout if c.dy_ch else 0, cin=c.Cin if c.pitch else 0, dilation=c.dil, defer=defer)


def check(c, dw, accumulate, what):
    want = E.reference(c)
    exact(dw, want + E.ACC_FILL if accumulate else want, "%s %s, %s, accumulate=%s" % (c.group, c.name, what, accumulate))


def run_case(ops, c):
    """direct, deferred and (where the batch takes the layer) batched, each assigning and accumulating: all exact"""
    from dahitra_amd import _lib
    show(ops, c)
    x, dy = operands(ops, c)
    with ops.f32_mma_mode(E.mma_of(c)):
        for accumulate in (False, True):
            dw = start(c, accumulate)
            launch(ops, c, x, dy, dw, accumulate, defer=False)
            check(c, dw, accumulate, "direct")
        plan = ops.WgradPlan("cuda")
        for accumulate in (False, True):          # the second pass reuses the plan's slab, with another job table
            dw = start(c, accumulate)
            with plan:
                launch(ops, c, x, dy, dw, accumulate, defer=True)
                plan.run()
            check(c, dw, accumulate, "deferred")
        if c.batch_row is not None:
            plan = ops.WgradPlan("cuda", batch=True)
            assert plan.batch
            for accumulate in (False, True):
                dw = start(c, accumulate)
                with plan:
                    launch(ops, c, x, dy, dw, accumulate, defer=True)
                    assert _lib.lib().dh_wgrad_batch_pending() == 1
                    plan.run()
                    assert _lib.lib().dh_wgrad_batch_pending() == 0
                check(c, dw, accumulate, "batched (%s, split-K %d)" % (E.FAMILIES[c.batch_row[0]], c.batch_row[1]))


@pytest.mark.parametrize("c", E.cases("GENERIC"), ids=E.ids(E.cases("GENERIC")))
def test_conv_wgrad_kernel_is_exact(ops, c):
    """conv_wgrad_kernel: every instantiation launch_generic reaches -- (ks, stride, dilation) in 3x3 / 3x3 dilated / 3x3 stride 2 /
    1x1 / 1x1 stride 2 / the 4x4 stem form, co tiles 16 / 32 / 64, 16 / 32 / 64 / 2 x 32 / 2 x 64 ci channels, bf16 with and without
    transpose reads, fp32 and the split fp32 form -- at 78 tiles in 9 uneven slices with a carry at every step and ragged last
    tile rows and columns; then even stride-2 inputs, dilation past a whole 8 x 8 map, two real channels in a padded dy, a wide
    channel pitch, ragged and unaligned channel tiles, BatchNorm on load, the one-slab direct form, per-image weights, 6 and 16
    tiles"""
    run_case(ops, c)


@pytest.mark.parametrize("c", E.cases("WS"), ids=E.ids(E.cases("WS")))
def test_wave_specialised_kernel_is_exact(ops, c):
    """conv_wgrad_ws_kernel<1 / 2>: one block and two (the XCD remap at 8 slices of 9 or 8 tiles), BatchNorm on load with two
    statistics groups, a split input of 2 x 64 channels; and each undilated layer alone in a batch (conv_wgrad_ws_multi_kernel)"""
    run_case(ops, c)


@pytest.mark.parametrize("c", E.cases("W1"), ids=E.ids(E.cases("W1")))
def test_wgrad1x1_kernel_is_exact(ops, c):
    """wgrad1x1_kernel<256, 128> on 3 x 3 ragged blocks: 27,869 pixels in 436 chunks over 29 slices (a ragged last chunk, slices of
    16 or 15 chunks), with the XCD remap at 32 slices, at stride 2 on an odd input; and the shape one image short of its
    threshold, which conv_wgrad_kernel takes"""
    run_case(ops, c)


@pytest.mark.parametrize("c", E.cases("PHASE"), ids=E.ids(E.cases("PHASE")))
def test_phase_form_is_exact(ops, c):
    """ops.conv_up2_wgrad: the four 2x2 phase gradients on a coarse grid that is uneven under the split and ragged at both edges,
    their reduce and dh_phase_wgrad_combine, against the gradient of conv2d(interpolate(x, 2, "nearest"), w, padding=1)"""
    run_case(ops, c)


def test_recorded_pass_is_exact(ops):
    """ops.WgradPlan(device, batch=True): eight layers recorded in one pass -- the wave-specialised family at 300 tiles (8 slices
    of 38 or 37), at 18 tiles (one slice), with two blocks (the remap inside conv_wgrad_ws_multi_kernel) and a split input; the
    32-wide family at 300 and 18 tiles and with BatchNorm on load over two ci tiles; a 16-output-channel layer the batch refuses.
    Three passes on the same plan: the second repeats the first (the job table is reused), the third swaps assign and
    accumulate on every layer.  Every dW of every pass is exact."""
    from dahitra_amd import _lib
    layers = E.cases("BATCH")
    rows = [show(ops, c) for c in layers]
    taken = sum(r[0] in (E.WS_BATCH, E.C32_BATCH) for r in rows)
    assert taken == len(layers) - 1 and rows[-1][0] == E.GENERIC
    ins = [operands(ops, c) for c in layers]
    plan = ops.WgradPlan("cuda", batch=True)
    assert plan.batch
    for rep in range(3):
        acc = [(k + (rep == 2)) % 2 == 1 for k in range(len(layers))]
        dws = [start(c, a) for c, a in zip(layers, acc)]
        with plan:
            for c, (x, dy), dw, a in zip(layers, ins, dws, acc):
                launch(ops, c, x, dy, dw, a, defer=True)
            assert _lib.lib().dh_wgrad_batch_pending() == taken
            plan.run()
            assert _lib.lib().dh_wgrad_batch_pending() == 0
        for c, dw, a in zip(layers, dws, acc):
            check(c, dw, a, "pass %d" % rep)


def _reduce_launch(ops, jobs, accumulate, what):
    """one dh_wgrad_reduce_multi launch over `jobs` [(part, before, taps, I)]; every job exact"""
    from dahitra_amd import _lib
    J = ops.WgradPlan._Job
    parts = [p.cuda() for p, _, _, _ in jobs]
    dws = [b.clone().cuda() if accumulate else torch.full_like(b, E.SENTINEL).cuda() for _, b, _, _ in jobs]
    table, first = [], 0
    for (p, b, taps, I), pd, dw in zip(jobs, parts, dws):
        nb = -(-E.RED_O * I * taps // _lib.lib().dh_wgrad_reduce_outputs_per_block(I))
        table.append(J(pd.data_ptr(), dw.data_ptr(), p.shape[0], taps, E.RED_OSLAB, E.RED_O, I, int(accumulate), first, nb))
        first += nb
    dev = torch.frombuffer(bytearray(b"".join(bytes(j) for j in table)), dtype=torch.uint8).cuda()
    ops._call("dh_wgrad_reduce_multi", ops.P(dev), len(table), first, ops.S())
    torch.cuda.synchronize()
    for (p, b, taps, I), dw in zip(jobs, dws):
        exact(dw, E.reduce_ref(p, b, accumulate), "%s: splitk=%d taps=%d I=%d accumulate=%s" % (what, p.shape[0], taps, I, accumulate))


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("splitk", E.RED_SPLITK)
def test_reduce_alone_on_synthetic_partials(ops, splitk, accumulate):
    """dh_wgrad_reduce_multi with no weight-gradient kernel in front of it: integer partial slabs [splitk][taps][Oslab = 8][I] with
    NaN in the rows past O = 5 (never to be read), the 16-byte form (I = 12) and the element form (I = 6), taps 1 / 4 / 9 / 16, a
    ragged last block, four jobs in one launch (the first_block search) and each job alone, assign over a sentinel and accumulate
    onto integers -- against the float64 sum of the same partials"""
    for swap in (0, 1):
        jobs = [E.reduce_job(splitk, taps, I, swap) + (taps, I) for taps, I in E.reduce_jobs(splitk, swap)]
        _reduce_launch(ops, jobs, accumulate, "four jobs")
        for job in jobs:
            _reduce_launch(ops, [job], accumulate, "one job")
