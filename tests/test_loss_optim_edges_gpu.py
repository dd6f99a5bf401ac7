"""The kernels that turn logits into a loss, a gradient, a metric and a weight update (csrc/loss_optim.hip, csrc/xbd_step.hip) and the
pool / resample kernels of csrc/pointwise.hip, past one grid-stride pass and at their edges: every class count of the generic focal
kernel, arg-max ties, labels outside 0..C-1, logit gaps at which expf underflows to 0, an all-ignored target, odd and one-pixel
maps, the n & 3 tail of the gradient norm.

The reference is the oracle's function of the same name (or plain torch) on the CPU in FLOAT64, on the same float32 inputs cast up.
Bounds are those tests/test_kernels_gpu.py and tests/test_xbd_gpu.py state for the same quantity; the one place where a correct
float32 kernel cannot meet them says so, with the float32 oracle's own distance from the float64 oracle measured on that input
(tests/test_loss_optim_edges_cpu.py repeats the measurement).  Every figure is printed before it is asserted."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cdnet_ref as O
import _loss_edge_cases as E
from _bounds import close, tol

pytestmark = pytest.mark.gpu
F32 = torch.float32


@pytest.fixture(scope="module")
def ops():
    from dahitra_amd import ops as o
    return o


def rnd(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).float()      # representable in `dtype`, float32 on the CPU


def nhwc(x, dtype):       # NCHW cpu -> NHWC device
    return x.detach().permute(0, 2, 3, 1).to(dtype).cuda().contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2)


def confusion_ref(pred, tgt, C):
    """misc/metric_tool.py:141-158: counts[gt * C + pred] over the pixels whose label lies in 0..C-1"""
    gt, pr = tgt.reshape(-1).numpy(), pred.reshape(-1).numpy()
    ok = (gt >= 0) & (gt < C)
    return torch.from_numpy(np.bincount(gt[ok] * C + pr[ok], minlength=C * C).reshape(C, C))


def check_focal(ops, logits, tgt, what):
    ref = logits.double().requires_grad_(True)
    want = O.focal_loss(ref, tgt)
    want.backward()
    l, dl = ops.focal_loss(logits.cuda(), tgt.cuda())
    print("%s: focal loss %.7f, |kernel - float64 oracle| %.3e (bound 1e-6); gradient max err %.3e of max %.3e"
          % (what, float(want), abs(float(l) - float(want)), float((dl.cpu() - ref.grad).abs().max()), float(ref.grad.abs().max())))
    assert math.isfinite(float(l)) and bool(torch.isfinite(dl).all())
    assert abs(float(l) - float(want)) < 1e-6
    close(dl, ref.grad, F32, "focal grad " + what, factor=2)


# ---- 1. past one grid-stride pass ------------------------------------------------------------------------------------------------
PASS_CASES = [pytest.param(s, C, id="%s-C%d" % (E.shape_id(s), C)) for s in E.PASS_SHAPES for C in (2, 5)]
GENERIC_PASS = [pytest.param(E.GENERIC_SHAPE, C, id="%s-C%d" % (E.shape_id(E.GENERIC_SHAPE), C)) for C in (3, 8)]


@pytest.mark.parametrize("shape,C", PASS_CASES + GENERIC_PASS)
def test_focal_loss_and_gradient_past_one_grid_pass(ops, shape, C):
    logits, tgt, _ = E.pass_inputs(shape, C)
    check_focal(ops, logits, tgt, "%s C=%d" % (E.shape_id(shape), C))


@pytest.mark.parametrize("shape,C", PASS_CASES)
def test_cross_entropy_forward_past_one_grid_pass(ops, shape, C):
    logits, tgt, _ = E.pass_inputs(shape, C, 3)
    want = float(O.cross_entropy(logits.double(), tgt))
    out = ops.cross_entropy_fwd(logits.cuda(), tgt.cuda()).cpu()
    print("cross entropy %s C=%d: %.7f, rel err %.3e (bound 2e-6)" % (E.shape_id(shape), C, want, abs(float(out[0]) - want) / want))
    assert abs(float(out[0]) - want) <= 2e-6 * abs(want)
    assert float(out[1]) == float((tgt != E.IGNORE).sum())           # the count the backward divides by (exact below 2^24)


@pytest.mark.parametrize("shape,C", PASS_CASES)
def test_argmax_confusion_and_dice_past_one_grid_pass(ops, shape, C):
    logits, tgt, binary = E.pass_inputs(shape, C)
    want = torch.argmax(logits, 1)
    lg, td = logits.cuda(), tgt.cuda()
    assert torch.equal(ops.argmax_nchw(lg).cpu(), want)
    counts_ref = confusion_ref(want, tgt, C)
    counts = torch.zeros(C, C, dtype=torch.int64, device="cuda")
    assert ops.confusion_matrix(lg, td, counts) is None              # without the mask output
    assert torch.equal(counts.cpu(), counts_ref)
    counts.zero_()
    mask = ops.confusion_matrix(lg, td, counts, want_mask=True)
    assert torch.equal(mask.cpu(), want)
    assert torch.equal(counts.cpu(), counts_ref)
    dice = float(E.dice_constant64(logits, binary))
    got = float(ops.dice_argmax_constant(lg, binary[:, 0].contiguous().cuda()))
    print("dice %s C=%d: %.7f, err %.3e (bound 1e-6)" % (E.shape_id(shape), C, dice, abs(got - dice)))
    assert abs(got - dice) <= 1e-6


@pytest.mark.parametrize("C", [2, 5])
def test_cross_entropy_backward_past_one_grid_pass(C):
    from dahitra_amd.models import losses
    logits, tgt, _ = E.pass_inputs(E.CE_BWD_SHAPE, C, 40)
    ref = logits.double().requires_grad_(True)
    want = O.cross_entropy(ref, tgt)
    (want * 0.7).backward()
    lg = logits.cuda().requires_grad_(True)
    got = losses.cross_entropy(lg, tgt.cuda())
    (got * 0.7).backward()
    err = float((lg.grad.cpu() - ref.grad).abs().max())
    print("cross entropy bwd C=%d: loss rel err %.3e (bound 2e-6), gradient err %.3e of max %.3e (bound 1e-6)"
          % (C, abs(float(got) - float(want)) / float(want), err, float(ref.grad.abs().max())))
    assert abs(float(got) - float(want)) <= 2e-6 * abs(float(want))
    assert err <= 1e-6 * float(ref.grad.abs().max()) + 1e-12
    H = E.CE_BWD_SHAPE[1]
    assert float(lg.grad[0, :, H // 3:H // 3 + 40].abs().max()) == 0.0


# ---- 2. the generic focal kernel (every class count but 2 and 5) ------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 4, 6, 7, 8])
def test_generic_focal_kernel_at_every_class_count(ops, C):
    logits = rnd((2, C, 24, 20), F32, 200 + C, 2.0)
    tgt = torch.randint(0, C, (2, 24, 20), generator=torch.Generator().manual_seed(300 + C))
    check_focal(ops, logits, tgt, "C=%d" % C)


def test_focal_loss_refuses_nine_classes(ops):
    from dahitra_amd._lib import HipLibraryError
    with pytest.raises(HipLibraryError, match="focal_loss: n_class=9"):
        ops.focal_loss(torch.zeros(2, 9, 24, 20, device="cuda"), torch.zeros(2, 24, 20, dtype=torch.int64, device="cuda"))


# ---- 3. ties and labels outside 0..C-1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 5])
def test_first_maximum_wins_and_foreign_labels_are_skipped(ops, C):
    z, tgt, binary = E.tie_inputs(C)
    frac = E.tied_fraction(z)
    assert frac >= 0.5, frac                                         # the case stays a case about ties
    assert bool((z[:, :, :3] == z[:, :1, :3]).all())                 # all classes equal
    last2 = z[:, C - 2:, 3:6]
    assert bool((last2 == 1.0).all()) and (C == 2 or float(z[:, :C - 2, 3:6].max()) < 1.0)     # only the last two tie
    assert all(int((tgt == v).sum()) > 0 for v in (255, C, -1))
    want = torch.argmax(z, 1)
    assert bool((want[:, :3] == 0).all()) and bool((want[:, 3:6] == C - 2).all())
    lg, td = z.cuda(), tgt.cuda()
    assert torch.equal(ops.argmax_nchw(lg).cpu(), want)
    counts_ref = confusion_ref(want, tgt, C)
    assert int(counts_ref.sum()) == int(((tgt >= 0) & (tgt < C)).sum()) < tgt.numel()
    counts = torch.zeros(C, C, dtype=torch.int64, device="cuda")
    mask = ops.confusion_matrix(lg, td, counts, want_mask=True)
    assert torch.equal(mask.cpu(), want)
    assert torch.equal(counts.cpu(), counts_ref)
    ops.confusion_matrix(lg, td, counts)                             # accumulates
    assert torch.equal(counts.cpu(), 2 * counts_ref)
    dice = float(E.dice_constant64(z, binary))
    got = float(ops.dice_argmax_constant(lg, binary[:, 0].contiguous().cuda()))
    assert abs(got - dice) <= 1e-6, (got, dice)


# ---- 4. saturation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 5])
def test_focal_and_cross_entropy_where_expf_underflows(ops, C):
    from dahitra_amd.models import losses
    z, tgt = E.saturation_inputs(C)
    gap = (z.max(1).values - z.min(1).values).reshape(-1)
    assert float(gap.max()) > 190.0 and int((gap > 104.0).sum()) >= 8      # expf(-gap) == 0 on those
    check_focal(ops, z, tgt, "saturated C=%d" % C)
    ref = z.double().requires_grad_(True)
    want = O.cross_entropy(ref, tgt)
    (want * 0.7).backward()
    lg = z.cuda().requires_grad_(True)
    got = losses.cross_entropy(lg, tgt.cuda())
    (got * 0.7).backward()
    err = float((lg.grad.cpu() - ref.grad).abs().max())
    print("saturated cross entropy C=%d: %.6f rel err %.3e, gradient err %.3e of max %.3e"
          % (C, float(want), abs(float(got) - float(want)) / float(want), err, float(ref.grad.abs().max())))
    assert math.isfinite(float(got)) and bool(torch.isfinite(lg.grad).all())
    assert abs(float(got) - float(want)) <= 2e-6 * abs(float(want))
    assert err <= 1e-6 * float(ref.grad.abs().max()) + 1e-12


def test_cross_entropy_of_an_all_ignored_target_is_nan_with_a_zero_gradient():
    from dahitra_amd.models import losses
    z = rnd((1, 2, 16, 16), F32, 410, 2.0)
    tgt = torch.full((1, 16, 16), E.IGNORE, dtype=torch.int64)
    assert math.isnan(float(O.cross_entropy(z.double(), tgt)))       # 0 / 0, as torch
    lg = z.cuda().requires_grad_(True)
    got = losses.cross_entropy(lg, tgt.cuda())
    assert math.isnan(float(got))
    (got * 0.7).backward()
    assert torch.equal(lg.grad, torch.zeros_like(lg.grad))


def combo_case(ops, z, m, w, upstream):
    """kernel and float64 oracle on the same inputs: (loss, channel losses, gradient) twice"""
    want = E.combo_ref(z, m, w, upstream)
    zd, md, wd = z.cuda(), m.cuda(), w.cuda()
    loss, ch, sums = ops.combo_loss_fwd(zd, md, wd)
    dl = ops.combo_loss_bwd(zd, md, sums, wd, torch.tensor([upstream], device="cuda"))
    return (float(loss), ch.cpu().tolist(), dl.cpu()), want, (zd, md, wd, sums)


def test_combo_loss_outside_both_clamps_on_both_mask_values(ops):
    z, m, rows = E.combo_saturation_inputs()
    w = torch.tensor(O.XBD_CHANNEL_WEIGHTS)
    (loss, ch, dl), (wl, wch, wgrad), (zd, md, wd, sums) = combo_case(ops, z, m, w, 1.7)
    err = float((dl - wgrad).abs().max())
    print("saturated combo loss %.6f rel err %.3e, channels %s, gradient err %.3e of max %.3e"
          % (wl, abs(loss - wl) / wl, ["%.2e" % (abs(a - b) / max(1.0, b)) for a, b in zip(ch, wch)], err, float(wgrad.abs().max())))
    # FocalLoss2d clamps the sigmoid to 1 - 1e-6 and then reads 1 - o: float32 has 1.0133e-6 there, the log of the wrong-side pixels is
    # 0.007 off, and the float32 ORACLE is 1.974e-4 (loss) / 2.004e-4 (worst channel) away from its float64 self on this input --
    # no float32 kernel meets 2e-6 here.  Bound: 4 x that distance = 7.9e-4 / 8.0e-4 (the kernel sums in another order) ...
    assert abs(loss - wl) <= 7.9e-4 * wl
    for a, b in zip(ch, wch):
        assert abs(a - b) <= 8.0e-4 * max(1.0, b)
    # ... and, so that the case still bites, the stated 2e-6 against the float32 oracle, whose arithmetic the kernel restates (as
    # tests/test_xbd_gpu.py does with its +-25 rows)
    l32 = float(O.xbd_loss(z, m))
    print("  against the float32 oracle: rel err %.3e (bound 2e-6)" % (abs(loss - l32) / l32))
    assert abs(loss - l32) <= 2e-6 * l32
    # the gradient has no such term (float32 oracle 2.6e-7 of the maximum from float64): the stated bound
    assert err <= 1e-5 * float(wgrad.abs().max()) + 1e-10
    # both sides take the focal gradient to be exactly 0 outside the clamp: the kernel's focal-only gradient ...
    focal_only = ops.combo_loss_bwd(zd, md, sums, wd, torch.tensor([1.7], device="cuda"), dice_weight=0.0)
    assert float(focal_only[:, :, :rows].abs().max()) == 0.0 and float(focal_only[:, :, rows:].abs().min()) > 0.0
    # ... and the oracle's (FocalLoss2d alone, xBD_code/losses.py:273-288)
    lg = z.double().requires_grad_(True)
    o = torch.sigmoid(lg).clamp(O.XBD_EPS, 1.0 - O.XBD_EPS)
    tt = m.clamp(O.XBD_EPS, 1.0 - O.XBD_EPS).double()
    pt = (1 - tt) * (1 - o) + tt * o
    (-(1.0 - pt) ** 2 * torch.log(pt)).sum().backward()
    assert float(lg.grad[:, :, :rows].abs().max()) == 0.0 and float(lg.grad[:, :, rows:].abs().min()) > 0.0


# ---- 5. combo loss past one pass and at the channel limits ---------------------------------------------------------------------------
def check_combo(ops, shape, w, seed, want_grad=True):
    z, m = E.combo_inputs(*shape, seed)
    (loss, ch, dl), (wl, wch, wgrad), _ = combo_case(ops, z, m, w, 1.7)
    print("combo %s: loss %.6f rel err %.3e (bound 2e-6), worst channel %.3e" % (E.shape_id(shape), wl, abs(loss - wl) / wl,
                                                                                max(abs(a - b) / max(1.0, b) for a, b in zip(ch, wch))))
    assert abs(loss - wl) <= 2e-6 * abs(wl)
    for a, b in zip(ch, wch):
        assert abs(a - b) <= 2e-6 * max(1.0, b)
    if want_grad:
        err = float((dl - wgrad).abs().max())
        print("  gradient err %.3e of max %.3e (bound 1e-5)" % (err, float(wgrad.abs().max())))
        assert err <= 1e-5 * float(wgrad.abs().max()) + 1e-10


@pytest.mark.parametrize("shape,want_grad", [pytest.param((3, 5, 211, 157), False, id="3x5x211x157-fwd"),       # 99381 pixels per channel
                                             pytest.param((3, 5, 531, 527), True, id="3x5x531x527")])          # 4197555 elements
def test_combo_loss_past_one_grid_pass(ops, shape, want_grad):
    check_combo(ops, shape, torch.tensor(O.XBD_CHANNEL_WEIGHTS), 5100 + shape[2], want_grad)


@pytest.mark.parametrize("C", [1, 16])
def test_combo_loss_at_the_channel_limits(ops, C):
    w = torch.rand(C, generator=torch.Generator().manual_seed(5200 + C)) + 0.05
    check_combo(ops, (2, C, 24, 20), w, 5300 + C)


def test_combo_loss_refuses_seventeen_channels(ops):
    from dahitra_amd._lib import HipLibraryError
    z = torch.zeros(2, 17, 24, 20, device="cuda")
    with pytest.raises(HipLibraryError, match="combo_loss: C=17"):
        ops.combo_loss_fwd(z, z, torch.ones(17, device="cuda"))


# ---- 6. optimizers, norm and scale past one pass -----------------------------------------------------------------------------------
LR, B1, B2, EPS, WD = (float(np.float32(v)) for v in (1e-2, 0.9, 0.999, 1e-8, 1e-2))      # what the kernels receive, exactly


def test_adamw_past_one_grid_pass(ops):
    n, gs = E.OPT_N, 0.375                                           # grad_scale exact in float32: both sides see the same gradient
    p0 = rnd((n,), F32, 600)
    ref = p0.double().requires_grad_(True)
    opt = torch.optim.AdamW([ref], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD)
    pd, m, v = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    for step in range(1, 4):
        g = rnd((n,), F32, 600 + step)
        ref.grad = g.double() * gs
        opt.step()
        ops.adamw_step(pd, g.cuda(), m, v, LR, B1, B2, EPS, WD, step, grad_scale=gs)
        close(pd, ref.detach(), F32, "adamw step %d" % step, factor=1)
    close(m, opt.state[ref]["exp_avg"], F32, "adamw exp_avg", factor=1)
    close(v, opt.state[ref]["exp_avg_sq"], F32, "adamw exp_avg_sq", factor=1)


def test_adamw_xbd_past_one_grid_pass_with_a_device_grad_scale(ops):
    n = E.OPT_N
    p0 = rnd((n,), F32, 610)
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    pd, md, vd = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    gs = torch.tensor([0.625], device="cuda")
    for t, s in enumerate((3.0, 1e-3, 1e-9), 1):                     # the last one: eps dominates sqrt(v)
        g = rnd((n,), F32, 610 + t, s)
        E.adamw_xbd_ref(p, m, v, g.double() * 0.625, t, LR, B1, B2, EPS, WD)
        ops.adamw_xbd_step(pd, g.cuda(), md, vd, LR, B1, B2, EPS, WD, t, gs)
        err = float((pd.cpu() - p).abs().max())
        print("xBD AdamW step %d: max err %.3e (bound 2e-6)" % (t, err))
        assert err <= 2e-6, t
    assert float((md.cpu() - m).abs().max()) <= 1e-6 * float(m.abs().max())
    assert float((vd.cpu() - v).abs().max()) <= 1e-6 * float(v.abs().max())


@pytest.mark.parametrize("rule", ["torch", "xbd"])
def test_graph_form_of_the_optimizer_is_bit_equal_to_the_eager_form(ops, rule):
    """dh_adamw_step_graph / dh_adamw_xbd_step_graph called directly (no capture): hyper-parameters and the step counter in device
    memory, the bias corrections computed by a one-thread kernel.  (This case found adamw_kernel and adamw_dev_kernel fused
    differently by the compiler, 23253 of 3145805 parameters apart after two steps; both now call one adamw_update().)"""
    n, gs = E.OPT_N, 0.375
    p0 = rnd((n,), F32, 620)
    grads = [rnd((n,), F32, 621 + t).cuda() for t in range(2)]
    gs_dev = torch.tensor([gs], device="cuda")
    eager = [p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")]
    graph = [p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")]
    hyper = torch.tensor([LR, B1, B2, EPS, WD, gs, 0.0, 0.0], dtype=torch.float32).cuda()
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    for t, g in enumerate(grads, 1):
        if rule == "xbd":
            ops.adamw_xbd_step(*eager[:1], g, *eager[1:], LR, B1, B2, EPS, WD, t, gs_dev)
            ops._call("dh_adamw_xbd_step_graph", ops.P(graph[0]), ops.P(g), ops.P(graph[1]), ops.P(graph[2]), n, ops.P(hyper),
                      ops.P(count), ops.P(gs_dev), ops.S())
        else:
            ops.adamw_step(*eager[:1], g, *eager[1:], LR, B1, B2, EPS, WD, t, grad_scale=gs)
            ops._call("dh_adamw_step_graph", ops.P(graph[0]), ops.P(g), ops.P(graph[1]), ops.P(graph[2]), n, ops.P(hyper),
                      ops.P(count), ops.S())
    assert int(count) == 2
    for a, b, what in zip(eager, graph, ("param", "exp_avg", "exp_avg_sq")):
        assert not torch.equal(a.cpu(), p0 if what == "param" else torch.zeros(n)), what       # it moved ...
        assert torch.equal(a, b), "%s: %d elements differ" % (what, int((a != b).sum()))        # ... to the same bits


@pytest.mark.parametrize("n", E.NORM_TAILS + (E.OPT_N,))
def test_gradient_norm_and_clip_coefficient(ops, n):
    g = rnd((n,), F32, 630 + (n & 1023), 3.0)
    norm = float(g.double().norm())
    out = torch.empty(2, device="cuda")
    for max_norm in (0.999, 1e-2):                                   # 1e-2: the coefficient is below 1 at every n
        coef = min(1.0, max_norm / (norm + 1e-6))
        ops.grad_norm_clip_coef(g.cuda(), max_norm, out)
        print("n=%d max_norm %g: norm rel err %.3e, coefficient rel err %.3e (bounds 1e-6)"
              % (n, max_norm, abs(float(out[0]) - norm) / norm, abs(float(out[1]) - coef) / coef))
        assert abs(float(out[0]) - norm) <= 1e-6 * norm
        assert abs(float(out[1]) - coef) <= 1e-6 * coef
    assert coef < 1.0


@pytest.mark.parametrize("n", [5, E.OPT_N])
def test_zero_gradient_has_norm_0_coefficient_1_and_leaves_the_moments_at_0(ops, n):
    g = torch.zeros(n, device="cuda")
    out = torch.empty(2, device="cuda")
    ops.grad_norm_clip_coef(g, 0.999, out)
    assert out.cpu().tolist() == [0.0, 1.0]
    p0 = rnd((n,), F32, 640)
    pd, m, v = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    ops.adamw_xbd_step(pd, g, m, v, LR, B1, B2, EPS, WD, 1, out[1:2])
    assert float(m.abs().max()) == 0.0 and float(v.abs().max()) == 0.0
    want = p0.double() * (1.0 - WD * LR)                             # the decoupled decay alone
    assert float((pd.cpu() - want).abs().max()) <= 2e-6


def test_scale_into_past_one_grid_pass(ops):
    src = rnd((E.OPT_N,), F32, 650)
    s = torch.tensor([0.3], dtype=torch.float32)
    dst = torch.full((E.OPT_N,), float("nan"), device="cuda")
    ops.scale_into(src.cuda(), s.cuda(), dst)
    # the float64 product of two float32 values is exact, so its rounding to float32 is the one correct float32 product
    assert torch.equal(dst.cpu(), (src.double() * s.double()).float())


# ---- 7. pool and resample at odd and degenerate sizes ------------------------------------------------------------------------------
def check_maxpool(ops, dtype, N, C, H, W, seed):
    x = F.relu(rnd((N, C, H, W), dtype, seed)).double().requires_grad_(True)     # many exact ties at 0
    y = F.max_pool2d(x, 3, 2, 1)
    dy = rnd(tuple(y.shape), dtype, seed + 1).double()
    y.backward(dy)
    xd = nhwc(x, dtype)
    yd, arg = ops.maxpool(xd, want_arg=True)
    assert tuple(yd.shape) == (N, y.shape[2], y.shape[3], C)
    close(nchw(yd), y.detach(), dtype, "maxpool %dx%d" % (H, W))
    close(nchw(ops.maxpool_bwd(arg, nhwc(dy, dtype), xd.shape)), x.grad, dtype, "maxpool bwd %dx%d" % (H, W), factor=2)


@pytest.mark.parametrize("hw", E.POOL_SHAPES, ids=E.shape_id)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_pool_and_resample_at_odd_and_one_pixel_sizes(ops, dtype, hw):
    N, C, (H, W) = 2, 32, hw
    check_maxpool(ops, dtype, N, C, H, W, 700)
    x2 = rnd((N, C, H, W), dtype, 702).double().requires_grad_(True)
    u = F.interpolate(x2, scale_factor=2, mode="nearest")
    du = rnd(tuple(u.shape), dtype, 703).double()
    u.backward(du)
    close(nchw(ops.upsample2(nhwc(x2, dtype))), u.detach(), dtype, "up2")
    close(nchw(ops.upsample2_bwd(nhwc(du, dtype))), x2.grad, dtype, "up2 bwd", factor=2)
    a = rnd((N, C, H, W), dtype, 704).double().requires_grad_(True)
    b = rnd((N, C, H, W), dtype, 705).double().requires_grad_(True)
    o = F.interpolate(torch.abs(a - b), scale_factor=4, mode="bilinear", align_corners=False)
    do = rnd(tuple(o.shape), dtype, 706).double()
    o.backward(do)
    ad, bd = nhwc(a, dtype), nhwc(b, dtype)
    close(nchw(ops.absdiff_upsample4(ad, bd)), o.detach(), dtype, "absdiff+bilinear")
    da, db = ops.absdiff_upsample4_bwd(ad, bd, nhwc(do, dtype))
    close(nchw(da), a.grad, dtype, "bilinear bwd a", factor=4)
    close(nchw(db), b.grad, dtype, "bilinear bwd b", factor=4)


def test_maxpool_past_one_grid_pass(ops):
    check_maxpool(ops, torch.float32, *E.POOL_LARGE, 710)
