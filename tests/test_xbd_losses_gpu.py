"""The Lovasz, Jaccard and BCE kernels (csrc/xbd_seg_losses.hip) and dahitra_amd.models.xbd_losses on the MI355X: the sort's order
exactly, loss and gradient against the float64 restatement of tests/_xbd_losses_cases.py under derived bounds, the module against
the reference's recorded results (tests/golden/xbd_losses.npz), determinism, HIP-graph capture and the refusals."""
import ctypes

import numpy as np
import pytest
import torch

import _xbd_losses_cases as K
from dahitra_amd import _lib, ops
from dahitra_amd.models import xbd, xbd_losses

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = ops.XBD_LOVASZ_TILE
SCAN_ROW = 256                # digit rows are scanned 256 workgroups' counts at a time: more tiles than that take a second step
LENGTHS = (1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3)
SHAPES = [(1, 1, n) for n in LENGTHS] + [(1, 1, 4 * T + 1), (3, 1, 37, 53), (2, 5, 48, 40)]      # 4 T + 1: room for a run above 2 T
IDS = ["x".join(map(str, s)) for s in SHAPES]


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.tensor(a, dtype=dtype, device=DEV)


def test_tile_is_the_librarys():
    assert _lib.lib().dh_xbd_lovasz_tile() == T


# ---- order, exact ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_image", (False, True))
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_order_is_the_stable_order(shape, per_image):
    x, t = K.hinge_inputs(shape, 11, T)
    for mode in (0, 1):
        got = ops.xbd_lovasz_order(dev(x), dev(t), mode, per_image).cpu().numpy()
        assert np.array_equal(got, K.lovasz_order(x, t, mode, per_image)), (shape, mode)


def test_inputs_reach_every_key_byte_both_signs_zero_and_a_long_run():
    x, t = K.hinge_inputs((1, 1, 4 * T + 1), 11, T)
    e, _ = K.errors(x.reshape(-1), t.reshape(-1).astype(np.int64), 0)
    bits = e.view(np.uint32)
    for byte in range(4):
        assert len(set(((bits >> (8 * byte)) & 255).tolist())) > (8 if byte == 3 else 64)          # the top byte: sign and exponent
    assert (e > 0).any() and (e < 0).any() and (bits == 0).any()
    assert np.bincount(np.unique(e, return_inverse=True)[1]).max() > 2 * T
    x1 = np.array([0.0, -0.0, 0.0, -0.0], dtype=np.float32).reshape(1, 1, 4)          # mode 1, target 0: errors |0 - +-0|
    assert ops.xbd_lovasz_order(dev(x1), dev(np.zeros((1, 1, 4), np.uint8)), 1).cpu().tolist() == [0, 1, 2, 3]


@pytest.mark.parametrize("per_image", (False, True))
def test_constant_input_keeps_the_identity(per_image):
    shape = (2, 3, 2 * T + 3)
    x = torch.full(shape, 0.75, device=DEV)
    t = torch.ones(shape, dtype=torch.uint8, device=DEV)
    got = ops.xbd_lovasz_order(x, t, 0, per_image).cpu().numpy()
    seg, nseg = K.segment_ids(shape, per_image)
    assert np.array_equal(got, np.argsort(seg, kind="stable"))


@pytest.mark.parametrize("shape", [(4, 1, 256, 256), (1, 1, SCAN_ROW * T + 5)], ids=("4x1x256x256", "past one scan step"))
def test_order_where_the_histogram_scan_takes_several_steps(shape):
    x, t = K.hinge_inputs(shape, 12, T)
    got = ops.xbd_lovasz_order(dev(x), dev(t), 0, False).cpu().numpy()
    assert np.array_equal(got, K.lovasz_order(x, t, 0, False))


# ---- values against the restatement ---------------------------------------------------------------------------------
def _special_targets(shape, t):
    """one image entirely 255, one without foreground, one with only foreground where the batch has them; a bad label"""
    t = t.copy()
    if shape[0] >= 3:
        t[0], t[1] = 255, 0
        t[2, 0] = 1
    elif shape[0] == 2:
        t[0, 0], t[0, 1], t[0, 2] = 255, 0, 1
    if t.size > 70:
        t.reshape(-1)[-3] = 7
        t.reshape(-1)[-9:-5] = 255
    return t


def _weights(C):
    return np.linspace(0.3, 1.1, C).astype(np.float32) if C > 1 else None


def _values(shape, mode, per_image, x, t):
    """Measured on the MI355X over every case of this file: loss within 0.5 ulp of the restatement, gradient within 0.5 * 2^-23
    (modes 0, 1) and 2.9 * 2^-23 (mode 2: the device's expf against numpy's)."""
    w = _weights(shape[1])
    ref = K.lovasz(x, t, mode, per_image, 255, w)
    yard = abs(K.lovasz_float32(x, t, mode, per_image, 255, w) - ref["loss"])
    bad = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    wd = None if w is None else dev(w)
    loss, channel, dx = ops.xbd_lovasz(dev(x), dev(t), mode, per_image, 255, wd, bad_out=bad)
    loss_f, channel_f, dx_f = ops.xbd_lovasz(dev(x), dev(t.astype(np.float32)), mode, per_image, 255, wd)
    assert torch.equal(loss, loss_f) and torch.equal(channel, channel_f) and torch.equal(dx, dx_f), "uint8 and float32 targets"
    got = dx.cpu().numpy().astype(np.float64)
    err = np.abs(got - ref["dx"])
    rel = float(np.max(np.where(err <= K.GRAD_ABS, 0.0, err / np.maximum(np.abs(ref["dx"]), 1e-300))))
    d_loss = abs(float(loss) - ref["loss"])
    print("%s mode %d per_image %d: loss off %.3e (bound %.3e), gradient %.2f * 2^-23 (bound %.0f)"
          % (shape, mode, per_image, d_loss, K.loss_bound(ref["loss"], yard), rel / K.ULP, K.GRAD_BOUND[mode] / K.ULP))
    assert int(bad) == ref["bad"]
    assert d_loss <= K.loss_bound(ref["loss"], yard)
    assert np.abs(channel.cpu().numpy() - ref["channel"]).max() <= K.loss_bound(np.abs(ref["channel"]).max(), yard)
    assert rel <= K.GRAD_BOUND[mode]
    return ref


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("per_image", (False, True))
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_values_on_logits_and_probabilities(shape, per_image, mode):
    x, t = K.hinge_inputs(shape, 13, T)
    _values(shape, mode, per_image, x, _special_targets(shape, t))


@pytest.mark.parametrize("per_image", (False, True))
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_values_through_the_sigmoid(shape, per_image):
    n = int(np.prod(shape))
    labels = _special_targets(shape, (np.random.default_rng(14).random(shape) < 0.4).astype(np.uint8))
    x, t = K.sigmoid_inputs(shape, 14, per_image, labels)
    assert x.size == n, "every element takes part: the share left out is 0"
    ref = _values(shape, 2, per_image, x, t)
    assert ref["gap"] >= 2.0 ** -19, "no last-bit difference of a sigmoid may reorder neighbours"


def test_seg_terms_against_float64():
    rng = np.random.default_rng(15)
    shape = (2, 5, 37, 41)
    # |x| stays below 8: past 16.6 a float32 sigmoid is 1 and mask_bceavg clamps its logarithm at -100, in the reference as here,
    # which no float64 evaluation shows
    x = (rng.standard_normal(shape) * 1.5).astype(np.float32)
    t = (rng.random(shape) < 0.4).astype(np.uint8)
    w = _weights(5)
    ref = K.seg_terms(x, t, w)
    for k, name in enumerate(("jaccard", "bce", "mask_bceavg", "dice")):
        kw = {name: 1.0}
        loss, terms, sums = ops.xbd_seg_terms_fwd(dev(x), dev(t), dev(w), **kw)
        loss_f, terms_f, sums_f = ops.xbd_seg_terms_fwd(dev(x), dev(t.astype(np.float32)), dev(w), **kw)
        assert torch.equal(loss, loss_f) and torch.equal(terms, terms_f)
        dx = ops.xbd_seg_terms_bwd(dev(x), dev(t), sums, dev(w), None, **kw).cpu().numpy()
        # float32 sigmoids summed in float64: the sums' relative error is far below 2^-23; four float operations finish a term
        assert np.abs(terms.cpu().numpy()[:, k] - ref["terms"][:, k]).max() <= 4 * K.ULP * np.abs(ref["terms"][:, k]).max(), name
        assert abs(float(loss) - float((w * ref["terms"][:, k]).sum())) <= 8 * K.ULP * abs(float(loss)), name
        g = ref["grads"][k]
        assert np.abs(dx - g).max() <= 4 * K.ULP * np.abs(g).max(), name
    none = ops.xbd_seg_terms_bwd(dev(x), dev(t), sums, dev(w), None).cpu().numpy()
    assert not none.any(), "zero weights: zero gradient"


# ---- module against the fixture -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return K.golden()


def _module_check(what, loss, grad, rec):
    l64, g64 = float(rec["loss64"]), rec["grad64"]
    yard_loss = abs(float(rec["loss32"]) - l64)
    yard_grad = float(np.abs(rec["grad32"].astype(np.float64) - g64).max() / np.abs(g64).max())
    d_loss, d_grad = abs(loss - l64), float(np.abs(grad - g64).max() / np.abs(g64).max())
    print("%s: loss off %.3e (bound %.3e), gradient %.3e (bound %.3e)" % (what, d_loss, K.loss_bound(l64, yard_loss), d_grad, 2 * yard_grad))
    assert d_loss <= K.loss_bound(l64, yard_loss), what
    assert d_grad <= 2 * yard_grad, what


def _run(loss_fn, logits, targets):
    x = dev(logits).requires_grad_(True)
    loss = loss_fn(x, dev(targets))
    loss.backward()
    return loss, x.grad


@pytest.mark.parametrize("per_image", (0, 1))
@pytest.mark.parametrize("case,term", [("plain", k) for k in K.TERMS] + [("void", "lovasz"), ("void", "lovasz_sigmoid")])
def test_every_term_against_the_reference(gold, case, term, per_image):
    key = "%s_%s_%d_" % (case, term, per_image)
    fn = xbd_losses.ComboLoss({term: 1}, per_image=bool(per_image))
    loss, grad = _run(fn, gold[case + "_logits"], gold[case + "_targets"])
    assert set(fn.values) == {term} and float(fn.values[term]) == float(loss)
    _module_check(key, float(loss), grad.cpu().numpy().astype(np.float64), {k: gold[key + k] for k in ("loss32", "grad32", "loss64", "grad64")})


@pytest.mark.parametrize("per_image", (0, 1))
def test_the_mix_is_the_weighted_sum_of_its_terms(gold, per_image):
    logits, targets = gold["plain_logits"], gold["plain_targets"]
    fn = xbd_losses.ComboLoss(dict(K.MIX), per_image=bool(per_image))
    loss, grad = _run(fn, logits, targets)
    assert set(fn.values) == set(K.MIX)
    l64 = sum(w * float(gold["plain_%s_%d_loss64" % (k, per_image)]) for k, w in K.MIX.items())
    g64 = sum(w * gold["plain_%s_%d_grad64" % (k, per_image)] for k, w in K.MIX.items())
    l32 = sum(w * float(gold["plain_%s_%d_loss32" % (k, per_image)]) for k, w in K.MIX.items())
    g32 = sum(w * gold["plain_%s_%d_grad32" % (k, per_image)].astype(np.float64) for k, w in K.MIX.items())
    _module_check("mix per_image=%d" % per_image, float(loss), grad.cpu().numpy().astype(np.float64),
                  {"loss32": l32, "grad32": g32, "loss64": l64, "grad64": g64})
    terms = sum(w * float(fn.values[k]) for k, w in K.MIX.items())
    assert abs(float(loss) - terms) <= 8 * K.ULP * abs(terms)


def test_four_dimensional_input_is_the_sum_over_channels():
    rng = np.random.default_rng(16)
    x = (rng.standard_normal((2, 3, 20, 24)) * 2).astype(np.float32)
    t = (rng.random(x.shape) < 0.4).astype(np.uint8)
    for per_image in (False, True):
        fn = xbd_losses.ComboLoss(dict(K.MIX, lovasz_sigmoid=0.1, mask_bceavg=0.1), per_image=per_image)
        loss, grad = _run(fn, x, t)
        parts = [_run(fn, x[:, c], t[:, c]) for c in range(3)]
        total = sum(float(p[0]) for p in parts)
        assert abs(float(loss) - total) <= 8 * K.ULP * abs(total)
        g = torch.stack([p[1] for p in parts], 1)
        assert float((grad - g).abs().max()) <= 8 * K.ULP * float(g.abs().max())


def test_functions_and_stand_alone_classes(gold):
    logits, targets, probs = gold["plain_logits"], gold["plain_targets"], gold["plain_probs"]
    for per_image in (False, True):
        hinge = K.lovasz(logits[:, None], targets[:, None], 0, per_image, None)
        got = xbd_losses.lovasz_hinge(dev(logits), dev(targets), per_image=per_image)
        assert abs(float(got) - hinge["loss"]) <= 2 * np.spacing(np.float32(hinge["loss"]))
        soft = K.lovasz(probs[:, None], targets[:, None], 1, per_image, None)
        got = xbd_losses.LovaszLossSigmoid(per_image=per_image)(dev(probs), dev(targets))
        assert abs(float(got) - soft["loss"]) <= 2 * np.spacing(np.float32(soft["loss"]))
    flat = K.lovasz(logits.reshape(1, 1, -1), targets.reshape(1, 1, -1), 0, False, None)
    assert abs(float(xbd_losses.lovasz_hinge_flat(dev(logits).view(-1), dev(targets).view(-1))) - flat["loss"]) <= 2 * np.spacing(np.float32(flat["loss"]))
    lab = np.sort(targets.reshape(-1))[::-1].copy()
    g = xbd_losses.lovasz_grad(dev(lab)).cpu().numpy()
    assert np.abs(g - K.closed_form_g(lab)).max() <= K.ULP * K.closed_form_g(lab).max()
    for fn, term in ((xbd_losses.jaccard, "jaccard"), (xbd_losses.DiceLoss(), "dice"), (xbd_losses.MaskLoss(), "mask_bceavg"),
                     (xbd_losses.FocalLoss2d(), "focal"), (xbd_losses.iou_round, "jaccard")):
        ref = float(gold["plain_%s_0_loss64" % term])              # on the recorded float32 probabilities: their rounding remains
        got = float(fn(dev(probs), dev(targets)))
        assert abs(got - ref) <= 16 * K.ULP * abs(ref), term
    ref = float(gold["plain_bce_0_loss64"])
    assert abs(float(xbd_losses.StableBCELoss()(dev(logits), dev(targets))) - ref) <= 4 * K.ULP * abs(ref)


@pytest.mark.parametrize("name,term", (("DiceLoss", "dice"), ("JaccardLoss", "jaccard"), ("MaskLoss", "mask_bceavg"),
                                       ("FocalLoss2d", "focal"), ("StableBCELoss", "bce")))
def test_stand_alone_classes_gradient_against_float64_autograd(gold, name, term):
    """the classes take probabilities (StableBCELoss: logits): d loss / d input of dh_xbd_seg_terms_bwd with probs=1, and of its
    dice and focal terms, against torch's float64 autograd of the expressions of xBD_code/losses.py on the same float32 input.
    The kernel works in fp64 and rounds once; I, S and T reach it as float32: 4 * 2^-23 of the largest element covers both."""
    given = gold["plain_logits"] if term == "bce" else gold["plain_probs"]
    targets = gold["plain_targets"].copy()
    if term == "focal":
        targets[0, :3] = 255                               # FocalLoss2d leaves them out
        given = given.copy()
        given[1, 0, :4], given[1, 1, :4] = 0.0, 1.0        # outside the clamp: no gradient
    x = torch.tensor(given, dtype=torch.float64, requires_grad=True)
    t = torch.tensor(targets, dtype=torch.float64)
    e = 1e-6
    if term == "dice":
        ref = 1 - (2 * (x * t).sum() + e) / (x.sum() + t.sum() + e)
    elif term == "jaccard":
        ref = 1 - ((x * t).sum() + e) / (x.sum() + t.sum() - (x * t).sum() + e)
    elif term == "mask_bceavg":
        ref = torch.nn.functional.binary_cross_entropy(x.view(-1), t.view(-1))
    elif term == "bce":
        ref = (x.clamp(min=0) - x * t + (1 + (-x.abs()).exp()).log()).mean()
    else:
        keep = t.view(-1) != 255
        o = torch.clamp(x.view(-1)[keep], float(np.float32(e)), float(np.float32(1) - np.float32(e)))
        tt = torch.clamp(t.view(-1)[keep], float(np.float32(e)), float(np.float32(1) - np.float32(e)))
        pt = (1 - tt) * (1 - o) + tt * o
        ref = (-(1 - pt) ** 2 * torch.log(pt)).mean()
    ref.backward()
    loss, grad = _run(getattr(xbd_losses, name)(), given, targets)
    g64 = x.grad.numpy()
    d_loss, d_grad = abs(float(loss) - float(ref)) / abs(float(ref)), float(np.abs(grad.cpu().numpy() - g64).max() / np.abs(g64).max())
    print("%s: loss off %.3e (relative), gradient %.3e of its maximum" % (name, d_loss, d_grad))
    assert d_loss <= 4 * K.ULP and d_grad <= 4 * K.ULP
    if term == "focal":
        assert not grad[0, :3].any() and not grad[1, :2, :4].any()


def test_xbd_loss_with_and_without_the_hinge():
    rng = np.random.default_rng(17)
    out = (rng.standard_normal((2, 5, 24, 20)) * 2).astype(np.float32)
    msk = (rng.random(out.shape) < 0.4).astype(np.float32)
    base, gbase = _run(lambda o, m: xbd.xbd_loss(o, m), out, msk)
    zero, gzero = _run(lambda o, m: xbd.xbd_loss(o, m, lovasz=0), out, msk)
    assert torch.equal(base, zero) and torch.equal(gbase, gzero)
    with_hinge, g = _run(lambda o, m: xbd.xbd_loss(o, m, lovasz=0.5), out, msk)
    w = np.array(xbd.CHANNEL_WEIGHTS, dtype=np.float32)
    ref = K.lovasz(out, msk, 0, False, None, w)
    want = float(base) + 0.5 * ref["loss"]
    assert abs(float(with_hinge) - want) <= 4 * K.ULP * abs(want)
    gw = gbase.cpu().numpy().astype(np.float64) + 0.5 * ref["dx"]
    assert np.abs(g.cpu().numpy() - gw).max() <= 4 * K.ULP * np.abs(gw).max()


# ---- determinism and capture ------------------------------------------------------------------------------------------
def test_two_calls_give_equal_bits():
    x, t = K.hinge_inputs((2, 5, 48, 40), 18, T)
    for mode in (0, 1, 2):
        a = ops.xbd_lovasz(dev(x), dev(t), mode, False, 255, dev(_weights(5)))
        b = ops.xbd_lovasz(dev(x), dev(t), mode, False, 255, dev(_weights(5)))
        assert all(torch.equal(p, q) for p, q in zip(a, b)), mode


def test_loss_and_backward_replay_from_a_graph():
    shape = (2, 3, 40, 36)
    rng = np.random.default_rng(19)
    inputs = [((rng.standard_normal(shape) * 2).astype(np.float32), (rng.random(shape) < 0.4).astype(np.uint8)) for _ in range(3)]
    fn = xbd_losses.ComboLoss(dict(K.MIX), per_image=True)
    eager = []
    for x, t in inputs:
        loss, grad = _run(fn, x, t)
        eager.append((loss.clone(), grad.clone()))
    sx = dev(inputs[0][0]).requires_grad_(True)
    st = dev(inputs[0][1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn(sx, st).backward()                                    # warm-up outside the capture: code objects loaded
    torch.cuda.current_stream().wait_stream(side)
    sx.grad = None
    # GraphedXbdStep's pattern: the capture stream inherits the workspace the warm-up grew, so that nothing the kernels use is
    # allocated inside the capture and no entry of a stream that is gone stays in ops._ws
    capture = torch.cuda.Stream()
    ops.rekey_workspace(sx.device, side, capture)
    held = ops._ws[(str(sx.device), capture.cuda_stream)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=capture):
        sloss = fn(sx, st)
        sloss.backward()
    assert ops._ws[(str(sx.device), capture.cuda_stream)] is held, "the capture grew no workspace"
    assert (str(sx.device), side.cuda_stream) not in ops._ws
    for (x, t), (loss, grad) in zip(inputs[::-1], eager[::-1]):
        with torch.no_grad():
            sx.copy_(dev(x))
            st.copy_(dev(t))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(sloss, loss) and torch.equal(sx.grad, grad)


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    L = _lib.lib()
    n = 1000
    x = torch.randn(1, 1, n, device=DEV)
    t = torch.ones(1, 1, n, dtype=torch.uint8, device=DEV)
    need = ops._ws_bytes("dh_xbd_lovasz_workspace_size", n, 1)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    out = torch.full((n + 2,), -7.0, device=DEV)
    order = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    P, S = ops.P, ops.S

    def fwd(xp=P(x), tp=P(t), B=1, C=1, HW=n, mode=0, per_image=0, wsp=P(ws), wsb=need, kind=1, lossp=P(out[n:n + 1])):
        return L.dh_xbd_lovasz_fwd(xp, tp, kind, B, C, HW, mode, per_image, 255, None, lossp, P(out[n + 1:]), P(out[:n]), None, wsp, wsb, S())

    for what, rc in (("null x", fwd(xp=None)), ("null target", fwd(tp=None)), ("null output", fwd(lossp=None)), ("empty", fwd(HW=0)),
                     ("no batch", fwd(B=0)), ("257 segments", fwd(C=257, HW=1)), ("257 planes", fwd(B=257, HW=1, per_image=1)),
                     ("short workspace", fwd(wsb=need - 1)), ("null workspace", fwd(wsp=None)), ("mode", fwd(mode=3)),
                     ("kind", fwd(kind=2)), ("beyond 2^30", fwd(B=2, C=1, HW=1 << 30)),
                     ("order: short workspace", L.dh_xbd_lovasz_order(P(x), P(t), 1, 1, 1, n, 0, 0, 255, P(order), P(ws), need - 1, S())),
                     ("order: null", L.dh_xbd_lovasz_order(P(x), P(t), 1, 1, 1, n, 0, 0, 255, None, P(ws), need, S()))):
        assert rc != 0, what
        assert L.dh_last_error().decode().startswith("xbd_lovasz"), what
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((order == -7).all()) and not bool(ws.any()), "nothing was written"
    with pytest.raises(ValueError):
        ops.xbd_lovasz(torch.zeros(1, 257, 4, device=DEV), torch.zeros(1, 257, 4, device=DEV), 0)
    with pytest.raises(ValueError):
        ops.xbd_lovasz(x, t.to(torch.int32), 0)
    with pytest.raises(ValueError):
        ops.xbd_lovasz(x, t, "softmax")
    assert fwd() == 0
    torch.cuda.synchronize()
    assert not bool((out == -7.0).any())
