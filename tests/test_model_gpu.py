"""End-to-end parity of the HIP path (through define_G / focal_loss / AdamW, i.e. through the C ABI)
against (a) the golden fixtures produced by the reference and (b) the CPU oracle on the same seeded
inputs.  fp32 mode: logits within 1e-3 relative (north-star bar; we assert 2e-4), masks identical
outside the tie band; bf16 mode: worst logit within 0.15 of the logit scale, mask disagreement < 3 %.

Gradient tolerances come from the MEASURED fp32 noise floor of this computation: tools/grad_noise_floor.py runs the oracle
in float64 and float32 on the inputs of the gradient test and commits the per-tensor distances
(tests/golden/grad_noise_floor.json; tests/test_oracle_golden.py re-measures them on the CPU).  With the well-conditioned
fixture weights the floor of the ResNet-18 nets is ~1e-5 (median) / 1e-3 (worst tensor, relative L2); the 50-layer ResNet-50
variant amplifies rounding to 1e-2 / 1.3e-2.  test_gradients_match_oracle_fp32 bounds the HIP gradients by a stated multiple
of those figures; the fixture-based train test keeps looser per-tensor bounds (GRAD_TOL*) because the fixture stores a
subset of the gradients only."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cdnet_ref as O
import _bounds as B

pytestmark = pytest.mark.gpu
BF16_MAX_ERR = 0.15    # a-priori bound on the worst bf16 logit error, in units of the reference's max |logit| (measured: 0.036 / 0.090)
# Fixture-based train test, of max|grad| per stored tensor (tests/_bounds.py; measured on MI355X, profiles/r06a_grad_fixture_values.txt):
GRAD_TOL = B.GRAD_TOL_TIE   # small per-channel tensors a flipped ReLU / max-pool tie can move (4.2e-2 exact mode, 1.7e-3 bf16x3)
GRAD_TOL_REST = 3e-3   # every other stored tensor: 3 x the worst measured (2.0e-5 exact mode, 9.5e-4 bf16x3)
GRAD_TOL_R50 = 0.15    # ResNet-50 (6.8e-2 / 4.8e-2 exact mode, 7.0e-2 / 9.9e-3 bf16x3; the oracle's own fp32-vs-fp64 floor is 0.13 rel-max)
NORM_TOL = 4e-3        # gradient norms of every tensor: 3 x the worst measured (1.2e-3 exact mode, 2.3e-4 bf16x3)
NORM_TOL_R50 = 3e-2    # (1.0e-2 exact mode, 3.3e-3 bf16x3)
# The two parity modes, held to the SAME bounds: "fp32" = exact fp32 MFMA; "bf16x3" = the same fp32
# pipeline with every matrix product on the 16-bit matrix cores as split products (dh_set_f32_mma_mode) -- the forward by default
# in the two-plane / three-product form on FP16 planes (mode 3: ~2^-21, operands inside fp16's range; the three-plane / six-product
# bf16 form, mode 2, 2^-23, is its fallback: DAHITRA_X3_FWD=2), data and weight gradients in the two-plane / three-product bf16 form
# (mode 1: 2^-17).  Measured on MI355X: logits 4e-6 .. 1.3e-5 of the logit scale (ResNet-50 train mode 8.5e-5), gradients of
# base_transformer_pos_s4 at 2.2e-5 median / 3.2e-5 worst tensor relative L2 from the oracle (exact mode: 1.3e-5 / 7.0e-4).
# (With the forward in the three-product form too the logits still pass -- 4e-5 .. 1.4e-4 -- but the gradients sit at
# 1.9e-3: they are ~20x more sensitive to activation error than the logits are.)
PARITY_MODES = ["fp32", "bf16x3"]

R50 = "base_transformer_pos_s4_resnet50"      # ctor-only model (networks.py:192-195): ResNet-50 trunk, dilation 2
NETS = ["base_transformer_pos_s4", "base_transformer_pos_s4_dd8", "base_transformer_pos_s4_dd8_o5",
        "base_transformer_pos_s4_dd8_dedim8", "base_transformer_pos_s4_dd8_t8_e2d4", "newUNetTrans", R50]


def make_net(name, dtype="fp32"):
    from dahitra_amd.models.networks import BASE_Transformer, define_G, init_net
    if name == R50:
        net = init_net(BASE_Transformer(input_nc=3, output_nc=2, token_len=4, resnet_stages_num=4, with_pos='learned',
                                        backbone='resnet50', compute_dtype=dtype), gpu_ids=[0])
    else:
        net = define_G(types.SimpleNamespace(net_G=name, compute_dtype=dtype), gpu_ids=[0])
    net.load_state_dict(O.deterministic_state(name))
    return net


@pytest.mark.parametrize("cdtype", PARITY_MODES)
@pytest.mark.parametrize("name", NETS)
def test_forward_matches_reference_golden_fp32(name, cdtype, golden_dir):
    g = np.load(os.path.join(golden_dir, "fwd_%s.npz" % name))
    cfg = O.get_config(name)
    bs, size, stride = int(g["batch"]), int(g["size"]), int(g["stride"])
    a, b, lab = O.synthetic_batch(bs, size, n_class=cfg["n_class"])
    for mode in ("eval", "train"):
        net = make_net(name, cdtype)
        net.train(mode == "train")
        with torch.no_grad():
            y = net(a.cuda(), b.cuda()).cpu()
        want = torch.from_numpy(g["logits_" + mode])
        got = y[..., ::stride, ::stride]
        scale = float(want.abs().max())
        err = float((got - want).abs().max()) / scale
        tol = 2e-4          # both modes (north star: 1e-3)
        print("%s %s %s: logits rel err %.3e (bound %.1e)" % (name, cdtype, mode, err, tol))
        assert err <= tol, "%s %s %s: logits rel err %.3e" % (name, cdtype, mode, err)
        assert abs(float(y.double().sum()) - float(g["sum_" + mode])) <= tol * float(g["abssum_" + mode])
        # class masks: identical wherever the reference margin is outside the fp32 tie band
        from dahitra_amd.models.losses import argmax_mask
        mask = argmax_mask(y.cuda()).cpu().numpy().astype(np.uint8)
        ref_mask = np.unpackbits(g["mask_" + mode])[:mask.size].reshape(mask.shape) if cfg["n_class"] == 2 \
            else np.asarray(g["mask_" + mode]).reshape(mask.shape)
        # tie band from the REFERENCE's stored margins (fixtures at stride 1 hold one per pixel); the strided 256x256
        # fixture falls back to the margins of the HIP logits (the large-margin test below covers that net per pixel)
        if stride == 1:
            margin = np.asarray(g["margin_" + mode]).astype(np.float32).reshape(mask.shape)
        else:
            top2 = y.topk(2, dim=1).values
            margin = (top2[:, 0] - top2[:, 1]).numpy()
        band = margin <= 2 * tol * scale
        diff = (mask != ref_mask)
        print("%s %s: mask flips total %d, outside the tie band %d, band fraction %.5f (reference margins: %s)"
              % (name, mode, int(diff.sum()), int((diff & ~band).sum()), float(band.mean()), stride == 1))
        assert int((diff & ~band).sum()) == 0, "%s %s: %d mask flips outside the tie band" % (name, mode, int((diff & ~band).sum()))
        assert band.mean() < 0.02
        if mode == "train":
            sd = net.state_dict()
            assert np.allclose(sd["resnet.bn1.running_mean"].cpu().numpy(), g["bn1_running_mean"], atol=2e-6)
            assert np.allclose(sd["resnet.bn1.running_var"].cpu().numpy(), g["bn1_running_var"], rtol=1e-5, atol=2e-6)
            from dahitra_amd.models.losses import focal_loss
            assert abs(float(focal_loss(y.cuda(), lab.cuda())) - float(g["focal"])) < 2e-5


@pytest.mark.parametrize("cdtype", PARITY_MODES)
@pytest.mark.parametrize("name", ["base_transformer_pos_s4", "newUNetTrans", R50])
def test_train_steps_match_reference_golden_fp32(name, cdtype, golden_dir):
    from dahitra_amd.models import losses
    from dahitra_amd.optim import AdamW
    g = np.load(os.path.join(golden_dir, "train_%s.npz" % name))
    cfg = O.get_config(name)
    a, b, lab = O.synthetic_batch(int(g["batch"]), int(g["size"]), n_class=cfg["n_class"])
    a, b, lab = a.cuda(), b.cuda(), lab.cuda()
    net = make_net(name, cdtype).train()
    opt = AdamW(net.parameters(), lr=float(g["lr"]), betas=(0.9, 0.999), weight_decay=0.01)
    got_losses = []
    for it in range(int(g["steps"])):
        y = net(a, b)
        opt.zero_grad()
        loss = losses.focal_loss(y, lab)
        loss.backward()
        if it == 0:
            params = dict(net.named_parameters())
            nograd = sorted(k for k, p in params.items() if p.grad is None)
            assert nograd == sorted(g["nograd_keys"].tolist())
            verbose = ("%s %s" % (name, cdtype)) if os.environ.get("DAHITRA_TEST_VERBOSE") else None
            worst = B.assert_grad_norms(params, g["gradnorm_keys"].tolist(), g["gradnorm_vals"].tolist(),
                                        NORM_TOL_R50 if name == R50 else NORM_TOL, verbose=verbose)
            # the gradients the fixture stores in full: small per-channel tensors, where ONE flipped tie of a ReLU or max-pool moves
            # an element by percents of the tensor's maximum, keep the tie-sized bound; the others 3 x the measured worst
            # (tests/_bounds.py); the oracle-based test below holds every tensor to a multiple of the measured noise floor
            n, worst_g = B.assert_stored_grads(params, g, GRAD_TOL_R50 if name == R50 else GRAD_TOL_REST,
                                               tol_tie=B.GRAD_TOL_TIE_R50 if name == R50 else B.GRAD_TOL_TIE, verbose=verbose)
            print("%s: %d stored gradients: worst |err| / max|grad| %.2e (tie-sized tensors) / %.2e (others); gradient norms: worst rel err %.2e"
                  % (name, n, worst_g["tie"], worst_g["rest"], worst))
        opt.step()
        got_losses.append(float(loss))
    # step 0 is a pure function of the fixture's weights: tight.  Later steps follow an Adam trajectory,
    # which is ill-conditioned (the first update is lr*sign(g): a near-zero gradient whose sign differs
    # inside the fp32 noise floor moves that weight by 2*lr), so they are only required to track.
    assert abs(got_losses[0] - float(g["losses"][0])) < 2e-5, (got_losses, g["losses"])
    assert np.allclose(got_losses, g["losses"], rtol=0.15), (got_losses, g["losses"])
    sd = net.state_dict()
    for k, v in zip(g["finalnorm_keys"].tolist(), g["finalnorm_vals"].tolist()):
        got = float(sd[k].double().norm())
        assert abs(got - v) <= 0.1 * max(v, 1e-8) + 1e-4, (k, got, v)      # trajectory quantity: tracks only
    assert int(sd["resnet.bn1.num_batches_tracked"]) == int(g["nbt"])


def _floor(name, golden_dir):
    """tests/golden/grad_noise_floor.json (tools/grad_noise_floor.py): the oracle's own float32-vs-float64 gradient distances;
    the bounds derived from it are tests/_bounds.py's (FLOOR_X_WORST / _MEDIAN / _COS)"""
    return B.floor(name, golden_dir)


@pytest.mark.parametrize("cdtype", PARITY_MODES)
@pytest.mark.parametrize("name", ["base_transformer_pos_s4", "base_transformer_pos_s4_dd8_t8_e2d4", "newUNetTrans", R50])
def test_gradients_match_oracle_fp32(name, cdtype, golden_dir):
    """every parameter gradient against the oracle's autograd on the case of tools/grad_noise_floor.py (odd batch, 64 x 64;
    newUNetTrans: 2 x 256 x 256), bounded by the measured fp32 noise floor of this computation: per-tensor relative L2 and
    the median over tensors, plus the per-tensor cosine.
    Both parity modes at the same bounds (bf16x3 measured: s4 median 2.2e-5, worst tensor 3.2e-5)."""
    from dahitra_amd.models import losses
    fl = _floor(name, golden_dir)
    cfg = O.get_config(name)
    a, b, lab = O.synthetic_batch(fl["case"]["batch"], fl["case"]["size"], seed=fl["case"]["seed"], n_class=cfg["n_class"])
    st = O.TrainState(name, O.deterministic_state(name), lr=0.01)
    logits = O.forward(st.sd, name, a, b, training=True)
    O.focal_loss(logits, lab).backward()
    net = make_net(name, cdtype).train()
    y = net(a.cuda(), b.cuda())
    losses.focal_loss(y, lab.cuda()).backward()
    got, ref = {}, {}
    for k, p in net.named_parameters():
        assert (p.grad is None) == (st.sd[k].grad is None), k
        if p.grad is not None:
            got[k], ref[k] = p.grad, st.sd[k].grad
    B.assert_grads_at_floor(got, ref, fl, "%s %s" % (name, cdtype))


@pytest.mark.parametrize("name", ["newUNetTrans", "base_transformer_pos_s4_dd8"])
def test_teacher_forced_second_and_third_steps_match_the_oracle(name):
    """Steps 2 and 3 of an AdamW trajectory, TEACHER-FORCED: the oracle takes three train steps on a fixed batch; its complete
    state at the start of step k (parameters, BatchNorm buffers, Adam moments and step count: what a checkpoint holds) is
    loaded into the HIP net + optimizer, ONE HIP step runs, and the result is compared with the oracle's own step k -- loss, and
    the parameter UPDATE element-wise wherever the gradient is well-conditioned (|g| > 1e-2 max|g| of its tensor: from step 2 on
    the update is smooth in g there, unlike the first update lr * sign(g)).  A free-running comparison would only measure how
    fast two fp32 trajectories diverge."""
    from dahitra_amd.models import losses
    from dahitra_amd.optim import AdamW
    lr = 1e-3
    size = 256 if name == "newUNetTrans" else 64
    a, b, lab = O.synthetic_batch(2, size, seed=41)
    st = O.TrainState(name, O.deterministic_state(name), lr=lr)
    tkeys = O.trainable_keys(name)
    cases = []
    for it in range(3):
        snap = None
        if it >= 1:
            snap = dict(sd={k: v.detach().clone() for k, v in st.sd.items()},
                        opt={k: {n: (t.clone() if torch.is_tensor(t) else t) for n, t in st.opt.state[p].items()}
                             for k, p in zip(tkeys, st.params) if p in st.opt.state})
        _, loss = st.step(a, b, lab)
        if snap is not None:
            snap.update(loss=loss, grads={k: p.grad.clone() for k, p in zip(tkeys, st.params) if p.grad is not None},
                        after={k: p.detach().clone() for k, p in zip(tkeys, st.params)})
            cases.append(snap)
    for step_no, c in zip((2, 3), cases):
        net = make_net(name)
        net.load_state_dict(c["sd"])
        net.train()
        opt = AdamW(net.parameters(), lr=lr, betas=(0.9, 0.999), weight_decay=0.01)
        names = [k for k, _ in net.named_parameters()]
        state = {i: {"step": torch.tensor(float(c["opt"][k]["step"])), "exp_avg": c["opt"][k]["exp_avg"].cuda(),
                     "exp_avg_sq": c["opt"][k]["exp_avg_sq"].cuda()} for i, k in enumerate(names) if k in c["opt"]}
        sd = opt.state_dict()
        sd["state"] = state
        opt.load_state_dict(sd)
        y = net(a.cuda(), b.cuda())
        opt.zero_grad()
        loss = losses.focal_loss(y, lab.cuda())
        loss.backward()
        opt.step()
        assert opt.step_count(net) == step_no
        assert abs(float(loss) - c["loss"]) <= 2e-5 * max(1.0, abs(c["loss"])), (step_no, float(loss), c["loss"])
        bad = tot = 0
        worst = 0.0
        for k, p in net.named_parameters():
            g = c["grads"].get(k)
            if g is None:
                continue
            sel = g.abs() > 1e-2 * g.abs().max()
            d_hip = (p.detach().cpu() - c["sd"][k])[sel]
            d_ref = (c["after"][k] - c["sd"][k])[sel]
            e = (d_hip - d_ref).abs()
            bad += int((e > 0.02 * lr).sum())
            tot += int(sel.sum())
            worst = max(worst, float(e.max()) / lr if e.numel() else 0.0)
        print("%s step %d (teacher-forced): loss %.7f (oracle %.7f); update differs by > 0.02 lr on %d of %d well-conditioned "
              "elements (worst %.3f lr)" % (name, step_no, float(loss), c["loss"], bad, tot, worst))
        assert tot > 1e5 and bad <= 2e-3 * tot          # (measured: <= 9.7e-4 of the elements, worst 0.26 lr)


@pytest.mark.parametrize("cdtype", PARITY_MODES)
@pytest.mark.parametrize("name", ["base_transformer_pos_s4", "newUNetTrans"])
def test_masks_bit_exact_on_large_margin_fixture_fp32(name, cdtype, golden_dir):
    """north star: "class masks bit-exact".  Fixture written by the reference with an antisymmetric head
    (oracle/cdnet_ref.large_margin_state): the reference's own per-pixel margins put < 0.1 % of the pixels inside the
    4e-4 * max|logit| band that a 2e-4 logit bound cannot decide; every other pixel must carry the reference's class."""
    g = np.load(os.path.join(golden_dir, "margin_%s.npz" % name))
    bs, size = int(g["batch"]), int(g["size"])
    a, b, _ = O.synthetic_batch(bs, size, seed=int(g["seed"]))
    from dahitra_amd.models.losses import argmax_mask
    for mode in ("eval", "train"):
        net = make_net(name, cdtype)
        net.load_state_dict(O.large_margin_state(name))
        net.train(mode == "train")
        with torch.no_grad():
            y = net(a.cuda(), b.cuda())
        scale = float(g["scale_" + mode])
        st = 4 if size > 64 else 1
        err = float((y.cpu()[..., ::st, ::st] - torch.from_numpy(g["logits_" + mode])).abs().max()) / scale
        assert err <= 2e-4, (name, mode, err)
        mask = argmax_mask(y).cpu().numpy().astype(np.uint8)
        ref_mask = np.unpackbits(g["mask_" + mode])[:mask.size].reshape(mask.shape)
        margin = np.asarray(g["margin_" + mode]).astype(np.float32)
        band = margin <= 4e-4 * scale
        diff = mask != ref_mask
        print("%s %s %s (large margins): flips total %d, outside band %d, band fraction %.5f, logits rel err %.2e"
              % (name, cdtype, mode, int(diff.sum()), int((diff & ~band).sum()), float(band.mean()), err))
        assert float(band.mean()) < 0.002
        assert int((diff & ~band).sum()) == 0


def _bf16_rounded(sd):
    return {k: (v.bfloat16().float() if v.dtype.is_floating_point and v.dim() > 1 else v) for k, v in sd.items()}


@pytest.mark.parametrize("name", ["base_transformer_pos_s4", "newUNetTrans"])
def test_bf16_mode_within_3x_the_bf16_input_rounding_error(name):
    """bf16 throughput mode against the fp32 oracle, bounded by the error the fp32 HIP pipeline itself shows when only
    its weights and images are rounded to bf16 (the unavoidable part of computing in bf16): relative L2 distance of
    the logits <= 3x that (measured on MI355X: 2.3x for base_transformer_pos_s4 at 128x128 -- the bf16 pipeline also
    rounds ~40 activation tensors, the comparison pipeline none; the ResNet-50 test uses the same 3x), mask flips
    with a reference margin above 2 x BF16_MAX_ERR (a fixed, a-priori bound on the worst bf16 logit error, asserted) = 0 on the
    large-margin state; flips above 0.05 of the logit scale: at most 0.4 % of the pixels."""
    cfg = O.get_config(name)
    size = 256 if name == "newUNetTrans" else 128
    a, b, lab = O.synthetic_batch(2, size, seed=5, n_class=cfg["n_class"])
    sd = O.large_margin_state(name)
    with torch.no_grad():
        ref = O.forward({k: v.clone() for k, v in sd.items()}, name, a, b, training=True)

    def run(dtype, state, x1, x2):
        net = make_net(name, dtype)
        net.load_state_dict(state)
        net.train()
        with torch.no_grad():
            return net(x1.cuda(), x2.cuda()).float().cpu()

    l2 = lambda u, v: float((u - v).norm() / v.norm())
    y32 = run("fp32", sd, a, b)
    y_round = run("fp32", _bf16_rounded(sd), a.bfloat16().float(), b.bfloat16().float())
    y = run("bf16", sd, a, b)
    sens, got = l2(y_round, ref), l2(y, ref)
    scale = float(ref.abs().max())
    err = float((y - ref).abs().max()) / scale
    err_round = float((y_round - ref).abs().max()) / scale
    # masks: FIXED bands from the reference-pinned margins (the oracle's logits; scale = its max |logit|), not from the error
    # measured here.  BF16_MAX_ERR bounds the worst bf16 logit a priori; a pixel whose margin exceeds twice that cannot flip
    # while the bound holds, and the bound is asserted.  Between 0.05 and 2 x BF16_MAX_ERR of the scale flips are possible
    # only where the error is near its maximum: a small, stated share.
    margin = (ref[:, 0] - ref[:, 1]).abs() / scale
    diff = torch.argmax(y, 1) != torch.argmax(ref, 1)
    outside = diff & (margin > 2.0 * BF16_MAX_ERR)
    mid = diff & (margin > 0.05)
    print("bf16 %s: logits l2 %.3e (fp32 pipeline on bf16-rounded inputs: %.3e, fp32 pipeline: %.1e); max err %.3e "
          "(rounded inputs %.3e, a-priori bound %.2f); mask flips %d of %d (%.3f %%); with reference margin > 0.05: %d (of %.1f %% "
          "of the pixels), > %.2f: %d (of %.1f %%)"
          % (name, got, sens, l2(y32, ref), err, err_round, BF16_MAX_ERR, int(diff.sum()), diff.numel(),
             100 * float(diff.float().mean()), int(mid.sum()), 100 * float((margin > 0.05).float().mean()), 2 * BF16_MAX_ERR,
             int(outside.sum()), 100 * float((margin > 2 * BF16_MAX_ERR).float().mean())))
    assert l2(y32, ref) <= 2e-4
    assert got <= 3.0 * sens, (got, sens)
    assert err <= BF16_MAX_ERR, err
    assert int(outside.sum()) == 0
    assert float((margin > 2.0 * BF16_MAX_ERR).float().mean()) > 0.2          # the band leaves a real share of the pixels to check
    assert int(mid.sum()) <= 4e-3 * diff.numel(), int(mid.sum())            # (measured: 0.1 % / 0)
    assert float(diff.float().mean()) < 0.03


def _bf16_grads(name, a, b, lab, monkeypatch=None, env=()):
    """gradients of one bf16 train-mode step of the HIP path (fresh net; `env`: engine switches read at construction)"""
    from dahitra_amd.models import losses
    for k in env:
        monkeypatch.setenv(k, "1")
    net = make_net(name, "bf16").train()
    for k in env:
        monkeypatch.delenv(k)
    y = net(a.cuda(), b.cuda())
    loss = losses.focal_loss(y, lab.cuda())
    loss.backward()
    return {k: p.grad.float().cpu() for k, p in net.named_parameters() if p.grad is not None}, y.detach().float().cpu(), float(loss)


UNET_FUSIONS = ("DAHITRA_NO_SPLIT_CAT", "DAHITRA_NO_PHASE_UPCONV", "DAHITRA_NO_FUSED_STEM_BWD_UNET")


@pytest.mark.parametrize("name", ["base_transformer_pos_s4", "newUNetTrans"])
def test_bf16_gradients_against_the_oracle_and_the_input_rounding_yardstick(name, monkeypatch):
    """the bf16 BACKWARD (the mode bench.py times) against the oracle's gradients: per-tensor cosines no further from 1 than 3x
    what the fp32 HIP pipeline loses when only its weights and images are rounded to bf16 (the yardstick of the forward
    tests).  For newUNetTrans additionally: the bf16-only fusions of the hierarchical model (concatenation read in place,
    up path as phase convolutions, the stem's tail backward with the second gradient folded in) switched OFF must give the
    same gradients as ON up to bf16 rounding of the tensors they no longer write -- a wrong fusion shows up as a cosine far
    from 1 in exactly the tensors behind it."""
    from dahitra_amd.models import losses
    size = 256 if name == "newUNetTrans" else 128
    a, b, lab = O.synthetic_batch(2, size, seed=31)
    sd = O.deterministic_state(name)
    st = O.TrainState(name, sd, lr=0.01)
    O.focal_loss(O.forward(st.sd, name, a, b, training=True), lab).backward()
    ref = {k: v.grad for k, v in st.sd.items() if getattr(v, "grad", None) is not None}

    def cosines(g):
        out = []
        for k, r in ref.items():
            if r.numel() >= 64 and float(r.norm()) > 0:
                out.append((float(F.cosine_similarity(g[k].double().flatten(), r.double().flatten(), dim=0)), k))
        return sorted(out)
    net = make_net(name, "fp32")
    net.load_state_dict(_bf16_rounded(sd))
    net.train()
    losses.focal_loss(net(a.bfloat16().float().cuda(), b.bfloat16().float().cuda()), lab.cuda()).backward()
    cos_round = cosines({k: p.grad.float().cpu() for k, p in net.named_parameters() if p.grad is not None})
    g_on, y_on, loss_on = _bf16_grads(name, a, b, lab)
    assert set(g_on) == set(ref)
    cos_on = cosines(g_on)
    med = lambda c: c[len(c) // 2][0]
    print("bf16 %s: gradient cosine vs oracle: min %.4f (%s), median %.5f | fp32 pipeline on bf16-rounded inputs: min %.4f (%s), "
          "median %.5f" % (name, cos_on[0][0], cos_on[0][1], med(cos_on), cos_round[0][0], cos_round[0][1], med(cos_round)))
    assert 1.0 - med(cos_on) <= 3.0 * (1.0 - med(cos_round)) + 1e-3
    assert 1.0 - cos_on[0][0] <= 3.0 * (1.0 - cos_round[0][0]) + 2e-2
    if name != "newUNetTrans":
        return
    g_off, y_off, loss_off = _bf16_grads(name, a, b, lab, monkeypatch, UNET_FUSIONS)
    worst = (1.0, "")
    for k, g in g_on.items():
        if g.numel() >= 64 and float(g_off[k].norm()) > 0:
            c = float(F.cosine_similarity(g.double().flatten(), g_off[k].double().flatten(), dim=0))
            worst = min(worst, (c, k))
    l2 = float((y_on - y_off).norm() / y_off.norm())
    print("bf16 newUNetTrans fusions on vs off: logits l2 %.2e, loss %.6f / %.6f, worst gradient cosine %.5f (%s)"
          % (l2, loss_on, loss_off, worst[0], worst[1]))
    assert l2 <= 2e-2 and abs(loss_on - loss_off) <= 1e-2 * abs(loss_off)        # (measured: 5.9e-3, 2.8e-3)
    assert worst[0] >= 0.995, worst


def test_bf16_mode_resnet50_within_the_nets_own_sensitivity():
    """The 50-layer trunk with RANDOM weights and batch-statistics BN is chaotic: rounding only the weights and
    images to bf16 inside the fp32 pipeline already moves the logits by ~0.3 (relative L2; tools/r50_bf16_diag.py).
    So the bf16 pipeline is held to (a) the usual bound in eval mode, where running statistics tame the net, and
    (b) a small multiple of that measured sensitivity in train mode."""
    a, b, lab = O.synthetic_batch(2, 128, seed=5)
    sd = O.deterministic_state(R50)
    sd_r = {k: (v.bfloat16().float() if v.dtype.is_floating_point and v.dim() > 1 else v) for k, v in sd.items()}

    def run(dtype, state, x1, x2, train):
        net = make_net(R50, dtype)
        net.load_state_dict(state)
        net.train(train)
        with torch.no_grad():
            return net(x1.cuda(), x2.cuda()).float().cpu()

    l2 = lambda u, v: float((u - v).norm() / v.norm())
    with torch.no_grad():
        ref_eval = O.forward({k: v.clone() for k, v in sd.items()}, R50, a, b, training=False)
    y_eval = run("bf16", sd, a, b, False)
    flips = float((y_eval.argmax(1) != ref_eval.argmax(1)).float().mean())
    err = float((y_eval - ref_eval).abs().max() / ref_eval.abs().max())
    print("bf16 resnet50 eval: rel err %.3e flips %.4f" % (err, flips))
    assert err < 0.15 and flips < 0.03
    ref = run("fp32", sd, a, b, True)
    sens = l2(run("fp32", sd_r, a.bfloat16().float(), b.bfloat16().float(), True), ref)
    got = l2(run("bf16", sd, a, b, True), ref)
    print("bf16 resnet50 train: l2 %.3f, sensitivity to bf16-rounded weights %.3f" % (got, sens))
    assert sens > 0.05            # the premise: this configuration amplifies bf16-sized perturbations
    assert got <= 3.0 * sens


def test_bf16_train_step_reduces_loss():
    from dahitra_amd.models import losses
    from dahitra_amd.optim import AdamW
    name = "base_transformer_pos_s4"
    a, b, lab = O.synthetic_batch(4, 128, seed=9)
    a, b, lab = a.cuda(), b.cuda(), lab.cuda()
    net = make_net(name, "bf16").train()
    opt = AdamW(net.parameters(), lr=0.002, betas=(0.9, 0.999), weight_decay=0.01)
    ls = []
    for it in range(8):
        y = net(a, b)
        opt.zero_grad()
        loss = losses.focal_loss(y, lab)
        loss.backward()
        opt.step()
        ls.append(float(loss))
    assert all(np.isfinite(ls)) and ls[-1] < 0.7 * ls[0], ls


@pytest.mark.parametrize("name", ["base_transformer_pos_s4", "newUNetTrans"])
def test_hip_graph_step_equals_eager_step(name):
    """GraphedTrainStep (one hipGraphLaunch per step) must reproduce the eager step: same kernels, same
    order, same losses; parameters to 1e-6."""
    from dahitra_amd.graph import GraphedTrainStep
    from dahitra_amd.models import losses
    from dahitra_amd.optim import AdamW
    size = 256 if name == "newUNetTrans" else 64
    a, b, lab = (t.cuda() for t in O.synthetic_batch(2, size, seed=11))
    res = {}
    for mode in ("eager", "graph"):
        net = make_net(name, "bf16").train()
        opt = AdamW(net.parameters(), lr=0.002, capturable=(mode == "graph"))
        ls = []
        if mode == "graph":
            step = GraphedTrainStep(net, opt, a, b, lab)
            for _ in range(3):
                ls.append(float(step(a, b, lab)))
        else:
            for _ in range(3):
                y = net(a, b)
                opt.zero_grad()
                loss = losses.focal_loss(y, lab)
                loss.backward()
                opt.step()
                ls.append(float(loss))
        res[mode] = (ls, net._arena.flat.clone(), net.state_dict()["resnet.bn1.running_var"].clone(),
                     int(net.state_dict()["resnet.bn1.num_batches_tracked"]))
    # same kernels in the same order; the device-side Adam bias correction rounds differently from the host's,
    # and training at this learning rate amplifies that, so later losses track rather than coincide
    assert res["eager"][0][0] == res["graph"][0][0]
    assert np.allclose(res["eager"][0], res["graph"][0], rtol=5e-3), (res["eager"][0], res["graph"][0])
    # (the device-side bias correction works from float-rounded betas: agreement to 1e-6, not bitwise)
    assert float((res["eager"][1] - res["graph"][1]).abs().max()) <= 2e-2 * float(res["eager"][1].abs().max())
    assert torch.allclose(res["eager"][2], res["graph"][2], rtol=1e-2)
    assert res["eager"][3] == res["graph"][3] == 6


@pytest.mark.parametrize("cdtype", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["base_transformer_pos_s4", "newUNetTrans"])
def test_hip_graph_eval_step_equals_the_eager_evaluation_forward(name, cdtype):
    """GraphedEvalStep (models/evaluator.py:156-164 as one hipGraphLaunch per batch: eval-mode weight re-pack, forward, arg-max +
    confusion count): logits and counts equal to the eager no-grad forward bit for bit, for a second batch through the same
    graph as well; and the replay reads the CURRENT parameters (a checkpoint loaded after the capture is what gets scored)"""
    from dahitra_amd import ops
    from dahitra_amd.graph import GraphedEvalStep
    size = 256 if name == "newUNetTrans" else 64
    a, b, lab = (t.cuda() for t in O.synthetic_batch(2, size, seed=21))
    a2, b2, lab2 = (t.cuda() for t in O.synthetic_batch(2, size, seed=22))
    net = make_net(name, cdtype).eval()

    def eager(x, y, l):
        cm = torch.zeros(2, 2, dtype=torch.int64, device="cuda")
        with torch.no_grad():
            lo = net(x, y)
        ops.confusion_matrix(lo.float().contiguous(), l[:, 0].contiguous(), cm)
        return lo.clone(), cm
    lo1, cm1 = eager(a, b, lab)
    lo2, cm2 = eager(a2, b2, lab2)
    conf = torch.zeros(2, 2, dtype=torch.int64, device="cuda")
    step = GraphedEvalStep(net, a, b, lab, confusion=conf)
    assert int(conf.sum()) == 0                                    # the warm-up and the capture left no counts behind
    g1 = step(a, b, lab).clone()
    assert torch.equal(g1, lo1) and torch.equal(conf, cm1)
    g2 = step(a2, b2, lab2).clone()
    assert torch.equal(g2, lo2) and torch.equal(conf, cm1 + cm2)
    # other weights, same graph
    sd = {k: (v * 1.5 if v.dtype.is_floating_point and v.dim() > 1 else v) for k, v in O.deterministic_state(name).items()}
    net.load_state_dict(sd)
    net.eval()
    lo3, _ = eager(a, b, lab)
    assert not torch.equal(lo3, lo1)
    assert torch.equal(step(a, b, lab), lo3)
    net.train()
    with pytest.raises(RuntimeError, match="eval-mode forward"):
        step(a, b, lab)
    # the arena is rebuilt (a parameter replaced): the graph holds the old one's addresses and refuses to replay
    net.eval()
    p = next(net.parameters())
    p.data = p.data.clone()
    net._ensure_arena(p.device)
    with pytest.raises(RuntimeError, match="rebuilt"):
        step(a, b, lab)


@pytest.mark.parametrize("name", ["base_transformer_pos_s4_dd8", "newUNetTrans"])
def test_fused_decoder_layer_matches_unfused_kernels(name):
    """csrc/decoder_fused.hip (one kernel per layer and direction) against the validated chain of separate
    kernels, both in bf16: same logits and same gradients up to bf16 rounding of the intermediates that the
    unfused path stores (and the fused one keeps in fp32 registers)."""
    from dahitra_amd.models import losses
    size = 256 if name == "newUNetTrans" else 128
    a, b, lab = (t.cuda() for t in O.synthetic_batch(2, size, seed=21))
    out = {}
    for mode in ("fused", "unfused", "fp32"):
        net = make_net(name, "fp32" if mode == "fp32" else "bf16").train()
        net._engine.fused_decoder = mode == "fused"
        y = net(a, b)
        losses.focal_loss(y, lab).backward()
        out[mode] = (y.detach().float().cpu(), {k: p.grad.clone().cpu() for k, p in net.named_parameters() if p.grad is not None})
    scale = float(out["fp32"][0].abs().max())
    ef = float((out["fused"][0] - out["fp32"][0]).abs().max()) / scale
    eu = float((out["unfused"][0] - out["fp32"][0]).abs().max()) / scale
    print("%s: logits vs fp32: fused %.3e, unfused %.3e" % (name, ef, eu))
    assert ef < max(1.5 * eu, 0.05)
    # gradients: both bf16 paths against the fp32 (parity-mode) gradients, by cosine similarity per tensor
    cos = torch.nn.functional.cosine_similarity
    worse, low = [], []
    for k, g32 in out["fp32"][1].items():
        if float(g32.norm()) < 1e-6:
            continue
        cf = float(cos(out["fused"][1][k].reshape(1, -1), g32.reshape(1, -1)))
        cu = float(cos(out["unfused"][1][k].reshape(1, -1), g32.reshape(1, -1)))
        if cf < cu - 0.03:
            worse.append((k, cf, cu))
        if cf < 0.9:
            low.append((k, cf, cu))
    print("%s: tensors where fused is worse than unfused by > 0.03: %d, below 0.9: %d" % (name, len(worse), len(low)))
    assert len(worse) <= 3, worse[:8]
    assert len(low) <= 3, low[:8]


def test_eager_step_is_deterministic():
    """no atomics, no races: two runs of the same step give bitwise identical parameters"""
    from dahitra_amd.models import losses
    from dahitra_amd.optim import AdamW
    a, b, lab = (t.cuda() for t in O.synthetic_batch(2, 256, seed=31))
    flats = []
    for _ in range(2):
        net = make_net("newUNetTrans", "bf16").train()
        opt = AdamW(net.parameters(), lr=0.001)
        for _ in range(2):
            y = net(a, b)
            opt.zero_grad()
            losses.focal_loss(y, lab).backward()
            opt.step()
        flats.append(net._arena.flat.clone())
    assert torch.equal(flats[0], flats[1])


def test_evaluator_confusion_matrix_and_checkpoint_interchange(tmp_path):
    """eval path (section 8f-1/2): a checkpoint written in the reference's format (trainer.py:150-158, with a
    DataParallel 'module.' prefix) loads; the on-device confusion matrix equals numpy's on the oracle's masks."""
    from dahitra_amd.models.evaluator import CDEvaluator, cm2score
    name = "base_transformer_pos_s4"
    sd = O.deterministic_state(name)
    torch.save({"epoch_id": 3, "best_val_acc": 0.5, "best_epoch_id": 2,
                "model_G_state_dict": {"module." + k: v for k, v in sd.items()}}, tmp_path / "best_ckpt.pt")
    batches = []
    for seed in (1, 2):
        a, b, lab = O.synthetic_batch(2, 64, seed=seed)
        batches.append({"A": a, "B": b, "L": lab})
    args = types.SimpleNamespace(net_G=name, compute_dtype="fp32", gpu_ids=[0], n_class=2, checkpoint_dir=str(tmp_path))
    ev = CDEvaluator(args, batches)
    with pytest.raises(FileNotFoundError):
        ev.eval_models("missing.pt")
    scores = ev.eval_models("best_ckpt.pt")
    cm = np.zeros((2, 2))
    sd2 = O.deterministic_state(name)
    for bt in batches:
        with torch.no_grad():
            y = O.forward(sd2, name, bt["A"], bt["B"], training=False)
        pred = torch.argmax(y, 1).numpy().ravel()
        gt = bt["L"].numpy().ravel()
        cm += np.bincount(2 * gt + pred, minlength=4).reshape(2, 2)
    got = ev.confusion.cpu().numpy()
    assert got.sum() == cm.sum()
    assert np.abs(got - cm).sum() <= 4            # at most a couple of tie-band pixels may differ
    ref = cm2score(cm)
    assert abs(scores["acc"] - ref["acc"]) < 1e-3 and abs(scores["mf1"] - ref["mf1"]) < 2e-3


def test_missing_library_fails_loudly(monkeypatch):
    from dahitra_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libdahitra_hip.so")
    with pytest.raises(_lib.HipLibraryError):
        _lib.lib()


def test_smoke_entry():
    from dahitra_amd import smoke
    smoke.run(verbose=False)


def test_trainer_step_branches_match_oracle():
    """CDTrainer._backward_G (models/trainer.py:254-262): batch > 1 -> dice constant + focal, batch == 1 -> cross entropy"""
    from dahitra_amd.models.trainer import CDTrainer
    name = "base_transformer_pos_s4"
    args = types.SimpleNamespace(net_G=name, gpu_ids=[0], lr=0.01, batch_size=2, max_epochs=1, n_class=2, lr_policy="linear",
                                 compute_dtype="fp32")
    for bs in (2, 1):
        tr = CDTrainer(args, dataloaders=None)
        tr.net_G.load_state_dict(O.deterministic_state(name))
        tr.net_G.train()
        a, b, lab = O.synthetic_batch(bs, 64, seed=31)
        st = O.TrainState(name, O.deterministic_state(name), lr=0.01)
        logits = O.forward(st.sd, name, a, b, training=True)
        want = (O.dice_constant(logits, lab) + O.focal_loss(logits, lab)) if bs != 1 else O.cross_entropy(logits, lab)
        want.backward()
        loss = tr.train_step({'A': a, 'B': b, 'L': lab})
        assert abs(float(loss) - float(want)) <= 2e-5 * max(1.0, abs(float(want))), (bs, float(loss), float(want))
        k = "classifier.3.bias"
        got = dict(tr.net_G.named_parameters())[k].grad.cpu()
        assert float((got - st.sd[k].grad).abs().max()) <= GRAD_TOL * float(st.sd[k].grad.abs().max())


@pytest.mark.parametrize("name", ["base_transformer_pos_s4", "newUNetTrans", R50])
def test_bn_backward_fused_into_dgrad_equals_two_pass(name, monkeypatch):
    """the gated data-gradient epilogue + bn_bwd_from_partials against the separate reduce / apply passes (fp32 mode)"""
    from dahitra_amd.models import losses
    size = 256 if name == "newUNetTrans" else 64
    a, b, lab = O.synthetic_batch(2, size, seed=41)
    grads = {}
    for off in ("1", "0"):
        monkeypatch.setenv("DAHITRA_BN_FUSION", "0" if off == "1" else "1")
        net = make_net(name).train()
        assert net._engine.fused_bn_bwd == (off == "0")
        losses.focal_loss(net(a.cuda(), b.cuda()), lab.cuda()).backward()
        grads[off] = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
    assert grads["0"].keys() == grads["1"].keys()
    worst = 0.0
    for k, g0 in grads["1"].items():
        s = float(g0.abs().max())
        worst = max(worst, float((grads["0"][k] - g0).abs().max()) / max(s, 1e-20))
    # same arithmetic, different summation order of the per-channel reductions
    assert worst <= 2e-3, worst


@pytest.mark.parametrize("name", ["base_transformer_pos_s4", "newUNetTrans"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_fused_token_encoder_equals_layerwise_kernels(name, dtype, monkeypatch):
    """csrc/encoder_fused.hip (3 launches) against the LayerNorm / linear / attention kernel sequence"""
    from dahitra_amd.models import losses
    size = 256 if name == "newUNetTrans" else 64
    a, b, lab = O.synthetic_batch(2, size, seed=43)
    res = {}
    for off in ("1", "0"):
        monkeypatch.setenv("DAHITRA_NO_FUSED_ENCODER", off)
        net = make_net(name, dtype).train()
        assert net._engine.fused_encoder == (off == "0")
        y = net(a.cuda(), b.cuda())
        losses.focal_loss(y, lab.cuda()).backward()
        res[off] = (y.detach().clone(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})
    y1, g1 = res["1"]
    y0, g0 = res["0"]
    tol = 1e-4 if dtype == "fp32" else 2e-2          # bf16: the pixel side amplifies last-bit token differences
    assert float((y0 - y1).abs().max()) <= tol * float(y1.abs().max())
    for k in g1:
        if k.startswith("transformer") and not k.startswith("transformer_decoder"):
            s = float(g1[k].abs().max())
            assert float((g0[k] - g1[k]).abs().max()) <= (1e-3 if dtype == "fp32" else 5e-2) * s + 1e-9, k


def test_recorded_token_side_launches_equal_the_separate_ones(monkeypatch):
    """the three levels' cross-attention operand preparations (forward, and the four kernels of their backward) and stack
    finalizes issued as one launch per kernel (ops.EncoderBatch -> dh_xprep_batch_*, the held-back
    dh_decoder_stack_bwd_finalize) against every level launching its own: the same workgroups on the same data --
    bit-identical logits and gradients"""
    from dahitra_amd.models import losses
    name = "newUNetTrans"
    a, b, lab = O.synthetic_batch(2, 256, seed=47)
    res = {}
    for on in ("0", "1"):
        monkeypatch.setenv("DAHITRA_XPREP_BATCH", on)
        net = make_net(name, "bf16").train()
        y = net(a.cuda(), b.cuda())
        losses.focal_loss(y, lab.cuda()).backward()
        torch.cuda.synchronize()
        res[on] = (y.detach().clone(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})
    assert torch.equal(res["0"][0], res["1"][0])
    assert res["0"][1].keys() == res["1"][1].keys()
    for k, g in res["0"][1].items():
        assert torch.equal(g, res["1"][1][k]), k
    assert any(float(g.abs().max()) > 0 for k, g in res["1"][1].items() if k.startswith("transformer_decoder"))


@pytest.mark.parametrize("cdtype", PARITY_MODES)
@pytest.mark.parametrize("name", ["base_transformer_pos_s4", "base_transformer_pos_s4_dd8_o5"])
def test_ragged_shapes_match_oracle_fp32(name, cdtype):
    """non-square input whose feature maps are not multiples of the kernel tiles (96x160: 24x40 / 12x20 maps, the
    fused decoder's 128-row blocks do not divide 960 rows -> layer-at-a-time path), odd batch"""
    from dahitra_amd.models import losses
    cfg = O.get_config(name)
    g = torch.Generator().manual_seed(9)
    a = torch.randn(3, 3, 96, 160, generator=g).clamp_(-1, 1)
    b = torch.randn(3, 3, 96, 160, generator=g).clamp_(-1, 1)
    lab = torch.randint(0, cfg["n_class"], (3, 1, 96, 160), generator=g)
    st = O.TrainState(name, O.deterministic_state(name), lr=0.01)
    ref = O.forward(st.sd, name, a, b, training=True)
    O.focal_loss(ref, lab).backward()
    net = make_net(name, cdtype).train()
    y = net(a.cuda(), b.cuda())
    losses.focal_loss(y, lab.cuda()).backward()
    err = float((y.detach().cpu() - ref.detach()).abs().max()) / float(ref.abs().max())
    assert err <= 2e-4, err
    # Max-norm distances of single tensors are dominated by individual tie flips of ReLU / |d1 - d2| (here: one decoder
    # element with |d1 - d2| = 7e-6 whose gradient is 6 % of the maximum flips sign, tools/ragged_diag.py; away from
    # the ties the decoder-output gradient agrees to 6e-3), so the bound per tensor is loose and the distribution tight.
    rels, coss = [], []
    for k, p in net.named_parameters():
        r = st.sd[k].grad
        assert (p.grad is None) == (r is None), k
        if r is not None:
            e, s = float((p.grad.cpu() - r).abs().max()), float(r.abs().max())
            assert e <= 0.2 * s + 1e-7, (k, e, s)
            rels.append(e / max(s, 1e-30))
            if r.numel() >= 64:
                coss.append(float(F.cosine_similarity(p.grad.cpu().double().flatten(), r.double().flatten(), dim=0)))
    print("%s %s ragged: logits %.2e, gradient rel-max median %.2e, p90 %.2e, min cosine %.5f"
          % (name, cdtype, err, float(np.median(rels)), float(np.quantile(rels, 0.9)), min(coss)))
    assert float(np.median(rels)) <= 1e-2, float(np.median(rels))
    assert float(np.quantile(rels, 0.9)) <= 6e-2, float(np.quantile(rels, 0.9))
    assert min(coss) >= 0.995, min(coss)


def test_ragged_shapes_bf16_runs_and_tracks():
    name = "base_transformer_pos_s4"
    g = torch.Generator().manual_seed(9)
    a = torch.randn(3, 3, 96, 160, generator=g).clamp_(-1, 1)
    b = torch.randn(3, 3, 96, 160, generator=g).clamp_(-1, 1)
    with torch.no_grad():
        ref = O.forward(O.deterministic_state(name), name, a, b, training=True)
    net = make_net(name, "bf16").train()
    from dahitra_amd.models import losses
    y = net(a.cuda(), b.cuda())
    losses.focal_loss(y, torch.zeros(3, 1, 96, 160, dtype=torch.long, device="cuda")).backward()
    err = float((y.detach().cpu() - ref).abs().max()) / float(ref.abs().max())
    assert err < 0.15, err
    assert all(torch.isfinite(p.grad).all() for p in net.parameters() if p.grad is not None)


@pytest.mark.parametrize("name", ["base_transformer_pos_s4", "newUNetTrans", R50])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_lazy_batchnorm_activations_equal_materialised(name, dtype, monkeypatch):
    """BatchNorm-apply + ReLU fused into the consumer's load (forward conv and weight gradient) against the path that
    writes the normalised activation: the same numbers enter the same MFMAs"""
    from dahitra_amd.models import losses
    size = 256 if name == "newUNetTrans" else 64
    a, b, lab = O.synthetic_batch(2, size, seed=51)
    res = {}
    for off in ("1", "0"):
        monkeypatch.setenv("DAHITRA_NO_LAZY_BN", off)
        net = make_net(name, dtype).train()
        assert net._engine.lazy_bn == (off == "0")
        y = net(a.cuda(), b.cuda())
        losses.focal_loss(y, lab.cuda()).backward()
        res[off] = (y.detach().clone(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})
    assert torch.equal(res["0"][0], res["1"][0])
    for k, g in res["1"][1].items():
        assert torch.equal(res["0"][1][k], g), k


def test_opt_in_paths_equal_default_paths_bf16(monkeypatch):
    """the measured-neutral path kept behind a switch stays correct: the class-head data gradient gated for the classifier's
    BatchNorm (sums taken in its epilogue), bf16 train step"""
    from dahitra_amd.models import losses
    a, b, lab = O.synthetic_batch(2, 64, seed=71)
    res = {}
    for on in ("0", "1"):
        monkeypatch.setenv("DAHITRA_GATED_HEAD", on)
        net = make_net("base_transformer_pos_s4", "bf16").train()
        assert net._engine.gated_head_dgrad == (on == "1")
        y = net(a.cuda(), b.cuda())
        losses.focal_loss(y, lab.cuda()).backward()
        res[on] = (y.detach().clone(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})
    assert torch.equal(res["0"][0], res["1"][0])                 # forward: same products in the same order
    for k, g in res["0"][1].items():
        h = res["1"][1][k]
        if float(g.abs().max()) < 1e-10:             # a gradient that cancels exactly (last decoder bias in |x1 - x2|)
            assert float(h.abs().max()) < 1e-8, k
            continue
        cos = float((g * h).sum() / (g.norm() * h.norm() + 1e-30))
        assert cos >= 0.9995 and float((g - h).abs().max()) <= 3e-2 * float(g.abs().max()) + 1e-9, (k, cos)


@pytest.mark.parametrize("cdtype", ["bf16", "fp32"])
def test_elementwise_launches_of_the_levels_in_one_job_table_equal_single_launches(cdtype, monkeypatch):
    """newUNetTrans train step with the levels' positional adds / channel concatenations / token differences and their gradients
    recorded into one dh_ew_multi launch per round (default) against DAHITRA_EW_BATCH=0: the same kernels' bodies in the same
    order per tensor -- bit-equal logits and gradients (fp32: only the token differences are table jobs)"""
    from dahitra_amd.models import losses
    a, b, lab = O.synthetic_batch(2, 256, seed=75)
    res = {}
    for off in ("1", "0"):
        monkeypatch.setenv("DAHITRA_EW_BATCH", off)
        net = make_net("newUNetTrans", cdtype).train()
        y = net(a.cuda(), b.cuda())
        losses.focal_loss(y, lab.cuda()).backward()
        res[off] = (y.detach().clone(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})
    assert torch.equal(res["0"][0], res["1"][0])
    for k, g in res["0"][1].items():
        assert torch.equal(res["1"][1][k], g), k


@pytest.mark.parametrize("cdtype", ["bf16", "bf16x3"])
@pytest.mark.parametrize("name", ["base_transformer_pos_s4", "newUNetTrans"])
def test_head_gradient_inside_the_batchnorm_backward_equals_three_kernel_path_bf16(name, cdtype, monkeypatch):
    """default bf16 step against DAHITRA_NO_FUSED_HEAD_BN=1.  s4: the class head's data gradient recomputed by both passes of
    classifier.1's backward with the head's weight / bias gradient from the first (engine.HeadGrad) against head_dgrad3x3 ->
    bn_bwd + conv2d_wgrad + colsum (the same gradient rounded to bf16 in between); newUNetTrans: the head behind a ReLU, data +
    weight + bias gradient in one pass (ops.head_relu_bwd) against head_dgrad3x3(relu_out) + conv2d_wgrad + colsum"""
    from dahitra_amd.models import losses
    a, b, lab = O.synthetic_batch(2, 256 if name == "newUNetTrans" else 64, seed=73)
    res = {}
    for off in ("0", "1"):
        monkeypatch.setenv("DAHITRA_NO_FUSED_HEAD_BN", off)
        net = make_net(name, cdtype).train()
        assert net._engine.fused_head_bn == (off == "0")
        y = net(a.cuda(), b.cuda())
        losses.focal_loss(y, lab.cuda()).backward()
        res[off] = (y.detach().clone(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})
    assert torch.equal(res["0"][0], res["1"][0])
    for k, g in res["0"][1].items():
        h = res["1"][1][k]
        if float(g.abs().max()) < 1e-10:
            assert float(h.abs().max()) < 1e-8, k
            continue
        cos = float((g * h).sum() / (g.norm() * h.norm() + 1e-30))
        bound = 3e-2 if cdtype == "bf16" else 2e-4          # bf16x3: both paths compute in fp32 with split products
        assert cos >= 0.9995 and float((g - h).abs().max()) <= bound * float(g.abs().max()) + 1e-9, (k, cos)


@pytest.mark.parametrize("name", ["base_transformer_pos_s4", "newUNetTrans"])
def test_phase_convolution_paths_equal_reference_paths(name, monkeypatch):
    """conv_pred as 2x2 phase convs and the stride-2 data gradient as output-parity phases (both: pre-summed / re-ordered
    taps, i.e. fp re-association only) against the upsample / zero-insert paths in fp32 mode"""
    from dahitra_amd.models import losses
    size = 256 if name == "newUNetTrans" else 64
    a, b, lab = O.synthetic_batch(2, size, seed=61)
    res = {}
    for off in ("1", "0"):
        monkeypatch.setenv("DAHITRA_NO_PHASE_CONV", off)
        monkeypatch.setenv("DAHITRA_NO_PHASE_S2", off)
        net = make_net(name).train()
        assert net._engine.phase_s2_dgrad == (off == "0")
        y = net(a.cuda(), b.cuda())
        losses.focal_loss(y, lab.cuda()).backward()
        res[off] = (y.detach().clone(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})
    s = float(res["1"][0].abs().max())
    assert float((res["0"][0] - res["1"][0]).abs().max()) <= 1e-5 * s
    for k, g in res["1"][1].items():
        gs = float(g.abs().max())
        assert float((res["0"][1][k] - g).abs().max()) <= 2e-3 * gs + 1e-9, k


@pytest.mark.parametrize("name", ["base_transformer_pos_s4_dd8", R50])
def test_fp8_attention_mode_tracks_bf16(name):
    """attn_dtype='fp8' (BASELINE configs[4]: fp8 MFMA operands in the decoder layers' forward products): logits within a
    small multiple of the bf16 pipeline's own distance to the fp32 oracle; the train step runs and produces finite grads"""
    from dahitra_amd.models import losses
    from dahitra_amd.models.networks import BASE_Transformer, define_G, init_net
    a, b, lab = O.synthetic_batch(2, 128, seed=71)
    sd = O.deterministic_state(name)
    with torch.no_grad():
        ref = O.forward({k: v.clone() for k, v in sd.items()}, name, a, b, training=False)
    out = {}
    for attn in ("bf16", "fp8"):
        if name == R50:
            net = init_net(BASE_Transformer(backbone='resnet50', compute_dtype="bf16", attn_dtype=attn), gpu_ids=[0])
        else:
            net = define_G(types.SimpleNamespace(net_G=name, compute_dtype="bf16", attn_dtype=attn), gpu_ids=[0])
        net.load_state_dict(sd)
        assert net._engine.attn_fp8 == (attn == "fp8")
        net.eval()
        with torch.no_grad():
            out[attn] = net(a.cuda(), b.cuda()).float().cpu()
        if attn == "fp8":
            net.train()
            y = net(a.cuda(), b.cuda())
            losses.focal_loss(y, lab.cuda()).backward()
            assert all(torch.isfinite(p.grad).all() for p in net.parameters() if p.grad is not None)
    l2 = lambda u, v: float((u - v).norm() / v.norm())
    e16, e8, d = l2(out["bf16"], ref), l2(out["fp8"], ref), l2(out["fp8"], out["bf16"])
    print("%s eval logits: bf16 vs oracle %.3e, fp8-attention vs oracle %.3e, fp8 vs bf16 %.3e" % (name, e16, e8, d))
    assert e8 <= 4.0 * e16 + 2e-2
    with pytest.raises(ValueError):
        define_G(types.SimpleNamespace(net_G="base_transformer_pos_s4", compute_dtype="fp32", attn_dtype="fp8"), gpu_ids=[0])


def test_resnet50_trunk_at_1024_matches_reference_golden(golden_dir):
    """BASELINE configs[4] geometry: ResNet-50 trunk (dilated layer3, K-deep 1x1 convolutions up to 1024 channels), 1024x1024
    input, batch 1 -- fp32 logits against the fixture the reference wrote (eval and train mode), masks outside the tie band,
    then the bf16 + fp8-attention configuration runs a train step at this size"""
    from dahitra_amd.models import losses
    from dahitra_amd.models.losses import argmax_mask
    from dahitra_amd.models.networks import BASE_Transformer, init_net
    g = np.load(os.path.join(golden_dir, "fwd1024_%s.npz" % R50))
    bs, size, st = int(g["batch"]), int(g["size"]), int(g["stride"])
    a, b, lab = O.synthetic_batch(bs, size, seed=int(g["seed"]))
    for mode in ("eval", "train"):
        net = make_net(R50)
        net.train(mode == "train")
        with torch.no_grad():
            y = net(a.cuda(), b.cuda())
        scale = float(g["scale_" + mode])
        err = float((y.cpu()[..., ::st, ::st] - torch.from_numpy(g["logits_" + mode])).abs().max()) / scale
        assert abs(float(y.double().sum()) - float(g["sum_" + mode])) <= 5e-4 * float(g["abssum_" + mode])
        mask = argmax_mask(y).cpu().numpy().astype(np.uint8)
        ref_mask = np.unpackbits(g["mask_" + mode])[:mask.size].reshape(mask.shape)
        margin = (y[:, 0] - y[:, 1]).abs().cpu().numpy()
        band = margin <= 1e-3 * scale
        diff = mask != ref_mask
        print("resnet50 1024x1024 %s: logits rel err %.2e, mask flips %d (outside the 1e-3 band: %d), band fraction %.5f"
              % (mode, err, int(diff.sum()), int((diff & ~band).sum()), float(band.mean())))
        assert err <= 5e-4
        assert int((diff & ~band).sum()) == 0
    net = init_net(BASE_Transformer(backbone='resnet50', compute_dtype="bf16", attn_dtype="fp8"), gpu_ids=[0])
    net.load_state_dict(O.deterministic_state(R50))
    net.train()
    y = net(a.cuda(), b.cuda())
    losses.focal_loss(y, lab.cuda()).backward()
    assert torch.isfinite(y).all() and all(torch.isfinite(p.grad).all() for p in net.parameters() if p.grad is not None)
