"""Residual blocks with a downsample without their two single-reader tensors (engine.Engine.block_copies):

* the shortcut's BatchNorm output is formed by the bn_apply of bn2 / bn3 while it loads its residual (ops.BnResidual ->
  dh_bn_apply_res_affine) instead of being written by a launch of its own and read back;
* the shortcut's BatchNorm backward reads the block's output gradient with bn2's ReLU mask bytes (the mask-bytes form of
  ops.bn_bwd) instead of the masked copy `dres` that bn2's backward used to write for it.

Both are exact selections of the same roundings, so every comparison here is torch.equal: against the two-step forms at the
kernel level, and against DAHITRA_BLOCK_COPIES=1 (both tensors written, as before) for whole train steps."""
import ctypes
import types

import pytest
import torch

import cdnet_ref as O

pytestmark = pytest.mark.gpu

R50 = "base_transformer_pos_s4_resnet50"


@pytest.fixture(scope="module")
def ops():
    from dahitra_amd import ops as o
    return o


def rnd(shape, dtype, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(*shape, generator=g, device="cuda") * scale).to(dtype).contiguous()


def make_net(name, dtype):
    from dahitra_amd.models.networks import BASE_Transformer, define_G, init_net
    if name == R50:
        net = init_net(BASE_Transformer(input_nc=3, output_nc=2, token_len=4, resnet_stages_num=4, with_pos='learned',
                                        backbone='resnet50', compute_dtype=dtype), gpu_ids=[0])
    else:
        net = define_G(types.SimpleNamespace(net_G=name, compute_dtype=dtype), gpu_ids=[0])
    net.load_state_dict(O.deterministic_state(name))
    return net


# ---- bn_apply whose residual is a BatchNorm output that is never written -------------------------------------------------
# pixels per group: with 16-byte pieces the hoisted kernel runs ceil(gvec / 512) workgroups per group and every thread takes
# pieces i and i + stride together (the paired loop) or, past gvec - stride, piece i alone (the tail): gvec = 512 k + r with
# k >= 1 and 0 < r < 512 has threads of both kinds and threads with nothing to do.  C = 96 divides neither 256 * 8 nor
# 256 * 4: the generic kernel (per-piece coefficient loads).
AFFINE_CASES = [(64, 205), (128, 205), (256, 205), (1024, 13), (96, 37)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("C,ppg", AFFINE_CASES)
def test_bn_apply_with_an_affine_residual_equals_the_two_launches(ops, C, ppg, groups, dtype):
    V = 8 if dtype == torch.bfloat16 else 4
    gvec = ppg * C // V
    hoisted = (256 * V) % C == 0
    assert hoisted == (C != 96)
    if hoisted:
        assert gvec > 512 and gvec % 512 != 0       # paired loop and tail both run
    npix = ppg * groups
    y = rnd((npix, C), dtype, 11)
    yds = rnd((npix, C), dtype, 12)
    scale = 1 + 0.2 * rnd((groups, C), torch.float32, 13)
    shift = 0.2 * rnd((groups, C), torch.float32, 14)
    rscale = 1 + 0.3 * rnd((groups, C), torch.float32, 15)
    rshift = 0.3 * rnd((groups, C), torch.float32, 16)
    idt = ops.bn_apply(yds, rscale, rshift, groups)                    # what the shortcut's launch stores
    lazy = ops.BnResidual(yds, rscale, rshift, groups)
    assert torch.equal(lazy.materialize(), idt)
    for act, want_bits in ((ops.ACT_NONE, False), (ops.ACT_RELU, False), (ops.ACT_RELU, True)):
        want = ops.bn_apply(y, scale, shift, groups, act, idt, want_bits=want_bits)
        got = ops.bn_apply(y, scale, shift, groups, act, lazy, want_bits=want_bits)
        if want_bits:
            assert want[1] is not None and got[1] is not None
            assert torch.equal(got[1], want[1]), "mask bytes"
            want, got = want[0], got[0]
        assert torch.equal(got, want), (C, groups, dtype, act)
    if dtype == torch.bfloat16:
        # the residual really is rounded through bf16: the unrounded sum differs somewhere at this size
        unr = (y.float().view(groups, ppg, C) * scale[:, None] + shift[:, None]) + (yds.float().view(groups, ppg, C) * rscale[:, None] + rshift[:, None])
        assert not torch.equal(unr.to(dtype).view(npix, C), ops.bn_apply(y, scale, shift, groups, ops.ACT_NONE, lazy))


def test_bn_apply_affine_residual_refuses_half_an_affine(ops):
    from dahitra_amd import _lib
    x = torch.zeros(8, 64, dtype=torch.bfloat16, device="cuda")
    s = torch.ones(1, 64, device="cuda")
    for rs, rb in ((None, s), (s, None)):
        with pytest.raises(_lib.HipLibraryError, match="bn_apply_res_affine"):
            ops._call("dh_bn_apply_res_affine", ops.dt(x), ops.P(x), ops.P(x), ops.P(rs), ops.P(rb), ops.P(x), ops.P(s), ops.P(s), 8, 64, 1,
                      ops.ACT_NONE, ops.P(None), ops.S())


# ---- the shortcut's BatchNorm backward fed (dout, mask bytes of another layer) ---------------------------------------------
# npix * C / 8 pieces: 2474 * 8 = 19792 and 618 * 32 = 19776, neither a multiple of 512 -- the persistent form's 256 workgroups
# and the two-pass form's 1024 include partial and idle ones
@pytest.mark.parametrize("persist", [False, True], ids=["two_pass", "persistent"])
@pytest.mark.parametrize("C,npix", [(64, 2474), (256, 618)])
def test_bn_backward_fed_the_block_gradient_and_mask_bytes_equals_the_masked_copy(ops, C, npix, persist, monkeypatch):
    G, dtype = 2, torch.bfloat16
    assert (npix * C // 8) % 512 != 0 and npix % G == 0
    yds = rnd((npix, C), dtype, 21)            # the shortcut conv's output: the BatchNorm input of the layer under test
    dout = rnd((npix, C), dtype, 22)           # gradient of the block's output
    g = torch.Generator(device="cuda").manual_seed(23)
    bits = torch.randint(0, 256, (npix * C // 8,), generator=g, device="cuda", dtype=torch.uint8)
    bits[::7] = 0
    bits[3::11] = 255
    mask = ((bits.to(torch.int32).unsqueeze(1) >> torch.arange(8, device="cuda", dtype=torch.int32)) & 1).bool().view(npix, C)
    dres = torch.where(mask, dout, torch.zeros_like(dout))
    mean = 0.1 * rnd((G, C), torch.float32, 24)
    invstd = (1 + 0.1 * rnd((G, C), torch.float32, 25)).abs()
    gamma = 1 + 0.1 * rnd((C,), torch.float32, 26)
    monkeypatch.setattr(ops, "BN_BWD_PERSIST", "force" if persist else False)
    n0 = ops.BN_PERSIST_LAUNCHES
    res = []
    for d, b in ((dres, None), (dout, bits)):
        dg, db = torch.full((C,), 0.5, device="cuda"), torch.full((C,), -0.25, device="cuda")
        dx = ops.bn_bwd(d, None, yds, mean, invstd, gamma, dg, db, G, accumulate=True, bits=b)
        res.append((dx, dg, db))
    assert ops.BN_PERSIST_LAUNCHES - n0 == (2 if persist else 0)
    ops.bn_persist_check(yds.device)
    for name, u, v in zip(("dx", "dgamma", "dbeta"), *res):
        assert torch.equal(u, v), name
    assert float(res[0][0].float().abs().max()) > 0 and float((res[0][1] - 0.5).abs().max()) > 0


# ---- whole train steps: default against DAHITRA_BLOCK_COPIES=1 ------------------------------------------------------------
SIZE = {"newUNetTrans": 256}       # its learned positional embeddings fix the input size; every other net: 64 x 64


def _eager_step(name, dtype, ops):
    from dahitra_amd.models import losses
    a, b, lab = O.synthetic_batch(2, SIZE.get(name, 64), seed=83)
    net = make_net(name, dtype).train()
    c0 = (ops.BN_SHORTCUT_APPLIES, ops.BN_DRES_REQUESTS, ops.BN_APPLY_LAUNCHES)
    y = net(a.cuda(), b.cuda())
    loss = losses.focal_loss(y, lab.cuda())
    loss.backward()
    torch.cuda.synchronize()
    ops.bn_persist_check()
    counts = tuple(n - m for n, m in zip((ops.BN_SHORTCUT_APPLIES, ops.BN_DRES_REQUESTS, ops.BN_APPLY_LAUNCHES), c0))
    grads = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
    bufs = {k: v.clone() for k, v in net.state_dict().items() if "running_" in k}
    return net, loss.detach().clone(), y.detach().clone(), grads, bufs, counts


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["base_transformer_pos_s4", "newUNetTrans", R50])
def test_eager_train_step_without_the_block_copies_is_bit_identical(ops, name, dtype, monkeypatch):
    """one eager train step (batch 2, 64 x 64; newUNetTrans 256 x 256): loss, logits, every gradient and the BatchNorm running statistics.  The ResNet-50
    net runs the Bottleneck path: a 1x1 conv1 behind the shortcut, strided and unstrided shortcuts."""
    res = {}
    for copies in ("1", "0"):
        monkeypatch.setenv("DAHITRA_BLOCK_COPIES", copies)
        res[copies] = _eager_step(name, dtype, ops)
        assert res[copies][0]._engine.block_copies == (copies == "1")
    (_, l1, y1, g1, b1, c1), (_, l0, y0, g0, b0, c0) = res["1"], res["0"]
    assert torch.equal(l0, l1) and torch.equal(y0, y1)
    assert g0.keys() == g1.keys() and b0.keys() == b1.keys()
    for k in g1:
        assert torch.equal(g0[k], g1[k]), k
    for k in b1:
        assert torch.equal(b0[k], b1[k]), k
    assert any(float(g.abs().max()) > 0 for k, g in g1.items() if ".downsample." in k)
    # launches: with the copies every block with a downsample launches a bn_apply for its shortcut and every residual block asks
    # its last BatchNorm backward for dres.  By default no shortcut is applied on its own and no backward is asked for dres whose
    # reader can select by the mask bytes: the shortcut's BatchNorm backward always can, conv1's data gradient where it is a 3x3
    # stride-1 layer (every BasicBlock) -- the Bottleneck's 1x1 conv1 cannot, so its blocks without a downsample keep the copy
    n_ds, n_res, n_apply = c1
    assert n_ds > 0 and n_res > n_ds
    assert c0 == (0, n_res - n_ds if name == R50 else 0, n_apply - n_ds), (c0, c1)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["base_transformer_pos_s4", "newUNetTrans"])
def test_graph_replay_without_the_block_copies_is_bit_identical(name, dtype, monkeypatch):
    """the recorded step (capture + one replay): the block's output gradient has to stay alive and unmodified until the shortcut's
    backward has read it -- loss and every parameter after the optimizer step"""
    from dahitra_amd.graph import GraphedTrainStep
    from dahitra_amd.optim import AdamW
    a, b, lab = (t.cuda() for t in O.synthetic_batch(2, SIZE.get(name, 64), seed=85))
    res = {}
    for copies in ("1", "0"):
        monkeypatch.setenv("DAHITRA_BLOCK_COPIES", copies)
        net = make_net(name, dtype).train()
        assert net._engine.block_copies == (copies == "1")
        step = GraphedTrainStep(net, AdamW(net.parameters(), lr=0.002, capturable=True), a, b, lab, warmup=1)
        losses_ = [step(a, b, lab).detach().clone() for _ in range(2)]
        torch.cuda.synchronize()
        res[copies] = (losses_, net._arena.flat.clone(), {k: v.clone() for k, v in net.state_dict().items() if "running_" in k})
    for u, v in zip(res["0"][0], res["1"][0]):
        assert torch.equal(u, v)
    assert torch.equal(res["0"][1], res["1"][1])
    for k, v in res["1"][2].items():
        assert torch.equal(res["0"][2][k], v), k


# ---- conv1's data gradient with the skip gradient as (dout, mask bytes) ---------------------------------------------------
# families of dh_conv2d_fwd_describe (out[0])
TAP_BF16, TAP_F32, STREAM = 0, 1, (6, 7, 8)


def _res_bits_plan(ops, dtype, N, H, W, C, frag):
    out = (ctypes.c_int * 30)()
    rc = ops._lib.lib().dh_conv2d_fwd_describe(5, int(dtype == torch.bfloat16), N, H, W, C, H, W, C, C, 3, 1, 1, 0, 0, 0, 1, 1, 1, 0,
                                               32 if frag else 0, 256, out)
    ops._lib.check(rc, "dh_conv2d_fwd_describe")
    return list(out)


# The stream kernel takes whole 8x16 tiles only (its plan leaves ragged shapes to the tap kernel), so "a partial last tile" exists
# on the tap kernel alone: every width runs one stream shape -- under dh_conv_wreg_mode(1), at 2.5 tiles per workgroup so that the
# epilogue inside the stream loop AND the one after it run (256 CUs: 512 / 128 / 64 workgroups per channel block) -- and the
# ragged 20 x 20 on the tap kernel; 9 x 13 at 64 channels; fp32 (4 elements per mask byte) on the tap kernel.
MASKED_CASES = [
    pytest.param(torch.bfloat16, 64, 2, 160, 512, True, id="bf16-64-stream"),
    pytest.param(torch.bfloat16, 128, 2, 80, 256, True, id="bf16-128-stream"),
    pytest.param(torch.bfloat16, 256, 2, 80, 128, True, id="bf16-256-stream"),
    pytest.param(torch.bfloat16, 64, 2, 20, 20, False, id="bf16-64-tap-ragged"),
    pytest.param(torch.bfloat16, 128, 2, 20, 20, False, id="bf16-128-tap-ragged"),
    pytest.param(torch.bfloat16, 256, 2, 20, 20, False, id="bf16-256-tap-ragged"),
    pytest.param(torch.bfloat16, 64, 2, 9, 13, False, id="bf16-64-tap-odd"),
    pytest.param(torch.float32, 64, 2, 20, 20, False, id="fp32-64-tap-ragged"),
]


@pytest.mark.parametrize("dtype,C,N,H,W,stream", MASKED_CASES)
def test_data_gradient_with_a_masked_residual_equals_the_masked_copy(ops, dtype, C, N, H, W, stream):
    V = 8 if dtype == torch.bfloat16 else 4
    L = ops._lib.lib()
    w = 0.05 * torch.randn(C, C, 3, 3, generator=torch.Generator().manual_seed(31))
    dy = rnd((N, H, W, C), dtype, 32)
    res = rnd((N, H, W, C), dtype, 33)
    g = torch.Generator(device="cuda").manual_seed(34)
    bits = torch.randint(0, 256, (N * H * W * C // V,), generator=g, device="cuda", dtype=torch.uint8)
    if V == 4:
        bits &= 15
    bits[::5] = 0
    bits[2::9] = 255 if V == 8 else 15
    mask = ((bits.to(torch.int32).unsqueeze(1) >> torch.arange(V, device="cuda", dtype=torch.int32)) & 1).bool().view(N, H, W, C)
    dres = torch.where(mask, res, torch.zeros_like(res))
    _, wd = ops.pack_weight(w.cuda(), dtype, dgrad_inner=C)
    wf = None
    if stream:
        packs = ops.PackPlan(torch.device("cuda"))
        _, wf = packs.add(w.cuda(), dtype, want_dgrad=True, dgrad_inner=C, frag=True)
        packs.run()
    prev = L.dh_conv_wreg_mode(1 if stream else -1)
    try:
        plan = _res_bits_plan(ops, dtype, N, H, W, C, stream)
        assert ops.conv3x3_res_bits_supported((N, H, W, C), C, wd, dtype, stream)
        got = ops.conv2d(dy, wd, C, 3, 1, 1, residual=res, res_bits=bits, w_frag=wf)
        want = ops.conv2d(dy, wd, C, 3, 1, 1, residual=dres, w_frag=wf)
        plain = ops.conv2d(dy, wd, C, 3, 1, 1, residual=res, w_frag=wf)
    finally:
        L.dh_conv_wreg_mode(prev)
    if stream:
        assert plan[0] == STREAM[(64, 128, 256).index(C)] and plan[18] == 1 and plan[19] == 0, plan       # RES, no ReLU
        tiles = N * (H // 8) * (W // 16)
        assert H % 8 == 0 and W % 16 == 0 and plan[20] < tiles < 3 * plan[20], (plan[20], tiles)           # 1 < tiles per workgroup < 3
    else:
        assert plan[0] == (TAP_BF16 if dtype == torch.bfloat16 else TAP_F32) and plan[7] == 1, plan       # compact epilogue
        assert H % (4 * plan[28]) != 0 and W % 16 != 0                                                     # ragged in both directions
    assert torch.equal(got, want), float((got.float() - want.float()).abs().max())
    assert not torch.equal(got, plain)          # the mask does something


def test_masked_residual_is_refused_where_no_kernel_applies_it(ops):
    """the 32 -> 32 stream form has no mask path and the shape is not handed to a slower kernel instead: unsupported, and conv2d
    raises rather than return an unmasked sum"""
    dtype, N, H, W, C = torch.bfloat16, 32, 256, 256, 32
    L = ops._lib.lib()
    assert L.dh_conv3x3_res_bits_supported(1, N, H, W, C, C, C, 0) == 0
    assert L.dh_conv3x3_res_bits_supported(1, 2, 20, 20, 64, 64, 64, 0) == 1
    x = torch.zeros(1, 16, 16, C, dtype=dtype, device="cuda")
    wd = torch.zeros(9, C, C, dtype=dtype, device="cuda")
    bits = torch.zeros(x.numel() // 8, dtype=torch.uint8, device="cuda")
    with pytest.raises(AssertionError):
        ops.conv2d(x, wd[:1], C, 1, 1, 0, residual=x, res_bits=bits)        # a 1x1 layer: not expressible at all
