"""The step of xBD_code/train_unettransformer.py on the GPU: the kernels of csrc/xbd_script_loss.hip against the float64 restatement of
tests/_xbd_unet_loss_cases.py and against the reference's own results (tests/golden/xbd_unet_loss.npz), the script as executed
against the existing combo kernels, and GraphedXbdUnetStep / train_epoch_unet against the eager step.

The measure is the reference's own float32 error: the distance of its float32 CPU results from its float64 ones on the fixture's
two cases, the largest of the two per quantity (tools/make_unet_loss_golden.py prints them, _xbd_unet_loss_cases.yardstick reads
them from the fixture):
    loss 1.49e-05, channel losses 2.55e-04, ce 3.15e-07, Dice meter 9.04e-08 (relative), gradient 7.97e-06 of its maximum.
(The channel figure is the focal term at its clamp: 1 - (1 - 1e-6) is 1.3 % off in float32.)  A kernel result may lie twice as
far from the float64 value: its sums are fp64, and the factor covers the device's expf / logf against the host's.  loss and
gradient take that bound as it stands.  The seven float32 parts take it with one floor: a float32 number cannot be held closer to
a float64 one than the format's spacing, 2^-23 relative, so their yardstick is max(measured, 2^-23) -- it lifts the Dice meter's
9.04e-08 to 1.19e-07 and nothing else.  parts[7] is a count and exact.
MEASURED_KERNEL below is what the kernels measured on the MI355X, for the record; no bound is derived from it.  On the fixture's
own inputs the kernels sit where the reference's float32 sits (loss 1.499e-05 against its 1.488e-05, gradient 7.87e-06 against
7.97e-06): the same float32 expressions, the same error.  The inputs of the other shapes are the fixture's pixels, resampled
(_xbd_unet_loss_cases.make_case says why: on fresh randn * 3 logits at 2 x 5 x 32 x 36 the gradient measured 5.9e-05)."""
import functools
import math
import os
import random
import socket
import sys

import numpy as np
import pytest
import torch

import _xbd_script_loss_checks as K
import _xbd_unet_loss_cases as C
import cdnet_ref as O

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23

# the kernels' largest distance from float64 over test_kernel_matches_the_restatement's shapes and the fixture's cases, as measured
MEASURED_KERNEL = {"loss": 1.50e-05, "channel": 2.60e-04, "ce": 2.15e-08, "dice": 7.89e-08, "grad": 7.87e-06}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "xbd_unet_loss.npz"))


@pytest.fixture(scope="module")
def bounds(golden):
    return K.bounds(C.yardstick(golden))


def kernel(logits, msk, lbl, labels, upstream=1.0):
    """xbd.unet_loss and its backward on the device -> (loss, parts [8], gradient) on the host"""
    from dahitra_amd.models import xbd
    lg = torch.as_tensor(logits).cuda().requires_grad_(True)
    loss, parts = xbd.unet_loss(lg, torch.as_tensor(msk).cuda(), None if lbl is None else torch.as_tensor(lbl).cuda(), labels,
                                want_parts=True)
    (loss * upstream).backward()
    return float(loss), parts.cpu().numpy().astype(np.float64), lg.grad.cpu().numpy()


def check(what, got, ref, bounds):
    """five channel losses, cross-entropy, Dice meter and gradient under their bounds; the count of bad labels exactly"""
    K.check(what, got, ref, bounds, 5, True, ref["parts"][7])


def shapes():
    from dahitra_amd import ops
    P = ops.XBD_UNET_LOSS_PASS
    return C.SHAPES + ((1, 1, P + 3, False),          # one pixel per lane: 3 pixels past one grid pass
                       (1, 4, P + 1, False))          # four pixels per lane: one quad past one grid pass


@functools.lru_cache(None)
def shape_case(k):
    """inputs (the fixture's pixels, resampled: _xbd_unet_loss_cases.make_case says why) and float64 reference of shape k, made once"""
    B, H, W, sat = shapes()[k]
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "xbd_unet_loss.npz"))
    logits, msk, lbl = C.make_case(golden, B, H, W, sat, seed=40 + k)
    return logits, msk, lbl, C.restate(logits.numpy(), msk.numpy(), lbl.numpy())


@pytest.mark.parametrize("k", range(6))
def test_kernel_matches_the_restatement(k, bounds):
    """loss, all eight parts and the gradient in both label modes; 'damage' is bit-equal to 'lbl_msk' with the label built on the
    host.  Shapes: _xbd_unet_loss_cases.SHAPES and two that exceed one grid pass, one per launch form."""
    from dahitra_amd import _lib, ops
    assert ops.XBD_UNET_LOSS_PASS == _lib.lib().dh_xbd_unet_loss_grid_pass()
    B, H, W, _ = shapes()[k]
    assert k < 4 or B * H * W > ops.XBD_UNET_LOSS_PASS * (4 if H * W % 4 == 0 else 1)
    logits, msk, lbl, ref = shape_case(k)
    host = kernel(logits, msk, lbl, "lbl_msk")
    check("%dx5x%dx%d lbl_msk" % (B, H, W), host, ref, bounds)
    derived = kernel(logits, msk, None, "damage")
    assert derived[0] == host[0] and np.array_equal(derived[1], host[1]) and np.array_equal(derived[2], host[2])
    assert np.array_equal(kernel(logits, msk, torch.full_like(lbl, 7), "damage")[2], host[2])          # lbl is not read


def test_kernel_matches_the_reference_fixture(golden, bounds):
    for name, modes in (("zero", ("lbl_msk",)), ("damage", ("lbl_msk", "damage"))):
        ref = {"loss": float(golden[name + "_loss64"]), "grad": golden[name + "_grad64"],
               "parts": np.concatenate([golden[name + "_channel64"], [golden[name + "_ce64"]], [golden[name + "_dice64"]], [0.0]])}
        for labels in modes:
            got = kernel(golden[name + "_logits"], golden[name + "_msk"], golden[name + "_lbl"], labels)
            check("fixture %s, labels=%s" % (name, labels), got, ref, bounds)


@pytest.fixture(scope="module")
def executed():
    """the script as executed: zero labels.  (kernel result, xbd_loss with the script's channel weights on the float masks)"""
    from dahitra_amd.models import xbd
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(2, 5, 48, 40, generator=g) * 3
    logits[0, 1, :4] = 25.0
    logits[1, 2, :4] = -25.0
    msk = O.xbd_masks(torch.randint(0, 5, (2, 1, 48, 40), generator=g)).to(torch.uint8)
    zero = torch.zeros(2, 48, 40, dtype=torch.uint8)
    got = kernel(logits, msk, zero, "lbl_msk")
    lg = logits.cuda().requires_grad_(True)
    combo = xbd.xbd_loss(lg, msk.cuda().float(), channel_weights=xbd.UNET_CHANNEL_WEIGHTS)
    combo.backward()
    return logits, msk, got, float(combo), lg.grad.cpu().numpy()


def test_script_as_executed_has_a_constant_cross_entropy(executed):
    _, msk, (loss, parts, grad), combo, combo_grad = executed
    assert abs(parts[5] - C.LN5) <= 2 * ULP * C.LN5                     # one logf and the conversion of the mean
    err = float(np.abs(grad - combo_grad).max())
    assert err <= 1e-5 * float(np.abs(combo_grad).max()) + 1e-10, err
    want = combo + 8 * C.LN5
    assert abs(loss - want) <= 2e-6 * abs(want), (loss, want)
    T, N = float(msk[:, 0].sum()), msk[:, 0].numel()
    meter = (T + 1e-6) / (0.5 * N + T + 1e-6)                           # sigmoid(0) everywhere
    assert abs(parts[6] - meter) <= 2 * ULP * meter and parts[7] == 0


def test_a_label_above_4_is_counted_and_gets_the_combo_gradient_only(bounds):
    logits, msk, lbl, _ = shape_case(0)
    zero_grad = kernel(logits, msk, torch.zeros_like(lbl), "lbl_msk")[2]
    lbl = lbl.clone()
    lbl[1, 7, 9] = 255
    loss, parts, grad = kernel(logits, msk, lbl, "lbl_msk")
    assert parts[7] == 1 and math.isfinite(loss) and np.isfinite(parts).all() and np.isfinite(grad).all()
    assert np.array_equal(grad[1, :, 7, 9], zero_grad[1, :, 7, 9])      # the zero-label gradient is the combo gradient alone
    building = (lbl.numpy() > 0) & (lbl.numpy() <= 4)
    assert (np.abs(grad - zero_grad).max(1)[building] > 0).mean() > 0.9       # the other building pixels have a cross-entropy gradient
    check("one label byte 255", (loss, parts, grad), C.restate(logits.numpy(), msk.numpy(), lbl.numpy()), bounds)


def test_two_calls_are_bit_equal():
    logits, msk, lbl, _ = shape_case(3)
    a, b = kernel(logits, msk, lbl, "lbl_msk"), kernel(logits, msk, lbl, "lbl_msk")
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    logits, msk, lbl, _ = shape_case(0)
    a, b = kernel(logits, msk, None, "damage"), kernel(logits, msk, None, "damage")
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_upstream_gradient_scales_the_gradient(bounds):
    logits, msk, lbl, _ = shape_case(0)
    one, scaled = kernel(logits, msk, lbl, "lbl_msk"), kernel(logits, msk, lbl, "lbl_msk", upstream=1.7)
    assert scaled[0] == one[0]
    assert float(np.abs(scaled[2] / 1.7 - one[2]).max()) <= 1e-6 * float(np.abs(one[2]).max())
    ref = C.restate(logits.numpy(), msk.numpy(), lbl.numpy(), upstream=1.7)
    check("upstream 1.7", scaled, ref, bounds)


def test_wrappers_refuse_on_the_device_what_the_kernel_cannot_read():
    from dahitra_amd import ops
    from dahitra_amd.models import xbd
    logits, msk, lbl = (t.cuda() for t in shape_case(2)[:3])
    w = xbd.unet_weights_dev(logits.device)
    with pytest.raises(ValueError, match="not contiguous"):
        ops.xbd_unet_loss_fwd(logits.permute(0, 1, 3, 2), msk.permute(0, 1, 3, 2), lbl.permute(0, 2, 1), "lbl_msk", w)
    with pytest.raises(ValueError, match="msk"):
        xbd.unet_loss(logits, msk.float(), lbl)
    with pytest.raises(ValueError, match="lbl_msk"):
        xbd.unet_loss(logits, msk, None)
    with pytest.raises(ValueError, match="weights_dev"):
        ops.xbd_unet_loss_fwd(logits, msk, lbl, "lbl_msk", w.cpu())


# ---- the step ---------------------------------------------------------------------------------------------------------------
NAME = "xbd_unet_transformer_nodecpos"


def make(dtype="fp32"):
    from dahitra_amd.models.xbd import BASE_Transformer_UNet
    net = BASE_Transformer_UNet(input_nc=3, output_nc=5, token_len=4, resnet_stages_num=4, with_pos='learned', with_decoder_pos=None,
                                enc_depth=1, dec_depth=8, compute_dtype=dtype).cuda()
    net.load_state_dict(O.deterministic_state(NAME))
    return net


def batch_256():
    a, b, lab = O.synthetic_batch(2, 256, seed=11, n_class=5)
    return torch.cat([a, b], 1).cuda(), O.xbd_masks(lab).to(torch.uint8).cuda()


def test_hip_graph_unet_step_equals_eager_step():
    """three steps with damage labels (the cross-entropy term has a gradient) and a MultiStepLR whose milestone follows the first
    step, at the bounds of test_hip_graph_xbd_step_equals_eager_step"""
    from dahitra_amd.graph import GraphedXbdUnetStep
    from dahitra_amd.models import xbd
    x6, msk = batch_256()
    eager = make().train()
    opt_e = xbd.AdamW(eager.parameters(), lr=1e-4, weight_decay=1e-6)
    sch_e = torch.optim.lr_scheduler.MultiStepLR(opt_e, milestones=[1], gamma=0.6)
    graphed = make().train()
    opt_g = xbd.AdamW(graphed.parameters(), lr=1e-4, weight_decay=1e-6, capturable=True)
    sch_g = torch.optim.lr_scheduler.MultiStepLR(opt_g, milestones=[1], gamma=0.6)
    step = GraphedXbdUnetStep(graphed, opt_g, x6, msk, None, labels='damage')
    assert step.lab.dtype == torch.uint8 and step.lbl is None
    for it in range(3):
        eager.zero_grad()
        le, pe = xbd.unet_loss(eager(x6), msk, None, 'damage', want_parts=True)
        le.backward()
        opt_e.step()
        sch_e.step()
        lg = step(x6, msk)
        sch_g.step()
        assert abs(float(le) - float(lg)) <= 1e-5 * abs(float(le)), (it, float(le), float(lg))
        pe, pg = pe.cpu().numpy(), step.parts.cpu().numpy()
        assert pg.shape == (8,) and pg[7] == pe[7] == 0
        assert np.all(np.abs(pe[:7] - pg[:7]) <= 1e-5 * np.abs(pe[:7])), (it, pe, pg)
    assert opt_e.param_groups[0]["lr"] == opt_g.param_groups[0]["lr"] == pytest.approx(0.6e-4)
    se, sg = eager.state_dict(), graphed.state_dict()
    for k in se:
        if se[k].dtype.is_floating_point:
            assert float((se[k] - sg[k]).abs().max()) <= 1e-6 + 1e-5 * float(se[k].abs().max()), k
    assert opt_g.step_count(graphed) == 3


def test_bf16_unet_loss_trains():
    from dahitra_amd.models import xbd
    x6, msk = batch_256()
    net = make("bf16").train()
    opt = xbd.AdamW(net.parameters(), lr=1e-3, weight_decay=1e-6)
    hist = []
    for _ in range(6):
        net.zero_grad()
        loss = xbd.unet_loss(net(x6), msk, None, 'damage')
        loss.backward()
        opt.step()                                                     # no clip: the script's is commented out
        hist.append(float(loss))
    assert hist[-1] < hist[0], hist


def test_train_epoch_unet_meters_are_the_means_of_the_steps(capsys):
    """two batches of a synthetic pipeline (unet_batches, crop 64): the epoch's meters, from its one read, against an eager twin
    whose values are read step by step"""
    from dahitra_amd.datasets.xbd_pipeline import GpuXbdPipeline
    from dahitra_amd.models import xbd
    g = torch.Generator().manual_seed(7)
    u8 = lambda *shape, hi=256: torch.randint(0, hi, shape, dtype=torch.uint8, generator=g).cuda()
    label = u8(4, 16, 16, hi=5).repeat_interleave(8, 1).repeat_interleave(8, 2)          # 8 x 8 blocks of the classes 0 .. 4
    pipe = GpuXbdPipeline(u8(4, 128, 128, 3), u8(4, 128, 128, 3), (label > 0).to(torch.uint8) * 255, label)
    batches = list(pipe.unet_batches(2, 64, random.Random(0)))
    assert len(batches) == 2 and batches[0]['msk'].dtype == torch.uint8
    net = make().train()
    opt = xbd.AdamW(net.parameters(), lr=1e-4, weight_decay=1e-6, capturable=True)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[1], gamma=0.6)
    capsys.readouterr()
    meters = xbd.train_epoch_unet(0, net, opt, sch, batches, labels='damage')
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("epoch: ")]
    twin = make().train()
    opt_t = xbd.AdamW(twin.parameters(), lr=1e-4, weight_decay=1e-6)
    rows = []
    for b in batches:
        twin.zero_grad()
        loss, parts = xbd.unet_loss(twin(b['img']), b['msk'], b['lbl_msk'], 'damage', want_parts=True)
        loss.backward()
        opt_t.step()
        rows.append([loss.item()] + [p.item() for p in parts])
    rows = np.asarray(rows, dtype=np.float64)
    assert meters['steps'] == 2 and meters['samples'] == 4 and meters['lr'] == pytest.approx(0.6e-4)
    for key, col in (('loss', 0), ('loss2', 3), ('loss3', 4), ('ce', 6), ('dice', 7)):
        want = rows[:, col].mean()
        assert abs(meters[key] - want) <= 1e-5 * abs(want), (key, meters[key], want)
    assert line == ["epoch: 0; lr 0.0000600; Loss {:.4f}; loss2 {:.4f}; Dice {:.4f}".format(meters['loss'], meters['loss2'],
                                                                                            meters['dice'])]
    assert len(net.__dict__['_xbd_unet_steps']) == 1                   # the recorded step is kept on the model


# ---- two data-parallel ranks and the held inputs, at the smallest shape this file runs the net at ---------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def batch_64(n, seed=13):
    """n pairs of 64 x 64 on the host: imgs [n, 6, 64, 64], the loader's uint8 msks [n, 5, 64, 64] and a label plane 0 .. 4"""
    a, b, lab = O.synthetic_batch(n, 64, seed=seed, n_class=5)
    return torch.cat([a, b], 1), O.xbd_masks(lab).to(torch.uint8), lab[:, 0].to(torch.uint8)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _unet_rank(rank, world, port, overlap, steps, out):
    """one gloo rank on cuda:0 (as tests/test_parallel_gpu.py::_worker): DAHITRA_OVERLAP=0 is one graph + one all-reduce + the
    update, DAHITRA_OVERLAP=1 two graphs around the all-reduce of the arena tail"""
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      DAHITRA_OVERLAP=overlap)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import torch.distributed as dist
    from dahitra_amd import parallel
    from dahitra_amd.graph import GraphedXbdUnetStep
    from dahitra_amd.models import xbd
    parallel.init_from_env("gloo")
    torch.cuda.set_device(0)
    net = make().train() if rank == 0 else xbd.BASE_Transformer_UNet(with_decoder_pos=None, compute_dtype="fp32").cuda().train()
    net._ensure_arena(torch.device("cuda", 0))
    parallel.broadcast_params_(net)                          # rank 1 keeps its random init: the broadcast must fix it
    x6, msk, _ = batch_64(2 * world)
    lo, hi = parallel.shard_batch(2 * world, rank, world)
    x6, msk = x6[lo:hi].cuda(), msk[lo:hi].cuda()
    opt = xbd.AdamW(net.parameters(), lr=1e-3, weight_decay=1e-6, capturable=True)
    step = GraphedXbdUnetStep(net, opt, x6, msk, None, labels='damage')
    assert step.exchange
    if overlap == "0":
        assert step.split_off is None
    else:
        assert step.split_off is not None and 0 < step.split_off < net._arena.n_active
    for _ in range(steps):
        step(x6, msk)
    torch.cuda.synchronize()
    torch.save({k: v.cpu() for k, v in net.state_dict().items()}, out % rank)
    dist.barrier()
    dist.destroy_process_group()


@functools.lru_cache(None)
def two_replica_emulation(steps=2):
    """the single-process emulation of two ranks, made once for both forms: per-shard gradients of two replicas, the sum of the
    two arenas scaled by 1 / 2, NO clip, xbd.AdamW.step() on every replica -> replica 0's state on the host"""
    from dahitra_amd import ops
    from dahitra_amd.models import xbd
    x6, msk, _ = batch_64(4)
    nets = [make().train() for _ in range(2)]
    opts = [xbd.AdamW(n.parameters(), lr=1e-3, weight_decay=1e-6) for n in nets]
    for _ in range(steps):
        for r, net in enumerate(nets):
            net.zero_grad()
            sl = slice(2 * r, 2 * r + 2)
            xbd.unet_loss(net(x6[sl].cuda()), msk[sl].cuda(), None, 'damage').backward()
        total = nets[0].flat_params()[1] + nets[1].flat_params()[1]
        for net, opt in zip(nets, opts):
            g = net.flat_params()[1]
            g.copy_(total)
            ops.scale_into(g, torch.tensor([0.5], device=g.device), g)
            opt.step()
    return {k: v.cpu() for k, v in nets[0].state_dict().items()}


@pytest.mark.parametrize("overlap", ["0", "1"])
def test_two_ranks_of_the_unet_step_match_the_single_process_emulation(tmp_path, overlap):
    """GraphedXbdUnetStep(labels='damage') on two gloo ranks, two steps, in the serial and in the overlapped form: both ranks end
    with equal parameters, within 2e-5 of the emulation (the bound tests/test_parallel_gpu.py holds the graphed xBD step to: the
    replay uses the device-side Adam bias corrections, the emulation the host-side ones)"""
    import torch.multiprocessing as mp
    out = str(tmp_path / "rank%d.pt")
    mp.start_processes(_unet_rank, args=(2, _free_port(), overlap, 2, out), nprocs=2, join=True, start_method="spawn")
    sd0, sd1 = torch.load(out % 0), torch.load(out % 1)
    ref = two_replica_emulation()
    worst = 0.0
    for k, v in sd0.items():
        if not v.dtype.is_floating_point or "running_" in k or "num_batches" in k:
            continue                                   # BatchNorm buffers are per replica
        assert torch.equal(v, sd1[k]), k               # same reduced gradient, same update on both ranks
        worst = max(worst, float((v - ref[k]).abs().max()))
    print("two ranks, DAHITRA_OVERLAP=%s: worst distance from the emulation %.3e" % (overlap, worst))
    assert worst <= 2e-5, worst


@pytest.mark.parametrize("labels", ["damage", "lbl_msk"])
def test_a_replay_on_the_held_inputs_equals_a_replay_given_them(labels):
    """two steps recorded on nets in the same state: one is handed (imgs, msks, lbl_msk) at every call, the other replays on what
    it holds.  Three replays, at the 1e-5 of graph against eager.  An lbl_msk handed to a 'damage' step is ignored."""
    from dahitra_amd.graph import GraphedXbdUnetStep
    from dahitra_amd.models import xbd
    x6, msk, lbl = (t.cuda() for t in batch_64(2))
    steps = []
    for _ in range(2):
        net = make().train()
        opt = xbd.AdamW(net.parameters(), lr=1e-4, weight_decay=1e-6, capturable=True)
        steps.append(GraphedXbdUnetStep(net, opt, x6, msk, lbl, labels=labels))
    given, held = steps
    worst = 0.0
    for it in range(3):
        lg, lh = float(given(x6.clone(), msk.clone(), lbl.clone())), float(held())
        pg, ph = given.parts.cpu().numpy(), held.parts.cpu().numpy()
        worst = max(worst, abs(lg - lh) / abs(lh), float(np.max(np.abs(pg[:7] - ph[:7]) / np.abs(ph[:7]))))
        assert abs(lg - lh) <= 1e-5 * abs(lh), (it, lg, lh)
        assert pg[7] == ph[7] == 0 and np.all(np.abs(pg[:7] - ph[:7]) <= 1e-5 * np.abs(ph[:7])), (it, pg, ph)
    print("held inputs, labels=%s: worst relative difference %.3e" % (labels, worst))
    for s in steps:
        assert (s.lbl is None) if labels == 'damage' else (s.lbl.dtype == torch.uint8 and torch.equal(s.lbl, lbl))
