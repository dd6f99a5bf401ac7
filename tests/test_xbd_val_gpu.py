"""The xBD validation score on the MI355X: dh_xbd_val_count (csrc/xbd_eval.hip) against the numpy restatement of the reference's
validate() (tests/_xbd_val_cases.py, xBD_code/train.py:258-288), then models/xbd.validate / evaluate_val and
graph.GraphedXbdEvalStep on the model.  The kernel comparison is exact: the synthetic logits are built so that no last bit of a
sigmoid can decide a pixel, and everything after the sigmoid is integer arithmetic."""
import math
import os

import numpy as np
import pytest
import torch

import _xbd_val_cases as V
import cdnet_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAME = "xbd_unet_transformer_nodecpos"
SENTINEL = -7
PREFILL = np.arange(12, dtype=np.int64).reshape(4, 3) * 1000 + 17


def run_kernel(x, msk_plane, lbl, select, thr=V.THR):
    """ops.xbd_val_count on device tensors; image_counts starts at a sentinel, class_counts at known values"""
    from dahitra_amd import ops
    ic = torch.full((x.shape[0], 3), SENTINEL, dtype=torch.int64, device=DEV)
    cc = torch.from_numpy(PREFILL.copy()).to(DEV)
    ops.xbd_val_count(x, msk_plane, lbl, ic, cc, thr=thr, select=select)
    torch.cuda.synchronize()
    return ic.cpu().numpy(), cc.cpu().numpy()


# B=3 37x37: HW odd, every plane aligned differently, less than one workgroup of vector work; B=2 40x40; B=1 1024x1024: the
# reference's own size, two passes of the capped grid
@pytest.mark.parametrize("B,S", [(3, 37), (2, 40), (1, 1024)])
def test_counts_equal_the_restatement_on_synthetic_logits(B, S):
    x, msk, lbl, planted = V.synthetic(B, S, seed=B * 100 + S)
    V.check_synthetic(x, msk, lbl, planted)
    dx, dmsk, dlbl = torch.from_numpy(x).to(DEV), torch.from_numpy(msk).to(DEV), torch.from_numpy(lbl).to(DEV)
    strided = dmsk[:, 0]
    assert B == 1 or not strided.is_contiguous()
    for select in ("reference", "building"):
        want_ic, want_cc = V.counts(x, msk[:, 0], lbl, select=select)
        assert want_cc.sum() > 0 and (want_cc[:, 0] > 0).all(), "every class is counted"
        for plane in (strided, strided.contiguous(), dmsk):      # channel 0 in place, a copy of it, the whole mask
            ic, cc = run_kernel(dx, plane, dlbl, select)
            assert np.array_equal(ic, want_ic), (select, ic.tolist(), want_ic.tolist())       # written over the sentinel
            assert np.array_equal(cc - PREFILL, want_cc), (select, (cc - PREFILL).tolist(), want_cc.tolist())      # accumulated
    # the reference's long masks, converted once
    ic, cc = run_kernel(dx, dmsk.long(), dlbl.long(), "reference")
    want_ic, want_cc = V.counts(x, msk[:, 0], lbl)
    assert np.array_equal(ic, want_ic) and np.array_equal(cc - PREFILL, want_cc)
    if planted["empty_image"] is not None:
        assert want_ic[planted["empty_image"]].tolist() == [0, 0, 0]
    # an argmax over the logits (instead of the fp32 sigmoids) would count the saturated block differently
    s_wrong = V.sigmoid32(x)
    blk = planted["block"]
    s_wrong[:, 3, blk[0], blk[1]] = 2.0
    assert not np.array_equal(V.counts(x, msk[:, 0], lbl, s=s_wrong)[1], want_cc)


def test_unaligned_base_pointers_take_the_scalar_path():
    """views that start 1 float / 1 byte into their buffers: no plane is aligned to its vector"""
    B, S = 2, 40
    x, msk, lbl, planted = V.synthetic(B, S, seed=7)
    from dahitra_amd import ops
    dx = torch.zeros(x.size + 1, dtype=torch.float32, device=DEV)[1:].view(x.shape)
    dx.copy_(torch.from_numpy(x))
    dm = torch.zeros(B * S * S + 1, dtype=torch.uint8, device=DEV)[1:].view(B, S, S)
    dm.copy_(torch.from_numpy(msk[:, 0]))
    dl = torch.zeros(B * S * S + 1, dtype=torch.uint8, device=DEV)[1:].view(B, S, S)
    dl.copy_(torch.from_numpy(lbl))
    assert dx.data_ptr() % 16 == 4 and dm.data_ptr() % 4 == 1 and dl.data_ptr() % 4 == 1
    for select in ("reference", "building"):
        want_ic, want_cc = V.counts(x, msk[:, 0], lbl, select=select)
        ic, cc = run_kernel(dx, dm, dl, select)
        assert np.array_equal(ic, want_ic) and np.array_equal(cc - PREFILL, want_cc), select


def test_refused_arguments_return_an_error_and_write_nothing():
    from dahitra_amd import _lib, ops
    L = _lib.lib()
    x = torch.zeros(2, 5, 8, 8, device=DEV)
    m = torch.ones(2, 8, 8, dtype=torch.uint8, device=DEV)
    lab = torch.ones(2, 8, 8, dtype=torch.uint8, device=DEV)
    ic = torch.full((2, 3), SENTINEL, dtype=torch.int64, device=DEV)
    cc = torch.from_numpy(PREFILL.copy()).to(DEV)
    P, S = ops.P, ops.S
    good = dict(logits=P(x), msk0=P(m), stride=64, lbl=P(lab), B=2, H=8, W=8, thr=0.3, select=0, ic=P(ic), cc=P(cc))
    order = ("logits", "msk0", "stride", "lbl", "B", "H", "W", "thr", "select", "ic", "cc")
    bad = [dict(H=4, W=16), dict(H=8, W=4), dict(B=0), dict(B=-1), dict(logits=P(None)), dict(msk0=P(None)), dict(lbl=P(None)),
           dict(ic=P(None)), dict(cc=P(None)), dict(thr=0.0), dict(thr=1.0), dict(thr=-0.3), dict(thr=1.5),
           dict(thr=float("nan")), dict(select=2), dict(stride=63)]
    for change in bad:
        args = dict(good, **change)
        rc = L.dh_xbd_val_count(*[args[k] for k in order], S())
        assert rc != 0, change
        assert L.dh_last_error().decode().startswith("xbd_val_count"), (change, L.dh_last_error())
    torch.cuda.synchronize()
    assert (ic == SENTINEL).all() and np.array_equal(cc.cpu().numpy(), PREFILL)
    # H != W is fine for the building selection, and the good call does write
    assert L.dh_xbd_val_count(*[dict(good, H=4, W=16, select=1)[k] for k in order], S()) == 0
    assert L.dh_xbd_val_count(*[good[k] for k in order], S()) == 0
    torch.cuda.synchronize()
    assert ic.cpu().tolist() == [[64, 64, 64]] * 2         # sigmoid(0) = 0.5 > 0.3
    with pytest.raises(ValueError):
        ops.xbd_val_count(x, m, lab, ic, cc, thr=1.0)
    with pytest.raises(ValueError):
        ops.xbd_val_count(x, m[:1], lab, ic, cc)
    with pytest.raises(ValueError):
        ops.xbd_val_count(x, m, lab, ic[:1], cc)


# ---- model level -------------------------------------------------------------------------------------------------------
def blocky(rng, n, h, w, values):
    """constant in 8 x 8 blocks (the recipe of tests/test_xbd_loader_gpu.py)"""
    small = rng.choice(np.asarray(values, dtype=np.uint8), size=(n, -(-h // 8), -(-w // 8)))
    return np.ascontiguousarray(np.kron(small, np.ones((1, 8, 8), dtype=np.uint8))[:, :h, :w])


def sources(n, H, W, seed):
    """pre, post (noise), pre mask (0 / 255), post label (0 .. 4)"""
    rng = np.random.RandomState(seed)
    pre = rng.randint(0, 256, (n, H, W, 3)).astype(np.uint8)
    post = rng.randint(0, 256, (n, H, W, 3)).astype(np.uint8)
    return pre, post, blocky(rng, n, H, W, [0, 255]), blocky(rng, n, H, W, [0, 1, 2, 3, 4])


@pytest.fixture(scope="module")
def model_case():
    """the net, a 4-image validation epoch in batches of 2 at 256 x 256, and the eager epoch's logits and counts (computed once)"""
    from dahitra_amd.datasets.xbd_pipeline import GpuXbdPipeline
    from dahitra_amd.models import xbd
    net = xbd.BASE_Transformer_UNet(input_nc=3, output_nc=5, token_len=4, resnet_stages_num=4, with_pos='learned',
                                    with_decoder_pos=None, enc_depth=1, dec_depth=8).cuda()
    net.load_state_dict(O.deterministic_state(NAME))
    pipe = GpuXbdPipeline(*(torch.from_numpy(a).to(DEV) for a in sources(4, 256, 256, seed=21)))
    batches = list(pipe.batches(2, 256, train=False))
    assert len(batches) == 2 and batches[0]["msk"].dtype == torch.uint8 and tuple(batches[0]["lbl_msk"].shape) == (2, 256, 256)
    seen = []
    hook = net.register_forward_hook(lambda mod, inp, out: seen.append(out.detach().float().cpu().numpy()))
    eager = {sel: xbd.validate(net, batches, select=sel, graph=False, want_counts=True) for sel in ("reference", "building")}
    hook.remove()
    assert len(seen) == 4
    return {"net": net, "batches": batches, "logits": seen[:2], "eager": eager}


def undecided(x):
    """pixels whose count may depend on the last bits of a float32 sigmoid: float64 |s0 - 0.3| <= 1e-6, or the top two damage
    sigmoids within 1e-6 of each other unless both logits are >= 20 (then both are 1.0f and the first wins on both sides)"""
    s = 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
    near_thr = np.abs(s[:, 0] - 0.3) <= 1e-6
    order = np.argsort(s[:, 1:], axis=1)
    top = np.take_along_axis(s[:, 1:], order[:, -1:], axis=1)[:, 0]
    second = np.take_along_axis(s[:, 1:], order[:, -2:-1], axis=1)[:, 0]
    xs = np.sort(x[:, 1:].astype(np.float64), axis=1)
    tie = (top - second <= 1e-6) & ~((xs[:, -1] >= 20) & (xs[:, -2] >= 20))
    return near_thr | tie


def test_eager_validate_agrees_with_the_restatement_on_the_nets_logits(model_case):
    from dahitra_amd.models import xbd
    batches, logits = model_case["batches"], model_case["logits"]
    n_und = sum(int(undecided(x).sum()) for x in logits)
    n_pix = sum(x.shape[0] * x.shape[2] * x.shape[3] for x in logits)
    per_image = max(int(undecided(x[j:j + 1]).sum()) for x in logits for j in range(x.shape[0]))
    print("undecided pixels: %d of %d (largest image: %d of %d)" % (n_und, n_pix, per_image, 256 * 256))
    assert per_image <= 1e-3 * 256 * 256, "condition: at most 0.1 % of an image is undecided"
    for sel in ("reference", "building"):
        sc, parts, ic, cc = model_case["eager"][sel]
        want = [V.counts(x, b["msk"][:, 0].cpu().numpy(), b["lbl_msk"].cpu().numpy(), select=sel) for x, b in zip(logits, batches)]
        want_ic, want_cc = np.concatenate([w[0] for w in want]), sum(w[1] for w in want)
        print(sel, "counts", cc.tolist(), "restatement", want_cc.tolist(), "score", sc)
        assert ic.shape == (4, 3) and cc.shape == (4, 3)
        assert np.abs(ic - want_ic).max() <= n_und and np.abs(cc - want_cc).max() <= n_und, (sel, ic, want_ic, cc, want_cc)
        assert np.array_equal(ic[:, 0], want_ic[:, 0])                     # |gt0| does not depend on the logits
        got = xbd.val_score(ic, cc)[0]
        assert (math.isnan(got) and math.isnan(sc)) or got == sc
        if n_und == 0:
            assert sc == V.score(want_ic, want_cc)[0] or (math.isnan(sc) and math.isnan(V.score(want_ic, want_cc)[0]))
    assert not math.isnan(model_case["eager"]["building"][0])


def test_graphed_step_replays_bit_equal_to_the_eager_path_and_checks_shapes(model_case):
    from dahitra_amd import ops
    from dahitra_amd.graph import GraphedXbdEvalStep
    from dahitra_amd.models import xbd
    net, batches = model_case["net"], model_case["batches"]
    b0, b1 = batches
    cc = torch.from_numpy(PREFILL.copy()).to(DEV)
    step = GraphedXbdEvalStep(net, b0["img"], b0["msk"], b0["lbl_msk"], cc)
    assert np.array_equal(cc.cpu().numpy(), PREFILL), "warm-up and capture leave the counts as they were"
    rows = []
    for b in (b0, b1):                                   # two replays, two different batches
        logits = step(b["img"], b["msk"], b["lbl_msk"])
        rows.append(step.image_counts.clone())
        eic = torch.full((2, 3), SENTINEL, dtype=torch.int64, device=DEV)
        ecc = torch.zeros(4, 3, dtype=torch.int64, device=DEV)
        with torch.no_grad():
            eager_logits = net(b["img"])
        ops.xbd_val_count(eager_logits, b["msk"], b["lbl_msk"], eic, ecc)
        assert logits.shape == eager_logits.shape
        assert torch.equal(rows[-1], eic)
    _, _, ic, ecc_epoch = model_case["eager"]["reference"]
    assert np.array_equal(torch.cat(rows).cpu().numpy(), ic)
    assert np.array_equal(cc.cpu().numpy() - PREFILL, ecc_epoch)
    # validate through the graph: the same integers, hence the same score
    sc, _, gic, gcc = xbd.validate(net, batches, graph=True, want_counts=True)
    assert np.array_equal(gic, ic) and np.array_equal(gcc, ecc_epoch)
    esc = model_case["eager"]["reference"][0]
    assert sc == esc or (math.isnan(sc) and math.isnan(esc))
    # a ragged last batch goes through the eager path inside validate ...
    ragged = {k: (v[:1] if torch.is_tensor(v) else v[:1]) for k, v in b1.items()}
    _, _, ric, _ = xbd.validate(net, [b0, ragged], graph=True, want_counts=True)
    assert ric.shape == (3, 3) and np.array_equal(ric[:2], ic[:2]) and ric[2, 0] == ic[2, 0]
    assert np.abs(ric[2] - ic[2]).max() <= 256 * 256 // 1000      # (a batch of one may run other kernels: last bits of the logits)
    # ... because the step refuses it instead of broadcasting it over its static batch
    before = cc.clone()
    for bad in ((b0["img"][:1], b0["msk"][:1], b0["lbl_msk"][:1]), (b0["img"], b0["msk"][:1], b0["lbl_msk"]),
                (b0["img"], b0["msk"], b0["lbl_msk"][:1]), (b0["img"][:, :, :128], b0["msk"], b0["lbl_msk"])):
        with pytest.raises(ValueError):
            step(*bad)
    assert torch.equal(cc, before)
    net.train()
    with pytest.raises(RuntimeError, match="eval-mode forward"):
        step(b0["img"], b0["msk"], b0["lbl_msk"])
    net.eval()
    # the arena is rebuilt (a parameter replaced): validate records a new step, the stale one refuses to replay
    p = next(net.parameters())
    p.data = p.data.clone()
    net._ensure_arena(p.device)
    _, _, ric, rcc = xbd.validate(net, batches, graph=True, want_counts=True)
    assert np.array_equal(ric, ic) and np.array_equal(rcc, ecc_epoch)
    assert any(kept._generation == net._arena.generation != step._generation for kept in net._xbd_eval_steps.values())
    with pytest.raises(RuntimeError, match="rebuilt"):
        step(b0["img"], b0["msk"], b0["lbl_msk"])
    assert torch.equal(cc, before)


def test_evaluate_val_saves_the_snapshot_only_when_the_score_improves(model_case, tmp_path, capsys):
    from dahitra_amd.models import xbd
    net, batches = model_case["net"], model_case["batches"]
    opt = xbd.AdamW(net.parameters(), lr=1e-4, weight_decay=1e-6)
    path = os.path.join(str(tmp_path), "weights", "snap_best")
    want = model_case["eager"]["building"][0]
    best = xbd.evaluate_val(batches, -1.0, net, opt, path, current_epoch=4, select="building")
    out = capsys.readouterr().out
    assert best == want and "Val Score: %s, Dice: " % want in out and "score: %s\tscore_best: %s" % (want, want) in out
    snap = torch.load(path, map_location="cpu", weights_only=False)
    assert sorted(snap) == ["best_score", "epoch", "optimizer", "state_dict"]
    assert snap["epoch"] == 5 and snap["best_score"] == want and set(snap["state_dict"]) == set(net.state_dict())
    # no improvement: the file stays as it is
    os.remove(path)
    assert xbd.evaluate_val(batches, best, net, opt, path, current_epoch=5, select="building") == best
    assert not os.path.exists(path)
    # a nan score (no first-row label anywhere: the reference's selection counts nothing) beats nothing
    blank = [dict(b, lbl_msk=torch.zeros_like(b["lbl_msk"])) for b in batches]
    assert xbd.evaluate_val(blank, -1.0, net, opt, path, current_epoch=6) == -1.0
    assert "score: nan\tscore_best: -1.0" in capsys.readouterr().out
    assert not os.path.exists(path)


def test_integration_epoch_loop_runs_as_written(model_case, tmp_path, monkeypatch):
    """INTEGRATION.md's loop -- device loader, recorded train step, evaluate_val -- for two epochs at 256 x 256; the graph's
    validation of the trained weights counts what the eager path counts"""
    import random
    from dahitra_amd.datasets.xbd_pipeline import GpuXbdPipeline
    from dahitra_amd.graph import GraphedXbdStep
    from dahitra_amd.models import xbd
    from dahitra_amd.models.xbd import evaluate_val
    monkeypatch.chdir(tmp_path)
    model = xbd.BASE_Transformer_UNet(with_decoder_pos=None).cuda().train()
    model.load_state_dict(O.deterministic_state(NAME))
    optimizer = xbd.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-6, capturable=True)
    pipe = val_pipe = GpuXbdPipeline(*(torch.from_numpy(a).to(DEV) for a in sources(4, 256, 256, seed=21)))
    rng, epochs, best = random.Random(0), 2, -1.0
    first = next(iter(pipe.batches(2, 256, train=True, rng=random.Random(1))))
    step = GraphedXbdStep(model, optimizer, first['img'], first['msk'])
    scores = []
    for epoch in range(epochs):
        for batch in pipe.batches(2, 256, train=True, rng=rng):
            loss = step(batch['img'], batch['msk'])
        best = evaluate_val(val_pipe.batches(2, 256, train=False), best, model, optimizer, 'weights/snap_best', epoch,
                            select='building')
        scores.append(best)
    assert math.isfinite(float(loss)) and all(math.isfinite(s) and s > -1.0 for s in scores)
    snap = torch.load(os.path.join(str(tmp_path), 'weights', 'snap_best'), map_location='cpu', weights_only=False)
    assert snap['best_score'] == best and snap['epoch'] in (1, 2)
    # the weights moved, and the recorded validation step read them at replay: graph and eager count the same integers
    assert not torch.equal(model.state_dict()['resnet.conv1.weight'].cpu(), model_case["net"].state_dict()['resnet.conv1.weight'].cpu())
    batches = list(val_pipe.batches(2, 256, train=False))
    g = xbd.validate(model, batches, select='building', want_counts=True)
    e = xbd.validate(model, batches, select='building', graph=False, want_counts=True)
    assert np.array_equal(g[2], e[2]) and np.array_equal(g[3], e[3]) and g[0] == e[0]
