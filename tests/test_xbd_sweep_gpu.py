"""The xBD threshold sweep on the MI355X: dh_xbd_val_sweep (csrc/xbd_eval.hip) against the numpy restatement of its histograms
(tests/_xbd_sweep_cases.py) and against dh_xbd_val_count, the single-threshold kernel of the same file, then
graph.GraphedXbdSweepStep and models/xbd.validate_sweep / evaluate_val_sweep on the model.  Every comparison is exact: the
synthetic logits and the grid are built so that no last bit of a sigmoid can decide a pixel, the two kernels share one sigmoid,
and everything after it is integer arithmetic."""
import math
import os

import numpy as np
import pytest
import torch

import _xbd_sweep_cases as W
import _xbd_val_cases as V
import cdnet_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAME = "xbd_unet_transformer_nodecpos"
SENTINEL = -7


def prefill(T):
    return np.arange((T + 1) * 20, dtype=np.int64).reshape(T + 1, 4, 5) * 1000 + 17


def run_sweep(x, msk_plane, lbl, thr, select):
    """ops.xbd_val_sweep on device tensors; image_hist starts at a sentinel, class_hist at known values"""
    from dahitra_amd import ops
    T = len(thr)
    ih = torch.full((x.shape[0], T + 1, 4, 2), SENTINEL, dtype=torch.int64, device=DEV)
    ch = torch.from_numpy(prefill(T)).to(DEV)
    ops.xbd_val_sweep(x, msk_plane, lbl, ih, ch, thr, select=select)
    torch.cuda.synchronize()
    return ih.cpu().numpy(), ch.cpu().numpy() - prefill(T)


def run_count(x, msk_plane, lbl, thr, select):
    from dahitra_amd import ops
    ic = torch.full((x.shape[0], 3), SENTINEL, dtype=torch.int64, device=DEV)
    cc = torch.zeros(4, 3, dtype=torch.int64, device=DEV)
    ops.xbd_val_count(x, msk_plane, lbl, ic, cc, thr=float(thr), select=select)
    torch.cuda.synchronize()
    return ic.cpu().numpy(), cc.cpu().numpy()


@pytest.fixture(scope="module")
def grid():
    thr = W.grid()
    W.check_grid(thr)
    return thr


# the shapes of test_xbd_val_gpu: HW odd with every plane aligned differently and less than one workgroup of vector work; 40 x 40;
# the reference's own size, two passes of the capped grid
@pytest.mark.parametrize("B,S", [(3, 37), (2, 40), (1, 1024)])
def test_histograms_equal_the_restatement_on_synthetic_logits(B, S, grid):
    x, msk, lbl, planted = V.synthetic(B, S, seed=B * 100 + S)
    V.check_synthetic(x, msk, lbl, planted)
    assert (x[:, 0] == 0).any(), "localisation logits that sit exactly on the threshold 0.5: the comparison is strict"
    s = V.sigmoid32(x)
    dx, dmsk, dlbl = torch.from_numpy(x).to(DEV), torch.from_numpy(msk).to(DEV), torch.from_numpy(lbl).to(DEV)
    strided = dmsk[:, 0]
    assert B == 1 or not strided.is_contiguous()
    for select in ("reference", "building"):
        want_ih, want_ch = W.hist(x, msk[:, 0], lbl, grid, select, s=s)
        assert np.count_nonzero(want_ih.sum(axis=(0, 2, 3))) > 40 and want_ch.sum() > 0
        for plane in (strided, strided.contiguous(), dmsk):      # channel 0 in place, a copy of it, the whole mask
            ih, ch = run_sweep(dx, plane, dlbl, grid, select)
            assert np.array_equal(ih, want_ih), (select, np.argwhere(ih != want_ih)[:8].tolist())      # written over the sentinel
            assert np.array_equal(ch, want_ch), (select, np.argwhere(ch != want_ch)[:8].tolist())      # accumulated
    # the reference's long masks, converted once; labels above 3 fall into the "other" cell
    lbl5 = lbl.copy()
    lbl5[:, S // 2:, :] = np.where(np.arange(S)[None, None, :] % 2 == 0, 4, 200)
    want_ih, want_ch = W.hist(x, msk[:, 0], lbl5, grid, "building", s=s)
    assert want_ch[:, :, 4].sum() > 0
    ih, ch = run_sweep(dx, dmsk.long(), torch.from_numpy(lbl5).to(DEV).long(), grid, "building")
    assert np.array_equal(ih, want_ih) and np.array_equal(ch, want_ch)


@pytest.mark.parametrize("B,S", [(3, 37), (2, 40)])
def test_sweep_reduces_to_the_single_threshold_kernel_bit_for_bit(B, S, grid):
    """T = 1 at 0.3, and every k of the 64-threshold grid: sweep_counts of the histograms is what dh_xbd_val_count writes"""
    from dahitra_amd.models.xbd import sweep_counts, sweep_loc_table
    x, msk, lbl, _ = V.synthetic(B, S, seed=B * 100 + S)
    dx, dmsk, dlbl = torch.from_numpy(x).to(DEV), torch.from_numpy(msk).to(DEV), torch.from_numpy(lbl).to(DEV)
    for select in ("reference", "building"):
        ih, ch = run_sweep(dx, dmsk, dlbl, [0.3], select)
        assert ih.shape == (B, 2, 4, 2) and ch.shape == (2, 4, 5)
        ic, cc = sweep_counts(ih, ch, sweep_loc_table(1, 0))
        want_ic, want_cc = run_count(dx, dmsk, dlbl, 0.3, select)
        assert np.array_equal(ic, want_ic) and np.array_equal(cc, want_cc), select
        ih, ch = run_sweep(dx, dmsk, dlbl, grid, select)
        for k in range(grid.size):
            ic, cc = sweep_counts(ih, ch, sweep_loc_table(grid.size, k))
            want_ic, want_cc = run_count(dx, dmsk, dlbl, grid[k], select)
            assert np.array_equal(ic, want_ic) and np.array_equal(cc, want_cc), (select, k, grid[k])


def test_unaligned_base_pointers_take_the_scalar_path(grid):
    """views that start 1 float / 1 byte into their buffers: no plane is aligned to its vector"""
    B, S = 2, 40
    x, msk, lbl, planted = V.synthetic(B, S, seed=7)
    dx = torch.zeros(x.size + 1, dtype=torch.float32, device=DEV)[1:].view(x.shape)
    dx.copy_(torch.from_numpy(x))
    dm = torch.zeros(B * S * S + 1, dtype=torch.uint8, device=DEV)[1:].view(B, S, S)
    dm.copy_(torch.from_numpy(msk[:, 0]))
    dl = torch.zeros(B * S * S + 1, dtype=torch.uint8, device=DEV)[1:].view(B, S, S)
    dl.copy_(torch.from_numpy(lbl))
    assert dx.data_ptr() % 16 == 4 and dm.data_ptr() % 4 == 1 and dl.data_ptr() % 4 == 1
    aligned = [torch.from_numpy(a).to(DEV) for a in (x, msk[:, 0].copy(), lbl)]
    for select in ("reference", "building"):
        want_ih, want_ch = W.hist(x, msk[:, 0], lbl, grid, select)
        ih, ch = run_sweep(dx, dm, dl, grid, select)
        assert np.array_equal(ih, want_ih) and np.array_equal(ch, want_ch), select
        ih, ch = run_sweep(*aligned, grid, select)
        assert np.array_equal(ih, want_ih) and np.array_equal(ch, want_ch), select


def test_refused_arguments_return_an_error_and_write_nothing():
    import ctypes
    from dahitra_amd import _lib, ops
    L = _lib.lib()
    x = torch.zeros(2, 5, 8, 8, device=DEV)
    m = torch.ones(2, 8, 8, dtype=torch.uint8, device=DEV)
    lab = torch.ones(2, 8, 8, dtype=torch.uint8, device=DEV)
    T = 2
    ih = torch.full((2, 65 + 1, 4, 2), SENTINEL, dtype=torch.int64, device=DEV)       # room for any T the table below passes
    ch = torch.from_numpy(prefill(65)).to(DEV)
    P, S = ops.P, ops.S

    def host(values):
        return (ctypes.c_float * max(len(values), 1))(*values)
    NULL = ctypes.c_void_p(0)
    good = dict(logits=P(x), msk0=P(m), stride=64, lbl=P(lab), B=2, H=8, W=8, thr=host([0.3, 0.6]), T=T, select=0, ih=P(ih), ch=P(ch))
    order = ("logits", "msk0", "stride", "lbl", "B", "H", "W", "thr", "T", "select", "ih", "ch")
    nan = float("nan")
    bad = [dict(H=4, W=16), dict(H=8, W=4), dict(B=0), dict(B=-1), dict(logits=P(None)), dict(msk0=P(None)), dict(lbl=P(None)),
           dict(ih=P(None)), dict(ch=P(None)), dict(select=2), dict(stride=63),
           # the sibling's thr cases, as a grid of one and inside a grid of two
           dict(thr=host([0.0]), T=1), dict(thr=host([1.0]), T=1), dict(thr=host([-0.3]), T=1), dict(thr=host([1.5]), T=1),
           dict(thr=host([nan]), T=1), dict(thr=host([0.0, 0.3])), dict(thr=host([0.3, 1.0])), dict(thr=host([0.3, nan])),
           dict(thr=host([nan, 0.3])), dict(thr=host([-0.3, 0.3])), dict(thr=host([0.3, 1.5])),
           dict(thr=NULL), dict(T=0), dict(T=-1), dict(thr=host([0.01 * (k + 1) for k in range(65)]), T=65),
           dict(thr=host([0.6, 0.3])), dict(thr=host([0.3, 0.3])),
           dict(thr=host([0.1, 0.2, 0.3, 0.25]), T=4), dict(thr=host([0.1, 0.2, 0.2, 0.3]), T=4)]
    for change in bad:
        args = dict(good, **change)
        rc = L.dh_xbd_val_sweep(*[args[k] for k in order], S())
        assert rc != 0, change
        assert L.dh_last_error().decode().startswith("xbd_val_sweep"), (change, L.dh_last_error())
    torch.cuda.synchronize()
    assert (ih == SENTINEL).all() and np.array_equal(ch.cpu().numpy(), prefill(65))
    # H != W is fine for the building selection, and the good call does write
    assert L.dh_xbd_val_sweep(*[dict(good, H=4, W=16, select=1)[k] for k in order], S()) == 0
    assert L.dh_xbd_val_sweep(*[good[k] for k in order], S()) == 0
    torch.cuda.synchronize()
    got = ih.cpu().numpy().reshape(-1)[:2 * (T + 1) * 8].reshape(2, T + 1, 4, 2)
    want = np.zeros((2, T + 1, 4, 2), dtype=np.int64)
    want[:, 1, 0, 1] = 64                                  # 0.3 < sigmoid(0) = 0.5 < 0.6; four equal sigmoids: arg 0; msk set
    assert np.array_equal(got, want)
    assert (ih.reshape(-1)[2 * (T + 1) * 8:] == SENTINEL).all(), "nothing is written past [B, T + 1, 4, 2]"
    # the Python wrapper refuses what it can see before the call
    ih2, ch2 = torch.zeros(2, 3, 4, 2, dtype=torch.int64, device=DEV), torch.zeros(3, 4, 5, dtype=torch.int64, device=DEV)
    for args in ((x, m, lab, ih2, ch2, [0.6, 0.3]), (x, m[:1], lab, ih2, ch2, [0.3, 0.6]), (x, m, lab, ih2[:1], ch2, [0.3, 0.6]),
                 (x, m, lab, ih2, ch2, [0.3]), (x, m, lab, ih2, ch2, [0.3, 1.0])):
        with pytest.raises(ValueError):
            ops.xbd_val_sweep(*args)
    with pytest.raises(_lib.HipLibraryError):
        ops.xbd_val_sweep(x, m, lab, ih2.cpu(), ch2, [0.3, 0.6])
    assert not ih2.any() and not ch2.any()


# ---- model level: the recipe of tests/test_xbd_val_gpu.py --------------------------------------------------------------
def blocky(rng, n, h, w, values):
    """constant in 8 x 8 blocks (the recipe of tests/test_xbd_loader_gpu.py)"""
    small = rng.choice(np.asarray(values, dtype=np.uint8), size=(n, -(-h // 8), -(-w // 8)))
    return np.ascontiguousarray(np.kron(small, np.ones((1, 8, 8), dtype=np.uint8))[:, :h, :w])


def sources(n, H, W_, seed):
    """pre, post (noise), pre mask (0 / 255), post label (0 .. 4)"""
    rng = np.random.RandomState(seed)
    pre = rng.randint(0, 256, (n, H, W_, 3)).astype(np.uint8)
    post = rng.randint(0, 256, (n, H, W_, 3)).astype(np.uint8)
    return pre, post, blocky(rng, n, H, W_, [0, 255]), blocky(rng, n, H, W_, [0, 1, 2, 3, 4])


THR19 = np.linspace(0.05, 0.95, 19).astype(np.float32)


@pytest.fixture(scope="module")
def model_case():
    """the net, a 4-image validation epoch in batches of 2 at 256 x 256, and per batch ONE eager forward with the sweep's
    histograms and the single-threshold kernel's counts at every threshold, both selections, on that same logits tensor"""
    from dahitra_amd import ops
    from dahitra_amd.datasets.xbd_pipeline import GpuXbdPipeline
    from dahitra_amd.models import xbd
    net = xbd.BASE_Transformer_UNet(input_nc=3, output_nc=5, token_len=4, resnet_stages_num=4, with_pos='learned',
                                    with_decoder_pos=None, enc_depth=1, dec_depth=8).cuda()
    net.load_state_dict(O.deterministic_state(NAME))
    net.eval()
    pipe = GpuXbdPipeline(*(torch.from_numpy(a).to(DEV) for a in sources(4, 256, 256, seed=21)))
    batches = list(pipe.batches(2, 256, train=False))
    assert len(batches) == 2 and tuple(batches[0]["lbl_msk"].shape) == (2, 256, 256)
    T = THR19.size
    eager = {sel: {"ih": [], "ch": torch.zeros(T + 1, 4, 5, dtype=torch.int64, device=DEV), "ic": [[] for _ in range(T)],
                   "cc": [torch.zeros(4, 3, dtype=torch.int64, device=DEV) for _ in range(T)]} for sel in ("reference", "building")}
    for b in batches:
        with torch.no_grad():
            logits = net(b["img"]).float()
        for sel, e in eager.items():
            ih = torch.full((2, T + 1, 4, 2), SENTINEL, dtype=torch.int64, device=DEV)
            ops.xbd_val_sweep(logits, b["msk"], b["lbl_msk"], ih, e["ch"], THR19, select=sel)
            e["ih"].append(ih)
            for k in range(T):
                ic = torch.full((2, 3), SENTINEL, dtype=torch.int64, device=DEV)
                ops.xbd_val_count(logits, b["msk"], b["lbl_msk"], ic, e["cc"][k], thr=float(THR19[k]), select=sel)
                e["ic"][k].append(ic)
    torch.cuda.synchronize()
    for e in eager.values():
        e["ih"] = torch.cat(e["ih"]).cpu().numpy()
        e["ch"] = e["ch"].cpu().numpy()
        e["ic"] = [torch.cat(rows).cpu().numpy() for rows in e["ic"]]
        e["cc"] = [c.cpu().numpy() for c in e["cc"]]
    return {"net": net, "batches": batches, "eager": eager}


def test_model_sweep_equals_the_single_threshold_kernel_on_the_same_logits(model_case):
    """exact, with no undecided band: both kernels take the same sigmoid of the same tensor"""
    from dahitra_amd.models.xbd import sweep_counts, sweep_loc_table
    for sel, e in model_case["eager"].items():
        assert (e["ih"].sum(axis=(1, 2, 3)) == 256 * 256).all()
        assert np.count_nonzero(e["ih"].sum(axis=(0, 2, 3))) >= 2, "the net's localisation sigmoids fall into more than one bin"
        for k in range(THR19.size):
            ic, cc = sweep_counts(e["ih"], e["ch"], sweep_loc_table(THR19.size, k))
            assert np.array_equal(ic, e["ic"][k]) and np.array_equal(cc, e["cc"][k]), (sel, k)


def same(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def test_recorded_step_and_validate_sweep_give_the_eager_integers(model_case, capsys):
    from dahitra_amd.graph import GraphedXbdSweepStep
    from dahitra_amd.models import xbd
    net, batches, eager = model_case["net"], model_case["batches"], model_case["eager"]
    b0, b1 = batches
    T = THR19.size
    ch = torch.from_numpy(prefill(T)).to(DEV)
    step = GraphedXbdSweepStep(net, b0["img"], b0["msk"], b0["lbl_msk"], ch, THR19)
    assert np.array_equal(ch.cpu().numpy(), prefill(T)), "warm-up and capture leave the histogram as it was"
    assert tuple(step.image_hist.shape) == (2, T + 1, 4, 2) and step.image_hist.dtype == torch.int64
    rows = []
    for b in (b0, b1):                                   # two replays, two different batches
        logits = step(b["img"], b["msk"], b["lbl_msk"])
        assert tuple(logits.shape) == (2, 5, 256, 256)
        rows.append(step.image_hist.clone())
    assert np.array_equal(torch.cat(rows).cpu().numpy(), eager["reference"]["ih"])
    assert np.array_equal(ch.cpu().numpy() - prefill(T), eager["reference"]["ch"])
    # the epoch through the graph and eagerly: the same integers, and the scores validate gives threshold by threshold
    for sel in ("reference", "building"):
        capsys.readouterr()
        g = xbd.validate_sweep(net, batches, THR19, select=sel, graph=True)
        out = capsys.readouterr().out
        e = xbd.validate_sweep(net, batches, THR19, select=sel, graph=False)
        for sweep in (g, e):
            assert np.array_equal(sweep.image_hist, eager[sel]["ih"]) and np.array_equal(sweep.class_hist, eager[sel]["ch"])
            assert sweep.thresholds.dtype == np.float32 and np.array_equal(sweep.thresholds, THR19)
            assert sweep.scores.shape == (T,) and sweep.scores.dtype == np.float64
        lines = [l for l in out.splitlines() if l.startswith("thr ")]
        assert len(lines) == T and lines[3].startswith("thr {}: Val Score: {}, Dice: ".format(str(THR19[3]), g.scores[3]))
        for k in range(T):
            want = xbd.validate(net, batches, thr=float(THR19[k]), select=sel, graph=False)
            assert same(g.scores[k], want) and same(e.scores[k], want), (sel, k, g.scores[k], want)
        thr, sc = g.best()
        if np.isnan(g.scores).all():
            assert thr is None and math.isnan(sc)
        else:
            k = int(np.nanargmax(g.scores))
            assert thr == float(THR19[k]) and sc == g.scores[k] and g.parts(k)["dice"] == xbd.val_score(*g.counts(k))[1]["dice"]
    assert not np.isnan(xbd.validate_sweep(net, batches, THR19, select="building").scores).all()
    # a second grid records a second step; the first one stays valid
    xbd.validate_sweep(net, batches, THR19[::2], select="building")
    again = xbd.validate_sweep(net, batches, THR19, select="building")
    assert np.array_equal(again.image_hist, eager["building"]["ih"]) and np.array_equal(again.class_hist, eager["building"]["ch"])
    assert len(net.__dict__["_xbd_sweep_steps"]) == 3
    # a ragged last batch goes through the eager path inside validate_sweep ...
    ih = eager["reference"]["ih"]
    ragged = {k: v[:1] for k, v in b1.items()}
    r = xbd.validate_sweep(net, [b0, ragged], THR19, graph=True)
    assert r.image_hist.shape == (3, T + 1, 4, 2) and np.array_equal(r.image_hist[:2], ih[:2])
    assert np.array_equal(r.image_hist[2].sum(axis=(0, 1)), ih[2].sum(axis=(0, 1)))          # |gt0| does not depend on the logits
    assert np.abs(r.image_hist[2] - ih[2]).sum() <= 2 * (256 * 256 // 1000)      # (a batch of one may run other kernels: last bits)
    # ... because the step refuses it instead of broadcasting it over its static batch
    before = ch.clone()
    for bad in ((b0["img"][:1], b0["msk"][:1], b0["lbl_msk"][:1]), (b0["img"], b0["msk"][:1], b0["lbl_msk"]),
                (b0["img"], b0["msk"], b0["lbl_msk"][:1]), (b0["img"][:, :, :128], b0["msk"], b0["lbl_msk"])):
        with pytest.raises(ValueError):
            step(*bad)
    assert torch.equal(ch, before)
    net.train()
    with pytest.raises(RuntimeError, match="eval-mode forward"):
        step(b0["img"], b0["msk"], b0["lbl_msk"])
    net.eval()
    with pytest.raises(ValueError):
        xbd.validate_sweep(net, batches, [0.5, 0.3])
    with pytest.raises(ValueError):
        xbd.validate_sweep(net, [], THR19)
    # the arena is rebuilt (a parameter replaced): the stale step refuses to replay and leaves the histogram alone
    p = next(net.parameters())
    p.data = p.data.clone()
    net._ensure_arena(p.device)
    with pytest.raises(RuntimeError, match="rebuilt"):
        step(b0["img"], b0["msk"], b0["lbl_msk"])
    assert torch.equal(ch, before)


def test_evaluate_val_sweep_saves_the_snapshot_with_its_threshold_only_when_the_score_improves(model_case, tmp_path, capsys):
    from dahitra_amd.models import xbd
    net, batches = model_case["net"], model_case["batches"]
    opt = xbd.AdamW(net.parameters(), lr=1e-4, weight_decay=1e-6)
    path = os.path.join(str(tmp_path), "weights", "snap_best")
    thr, want = xbd.validate_sweep(net, batches, THR19, select="building").best()
    assert thr is not None and not math.isnan(want)
    capsys.readouterr()
    best = xbd.evaluate_val_sweep(batches, -1.0, net, opt, path, 4, THR19, select="building")
    out = capsys.readouterr().out
    assert best == want and "score: %s\tscore_best: %s" % (want, want) in out and out.count("Val Score: ") == THR19.size
    snap = torch.load(path, map_location="cpu", weights_only=False)
    assert sorted(snap) == ["best_score", "epoch", "optimizer", "state_dict", "thr"]
    assert snap["epoch"] == 5 and snap["best_score"] == want and snap["thr"] == thr and thr in [float(t) for t in THR19]
    assert set(snap["state_dict"]) == set(net.state_dict())
    # no improvement: the file stays as it is
    os.remove(path)
    assert xbd.evaluate_val_sweep(batches, best, net, opt, path, 5, THR19, select="building") == best
    assert not os.path.exists(path)
    # nan scores everywhere (no first-row label anywhere: the reference's selection counts nothing) beat nothing
    blank = [dict(b, lbl_msk=torch.zeros_like(b["lbl_msk"])) for b in batches]
    assert xbd.evaluate_val_sweep(blank, -1.0, net, opt, path, 6, THR19) == -1.0
    assert "score: nan\tscore_best: -1.0" in capsys.readouterr().out
    assert not os.path.exists(path)
