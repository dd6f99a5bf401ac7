"""xBD_code/train_adapt.py without a GPU: the float64 restatement of its loss (tests/_xbd_adapt_cases.py) against the reference's own
float64 results (tests/golden/xbd_adapt_loss.npz, tools/make_adapt_loss_golden.py), the masks of its two datasets as a closed form
of the label byte, its file set, the four-class net's state layout, the scheduler, what the wrappers refuse before any kernel entry
is reached, and the meter arithmetic of train_epoch_adapt with a stand-in step."""
import os
import types

import numpy as np
import pytest
import torch

import _xbd_adapt_cases as C
from dahitra_amd import _lib, graph, netspec, ops
from dahitra_amd.datasets import xbd_pipeline as P
from dahitra_amd.models import xbd

U8, F32 = torch.uint8, torch.float32


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "xbd_adapt_loss.npz"))


# ---- the loss ---------------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_reference_in_float64(golden):
    """the numpy restatement, gradient included, against the reference's float64 results on both cases: 1e-12, relative for the
    scalars, of the largest gradient for the gradient (float64 rounding is a few 1e-16)"""
    worst = worst_grad = 0.0
    for name in C.CASES:
        r = C.restate(golden[name + "_logits"], golden[name + "_msk"])
        ref = C.fixture_reference(golden, name)
        got, want = np.concatenate([[r["loss"]], r["parts"][:5]]), np.concatenate([[ref["loss"]], ref["parts"][:5]])
        worst = max(worst, float(np.max(np.abs(got - want) / np.abs(want))))
        worst_grad = max(worst_grad, float(np.abs(r["grad"] - ref["grad"]).max() / np.abs(ref["grad"]).max()))
        assert r["parts"][5] == 0
        assert np.array_equal(r["label"], golden[name + "_lbl"])            # the label the script derived
    print("restatement against the reference's float64: scalars %.3e relative, gradient %.3e of its maximum" % (worst, worst_grad))
    assert worst <= 1e-12 and worst_grad <= 1e-12, (worst, worst_grad)


def test_fixture_is_what_the_tool_describes(golden):
    for name in C.CASES:
        x, m = golden[name + "_logits"], golden[name + "_msk"]
        assert x.shape == m.shape == (2, 4, 15, 17) and x.dtype == np.float32 and m.dtype == np.uint8 and m.max() == 1
        assert (x == 25.0).any() and (x == -25.0).any()                 # both clamps of the focal term are hit
        assert golden[name + "_grad32"].dtype == np.float32 and golden[name + "_grad64"].dtype == np.float64
        assert set(np.unique(golden[name + "_lbl"])) == {0, 1, 2, 3}
    t, v = golden["train_msk"], golden["val_msk"]
    assert np.array_equal(t[:, 0], t[:, 1:].max(1))                     # TrainData: channel 0 is the union
    lonely = (v[:, 0] == 1) & (v[:, 1:].max(1) == 0)                    # ValData: m0 set without a damage plane
    assert lonely.any() and not golden["val_lbl"][lonely].any()         # ... where the label is 0
    bare = (v[:, 0] == 0) & (v[:, 1:].max(1) == 1)                      # a damage plane without m0: 1 - m0 comes first
    assert bare.any() and not golden["val_lbl"][bare].any()
    y = C.yardstick(golden)
    print("yardstick (the reference's float32 against its float64): %s" % y)
    assert all(0 < val < 1e-3 for val in y.values()), y


def test_the_cross_entropy_has_a_gradient_on_every_pixel(golden):
    """unlike unet_loss's masked term: the gradient of 5 * ce alone is non-zero at every pixel, background included"""
    x, m = golden["train_logits"], golden["train_msk"]
    full = C.restate(x, m)["grad"]
    # the combo terms alone: the same restatement with the cross-entropy's part taken out through its own formula
    y = C.label(m)
    e = np.exp(x.astype(np.float64) - x.max(1, keepdims=True))
    soft = e / e.sum(1, keepdims=True)
    w = np.asarray(C.CE_WEIGHTS)[y]
    ce_grad = C.CE_SCALE * (w / w.sum())[:, None] * (soft - (np.arange(4)[None, :, None, None] == y[:, None]))
    assert (np.abs(ce_grad).max(1) > 0).all() and (y == 0).any()
    assert np.abs(full - ce_grad).max() > 0


# ---- the masks --------------------------------------------------------------------------------------------------------------
def test_the_closed_form_equals_the_scripts_masks_for_every_byte():
    """all 256 x 256 pairs of (post label byte, pre mask byte), one pixel each, through the literal code of lines 147-175 and
    216-236 -- priority lines included -- and through the closed form the kernel computes"""
    label, pre = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    for train, literal in ((True, C.train_masks_literal), (False, C.val_masks_literal)):
        m, l = literal(pre.copy(), label.copy())
        cm, cl = C.masks_closed(pre, label, train)
        assert np.array_equal(m.transpose(2, 0, 1), cm), train
        assert np.array_equal(l, cl), train
        assert cl.max() == 2 and not cm[1:, 5:].any() and not cl[5:].any()      # a label byte above 4 sets no damage plane
        if train:
            assert not cm[0, 5:].any()
        else:
            assert np.array_equal(cm[0], pre > 127)
    # the training mask does not depend on the pre mask at all (line 165)
    a, _ = C.train_masks_literal(np.zeros_like(pre), label.copy())
    b, _ = C.train_masks_literal(np.full_like(pre, 255), label.copy())
    assert np.array_equal(a, b)


def test_the_priority_lines_cannot_fire_on_planes_cut_from_one_byte():
    label = np.arange(256, dtype=np.uint8).reshape(16, 16)
    m1, m2, m3 = label == 1, label == 2, (label == 3) | (label == 4)
    assert not (m1 & (m2 | m3)).any() and not (m3 & m2).any()


# ---- the file set -------------------------------------------------------------------------------------------------------------
def test_adapt_files_is_the_name_filter_of_line_75():
    names = ["hurricane-michael_00000001_pre_disaster.png", "hurricane-michael_00000001_post_disaster.png",
             "AOI1-tile_3-4_pre_disaster.png", "AOI1-tile_3-4_post_disaster.png", "hurricane-harvey_00000002_pre_disaster.png",
             "x/AOI2_pre_disaster.png.bak"]
    want = [f for f in names if ('_pre_disaster.png' in f) and (('hurricane-michael' in f) or ('AOI' in f))]
    assert P.adapt_files(names) == want == [names[0], names[2], names[5]]


def synthetic_set(seed, n=23, hw=40 * 40):
    rng = np.random.RandomState(seed)
    names, labels = [], []
    for i in range(n):
        names.append(("AOI%d-tile_%d_pre_disaster.png" if rng.rand() < 0.6 else "hurricane-michael_%04d%d_pre_disaster.png") % (i, i))
        lab = np.zeros(hw, dtype=np.uint8)
        k = int(rng.choice([0, 100, 125, 126, 167, 250, 251, 400, 900]))          # sums around the bound of 500
        lab[:k] = 2 if k in (250, 251) else rng.choice([1, 2, 3, 4], size=k)          # 250 twos: exactly 500, not kept; 251: kept
        labels.append(rng.permutation(lab).reshape(40, 40))
    return names, labels


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_adapt_train_indices_equals_the_scripts_lists(seed):
    names, labels = synthetic_set(seed)
    table = np.stack([np.bincount(l.reshape(-1), minlength=6)[:6] for l in labels]).astype(np.int64)
    split = lambda n: P.split_indices(n, 0.15, seed)
    want_train, want_val = C.trainset_literal(names, labels, split)
    train_idxs, val_idxs, n_xbd, n_aoi = P.adapt_train_indices(table, names, seed)
    assert [names[i] for i in train_idxs] == want_train and [names[i] for i in val_idxs] == want_val
    assert n_xbd + n_aoi == len(train_idxs) and all('AOI' in names[i] for i in val_idxs)
    sums = np.array([int(l[l > 0].sum()) for l in labels])
    assert (sums > 500).any() and (sums <= 500).any() and ((sums == 500).any() or (sums == 502).any())      # the bound is exercised
    assert sorted(list(train_idxs) + list(val_idxs)) == [i for i in range(len(names)) if sums[i] > 500]


def test_adapt_train_indices_refuses_what_it_cannot_read():
    names, labels = synthetic_set(0)
    table = np.stack([np.bincount(l.reshape(-1), minlength=6)[:6] for l in labels]).astype(np.int64)
    bad = table.copy()
    bad[3, 5] = 1
    with pytest.raises(ValueError, match="above 4"):
        P.adapt_train_indices(bad, names)
    with pytest.raises(ValueError, match="files"):
        P.adapt_train_indices(table, names[:-1])
    with pytest.raises(ValueError):
        P.adapt_train_indices(table.astype(np.float64), names)
    with pytest.raises(ValueError):                                       # no AOI file: nothing to split
        P.adapt_train_indices(table, [n.replace("AOI", "aoi") for n in names])


# ---- the net --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("suffix", ["", "_nodecpos"])
def test_the_c4_state_spec_is_the_five_class_one_but_for_the_classifier(suffix):
    c4, c5 = netspec.state_spec("xbd_unet_transformer_c4" + suffix), netspec.state_spec("xbd_unet_transformer" + suffix)
    assert len(c4) == len(c5)
    differ = [(a, b) for a, b in zip(c4, c5) if a != b]
    assert [(a[0], a[1], b[1]) for a, b in differ] == [("classifier.weight", (4, 32, 3, 3), (5, 32, 3, 3)),
                                                      ("classifier.bias", (4,), (5,))]
    assert netspec.get_config("xbd_unet_transformer_c4" + suffix)["n_class"] == 4
    assert netspec.get_config("xbd_unet_transformer_c4" + suffix)["decoder_pos"] == (suffix == "")


def test_the_constructor_returns_the_c4_nets_and_refuses_other_counts(capsys):
    net = xbd.BASE_Transformer_UNet(input_nc=3, output_nc=4, token_len=4, resnet_stages_num=4, with_pos='learned',
                                    with_decoder_pos='learned', enc_depth=1, dec_depth=8)          # train_adapt.py:37-38
    assert net.net_G == "xbd_unet_transformer_c4" and tuple(net.state_dict()["classifier.weight"].shape) == (4, 32, 3, 3)
    assert xbd.BASE_Transformer_UNet(output_nc=4).net_G == "xbd_unet_transformer_c4_nodecpos"
    assert xbd.BASE_Transformer_UNet(output_nc=5).net_G == "xbd_unet_transformer_nodecpos"
    for nc in (2, 3, 6):
        with pytest.raises(NotImplementedError):
            xbd.BASE_Transformer_UNet(output_nc=nc)


def test_load_snapshot_keeps_the_classifier_of_a_c4_net(tmp_path, capsys):
    """train_adapt.py:399-417: the size-matched copy from a five-class snapshot -- everything but classifier.*"""
    five = xbd.BASE_Transformer_UNet(output_nc=5)
    four = xbd.BASE_Transformer_UNet(output_nc=4)
    before = {k: v.clone() for k, v in four.state_dict().items()}
    path = str(tmp_path / "snap")
    torch.save({'epoch': 3, 'state_dict': {'module.' + k: v for k, v in five.state_dict().items()}, 'best_score': 0.5}, path)
    assert xbd.load_snapshot(four, path) == (3, 0.5)
    after, src = four.state_dict(), five.state_dict()
    for k in after:
        if k.startswith("classifier."):
            assert torch.equal(after[k], before[k]) and after[k].shape != src[k].shape, k
        else:
            assert torch.equal(after[k], src[k]), k


# ---- scheduler, refusals, meters ------------------------------------------------------------------------------------------------
def test_adapt_scheduler_has_the_milestones_of_line_423():
    p = torch.nn.Parameter(torch.zeros(1))
    sch = xbd.adapt_scheduler(torch.optim.SGD([p], lr=1.0))
    want = [5, 11, 23, 29, 33, 47, 50, 60, 70, 90, 110, 130, 150, 170, 180, 190]
    assert sorted(sch.milestones) == want and 17 not in sch.milestones and sch.gamma == 0.6
    assert sorted(xbd.unet_scheduler(torch.optim.SGD([p], lr=1.0)).milestones) == sorted(want + [17])


def test_val_score_with_three_classes_is_the_scripts_arithmetic():
    rng = np.random.RandomState(3)
    ic = np.stack([[5, 7, 3], [0, 0, 0], [9, 4, 4]])
    cc = rng.randint(1, 50, (3, 3))
    sc, parts = xbd.val_score(ic, cc, classes=3)
    want = C.val_score_literal(ic, cc)
    assert sc == want[0] and parts['dice'] == want[1] and parts['f1'] == want[2] and np.array_equal(parts['f1_per_class'], want[3])
    with pytest.raises(ValueError):
        xbd.val_score(ic, cc, classes=5)
    with pytest.raises(ValueError):
        xbd.val_score(ic, np.zeros((4, 3)), classes=3)


def test_wrappers_refuse_before_any_launch():
    x, m, w = torch.zeros(2, 4, 6, 6), torch.zeros(2, 4, 6, 6, dtype=U8), torch.zeros(8)
    with pytest.raises(_lib.HipLibraryError):
        xbd.adapt_loss(x, m)
    with pytest.raises(_lib.HipLibraryError):
        ops.xbd_adapt_loss_fwd(x, m, w)
    with pytest.raises(ValueError, match="logits"):
        ops.xbd_adapt_loss_fwd(torch.zeros(2, 5, 6, 6), m, w)
    with pytest.raises(ValueError, match="msk"):
        ops.xbd_adapt_loss_fwd(x, m.float(), w)
    with pytest.raises(ValueError, match="msk"):
        ops.xbd_adapt_loss_fwd(x, m[:, :3], w)
    with pytest.raises(ValueError, match="weights_dev"):
        ops.xbd_adapt_loss_fwd(x, m, torch.zeros(10))
    with pytest.raises(ValueError, match="sums"):
        ops.xbd_adapt_loss_bwd(x, m, None, w)
    with pytest.raises(ValueError, match="sums"):
        ops.xbd_adapt_loss_bwd(x, m, torch.zeros(24), w)
    with pytest.raises(ValueError, match="4 numbers"):
        xbd.adapt_weights_dev("cpu", channel_weights=(1, 2, 3, 4, 5))
    with pytest.raises(ValueError, match="msks"):
        graph.GraphedXbdAdaptStep(None, None, torch.zeros(2, 6, 8, 8), torch.zeros(2, 5, 8, 8, dtype=U8))
    with pytest.raises(ValueError, match="classes"):
        ops.xbd_val_count(torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 4, 4, dtype=U8), torch.zeros(1, 4, 4, dtype=U8),
                          torch.zeros(1, 3, dtype=torch.int64), torch.zeros(3, 3, dtype=torch.int64), classes=2)
    with pytest.raises(ValueError, match=r"\[B, 4, H, W\]"):
        ops.xbd_val_count(torch.zeros(1, 5, 4, 4), torch.zeros(1, 4, 4, dtype=U8), torch.zeros(1, 4, 4, dtype=U8),
                          torch.zeros(1, 3, dtype=torch.int64), torch.zeros(3, 3, dtype=torch.int64), classes=3)
    assert ops.XBD_ADAPT_PARTS == ("loss0", "loss1", "loss2", "loss3", "ce", "zero")


def test_train_epoch_adapt_meters_and_line_with_a_stand_in_step(monkeypatch, capsys):
    """the epoch's arithmetic without a device: AverageMeter's means weighted by the batch size, and line 359 as printed --
    `loss2` is the meter of loss1, `Dice` the meter of loss3"""
    rows = [(3, [2.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.0]), (1, [6.0, 0.5, 0.6, 0.7, 0.8, 0.9, 0.0])]
    it = iter(rows)

    def fake(model, optimizer, first, graph):
        def run(batch):
            vals = next(it)[1]
            return torch.tensor(vals[0]), torch.tensor(vals[1:])
        return run
    monkeypatch.setattr(xbd, "_adapt_train_step", fake)
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=1e-4)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[1], gamma=0.6)
    model = types.SimpleNamespace(train=lambda: None)
    batches = [{'img': torch.zeros(n, 6, 4, 4), 'msk': torch.zeros(n, 4, 4, 4, dtype=U8)} for n, _ in rows]
    opt.step()
    meters = xbd.train_epoch_adapt(7, model, opt, sch, batches)
    avg = lambda col: (3 * rows[0][1][col] + 1 * rows[1][1][col]) / 4
    for key, col in (('loss', 0), ('loss0', 1), ('loss1', 2), ('loss2', 3), ('loss3', 4), ('ce', 5)):
        assert meters[key] == pytest.approx(avg(col), rel=1e-6), key
    assert meters['steps'] == 2 and meters['samples'] == 4 and meters['lr'] == pytest.approx(0.6e-4)
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("epoch: ")]
    assert line == ["epoch: 7; lr 0.0000600; Loss {:.4f}; loss2 {:.4f}; Dice {:.4f}".format(avg(0), avg(2), avg(4))]
    with pytest.raises(ValueError, match="no batches"):
        xbd.train_epoch_adapt(0, model, opt, sch, [])
