"""The step of xBD_code/train_unettransformer.py without a GPU: the float64 restatement of its loss (tests/_xbd_unet_loss_cases.py)
against the reference's own float64 results (tests/golden/xbd_unet_loss.npz, tools/make_unet_loss_golden.py), the identities of the
script as executed, the scheduler, what the new wrappers and the step's constructor refuse -- before any kernel entry of the
library is reached -- and the meter arithmetic of train_epoch_unet with a stand-in step."""
import math
import os
import types

import numpy as np
import pytest
import torch

import _xbd_unet_loss_cases as C
from dahitra_amd import _lib, graph, ops
from dahitra_amd.models import xbd

U8, F32 = torch.uint8, torch.float32


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "xbd_unet_loss.npz"))


@pytest.fixture(scope="module")
def case(golden):
    logits, msk, lbl = C.make_case(golden, 2, 19, 21, True, seed=5)
    return logits.numpy(), msk.numpy(), lbl.numpy()


# ---- the restatement against the reference ----------------------------------------------------------------------------------
def test_restatement_equals_the_reference_in_float64(golden):
    """Measured on the fixture (both cases): the largest relative difference of loss, channel losses, ce and Dice meter is
    2.76e-16, the largest gradient error over the largest gradient 1.13e-15: float64 rounding.  Asserted: ten times that,
    2.8e-15 and 1.2e-14, far inside the 1e-9 the bound may not exceed."""
    worst = worst_grad = 0.0
    for name in ("zero", "damage"):
        r = C.restate(golden[name + "_logits"], golden[name + "_msk"], golden[name + "_lbl"])
        want = np.concatenate([[golden[name + "_loss64"]], golden[name + "_channel64"], [golden[name + "_ce64"]],
                               [golden[name + "_dice64"]]])
        got = np.concatenate([[r["loss"]], r["parts"][:7]])
        worst = max(worst, float(np.max(np.abs(got - want) / np.abs(want))))
        g = golden[name + "_grad64"]
        worst_grad = max(worst_grad, float(np.abs(r["grad"] - g).max() / np.abs(g).max()))
        assert r["parts"][7] == 0
    print("restatement against the reference's float64: scalars %.3e relative, gradient %.3e of its maximum" % (worst, worst_grad))
    assert worst <= 2.8e-15 <= 1e-9 and worst_grad <= 1.2e-14 <= 1e-9, (worst, worst_grad)


def test_fixture_is_what_the_tool_describes(golden):
    assert golden["zero_logits"].dtype == np.float32 and golden["zero_msk"].dtype == np.uint8 and golden["zero_lbl"].dtype == np.uint8
    assert not golden["zero_lbl"].any() and golden["damage_lbl"].any()
    assert (golden["damage_lbl"] == C.damage_label(golden["damage_msk"])).all()
    for name in ("zero", "damage"):
        x = golden[name + "_logits"]
        assert (x == 25.0).any() and (x == -25.0).any()                 # both clamps of the focal term are hit
        assert golden[name + "_grad32"].dtype == np.float32 and golden[name + "_grad64"].dtype == np.float64
    y = C.yardstick(golden)
    assert all(0 < v < 1e-3 for v in y.values()), y


# ---- identities of the script as executed -----------------------------------------------------------------------------------
def test_zero_labels_make_the_cross_entropy_the_constant_ln5(case):
    logits, msk, _ = case
    r = C.restate(logits, msk, np.zeros_like(msk[:, 0]))
    assert abs(r["parts"][5] - C.LN5) <= 4e-16 * C.LN5
    assert abs(C.LN5 - 1.6094379124341003) < 1e-15


def test_zero_labels_leave_the_gradient_of_the_five_combo_terms(case):
    logits, msk, _ = case
    zero = np.zeros_like(msk[:, 0])
    full, combo = C.restate(logits, msk, zero), C.restate(logits, msk, zero, combo_only=True)
    assert np.array_equal(full["grad"], combo["grad"])
    assert abs(full["loss"] - (combo["loss"] + 8 * C.LN5)) <= 1e-15 * full["loss"]
    damage = C.restate(logits, msk, C.damage_label(msk))
    assert np.abs(damage["grad"] - combo["grad"]).max() > 1e-3 * np.abs(combo["grad"]).max()      # with labels the term has one


def test_zero_labels_make_the_dice_meter_a_function_of_the_mask(case):
    logits, msk, _ = case
    r = C.restate(logits, msk, np.zeros_like(msk[:, 0]))
    T, N = float(msk[:, 0].sum()), msk[:, 0].size
    want = (T + 1e-6) / (0.5 * N + T + 1e-6)
    assert abs(r["parts"][6] - want) <= 1e-15 * want


def test_damage_label_is_the_first_set_channel(case):
    _, msk, lbl = case
    m = msk[:, 1:]
    assert np.array_equal(lbl, np.where(m.any(1), m.argmax(1) + 1, 0))
    two = (m.sum(1) > 1)
    assert two.any() and set(np.unique(lbl)) == {0, 1, 2, 3, 4}
    first = np.full(lbl.shape, 0)
    for c in (4, 3, 2, 1):
        first = np.where(msk[:, c] != 0, c, first)
    assert np.array_equal(lbl, first)


def test_a_label_above_4_is_counted_and_has_no_term(case):
    logits, msk, lbl = case
    bad = lbl.copy()
    bad[1, 3, 4] = 255
    r, clean = C.restate(logits, msk, bad), C.restate(logits, msk, lbl)
    assert r["parts"][7] == 1 and clean["parts"][7] == 0 and np.isfinite(r["grad"]).all() and math.isfinite(r["loss"])
    combo = C.restate(logits, msk, lbl, combo_only=True)
    assert np.array_equal(r["grad"][1, :, 3, 4], combo["grad"][1, :, 3, 4])


# ---- scheduler --------------------------------------------------------------------------------------------------------------
def test_unet_scheduler_has_the_scripts_milestones_and_gamma():
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=1e-4)
    sch = xbd.unet_scheduler(opt)
    assert isinstance(sch, torch.optim.lr_scheduler.MultiStepLR)
    assert sorted(sch.milestones.elements()) == [5, 11, 17, 23, 29, 33, 47, 50, 60, 70, 90, 110, 130, 150, 170, 180, 190]
    assert sch.gamma == 0.6
    for epoch in range(12):
        assert abs(opt.param_groups[0]["lr"] - 1e-4 * 0.6 ** ((epoch >= 5) + (epoch >= 11))) < 1e-18, epoch
        opt.step()
        sch.step()
    assert xbd.UNET_CHANNEL_WEIGHTS == (0.1, 0.1, 0.6, 0.3, 1.0) and xbd.UNET_CE_WEIGHTS == (0.01, 0.10, 1.0, 0.80, 1.0)
    assert xbd.UNET_CE_SCALE == 8.0


# ---- refusals ---------------------------------------------------------------------------------------------------------------
class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was touched: %s" % name)


class Reached(Exception):
    """the wrapper accepted its arguments and went on to its C entry"""


@pytest.fixture
def no_library(monkeypatch):
    def entry(name, *args):
        raise Reached(name)
    monkeypatch.setattr(_lib, "lib", lambda: NoLibrary())
    monkeypatch.setattr(ops, "_call", entry)
    monkeypatch.setattr(ops, "S", lambda: None)


def good():
    B, H, W = 2, 4, 6
    return {"logits": torch.zeros(B, 5, H, W), "msk": torch.zeros(B, 5, H, W, dtype=U8), "lbl": torch.zeros(B, H, W, dtype=U8),
            "labels": "lbl_msk", "weights_dev": torch.zeros(10)}


BAD = [("msk", lambda a: a["msk"].float(), "msk"),                                       # masks that are not uint8
       ("msk", lambda a: a["msk"].to(torch.int64), "msk"),
       ("logits", lambda a: torch.zeros(2, 4, 4, 6), "logits"),                          # a channel count other than 5
       ("logits", lambda a: torch.zeros(2, 5, 4, 6, dtype=torch.float64), "logits"),
       ("logits", lambda a: torch.zeros(0, 5, 4, 6), "logits"),
       ("msk", lambda a: torch.zeros(2, 5, 4, 7, dtype=U8), "msk"),                      # mismatched shapes
       ("msk", lambda a: torch.zeros(2, 4, 4, 6, dtype=U8), "msk"),
       ("lbl", lambda a: torch.zeros(2, 4, 7, dtype=U8), "lbl"),
       ("lbl", lambda a: torch.zeros(2, 1, 4, 6, dtype=U8), "lbl"),
       ("lbl", lambda a: torch.zeros(2, 4, 6, dtype=torch.int64), "lbl"),
       ("lbl", lambda a: None, "lbl"),                                                   # label_mode 0 without lbl
       ("labels", lambda a: "building", "labels"),
       ("weights_dev", lambda a: torch.zeros(5), "weights_dev")]


@pytest.mark.parametrize("which", ["fwd", "bwd"])
@pytest.mark.parametrize("arg,make,named", BAD)
def test_loss_wrappers_refuse_what_does_not_fit(no_library, which, arg, make, named):
    a = good()
    a[arg] = make(a)
    with pytest.raises(ValueError, match=named) as e:
        if which == "fwd":
            ops.xbd_unet_loss_fwd(a["logits"], a["msk"], a["lbl"], a["labels"], a["weights_dev"])
        else:
            ops.xbd_unet_loss_bwd(a["logits"], a["msk"], a["lbl"], a["labels"], torch.zeros(24), a["weights_dev"])
    assert "xbd_unet_loss_" + which in str(e.value)


def test_loss_wrappers_refuse_cpu_tensors_and_bad_sums(no_library):
    a = good()
    with pytest.raises(_lib.HipLibraryError, match="xbd_unet_loss_fwd"):           # everything fits, but nothing is on the GPU
        ops.xbd_unet_loss_fwd(a["logits"], a["msk"], a["lbl"], a["labels"], a["weights_dev"])
    with pytest.raises(_lib.HipLibraryError, match="xbd_unet_loss_fwd"):           # 'damage' does not need lbl
        ops.xbd_unet_loss_fwd(a["logits"], a["msk"], None, "damage", a["weights_dev"])
    with pytest.raises(_lib.HipLibraryError, match="xbd_unet_loss_bwd"):
        ops.xbd_unet_loss_bwd(a["logits"], a["msk"], a["lbl"], a["labels"], torch.zeros(24), a["weights_dev"], torch.ones(1))
    for sums in (None, torch.zeros(20), torch.zeros(24, dtype=torch.float64)):
        with pytest.raises(ValueError, match="sums"):
            ops.xbd_unet_loss_bwd(a["logits"], a["msk"], a["lbl"], a["labels"], sums, a["weights_dev"])
    with pytest.raises(ValueError, match="upstream"):
        ops.xbd_unet_loss_bwd(a["logits"], a["msk"], a["lbl"], a["labels"], torch.zeros(24), a["weights_dev"], torch.ones(2))


def test_unet_loss_refuses_cpu_tensors_and_float_masks(no_library):
    a = good()
    with pytest.raises(_lib.HipLibraryError):
        xbd.unet_loss(a["logits"], a["msk"], a["lbl"])
    with pytest.raises(ValueError, match="5 numbers"):
        xbd.unet_weights_dev("cpu", (1, 2, 3), xbd.UNET_CE_WEIGHTS)
    assert xbd.unet_weights_dev("cpu").tolist() == pytest.approx(list(xbd.UNET_CHANNEL_WEIGHTS + xbd.UNET_CE_WEIGHTS))


def test_step_constructor_refuses_what_does_not_fit(no_library):
    net, opt = types.SimpleNamespace(), types.SimpleNamespace(capturable=True)
    imgs, msks, lbl = torch.zeros(2, 6, 8, 8), torch.zeros(2, 5, 8, 8, dtype=U8), torch.zeros(2, 8, 8, dtype=U8)
    S = graph.GraphedXbdUnetStep
    for args, named in (((imgs, msks, lbl, "building"), "labels"),
                        ((imgs, msks, None, "lbl_msk"), "lbl_msk"),
                        ((imgs, msks.float(), lbl, "lbl_msk"), "msks"),
                        ((imgs, msks.float(), None, "damage"), "msks"),
                        ((imgs[:, :3], msks, lbl, "lbl_msk"), "imgs"),
                        ((imgs, msks[:, :4], lbl, "lbl_msk"), "msks"),
                        ((imgs, msks[:1], lbl, "lbl_msk"), "msks"),
                        ((imgs, msks, lbl[:, :4], "lbl_msk"), "lbl_msk"),
                        ((imgs, msks, lbl.float(), "lbl_msk"), "lbl_msk")):
        with pytest.raises(ValueError, match=named) as e:
            S(net, opt, *args)
        assert "GraphedXbdUnetStep" in str(e.value)
    with pytest.raises(_lib.HipLibraryError, match="GraphedXbdUnetStep"):           # everything fits, but on the CPU
        S(net, opt, imgs, msks, lbl)
    with pytest.raises(_lib.HipLibraryError, match="GraphedXbdUnetStep"):
        S(net, opt, imgs, msks, None, "damage")
    assert issubclass(S, graph.GraphedXbdStep)


# ---- the epoch --------------------------------------------------------------------------------------------------------------
class StubModel:
    def __init__(self):
        self.mode = None

    def train(self):
        self.mode = "train"


def stub_epoch(monkeypatch, rows, sizes, graph_flag=True):
    """train_epoch_unet with a stand-in step that answers row k = [loss, parts...] for batch k"""
    seen = []

    def stand_in(model, optimizer, first, labels, graph):
        seen.append((labels, graph))
        state = {"k": 0}

        def run(batch):
            r = torch.tensor(rows[state["k"]], dtype=F32)
            state["k"] += 1
            return r[0], r[1:]
        return run
    monkeypatch.setattr(xbd, "_unet_train_step", stand_in)
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=1e-4)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[1], gamma=0.6)
    batches = ({"img": torch.zeros(n, 6, 2, 2)} for n in sizes)
    return opt, sch, batches, seen


def test_train_epoch_unet_meters_are_average_meters_and_the_line_is_the_scripts(monkeypatch, capsys):
    rng = np.random.RandomState(3)
    n_steps = 70                                                   # past the first 64 rows of the device buffer
    rows = rng.rand(n_steps, 9).astype(np.float32)
    rows[:, 8] = 0
    sizes = [16] * (n_steps - 1) + [5]                             # a ragged last batch weighs less
    opt, sch, batches, seen = stub_epoch(monkeypatch, rows, sizes)
    model = StubModel()
    opt.step()
    m = xbd.train_epoch_unet(0, model, opt, sch, batches, labels="damage")
    w = np.asarray(sizes, dtype=np.float64)
    avg = lambda col: float((rows[:, col].astype(np.float64) * w).sum() / w.sum())
    assert model.mode == "train" and seen == [("damage", True)]
    assert m["steps"] == n_steps and m["samples"] == int(w.sum())
    for key, col in (("loss", 0), ("loss2", 3), ("loss3", 4), ("ce", 6), ("dice", 7)):
        assert abs(m[key] - avg(col)) <= 1e-12, key
    assert abs(m["lr"] - 0.6e-4) < 1e-18                           # the scheduler stepped: the rate of the next epoch
    line = "epoch: 0; lr {:.7f}; Loss {:.4f}; loss2 {:.4f}; Dice {:.4f}".format(0.6e-4, avg(0), avg(3), avg(7))
    assert capsys.readouterr().out == line + "\n"
    assert line.startswith("epoch: 0; lr 0.0000600; Loss ")


def test_train_epoch_unet_raises_for_a_counted_bad_label_and_for_no_batches(monkeypatch):
    rows = np.zeros((3, 9), dtype=np.float32)
    rows[1, 8] = 2
    opt, sch, batches, _ = stub_epoch(monkeypatch, rows, [4, 4, 4])
    with pytest.raises(IndexError, match="2 label bytes above 4"):
        xbd.train_epoch_unet(7, StubModel(), opt, sch, batches)
    assert opt.param_groups[0]["lr"] == 1e-4                       # the scheduler did not move
    opt, sch, batches, _ = stub_epoch(monkeypatch, rows, [])
    with pytest.raises(ValueError, match="no batches"):
        xbd.train_epoch_unet(0, StubModel(), opt, sch, batches)
    with pytest.raises(ValueError, match="labels"):
        xbd.train_epoch_unet(0, StubModel(), opt, sch, batches, labels="building")


def test_unet_val_batches_is_the_fixed_crop_in_order():
    calls = []

    class Pipe:
        def __len__(self):
            return 5

        def make_batch(self, ind, crop, params, train):
            calls.append((list(ind), crop, [list(r) for r in params], train))
            return len(calls)
    assert list(xbd.unet_val_batches(Pipe(), batch_size=2, crop=256)) == [1, 2, 3]
    row = [512, 512, 0, 0, 0, 0, 0, 256, 256]
    assert calls == [([0, 1], 256, [row, row], False), ([2, 3], 256, [row, row], False), ([4], 256, [row], False)]
