"""dahitra_amd.models.xbd_losses without a GPU: the numpy restatement the kernel tests use (tests/_xbd_losses_cases.py) against the
reference's recorded results (tests/golden/xbd_losses.npz, tools/make_xbd_losses_golden.py), the properties of the closed-form
gradient, the module's names and refusals, the header and the built library."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _xbd_losses_cases as K
from dahitra_amd import _lib
from dahitra_amd.models import xbd, xbd_losses

LOVASZ = {"lovasz": 0, "lovasz_sigmoid": 1}          # the mode the restatement is run in: the sigmoid term on the recorded probabilities
SYMBOLS = ("dh_xbd_lovasz_tile", "dh_xbd_lovasz_workspace_size", "dh_xbd_lovasz_fwd", "dh_xbd_lovasz_order",
           "dh_xbd_seg_terms_workspace_size", "dh_xbd_seg_terms_fwd", "dh_xbd_seg_terms_bwd")


@pytest.fixture(scope="module")
def gold():
    return K.golden()


def _recorded(gold, case, term, per_image):
    key = "%s_%s_%d_" % (case, term, per_image)
    return {k: gold[key + k] for k in ("loss32", "grad32", "loss64", "grad64")}


def _check(what, loss, grad, rec):
    """the rule of tests/_xbd_script_loss_checks.py:bounds -- loss within max(2 * yardstick, 2 ulp), gradient within twice the
    reference's own float32 distance from float64, as a share of the gradient's maximum"""
    l64, g64 = float(rec["loss64"]), rec["grad64"]
    yard_loss = abs(float(rec["loss32"]) - l64)
    yard_grad = float(np.abs(rec["grad32"].astype(np.float64) - g64).max() / np.abs(g64).max())
    d_loss = abs(loss - l64)
    d_grad = float(np.abs(grad - g64).max() / np.abs(g64).max())
    print("%s: loss off %.3e (bound %.3e), gradient %.3e (bound %.3e)" % (what, d_loss, K.loss_bound(l64, yard_loss), d_grad, 2 * yard_grad))
    assert d_loss <= K.loss_bound(l64, yard_loss), what
    assert d_grad <= 2 * yard_grad, what


@pytest.mark.parametrize("per_image", (0, 1))
@pytest.mark.parametrize("term", sorted(LOVASZ))
@pytest.mark.parametrize("case", ("plain", "void"))
def test_restatement_equals_the_reference_lovasz(gold, case, term, per_image):
    logits, targets = gold[case + "_logits"], gold[case + "_targets"]
    x = (logits if term == "lovasz" else gold[case + "_probs"])[:, None]
    r = K.lovasz(x, targets[:, None], LOVASZ[term], bool(per_image), 255)
    dx = r["dx"][:, 0]
    if term == "lovasz_sigmoid":          # the recorded gradient is with respect to the logits: through the recorded probabilities
        p = gold[case + "_probs"].astype(np.float64)
        dx = dx * p * (1.0 - p)
    assert r["gap"] > 0, "the fixture's errors are pairwise distinct"
    _check("%s %s per_image=%d" % (case, term, per_image), r["loss"], dx, _recorded(gold, case, term, per_image))


@pytest.mark.parametrize("per_image", (0, 1))
@pytest.mark.parametrize("k,term", list(enumerate(("jaccard", "bce", "mask_bceavg", "dice"))))
def test_restatement_equals_the_reference_terms(gold, k, term, per_image):
    r = K.seg_terms(gold["plain_logits"][:, None], gold["plain_targets"][:, None])
    _check("plain %s per_image=%d" % (term, per_image), float(r["terms"][0, k]), r["grads"][k][:, 0], _recorded(gold, "plain", term, per_image))


def test_fixture_holds_every_term_and_is_small(gold):
    for term in K.TERMS:
        for p in (0, 1):
            assert "plain_%s_%d_loss32" % (term, p) in gold.files
    assert os.path.getsize(K.GOLDEN) < 1 << 20


@pytest.mark.parametrize("n,ones", ((1, 0), (1, 1), (2, 1), (257, 0), (257, 257), (5000, 1800)))
def test_closed_form_equals_the_differences(n, ones):
    rng = np.random.default_rng(n + ones)
    lab = np.zeros(n, dtype=np.int64)
    lab[rng.permutation(n)[:ones]] = 1
    g = K.closed_form_g(lab)
    diff, jac = K.jaccard_differences(lab)
    assert np.abs(g - diff).max() <= 4 * np.finfo(np.float64).eps          # differences of numbers <= 1
    assert abs(g.sum() - jac[-1]) <= n * np.finfo(np.float64).eps          # g sums to the last Jaccard value
    assert (g >= 0).all()


@pytest.mark.parametrize("mode", (0, 1))
def test_loss_is_unchanged_inside_runs_of_equal_errors(mode):
    rng = np.random.default_rng(5)
    n = 3000
    t = (rng.random(n) < 0.4).astype(np.uint8)
    e = rng.integers(0, 40, n) / 16.0                    # many ties, exact in float32
    x = (np.where(t == 1, 1 - e, e - 1) if mode == 0 else np.where(t == 1, 1 - e, e)).astype(np.float32)
    x, t = x.reshape(1, 1, n), t.reshape(1, 1, n)
    base = K.lovasz(x, t, mode)
    order = base["order"].copy()
    err, _ = K.errors(x.reshape(-1), t.reshape(-1).astype(np.int64), mode)
    es = err[order]
    start = 0
    for stop in list(np.nonzero(np.diff(es))[0] + 1) + [n]:          # a random permutation inside every run
        order[start:stop] = rng.permutation(order[start:stop])
        start = stop
    assert not np.array_equal(order, base["order"])
    shuffled = K.lovasz(x, t, mode, order=order)
    assert abs(shuffled["loss"] - base["loss"]) <= 1e-13 * abs(base["loss"])
    assert np.abs(shuffled["dx"] - base["dx"]).max() > 0, "the gradient does depend on the order: it has to be defined"


def test_ignored_and_bad_targets_are_dropped():
    rng = np.random.default_rng(6)
    x = rng.standard_normal((2, 1, 50)).astype(np.float32)
    t = (rng.random((2, 1, 50)) < 0.5).astype(np.uint8)
    t[0] = 255                      # an image that is all void
    t[1, 0, 3] = 9                  # no label at all
    r = K.lovasz(x, t, 0, True, 255)
    keep = np.ones(50, dtype=bool)
    keep[3] = False
    alone = K.lovasz(x[1:, :, keep], t[1:, :, keep], 0, False, 255)
    assert r["bad"] == 1 and np.all(r["dx"][0] == 0) and r["dx"][1, 0, 3] == 0
    assert abs(r["loss"] - alone["loss"] / 2) < 1e-15          # the void image counts 0 in the mean over two images
    assert np.array_equal(r["order"][:50], np.arange(50))      # dropped elements keep index order


def test_module_exports_every_name_of_the_reference():
    missing = [n for n in K.names() if not hasattr(xbd_losses, n)]
    assert not missing, missing
    assert xbd_losses.eps == 1e-6


def test_cpu_tensors_raise():
    x, t = torch.zeros(2, 4, 4), torch.zeros(2, 4, 4)
    for call in (lambda: xbd_losses.ComboLoss({'lovasz': 1})(x, t), lambda: xbd_losses.lovasz_hinge(x, t),
                 lambda: xbd_losses.lovasz_sigmoid_flat(x.view(-1), t.view(-1)), lambda: xbd_losses.lovasz_grad(t.view(-1)),
                 lambda: xbd_losses.jaccard(x, t), lambda: xbd_losses.StableBCELoss()(x, t), lambda: xbd_losses.FocalLoss2d()(x, t),
                 lambda: xbd_losses.LovaszLoss()(x, t), lambda: xbd.xbd_loss(x[:, None], t[:, None], lovasz=0.5)):
        with pytest.raises(_lib.HipLibraryError):
            call()


def test_the_step_class_still_refuses_and_the_new_one_accepts():
    with pytest.raises(NotImplementedError):
        xbd.ComboLoss({'dice': 1, 'lovasz': 1})
    loss = xbd_losses.ComboLoss({'dice': 1, 'lovasz': 1}, per_image=True)
    assert loss.weights == {'dice': 1, 'lovasz': 1} and loss.values == {}
    with pytest.raises(KeyError):
        xbd_losses.ComboLoss({'hinge': 1})
    with pytest.raises(NotImplementedError):
        xbd_losses.jaccard(torch.zeros(1), torch.zeros(1), per_image=True)


def test_header_declares_and_library_exports_the_entries():
    protos = _lib.prototypes()
    for name in SYMBOLS:
        assert name in protos, name
    assert protos["dh_xbd_lovasz_tile"] == (ctypes.c_int, [])
    assert len(protos["dh_xbd_lovasz_fwd"][1]) == 17 and len(protos["dh_xbd_lovasz_order"][1]) == 13
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(dll, name), name


def test_sizes_and_refusals_of_the_size_query():
    L = _lib.lib()
    T = L.dh_xbd_lovasz_tile()
    assert T > 0 and T % 64 == 0
    n = ctypes.c_long(0)
    assert L.dh_xbd_lovasz_workspace_size(1, 1, ctypes.byref(n)) == 0 and n.value >= 16
    small = n.value
    assert L.dh_xbd_lovasz_workspace_size(1 << 30, 1, ctypes.byref(n)) == 0 and n.value > 16 * (1 << 30) > small
    for bad in ((0, 1), ((1 << 30) + 1, 1), (512, 257), (10, 3)):
        assert L.dh_xbd_lovasz_workspace_size(*bad, ctypes.byref(n)) != 0
        assert L.dh_last_error().decode().startswith("xbd_lovasz")
