"""What the kernel tests of the two script losses (test_xbd_unet_step_gpu.py, test_xbd_adapt_gpu.py; csrc/xbd_script_loss.hip) share:
the bound rule, the distances of a kernel result from its float64 reference and the check of both.  A result is (loss, parts,
gradient) on the host; the parts are nc channel losses, the cross-entropy and, with `dice`, the Dice meter."""
import numpy as np

ULP = 2.0 ** -23


def bounds(yardstick):
    """twice the reference's own float32 error per quantity (a `yardstick` of the cases modules), and for the quantities that are
    single floats or nearly so -- all but 'loss' and 'grad' -- not less than two float32 ulp"""
    return {k: 2 * (v if k in ("loss", "grad") else max(v, ULP)) for k, v in yardstick.items()}


def distances(got, ref, nc, dice):
    loss, parts, grad = got
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b) / np.abs(b)))
    d = {"loss": rel(loss, ref["loss"]), "channel": rel(parts[:nc], ref["parts"][:nc]), "ce": rel(parts[nc], ref["parts"][nc])}
    if dice:
        d["dice"] = rel(parts[nc + 1], ref["parts"][nc + 1])
    d["grad"] = float(np.abs(grad.astype(np.float64) - ref["grad"]).max() / np.abs(ref["grad"]).max())
    return d


def check(what, got, ref, bounds, nc, dice, last):
    """every distance printed, then asserted under its bound; the last entry of parts equals `last` exactly"""
    d = distances(got, ref, nc, dice)
    print("%s: %s" % (what, ", ".join("%s %.3e (bound %.3e)" % (k, v, bounds[k]) for k, v in d.items())))
    assert got[1][-1] == last, what
    for k, v in d.items():
        assert v <= bounds[k], (what, k, v, bounds[k])
