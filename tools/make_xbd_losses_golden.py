#!/usr/bin/env python
"""Write tests/golden/xbd_losses.npz and tests/golden/xbd_losses_names.json FROM THE REFERENCE's xBD_code/losses.py (needs the
reference tree; no GPU), for tests/test_xbd_losses_cpu.py and tests/test_xbd_losses_gpu.py to hold dahitra_amd's restatement,
kernels and dahitra_amd.models.xbd_losses to.  losses.py is loaded by path (it imports numpy and torch only), as
tools/make_adapt_loss_golden.py does.  Inputs and results only: no program text of the reference is written.

Cases, logits [2, 24, 20] with pairwise distinct errors in every sort (asserted):
    plain    targets 0 / 1; every term of ComboLoss, per_image False and True
    void     the same with 255s sprinkled in and two rows of image 0 entirely 255; the two Lovasz terms only (the other terms of
             the reference read a 255 as the number 255, or, focal, drop it: nothing a mask of the loaders holds)
Per case <c>, term <k>, per_image <p> in (0, 1):
    <c>_<k>_<p>_loss32, _grad32   ComboLoss({k: 1}, per_image=p)(logits, targets) and d loss / d logits, float32 on the CPU
    <c>_<k>_<p>_loss64, _grad64   the yardstick, float64.  For dice, focal and jaccard: the reference's own code run on float64
                                  logits.  For bce and mask_bceavg, whose classes cast to float32 themselves: their expressions
                                  on float64 logits.  For the two Lovasz terms the reference's code cannot serve (lovasz_grad casts to
                                  float32 inside), so the same expressions are evaluated here in float64 on the reference's OWN
                                  float32 errors and ITS sort order: cumulative sums, 1 - I / U, its differences, the dot product,
                                  and the chain rule through relu / abs / the float32 sigmoid the reference took.
    <c>_logits fp32, <c>_targets uint8, <c>_probs fp32 (torch.sigmoid(logits), what the sigmoid terms were handed)

    python tools/make_xbd_losses_golden.py [--reference DIR]       # DIR defaults to $DAHITRA_REFERENCE"""
import argparse
import importlib.util
import inspect
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (2, 24, 20)
TERMS = ("bce", "dice", "focal", "jaccard", "lovasz", "lovasz_sigmoid", "mask_bceavg")


def inputs(seed, void):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(*SHAPE, generator=g) * 2.5
    targets = (torch.rand(*SHAPE, generator=g) < 0.4).to(torch.uint8)
    if void:
        targets[torch.rand(*SHAPE, generator=g) < 0.1] = 255
        targets[0, :2] = 255
    return logits, targets


def lovasz64(L, logits, targets, sigmoid, per_image):
    """float64 loss and gradient of the reference's lovasz / lovasz_sigmoid term on its own float32 errors and sort order, the
    chain rule in float64 too: relu' / sign as torch has them, the sigmoid's slope p (1 - p) from the float32 p the reference took"""
    x32 = logits.detach()
    p32 = torch.sigmoid(x32)
    grad = torch.zeros(x32.shape, dtype=torch.float64)
    total, count = 0.0, 0
    groups = [(slice(b, b + 1),) for b in range(x32.shape[0])] if per_image else [(slice(None),)]
    for sel in groups:
        count += 1
        xs, ps, ts = x32[sel].reshape(-1), p32[sel].reshape(-1), targets[sel].reshape(-1)
        valid = ts != 255
        idx = torch.nonzero(valid).reshape(-1)
        lab = ts[idx].float()
        if idx.numel() == 0:
            continue
        errors32 = (lab - ps[idx]).abs() if sigmoid else 1. - xs[idx] * (2. * lab - 1.)
        assert torch.unique(errors32).numel() == errors32.numel(), "errors are not distinct"
        _, perm = torch.sort(errors32, dim=0, descending=True)
        gt = lab[perm].double()
        inter = gt.sum() - gt.cumsum(0)
        union = gt.sum() + (1 - gt).cumsum(0)
        jac = 1. - inter / union
        jac[1:] = jac[1:] - jac[:-1].clone()
        e = errors32.double()[perm]
        total = total + float(torch.dot(torch.relu(e) if not sigmoid else e, jac))
        if sigmoid:
            pd = ps[idx][perm].double()
            slope = -torch.sign(gt - pd) * pd * (1 - pd)
        else:
            slope = torch.where(e > 0, -(2. * gt - 1.), torch.zeros_like(e))
        g = torch.zeros(xs.numel(), dtype=torch.float64)
        g[idx[perm]] = jac * slope
        grad[sel] += g.reshape(grad[sel].shape)
    return np.asarray(total / count, dtype=np.float64), (grad / count).numpy()


def cast_terms64(term, logits, targets):
    """bce and mask_bceavg in float64: the reference's StableBCELoss and MaskLoss cast their input to float32 themselves, so its
    own code cannot serve; the expressions of losses.py:74-92 on float64 logits, the gradient by autograd"""
    x = logits.detach().clone().double().requires_grad_(True)
    t = targets.double().view(-1)
    v = x.view(-1)
    if term == "bce":
        loss = (v.clamp(min=0) - v * t + (1 + (-v.abs()).exp()).log()).mean()
    else:
        loss = torch.nn.functional.binary_cross_entropy(torch.sigmoid(v), t)
    loss.backward()
    return np.asarray(loss.item(), dtype=np.float64), x.grad.numpy().astype(np.float64)


def evaluate(L, term, per_image, logits, targets, dtype):
    loss_fn = L.ComboLoss({term: 1}, per_image=per_image)
    x = logits.detach().clone().to(dtype).requires_grad_(True)
    loss = loss_fn(x, targets)
    loss.backward()
    np_dtype = np.float32 if dtype == torch.float32 else np.float64
    return np.asarray(loss.item(), dtype=np_dtype), x.grad.numpy().astype(np_dtype)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", default=os.environ.get("DAHITRA_REFERENCE"), help="the reference tree (holds xBD_code/losses.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "xbd_losses.npz"))
    ap.add_argument("--names", default=os.path.join(ROOT, "tests", "golden", "xbd_losses_names.json"))
    args = ap.parse_args()
    path = os.path.join(args.reference or "", "xBD_code", "losses.py")
    if not os.path.exists(path):
        sys.exit("no xBD_code/losses.py under --reference / $DAHITRA_REFERENCE (%r)" % args.reference)
    spec = importlib.util.spec_from_file_location("_reference_xbd_losses", path)
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)
    torch.set_num_threads(1)              # one summation order for the float32 sums, whatever the machine

    # the names the file itself defines: its functions and classes, and `eps`
    public = sorted(n for n, v in vars(L).items() if not n.startswith("_") and
                    ((inspect.isfunction(v) or inspect.isclass(v)) and v.__module__ == L.__name__ or n == "eps"))
    json.dump(public, open(args.names, "w"), indent=1)
    print("%s: %d names" % (args.names, len(public)))

    data = {"torch_version": np.array(torch.__version__)}
    for case, seed, void in (("plain", 41, False), ("void", 42, True)):
        logits, targets = inputs(seed, void)
        data.update({case + "_logits": logits.numpy(), case + "_targets": targets.numpy(), case + "_probs": torch.sigmoid(logits).numpy()})
        for term in TERMS:
            if void and not term.startswith("lovasz"):
                continue
            for p in (0, 1):
                l32, g32 = evaluate(L, term, bool(p), logits, targets, torch.float32)
                if term.startswith("lovasz"):
                    l64, g64 = lovasz64(L, logits, targets, term == "lovasz_sigmoid", bool(p))
                elif term in ("bce", "mask_bceavg"):
                    l64, g64 = cast_terms64(term, logits, targets)
                else:
                    l64, g64 = evaluate(L, term, bool(p), logits, targets, torch.float64)
                key = "%s_%s_%d_" % (case, term, p)
                data.update({key + "loss32": l32, key + "grad32": g32, key + "loss64": l64, key + "grad64": g64})
                print("%s%s float32 against float64: loss %.3e (relative), gradient %.3e of its maximum %.3e"
                      % (key, " " * (28 - len(key)), abs(float(l32) - float(l64)) / abs(float(l64)),
                         float(np.abs(g32.astype(np.float64) - g64).max() / np.abs(g64).max()), float(np.abs(g64).max())))
    for v in data.values():
        assert v.dtype != object
    np.savez_compressed(args.out, **data)
    print("%s: %d arrays, %d bytes" % (args.out, len(data), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
