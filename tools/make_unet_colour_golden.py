#!/usr/bin/env python
"""Write tests/golden/xbd_unet_colour.npz FROM THE REFERENCE's xBD_code/utils.py (needs the reference tree; no GPU): what its
saturation, brightness, contrast and gauss_noise return on a few seeded images, for tests/test_xbd_unet_colour_cpu.py to hold
datasets/xbd_pipeline's restatements to.  The file is loaded by path (it imports numpy and torch only; its cv2 functions are not
called).  The script's images are BGR: the fixture stores the images as the reference took them, `bgr_<i>`, and its outputs as
`blend_<i>` [3 operations (OPS), 5 factors, h, w, 3] and `gauss_noise_<i>` [seeds, h, w, 3] (np.random.seed(k) before each call).

    python tools/make_unet_colour_golden.py [--reference DIR]       # DIR defaults to $DAHITRA_REFERENCE
"""
import argparse
import importlib.util
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((24, 20), (33, 33))
NOISE_SEEDS = (0, 7)
OPS = ("saturation", "brightness", "contrast")


def images():
    out = []
    for i, (h, w) in enumerate(SIZES):
        img = np.random.RandomState(100 + i).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        edge = np.array([0, 1, 127, 128, 254, 255], dtype=np.uint8)
        img[:6, :6] = edge[:, None, None]                                   # greys, and bytes that clip at either end
        img[6:12, :6, 0], img[6:12, :6, 2] = edge[:, None], edge[None, :]
        out.append(img)
    return out


def factors():
    rng = random.Random(11)
    return [0.9, 1.0, 1.0999] + [0.9 + rng.random() * 0.2 for _ in range(2)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", default=os.environ.get("DAHITRA_REFERENCE"), help="the reference tree (holds xBD_code/utils.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "xbd_unet_colour.npz"))
    args = ap.parse_args()
    if not args.reference or not os.path.exists(os.path.join(args.reference, "xBD_code", "utils.py")):
        sys.exit("no xBD_code/utils.py under --reference / $DAHITRA_REFERENCE (%r)" % args.reference)
    spec = importlib.util.spec_from_file_location("_reference_xbd_utils", os.path.join(args.reference, "xBD_code", "utils.py"))
    utils = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(utils)

    data = {"factors": np.array(factors(), dtype=np.float64), "noise_seeds": np.array(NOISE_SEEDS, dtype=np.int64),
            "numpy_version": np.array(np.__version__)}
    for i, bgr in enumerate(images()):
        data["bgr_%d" % i] = bgr
        data["blend_%d" % i] = np.stack([np.stack([getattr(utils, op)(bgr.copy(), alpha) for alpha in factors()]) for op in OPS])
        noisy = []
        for seed in NOISE_SEEDS:
            np.random.seed(seed)
            noisy.append(utils.gauss_noise(bgr.copy()))
        data["gauss_noise_%d" % i] = np.stack(noisy)
    for v in data.values():
        assert v.dtype != object and (v.dtype == np.uint8 or v.ndim <= 1)
    np.savez_compressed(args.out, **data)
    print("%s: %d arrays, %d bytes" % (args.out, len(data), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
