"""Cases shared by test_xbd_unet_colour_cpu.py and test_xbd_unet_colour_gpu.py: the colour stage of
xBD_code/train_unettransformer.py (lines 211-244) on the device (dh_xbd_unet_colour_u8, datasets/xbd_pipeline.make_unet_batch).

    lattice          the colours change_hsv is tested on: greys, V == 0, all six channel orders, two-channel ties, 0 and 255
    lattice_image    the lattice as an S x S image
    colour_batch     the colour dicts every shape is tested with: every operation alone, change_hsv followed by each block
                     operation, both images of one sample, and samples without a job
    HSV_SHIFTS       the (h, s, v) the lattice is shifted by
"""
import itertools

import numpy as np

from dahitra_amd.datasets import xbd_pipeline as X

LEVELS = (0, 1, 64, 127, 128, 254, 255)
FACTORS = (0.9, 1.0, 1.0999, 0.9 + 0.2 * 0.6394267984578837)          # the ends of the script's range and a drawn one
HSV_SHIFTS = ((0, 0, 0), (5, -5, 5), (-5, 5, -5), (3, 0, -2), (0, -255, 0), (100, 4, 1), (-255, 255, -255), (255, 255, 255))


def lattice():
    """[n, 3] uint8 R, G, B: every triple of LEVELS (all six orders of three different levels, every two-channel tie, the greys
    of the levels, black and white) and the 256 greys"""
    cube = np.array(list(itertools.product(LEVELS, repeat=3)), dtype=np.uint8)
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    return np.concatenate([cube, grey])


def lattice_image(S):
    """the lattice, repeated, as an [S, S, 3] image (S = 33 holds all of it)"""
    lat = lattice()
    return np.ascontiguousarray(lat[np.arange(S * S) % len(lat)].reshape(S, S, 3))


def empty():
    return {"hsv": None, "pre": None, "post": None}


def colour_batch(S, seed=5):
    """one colour dict (or None) per sample"""
    rng = np.random.RandomState(seed)
    noise = lambda: X.draw_unet_noise(rng, S)
    value = {"gauss_noise": noise, "blur": lambda: None, "saturation": lambda: FACTORS[0], "brightness": lambda: FACTORS[2],
             "contrast": lambda: FACTORS[3]}
    ops = list(X.UNET_COLOUR_OPS)
    batch = []
    for i, op in enumerate(ops):                                               # every operation alone, pre and post in turn
        batch.append(dict(empty(), **{("pre", "post")[i % 2]: (op, value[op]())}))
    batch.append(None)                                                         # no job
    batch.append(dict(empty(), hsv=(1, 5, -5, 3)))                             # change_hsv alone
    batch.append(dict(empty(), hsv=(2, -5, 5, -5)))
    for i, op in enumerate(ops):                                               # change_hsv, then each block operation
        im = ("post", "pre")[i % 2]
        batch.append(dict(empty(), hsv=(1 + (im == "post"), 4 - i, i - 2, (-3) ** (i % 2)), **{im: (op, value[op]())}))
    batch.append(empty())                                                      # no job
    # both images of one sample: change_hsv and blur on one, contrast / noise / saturation at another factor on the other
    batch.append({"hsv": (1, -2, 3, 5), "pre": ("blur", None), "post": ("contrast", FACTORS[0])})
    batch.append({"hsv": (2, 2, -3, -5), "pre": ("gauss_noise", noise()), "post": ("saturation", FACTORS[2])})
    batch.append({"hsv": None, "pre": ("contrast", FACTORS[1]), "post": ("brightness", FACTORS[0])})
    return batch
