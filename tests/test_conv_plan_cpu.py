"""The forward / data-gradient convolution's launch plan (dahitra_amd/csrc/conv_mfma.hip: conv_plan) against
tests/golden/conv_plan.npz.  The fixture was recorded from the library BEFORE the plan existed: a throwaway hook at each of its
five kernel-launch sites stored the template arguments, grid, workgroup and LDS bytes and returned before any HIP call, while
the C entry points were driven with non-null dummy pointers over the cases below.  The plan must take exactly those decisions.
Host code only: nothing here touches a device.

The fixture holds integer arrays: which cases the library refused, and one COLUMN per accepted launch (describe [30][launches]:
columns compress far better than rows).  The grid is the
issue's, thinned to keep the file small: every shape runs in bf16 under the default (wreg mode -1, 256 CUs); each fp32 mode, and
each further (wreg mode, CU count) pair of the bf16 3x3 layers, visits every fourth shape, rotating so that every shape is seen
by some of them; layers other than 3x3 / 1x1 stride 1 take four of the eight flag sets."""
import ctypes
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_plan.npz")
NS = (1, 2, 8, 64)
SPATIAL = (8, 16, 24, 32, 64, 128, 256)
CHANNELS = (16, 32, 64, 128, 256, 512, 1024)
COUTS = ((2, 16),) + tuple((c, c) for c in CHANNELS)            # (Cout, CoutPad)
GEOMETRIES = ((1, 1, 0, 1, 0), (1, 2, 0, 1, 0), (3, 1, 1, 1, 0), (3, 1, 2, 2, 0), (3, 2, 1, 1, 0), (4, 1, 2, 1, 0),
              (2, 1, 1, 1, 1), (2, 1, 1, 1, 2))                    # ks, stride, pad, dilation, phase mode
BF16, F32 = 1, 0
MODES = ((BF16, 0), (F32, 0), (F32, 1), (F32, 2), (F32, 3))       # dtype, dh_set_f32_mma_mode
WREG_CUS = ((-1, 256), (-1, 64), (0, 256), (1, 256), (1, 64), (0, 64))      # dh_conv_wreg_mode, CU count; the first is the default
RES, STATS, PREACT, GATE, IN_SCALE, W_FRAG, X_SPLIT, Y_SPLIT = (1 << i for i in range(8))
NONE, RELU, GELU = 0, 1, 2
# (flags, act, in_groups): none, residual + ReLU, stats, BatchNorm on load with 1 / 8 groups, fragment-order weights, the
# BatchNorm-backward gate (which needs the stats buffer), pre-activation copy + GELU
FLAG_SETS = ((0, NONE, 1), (RES, RELU, 1), (STATS, NONE, 1), (IN_SCALE, NONE, 1), (IN_SCALE, NONE, 8), (W_FRAG, NONE, 1),
             (GATE | STATS, NONE, 1), (PREACT, GELU, 1))
FAMILIES = {"TAP_BF16": 0, "TAP_F32": 1, "TAP_X3": 2, "TAP_X6": 3, "TAP_H3": 4, "GEMM": 5, "WREG64": 6, "WREG128": 7, "WREG256": 8,
            "WREG32": 9, "WREG32_UP4": 10}
FAMILY, NT, RW_T, LDS, RW, STATS_ROWS, NFIELDS = 0, 3, 4, 25, 28, 29, 30       # columns of a describe row
THIN = 4
KNOBS = ("DAHITRA_NO_WREG", "DAHITRA_UP4_", "DAHITRA_NO_GEMM1X1", "DAHITRA_GEMM1X1_", "DAHITRA_X_RW4", "DAHITRA_F32_MMA",
         "DAHITRA_NO_XCD_REMAP")


def shapes():
    return itertools.product(NS, SPATIAL, CHANNELS, COUTS)


def cases():
    """(wreg mode, f32 mma mode, the arguments of dh_conv2d_fwd_describe without `out`), grouped by the two modes"""
    for mi, (dtype, fmode) in enumerate(MODES):
        for wi, (wmode, cus) in enumerate(WREG_CUS if dtype == BF16 else WREG_CUS[:1]):
            variant = mi + wi                     # 0: bf16 under the default, every shape; the others every THIN-th, rotating
            for si, (n, s, cin, (cout, cpad)) in enumerate(shapes()):
                if variant and (si + variant) % THIN:
                    continue
                for ks, stride, pad, dil, phase in GEOMETRIES:
                    if wi and not (ks == 3 and stride == 1 and dil == 1):
                        continue                  # the register-resident-weights kernels serve these layers only
                    plain = (ks == 3 and dil == 1 or ks == 1) and stride == 1
                    h = s * stride
                    for flags, act, groups in (FLAG_SETS if plain else FLAG_SETS[:4]):
                        yield wmode, fmode, (0, dtype, n, h, h, cin, s, s, cout, cpad, ks, stride, pad, act, 0, 0, dil, 1, groups,
                                             phase, flags, cus)
    for (dtype, fmode), n, s, cin, cout, flags in itertools.product(MODES, (1, 8), (16, 24, 256), (32, 64), (2, 16), (0, IN_SCALE)):
        yield -1, fmode, (1, dtype, n, s, s, cin, s, s, cout, 16, 3, 1, 1, NONE, 0, 0, 1, 1, 2, 0, flags, 256)       # class head
    for (wmode, cus), n, s, (cin, cout, side), more in itertools.product(
            WREG_CUS, (2, 8, 64), (16, 24, 64, 128), ((256, 128, X_SPLIT), (128, 256, Y_SPLIT), (128, 64, X_SPLIT), (64, 64, X_SPLIT)),
            (0, W_FRAG, W_FRAG | STATS)):
        yield wmode, 0, (2, BF16, n, s, s, cin, s, s, cout, cout, 3, 1, 1, NONE, 0, 0, 1, 1, 1, 0, side | more, cus)   # split
    for (wmode, cus), n, s, act, flags in itertools.product(WREG_CUS, (1, 8, 32), (24, 64, 256), (NONE, RELU), (0, STATS)):
        yield wmode, 0, (3, BF16, n, s, s, 32, s, s, 32, 32, 3, 1, 1, act, 0, 0, 1, 1, 1, 0, flags, cus)               # up4 forward
    for dtype, n, s, k in itertools.product((BF16, F32), (1, 8, 32), (16, 24, 256), (32, 64, 128)):
        yield -1, 0, (4, dtype, n, s, s, k, s, s, 32, 32, 3, 1, 1, NONE, 0, 0, 1, 1, 1, 0, 0, 256)                     # up4 dgrad


def query_cases():
    """dh_conv2d_fwd_num_tiles over (dtype, mode) x N x size x Cin x (ks, stride); dh_conv3x3_split_supported over wreg mode x
    N x size x Cin x Cout"""
    tiles = [(fmode, (dtype, n, s, s, cin, ks, stride)) for (dtype, fmode), n, s, cin, (ks, stride) in
             itertools.product(MODES, NS, SPATIAL, CHANNELS, ((1, 1), (3, 1), (3, 2), (2, 1), (4, 1)))]
    split = [(wmode, (n, s, s, cin, cout)) for wmode, n, s, cin, cout in itertools.product((-1, 0, 1), NS, SPATIAL, CHANNELS, CHANNELS)]
    return tiles, split


def run(lib, describe):
    """every case through `describe` (all -1 where the launch is refused) and the two queries, under the modes each asks for"""
    out = (ctypes.c_int * NFIELDS)()
    rows, stats_tiles = [], []
    f0, w0 = lib.dh_get_f32_mma_mode(), lib.dh_conv_wreg_mode(-1)
    try:
        for (wmode, fmode), group in itertools.groupby(cases(), key=lambda c: c[:2]):
            lib.dh_conv_wreg_mode(wmode)
            lib.dh_set_f32_mma_mode(fmode)
            for _, _, a in group:
                rows.append(list(out) if describe(*a, out) == 0 else [-1] * NFIELDS)
                if a[20] & STATS:       # the rows callers size its stats_partial buffer with (split and up4 forward: bf16, 3x3, stride 1)
                    stats_tiles.append(lib.dh_conv2d_fwd_num_tiles(a[1], a[2], a[6], a[7], a[5], a[10], a[11]))
        tiles, split = query_cases()
        num_tiles, supported = [], []
        for fmode, a in tiles:
            lib.dh_set_f32_mma_mode(fmode)
            num_tiles.append(lib.dh_conv2d_fwd_num_tiles(*a))
        for wmode, a in split:
            lib.dh_conv_wreg_mode(wmode)
            supported.append(lib.dh_conv3x3_split_supported(*a))
    finally:
        lib.dh_set_f32_mma_mode(f0)
        lib.dh_conv_wreg_mode(w0)
    return {"describe": rows, "stats_tiles": stats_tiles, "num_tiles": num_tiles, "split_supported": supported}


def current():
    sys.path.insert(0, ROOT)
    from dahitra_amd import _lib
    lib = _lib.lib()
    return run(lib, lib.dh_conv2d_fwd_describe)


@pytest.fixture(scope="module")
def got():
    if not any(k.startswith(KNOBS) for k in os.environ):
        return current()
    # the library reads its switches once per process: ask a child that never saw them
    env = {k: v for k, v in os.environ.items() if not k.startswith(KNOBS)}
    return json.loads(subprocess.check_output([sys.executable, os.path.abspath(__file__)], env=env))


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as g:
        rows = np.full((len(g["refused"]), NFIELDS), -1)
        rows[~g["refused"]] = g["describe"].T
        return {"describe": rows.tolist(), "num_tiles": g["num_tiles"].tolist(), "split_supported": g["split_supported"].tolist()}


def test_plan_chooses_the_recorded_family_and_geometry(got, gold):
    assert len(got["describe"]) == len(gold["describe"]) == sum(1 for _ in cases())
    bad = [(c, a, b) for c, a, b in zip(cases(), got["describe"], gold["describe"]) if a != b]
    assert not bad, "%d rows differ, first (case, got, recorded): %s" % (len(bad), bad[:3])


def test_shape_queries_keep_their_values(got, gold):
    tiles, split = query_cases()
    assert len(got["num_tiles"]) == len(gold["num_tiles"]) == len(tiles)
    bad = [(c, a, b) for c, a, b in zip(tiles, got["num_tiles"], gold["num_tiles"]) if a != b]
    assert not bad, "%d tile counts differ, first (case, got, recorded): %s" % (len(bad), bad[:3])
    assert len(got["split_supported"]) == len(gold["split_supported"]) == len(split)
    bad = [(c, a, b) for c, a, b in zip(split, got["split_supported"], gold["split_supported"]) if a != b]
    assert not bad, "%d split answers differ, first (case, got, recorded): %s" % (len(bad), bad[:3])
    assert {0, 1} == set(gold["split_supported"])


def test_stats_rows_are_what_num_tiles_sizes_the_buffer_with(got, gold):
    """Three kernel families write stats_partial, each with its own row arithmetic (the tap kernel's grid x, the weights-resident
    stream's units, the GEMM's 128-pixel halves): every one indexes exactly dh_conv2d_fwd_num_tiles rows -- in the recorded
    launches as in the plan's, for dh_conv2d_fwd, the split form (whose stream pairs tiles where the rule says 16 rows) and the
    bilinear-x4 forward (8-row tiles whatever the shape) alike"""
    for rows in (got["describe"], gold["describe"]):
        with_stats = [r for (_, _, a), r in zip(cases(), rows) if a[20] & STATS]
        assert len(with_stats) == len(got["stats_tiles"]) > 1000
        bad = [(r, t) for r, t in zip(with_stats, got["stats_tiles"]) if r[FAMILY] >= 0 and r[STATS_ROWS] != t]
        assert not bad, "%d launches index other rows than the query counts, first (row, query): %s" % (len(bad), bad[:3])
        assert {r[FAMILY] for r in with_stats} >= {FAMILIES[f] for f in ("TAP_BF16", "TAP_X3", "GEMM", "WREG64", "WREG128", "WREG256", "WREG32",
                                                                        "WREG32_UP4")}


def test_every_family_and_both_outcomes_of_the_split_precision_fit_appear_in_the_fixture(gold):
    assert {r[FAMILY] for r in gold["describe"]} - {-1} == set(FAMILIES.values())
    # an fp32 launch in a split mode with whole 32-channel chunks: its planes fit the LDS at some tile width, or it runs exact
    split = [r[FAMILY] for (_, fmode, a), r in zip(cases(), gold["describe"]) if a[1] == F32 and fmode and a[5] % 32 == 0 and r[FAMILY] >= 0]
    assert {FAMILIES["TAP_F32"], FAMILIES["TAP_X3"], FAMILIES["TAP_X6"], FAMILIES["TAP_H3"]} == set(split)


if __name__ == "__main__":
    json.dump(current(), sys.stdout)
