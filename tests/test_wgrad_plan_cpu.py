"""The weight gradient's launch plan (dahitra_amd/csrc/conv_wgrad.hip: wg_plan) against tests/golden/wgrad_plan.npz, which
was recorded from the library BEFORE the plan existed: the five public shape queries straight from that build, and -- through a
print in its launch functions -- the kernel family, tiles, split-K, grid and LDS of every launch of the grid below.  The plan
must take exactly those decisions.  Host code only: nothing here touches a device.

The fixture holds integer arrays, one COLUMN per row of each array (queries [4][shapes], describe [12][launches]: columns
compress to a fifth of the row-major form), and the phase workspace sizes."""
import ctypes
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "wgrad_plan.npz")
NS = (2, 8, 64)
SPATIAL = (8, 16, 32, 64, 128, 256)
CHANNELS = (16, 32, 64, 128, 256, 512, 1024, 2048)
BF16, F32 = 1, 0
FAMILIES = {"W1": 0, "WS": 1, "WS_BATCH": 2, "C32_BATCH": 3, "GENERIC": 4, "PHASE": 5}
KNOBS = ("DAHITRA_WGRAD_", "DAHITRA_W1_")


def shapes():
    for n, s, cin, cout in itertools.product(NS, SPATIAL, CHANNELS, CHANNELS):
        for ks in (1, 3, 4):
            for groups in ((1, n) if ks == 1 else (1,)):
                yield n, s, cin, cout, ks, groups


def query_rows(lib):
    """[splitk, workspace bytes, 1x1 blocks, split supported] per shape; the phase workspace over Cin 32 / 64"""
    rows = [[lib.dh_conv2d_wgrad_splitk(n, s, s, cin, cout, ks, g), lib.dh_conv2d_wgrad_workspace_size(n, s, s, cin, cout, ks, g),
             lib.dh_conv2d_wgrad_1x1_blocks(n, s, s, cin, cout), lib.dh_conv3x3_split_supported(n, s, s, cin, cout)]
            for n, s, cin, cout, ks, g in shapes()]
    phase = [lib.dh_conv2d_wgrad_phase_workspace_size(n, s, s, cin) for n in NS for s in SPATIAL for cin in (32, 64)]
    return rows, phase


def describe_rows(lib, describe):
    """`describe`'s 12 ints (all -1 where the library refuses the launch) over the shapes x (bf16, f32, f32 in mma mode 1) x
    stride x dilation x (plain, scale / shift on load, split input) x batch (closed, open), then the phase form (ks = 2)"""
    out = (ctypes.c_int * 12)()
    rows = []

    def row(*a):
        rows.append(list(out) if describe(*a, out) == 0 else [-1] * 12)

    try:
        for dtype, mode in ((BF16, 0), (F32, 0), (F32, 1)):
            lib.dh_set_f32_mma_mode(mode)
            for n, s, cin, cout, ks, g in shapes():
                for stride, dil, inp, batch in itertools.product((1, 2), (1, 2), (0, 1, 2), (0, 1)):
                    if dil == 2 and (ks != 3 or stride != 1):
                        continue                          # the library has dilation 2 for 3x3 / stride 1 only
                    if ks == 4 and stride == 2:
                        continue                          # the 4x4 form is the stride-1 stem
                    if inp and g != 1:
                        continue                          # the on-load forms take one weight group
                    if inp == 2 and not (dtype == BF16 and ks == 3 and stride == 1 and dil == 1):
                        continue                          # a split input: dh_conv2d_wgrad_split is bf16, 3x3, stride 1, undilated
                    pad = {1: 0, 3: dil, 4: 2}[ks]
                    h = s if ks == 4 else s * stride
                    row(dtype, 0, n, h, h, cin, s, s, cout, ks, stride, pad, g, 0, 1, 0, 0, dil, 2, int(inp == 1), int(inp == 2), batch)
            for n, s, cin in itertools.product(NS, SPATIAL, (32, 64)):
                row(dtype, 0, n, s, s, cin, s, s, 32, 2, 1, 1, 1, 0, 1, 0, 0, 1, 1, 0, 0, 0)
    finally:
        lib.dh_set_f32_mma_mode(0)
    return rows


def current():
    sys.path.insert(0, ROOT)
    from dahitra_amd import _lib
    lib = _lib.lib()
    queries, phase = query_rows(lib)
    return {"queries": queries, "phase": phase, "describe": describe_rows(lib, lib.dh_conv2d_wgrad_describe)}


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
        return {"queries": g["queries"].T.tolist(), "describe": g["describe"].T.tolist(), "phase": g["phase"].tolist()}


def test_public_shape_queries_keep_their_values(got, gold):
    assert len(got["queries"]) == len(gold["queries"]) == len(list(shapes()))
    bad = [(s, a, b) for s, a, b in zip(shapes(), got["queries"], gold["queries"]) if a != b]
    assert not bad, "%d rows differ, first (shape, got, recorded): %s" % (len(bad), bad[:3])
    assert got["phase"] == gold["phase"]


def test_plan_chooses_the_recorded_family_and_geometry(got, gold):
    assert len(got["describe"]) == len(gold["describe"])
    bad = [(i, a, b) for i, (a, b) in enumerate(zip(got["describe"], gold["describe"])) if a != b]
    assert not bad, "%d rows differ, first (row, got, recorded): %s" % (len(bad), bad[:3])


def test_1x1_blocks_is_zero_where_the_launch_goes_direct():
    """Beyond the recorded grid (4096 channels, one 7 x 7 image): split-K is 1, so the launch writes dW directly through
    conv_wgrad_kernel; the query says 0 there (it said 512, the blocks wgrad1x1_kernel would have had, before it read the plan)"""
    sys.path.insert(0, ROOT)
    from dahitra_amd import _lib
    lib, out = _lib.lib(), (ctypes.c_int * 12)()
    assert lib.dh_conv2d_wgrad_describe(BF16, 0, 1, 7, 7, 4096, 7, 7, 4096, 1, 1, 0, 1, 0, 1, 0, 0, 1, 1, 0, 0, 0, out) == 0
    assert (out[0], out[5], out[6]) == (FAMILIES["GENERIC"], 1, 1)
    assert lib.dh_conv2d_wgrad_1x1_blocks(1, 7, 7, 4096, 4096) == 0


def test_every_family_appears_in_the_fixture(gold):
    assert {r[0] for r in gold["describe"]} - {-1} == set(FAMILIES.values())


if __name__ == "__main__":
    json.dump(current(), sys.stdout)
