"""The fused decoder's launch plan (dahitra_amd/csrc/decoder_fused.hip: dec_plan_launch) against tests/golden/decoder_plan.npz.
The fixture was recorded from the library BEFORE the plan existed: a throwaway hook at each of its launch sites stored the
kernel, grid, workgroup, LDS bytes and every job's block layout and returned before any HIP call, the CU count came from the
case, and the real entry points (layer / stack, forward / backward, finalize; eager and between dh_decoder_batch_begin and
_launch) were driven with non-null dummy pointers over the cases below.  dh_decoder_plan_describe must take exactly those
decisions.  Host code only: nothing here touches a device.

The library reads its DAHITRA_DEC_* switches once per process, so every setting -- the default included -- is asked of a child
process that sees that setting and no other.  The default run takes every case, each switch every fifth, rotating.

The fixture holds integer arrays: which rows were refused, one COLUMN per accepted launch (describe [41][launches]) and the
dh_decoder_layer_bwd_workspace_size answers of every run."""
import ctypes
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "decoder_plan.npz")
RPI = (128, 256, 512, 1024, 4096, 16384, 65536, 192)          # rows per image; 192 is refused
IMAGES = (1, 2, 3, 4, 6, 8, 16, 32, 64)
DEPTHS = (1, 2, 4, 8, 9)                                        # 9 is refused for stacks
MLPS = (32, 64, 48)                                             # 48 is refused
CUS = (0, 64, 256, 304)
RUNS = ({}, {"DAHITRA_DEC_BALANCE": "0"}, {"DAHITRA_DEC_UPB_BWD": "3"}, {"DAHITRA_DEC_UPB_FWD": "8"}, {"DAHITRA_DEC_NO_SORT": "1"},
        {"DAHITRA_DEC_BWD_MAXRPB64": "512"}, {"DAHITRA_DEC_FWD_MINBLK": "256"})
THIN = 5
PL_SIZE = {32: 4320, 64: 6400}                                  # floats of one workgroup's partial (PL<MLP>::SIZE)
# out[41] of dh_decoder_plan_describe
FAMILY, GRID, THREADS, LDS, NJOBS, JOB0, FIN0, NFIELDS = 0, 1, 2, 3, 4, 5, 25, 41
SRC, UPB, BPI, FIRST, BLOCKS = range(5)                         # + JOB0 + 5 j
WS, FIN_NBLK, FIN_BPI, FIN_GRID = range(4)                      # + FIN0 + 4 j


def all_cases():
    """(backward, stack, mlp, batch open, ((images, rows per image, depth), ...), CU count)"""
    out = []
    # single launches, eager and as the only job of an open batch; depth and CU count rotate
    for i, (rpi, images, mlp, bwd, stack, batch) in enumerate(itertools.product(RPI, IMAGES, MLPS[:2], (0, 1), (0, 1), (0, 1))):
        out.append((bwd, stack, mlp, batch, ((images, rpi, DEPTHS[i % 5]),), CUS[(i // 5) % 4]))
    sets = []
    for i, images in enumerate(IMAGES):                         # DAHiTra's three levels, in both orders
        d = DEPTHS[i % 4]
        sets += [((images, 256, d), (images, 1024, d), (images, 4096, d)), ((images, 4096, d), (images, 1024, d), (images, 256, d))]
    for i, (ra, rb) in enumerate(itertools.product(RPI[:7], RPI[:7])):          # every ordered pair of sizes
        sets.append(((IMAGES[i % 9], ra, DEPTHS[i % 4]), (IMAGES[(i // 3) % 9], rb, DEPTHS[(i // 2) % 4])))
    four = ((2, 128, 8), (16, 512, 1), (1, 16384, 2), (8, 1024, 4))
    more = ((1, 65536, 1), (64, 128, 4), (32, 256, 2), (6, 4096, 8))
    sets += [four, four[::-1], more, more[::-1], four[:3], more[1:], four + more[:1],            # ... and a fifth job: refused
             ((4, 256, 2), (4, 192, 2)), ((4, 256, 9), (4, 1024, 2)), ((64, 4096, 4), (64, 1024, 4), (64, 256, 4), (3, 512, 1))]
    for ci, (cus, bwd, stack, mlp) in enumerate(itertools.product(CUS, (0, 1), (0, 1), MLPS[:2])):
        for si, jobs in enumerate(sets):
            if len(jobs) != 2 or si >= len(sets) - 3 or (si + ci) % 2 == 0:          # the pairs of sizes: every other one, rotating
                out.append((bwd, stack, mlp, 1, jobs, cus))
    out += [(bwd, stack, MLPS[2], batch, sets[0][:1 if not batch else 3], 256) for bwd, stack, batch in itertools.product((0, 1), (0, 1), (0, 1))]
    return out


def cases(run):
    return [c for i, c in enumerate(all_cases()) if run == 0 or (i + run) % THIN == 0]


def size_queries():
    return list(itertools.product(RPI[:7], IMAGES, (32, 64)))


def run_cases(lib, describe, run):
    """every case of `run` through `describe` (all -1 where the launch is refused), and the workspace sizes"""
    out = (ctypes.c_long * NFIELDS)()
    rows = []
    for bwd, stack, mlp, batch, jobs, cus in cases(run):
        n = len(jobs)
        a = ((ctypes.c_long * n)(*(im * rpi for im, rpi, _ in jobs)), (ctypes.c_int * n)(*(rpi for _, rpi, _ in jobs)),
             (ctypes.c_int * n)(*(d for _, _, d in jobs)))
        rows.append(list(out) if describe(bwd, stack, mlp, batch, n, *a, cus, out) == 0 else [-1] * NFIELDS)
    return {"describe": rows, "sizes": [lib.dh_decoder_layer_bwd_workspace_size(im * rpi, rpi, mlp) for rpi, im, mlp in size_queries()]}


def current(run):
    sys.path.insert(0, ROOT)
    from dahitra_amd import _lib
    lib = _lib.lib()
    return run_cases(lib, lib.dh_decoder_plan_describe, run)


def child_env(run):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DAHITRA_DEC_")}
    env.update(RUNS[run])
    return env


@pytest.fixture(scope="module")
def got():
    res = [json.loads(subprocess.check_output([sys.executable, os.path.abspath(__file__), str(r)], env=child_env(r))) for r in range(len(RUNS))]
    return {"describe": [row for r in res for row in r["describe"]], "sizes": [s for r in res for s in r["sizes"]]}


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as g:
        rows = np.full((len(g["refused"]), NFIELDS), -1, dtype=np.int64)
        rows[~g["refused"]] = g["describe"].T
        return {"describe": rows.tolist(), "sizes": g["sizes"].tolist()}


def every_case():
    return [(r, c) for r in range(len(RUNS)) for c in cases(r)]


def test_plan_chooses_the_recorded_kernel_blocks_and_order(got, gold):
    assert len(got["describe"]) == len(gold["describe"]) == len(every_case())
    bad = [(c, a, b) for c, a, b in zip(every_case(), got["describe"], gold["describe"]) if a != b]
    assert not bad, "%d rows differ, first (case, got, recorded): %s" % (len(bad), bad[:3])


def test_workspace_sizes_keep_their_values(got, gold):
    assert len(got["sizes"]) == len(gold["sizes"]) == len(RUNS) * len(size_queries())
    assert got["sizes"] == gold["sizes"]


def test_no_backward_job_writes_past_its_workspace_and_the_finalize_sums_its_blocks(got, gold):
    """every backward job of every launch, recorded and planned: images x bpi partials of PL<MLP>::SIZE floats fit the bytes
    dh_decoder_layer_bwd_workspace_size gave for one layer, and the finalize reads exactly the blocks that job wrote"""
    sizes = {}
    for r in range(len(RUNS)):
        for (rpi, im, mlp), s in zip(size_queries(), got["sizes"][r * len(size_queries()):]):
            sizes[r, rpi, im, mlp] = s
    for rows in (got["describe"], gold["describe"]):
        seen = 0
        for (r, (bwd, stack, mlp, batch, jobs, cus)), row in zip(every_case(), rows):
            if not bwd or row[FAMILY] < 0:
                continue
            for j in range(row[NJOBS]):
                job, fin = row[JOB0 + 5 * j:JOB0 + 5 * j + 5], row[FIN0 + 4 * j:FIN0 + 4 * j + 4]
                images, rpi, depth = jobs[job[SRC]]
                assert fin[WS] == sizes[r, rpi, images, mlp], (r, jobs, row)
                assert images * job[BPI] * PL_SIZE[mlp] * 4 <= fin[WS], (r, jobs, row)
                assert job[BLOCKS] == images * job[BPI] and job[BPI] == -(-(rpi // 64) // job[UPB]), (r, jobs, row)
                assert (fin[FIN_NBLK], fin[FIN_BPI]) == (job[BLOCKS], job[BPI]), (r, jobs, row)
                assert fin[FIN_GRID] == ((PL_SIZE[mlp] - 2048) // 32 + 8 * images) * max(depth, 1), (r, jobs, row)
                seen += 1
        assert seen > 2000


def test_every_kernel_a_replan_and_a_reorder_appear_in_the_fixture(gold):
    rows = [(c, row) for (r, c), row in zip(every_case(), gold["describe"]) if r == 0 and row[FAMILY] >= 0]
    for bwd in (0, 1):
        assert {row[FAMILY] for c, row in rows if c[0] == bwd} == set(range(8))         # (MLP 64) + 2 stack + 4 multi
    lone = {(c[0], c[2]) + c[4][0][:2]: row[JOB0 + BPI] for c, row in rows if c[3] and len(c[4]) == 1}
    replanned = [c for c, row in rows for j in range(row[NJOBS]) if len(c[4]) > 1
                 and row[JOB0 + 5 * j + BPI] != lone[(c[0], c[2]) + c[4][row[JOB0 + 5 * j + SRC]][:2]]]
    reordered = [c for c, row in rows if [row[JOB0 + 5 * j + SRC] for j in range(row[NJOBS])] != list(range(row[NJOBS]))]
    assert len(replanned) > 100 and len(reordered) > 100
    assert {0, 1} == {c[0] for c in replanned} == {c[0] for c in reordered}


if __name__ == "__main__":
    json.dump(current(int(sys.argv[1])), sys.stdout)
