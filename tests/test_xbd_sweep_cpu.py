"""The host side of the xBD threshold sweep (models/xbd.sweep_loc_table / sweep_rule_table / sweep_counts / XbdSweep) against
the numpy restatements of tests/_xbd_val_cases.py and tests/_xbd_sweep_cases.py, and the Python-side argument checks of
ops.xbd_val_sweep.  No GPU."""
import math
import re

import numpy as np
import pytest
import torch

import _xbd_sweep_cases as W
import _xbd_val_cases as V

CASES = [(3, 37, 337), (2, 40, 240)]


@pytest.fixture(scope="module")
def cases():
    """the synthetic inputs, their sigmoids and the restated histograms for both selections (computed once)"""
    thr = W.grid()
    out = {}
    for B, S, seed in CASES:
        x, msk, lbl, planted = V.synthetic(B, S, seed)
        V.check_synthetic(x, msk, lbl, planted)
        s = V.sigmoid32(x)
        out[(B, S)] = dict(x=x, msk0=msk[:, 0], lbl=lbl, s=s,
                           hist={sel: W.hist(x, msk[:, 0], lbl, thr, sel, s=s) for sel in ("reference", "building")})
    return thr, out


def test_grid_meets_its_conditions():
    thr = W.grid()
    W.check_grid(thr)
    sg = W.logit_sigmoids().astype(np.float64)
    dist = np.abs(thr.astype(np.float64)[:, None] - sg[None, :])
    dist[thr == np.float32(0.5), 64] = 1.0
    print("minimum margin %.3g, minimum gap %.3g" % (dist.min(), np.diff(thr.astype(np.float64)).min()))
    x = V.synthetic(3, 37, 337)[0]
    assert (x[:, 0] == 0).sum() == 34, "localisation logits that sit exactly on the threshold 0.5"


def test_histogram_holds_every_pixel_once(cases):
    thr, data = cases
    for (B, S), d in data.items():
        for sel in ("reference", "building"):
            ih, ch = d["hist"][sel]
            assert ih.shape == (B, 65, 4, 2) and ch.shape == (65, 4, 5)
            assert (ih.sum(axis=(1, 2, 3)) == S * S).all()
            n_sel = sum(int(V.row_selection(d["lbl"][j]).sum()) if sel == "reference" else int((d["msk0"][j] > 0).sum())
                        for j in range(B))
            assert ch.sum() == n_sel and ch[:, :, 4].sum() == 0
        assert (np.count_nonzero(d["hist"]["building"][0].sum(axis=(0, 2, 3))) > 40), "the logits spread over the bins"


@pytest.mark.parametrize("select", ["reference", "building"])
def test_sweep_counts_at_every_grid_index_equal_the_single_threshold_restatement(cases, select):
    from dahitra_amd.models.xbd import sweep_counts, sweep_loc_table
    thr, data = cases
    for key, d in data.items():
        ih, ch = d["hist"][select]
        for k in range(thr.size):
            want_ic, want_cc = V.counts(d["x"], d["msk0"], d["lbl"], thr=thr[k], select=select, s=d["s"])
            ic, cc = sweep_counts(ih, ch, sweep_loc_table(thr.size, k))
            assert ic.dtype == np.int64 and cc.dtype == np.int64 and ic.shape == want_ic.shape and cc.shape == (4, 3)
            assert np.array_equal(ic, want_ic) and np.array_equal(cc, want_cc), (key, k, thr[k])


def test_loc_table_takes_one_index_or_one_per_arg():
    from dahitra_amd.models.xbd import sweep_loc_table
    t = sweep_loc_table(3, 1)
    assert t.dtype == np.bool_ and t.tolist() == [[False] * 4, [False] * 4, [True] * 4, [True] * 4]
    t = sweep_loc_table(3, [0, 2, 1, 0])
    assert t.tolist() == [[False, False, False, False], [True, False, False, True], [True, False, True, True], [True, True, True, True]]
    for bad in (3, -1, [0, 1], [0, 1, 2, 3], 0.5):
        with pytest.raises(ValueError):
            sweep_loc_table(3, bad)


def test_rule_table_is_line_209_of_visualize_results(cases):
    from dahitra_amd.models.xbd import sweep_counts, sweep_loc_table, sweep_rule_table
    thr, data = cases
    # the script's 0.38 / 0.13 / 0.14 on the grid: the members next to 0.38 and 0.13, and the one above the latter (this grid is
    # too coarse to part 0.13 from 0.14)
    k13 = int(np.abs(thr - np.float32(0.13)).argmin())
    a, b, c = float(thr[np.abs(thr - np.float32(0.38)).argmin()]), float(thr[k13]), float(thr[k13 + 1])
    assert b < c < a
    triples = [(a, b, c),                                     # the script's _thr
               (b, a, c),                                     # t1 > t0: t1 then changes nothing
               (c, b, a),                                     # t0 between the two: arg 0 and arg 3 share t0
               (float(thr[5]), float(thr[5]), float(thr[5])),
               (float(thr[63]), float(thr[0]), float(thr[31]))]
    assert len({t for tr in triples[:3] for t in tr}) == 3
    for t0, t1, t2 in triples:
        table = sweep_rule_table(thr, t0, t1, t2)
        ks = [int(np.nonzero(thr == np.float32(v))[0][0]) for v in (t0, min(t0, t1, t2), min(t0, t1, t2), min(t0, t2))]
        assert np.array_equal(table, sweep_loc_table(thr.size, ks))
        for key, d in data.items():
            for sel in ("reference", "building"):
                want = W.rule_counts(d["x"], d["msk0"], d["lbl"], t0, t1, t2, select=sel, s=d["s"])
                got = sweep_counts(*d["hist"][sel], table)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (key, sel, t0, t1, t2)
    # the rule with three equal thresholds is the plain threshold
    assert np.array_equal(sweep_rule_table(thr, float(thr[9]), float(thr[9]), float(thr[9])), sweep_loc_table(thr.size, 9))
    # a float64 that rounds to a grid member is that member; anything else is refused
    assert np.array_equal(sweep_rule_table(thr, 0.3, 0.3, 0.5), sweep_loc_table(thr.size, [int(np.nonzero(thr == np.float32(0.3))[0][0])] * 4))
    for bad in ((0.31, 0.3, 0.3), (0.3, 0.31, 0.3), (0.3, 0.3, float("nan"))):
        with pytest.raises(ValueError, match="not a threshold of the grid"):
            sweep_rule_table(thr, *bad)


def test_labels_above_three_are_other_and_count_as_fp_only(cases):
    """lbl >= 4 lands in t = 4: no class's tp or fn, an fp of the predicted class -- what `pred == c && t != c` gives for any t"""
    from dahitra_amd.models.xbd import sweep_counts, sweep_loc_table
    thr, data = cases
    d = data[(2, 40)]
    lbl = d["lbl"].copy()
    lbl[0, 0, 1::2] = 1                       # the selected rows stay selected
    lbl[:, 5:20, :] = np.where(np.arange(40)[None, None, :] % 2 == 0, 4, 9)
    lbl[:, 20:23, :] = 255
    for sel in ("reference", "building"):
        ih, ch = W.hist(d["x"], d["msk0"], lbl, thr, sel, s=d["s"])
        assert ch[:, :, 4].sum() > 0
        k = int(np.nonzero(thr == np.float32(0.3))[0][0])
        ic, cc = sweep_counts(ih, ch, sweep_loc_table(thr.size, k))
        want_ic, want_cc = V.counts(d["x"], d["msk0"], lbl, thr=thr[k], select=sel, s=d["s"])
        assert np.array_equal(ic, want_ic) and np.array_equal(cc, want_cc)
        # without the "other" pixels: tp and fn are the same, every fp is smaller or equal, and the difference is their number
        ch0 = ch.copy()
        ch0[:, :, 4] = 0
        _, cc0 = sweep_counts(ih, ch0, sweep_loc_table(thr.size, k))
        assert np.array_equal(cc0[:, :2], cc[:, :2]) and (cc[:, 2] - cc0[:, 2]).sum() == ch[:, :, 4].sum()


def test_best_ignores_nan_and_the_lowest_index_wins_a_tie():
    from dahitra_amd.models.xbd import XbdSweep
    thr = np.asarray([0.2, 0.4, 0.6, 0.8], dtype=np.float32)
    sweep = XbdSweep(thr, np.zeros((1, 5, 4, 2), dtype=np.int64), np.zeros((5, 4, 5), dtype=np.int64))
    assert sweep.scores.shape == (4,) and np.isnan(sweep.scores).all()          # nothing counted: every score is nan
    best = sweep.best()
    assert best[0] is None and math.isnan(best[1])
    sweep.scores = np.array([float("nan"), 0.5, 0.5, 0.25])
    assert sweep.best() == (float(np.float32(0.4)), 0.5)
    sweep.scores = np.array([0.1, float("nan"), 0.7, float("nan")])
    assert sweep.best() == (float(np.float32(0.6)), 0.7)


def test_sweep_object_scores_and_parts_are_val_score_on_the_counts(cases):
    from dahitra_amd.models.xbd import XbdSweep, val_score
    thr, data = cases
    d = data[(3, 37)]
    ih, ch = d["hist"]["building"]
    sweep = XbdSweep(thr, ih, ch)
    assert sweep.thresholds.dtype == np.float32 and np.array_equal(sweep.thresholds, thr) and sweep.scores.dtype == np.float64
    for k in (0, 17, 63):
        want = V.counts(d["x"], d["msk0"], d["lbl"], thr=thr[k], select="building", s=d["s"])
        got = sweep.counts(k)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        sc, parts = val_score(*want)
        assert sweep.scores[k] == sc or (math.isnan(sc) and math.isnan(sweep.scores[k]))
        assert sweep.parts(k)["dice"] == parts["dice"]
    k13 = int(np.abs(thr - np.float32(0.13)).argmin())
    t0, t1, t2 = float(thr[np.abs(thr - np.float32(0.38)).argmin()]), float(thr[k13]), float(thr[k13 + 1])
    sc, parts = sweep.score_rule(t0, t1, t2)
    want = val_score(*W.rule_counts(d["x"], d["msk0"], d["lbl"], t0, t1, t2, select="building", s=d["s"]))
    assert (sc == want[0] or (math.isnan(sc) and math.isnan(want[0]))) and parts["dice"] == want[1]["dice"]
    assert not np.isnan(sweep.scores).all() and sweep.best()[1] == np.nanmax(sweep.scores)


def test_python_side_checks_come_before_the_device():
    from dahitra_amd import _lib, ops
    assert ops.XBD_SWEEP_MAX == 64
    logits = torch.zeros(2, 5, 8, 8)
    msk, lab = torch.zeros(2, 5, 8, 8, dtype=torch.uint8), torch.zeros(2, 8, 8, dtype=torch.uint8)
    hists = lambda T: (torch.zeros(2, T + 1, 4, 2, dtype=torch.int64), torch.zeros(T + 1, 4, 5, dtype=torch.int64))
    bad_grids = {"unsorted": [0.5, 0.3], "equal": [0.3, 0.3], "zero": [0.0, 0.3], "one": [0.3, 1.0], "nan": [0.3, float("nan")],
                 "empty": [], "65": list(np.linspace(0.1, 0.9, 65)), "2-D": [[0.3, 0.5]], "text": ["a"],
                 "equal as float32": [0.3, 0.3 + 1e-12], "negative": [-0.1, 0.3], "scalar": 0.3}
    for name, g in bad_grids.items():
        T = max(np.size(g), 1)
        with pytest.raises(ValueError, match="xbd_val_sweep"):
            ops.xbd_val_sweep(logits, msk, lab, *hists(T), g)
    ih, ch = hists(2)
    good = [0.3, 0.5]
    for args, kw in (((logits, msk, lab, ih[:1], ch, good), {}), ((logits, msk, lab, ih.int(), ch, good), {}),
                     ((logits, msk, lab, ih, ch[:2], good), {}), ((logits, msk, lab, ih, ch.int(), good), {}),
                     ((logits, msk, lab, *hists(3), good), {}), ((logits, msk[:1], lab, ih, ch, good), {}),
                     ((logits, msk, lab[:, :, :4], ih, ch, good), {}), ((logits.double(), msk, lab, ih, ch, good), {}),
                     ((logits, msk.float(), lab, ih, ch, good), {}), ((logits, msk, lab, ih, ch, good), {"select": "rows"}),
                     ((logits[:, :, :4], msk[:, :, :4], lab[:, :4], ih, ch, good), {})):          # H != W under 'reference'
        with pytest.raises(ValueError, match="xbd_val_sweep"):
            ops.xbd_val_sweep(*args, **kw)
    # everything fits: the call is refused for want of a device, not computed somewhere else
    for g in (good, np.asarray(good), torch.tensor(good), tuple(good), list(np.linspace(0.1, 0.9, 64))):
        T = len(g)
        with pytest.raises(_lib.HipLibraryError, match="MI355X"):
            ops.xbd_val_sweep(logits, msk, lab, *hists(T), g)
    assert ops.xbd_sweep_thresholds(good).dtype == np.float32


def test_header_declares_the_sweep_returning_int():
    import ctypes
    from dahitra_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    assert re.search(r"^int\s+dh_xbd_val_sweep\s*\(", code, flags=re.M)
    restype, argtypes = _lib.prototypes()["dh_xbd_val_sweep"]
    vp = ctypes.c_void_p
    assert restype is ctypes.c_int
    assert argtypes == [vp, vp, ctypes.c_long, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp]
