"""The matching of two label maps (csrc/xbd_buildings.hip: dh_xbd_cc_match, models/xbd.building_match) restated in plain numpy,
and the pattern pairs its tests share.

The definition, all integer: A holds the predicted buildings 1 .. cap_a, B the true ones 1 .. cap_b, anything else is background.
For a label a: area(a) = #(A == a), inter(a, b) = #(A == a and B == b), maj(a) = the b >= 1 with 2 inter(a, b) > area(a) or 0,
inter = inter(a, maj), maj_area = area_B(maj) (both 0 without a maj), match(a) = maj if inter * den > num * (area + maj_area -
inter) else 0; match_b[match - 1] = a.  cc_match takes the pairs from np.unique over a * (cap_b + 1) + b and applies that
literally.  Its `mutate` argument builds the WRONG variants with which test_xbd_match_cpu.py shows that its comparisons can fail."""
import numpy as np

import _xbd_buildings_cases as B

COLS = 5           # area, maj, inter, maj_area, match
MUTANTS = ("ge", "ratio", "noverify", "no_match_b")


# ---- the restatement -------------------------------------------------------------------------------------------------
def _clamped(L, cap):
    L = L.astype(np.int64)
    return np.where((L >= 1) & (L <= cap), L, 0).ravel()


def bit_candidates(A, B_, cap_a, cap_b):
    """int64 [N, cap_a]: OR over the bits k < bit_length(cap_b) of (2 * ones[a][k] > area(a)) << k, ones[a][k] the pixels of a
    whose B label has bit k set.  Equal to maj(a) wherever that is not 0; anything elsewhere."""
    N = A.shape[0]
    cand = np.zeros((N, cap_a), dtype=np.int64)
    for n in range(N):
        a, b = _clamped(A[n], cap_a), _clamped(B_[n], cap_b)
        area = np.bincount(a, minlength=cap_a + 1)
        for k in range(int(cap_b).bit_length()):
            ones = np.bincount(a[(b >> k) & 1 == 1], minlength=cap_a + 1)
            cand[n] |= (2 * ones[1:] > area[1:]).astype(np.int64) << k
    return cand


def cc_match(A, B_, cap_a, cap_b, num=1, den=2, mutate=None):
    """(match_a int32 [N, cap_a, 5], match_b int32 [N, cap_b])"""
    assert A.shape == B_.shape and A.ndim == 3 and 1 <= num <= den <= 32768 and 2 * num >= den and mutate in (None,) + MUTANTS
    N = A.shape[0]
    match_a = np.zeros((N, cap_a, COLS), dtype=np.int32)
    match_b = np.zeros((N, cap_b), dtype=np.int32)
    cand = bit_candidates(A, B_, cap_a, cap_b) if mutate == "noverify" else None
    for n in range(N):
        a, b = _clamped(A[n], cap_a), _clamped(B_[n], cap_b)
        area_a, area_b = np.bincount(a, minlength=cap_a + 1), np.bincount(b, minlength=cap_b + 1)
        pairs, cnt = np.unique(a * (cap_b + 1) + b, return_counts=True)
        inter_of = {(int(p) // (cap_b + 1), int(p) % (cap_b + 1)): int(c) for p, c in zip(pairs, cnt)}
        partners = {}                                           # a -> the labels of B it meets
        for ia, jb in inter_of:
            partners.setdefault(ia, []).append(jb)
        for i in range(1, cap_a + 1):
            area = int(area_a[i])
            if area == 0:
                continue
            maj = 0
            if mutate == "noverify":                            # WRONG: the bits' candidate taken for the majority label
                c = int(cand[n, i - 1])
                maj = c if 1 <= c <= cap_b and area_b[c] > 0 else 0
            else:
                for jb in partners[i]:
                    if jb >= 1 and 2 * inter_of[i, jb] > area:
                        assert maj == 0, "two labels cannot both cover more than half"
                        maj = jb
            inter = inter_of.get((i, maj), 0) if maj else 0
            maj_area = int(area_b[maj]) if maj else 0
            union = area + maj_area - inter
            if mutate == "ge":                                  # WRONG: not strict
                ok = inter * den >= num * union
            elif mutate == "ratio":                             # WRONG: the covered share of a in place of the IoU
                ok = inter * den > num * area
            else:
                ok = inter * den > num * union
            match = maj if (maj and ok) else 0
            match_a[n, i - 1] = (area, maj, inter, maj_area, match)
            if match and mutate != "no_match_b":                # WRONG when skipped: match_b left unset
                match_b[n, match - 1] = i
    return match_a, match_b


def cc_match_fast(A, B_, cap_a, cap_b, num=1, den=2):
    """cc_match without mutants and without the per-label Python loop, for the shapes with thousands of labels: the same pairs
    from np.unique, the definition applied to whole arrays.  test_xbd_match_cpu.py holds it against cc_match."""
    N = A.shape[0]
    match_a = np.zeros((N, cap_a, COLS), dtype=np.int64)
    match_b = np.zeros((N, cap_b), dtype=np.int32)
    for n in range(N):
        a, b = _clamped(A[n], cap_a), _clamped(B_[n], cap_b)
        area_a, area_b = np.bincount(a, minlength=cap_a + 1), np.bincount(b, minlength=cap_b + 1)
        pairs, cnt = np.unique(a * (cap_b + 1) + b, return_counts=True)
        pa, pb = pairs // (cap_b + 1), pairs % (cap_b + 1)
        sel = (pa >= 1) & (pb >= 1) & (2 * cnt > area_a[pa])
        rows = pa[sel] - 1
        assert len(np.unique(rows)) == len(rows)
        m = match_a[n]
        m[:, 0] = area_a[1:]
        m[rows, 1], m[rows, 2], m[rows, 3] = pb[sel], cnt[sel], area_b[pb[sel]]
        ok = (m[:, 1] > 0) & (m[:, 2] * den > num * (m[:, 0] + m[:, 3] - m[:, 2]))
        m[:, 4] = np.where(ok, m[:, 1], 0)
        hit = np.flatnonzero(ok)
        match_b[n, m[hit, 4] - 1] = hit + 1
    return match_a.astype(np.int32), match_b


def building_match(pred_map, gt, num=1, den=2, conn=8, cap=4096, mutate=None):
    """dict of models/xbd.building_match's fields: the label maps and counts, match_pred, match_gt, pred_cls, gt_cls and the
    three host tables loc [3], confusion [4, 5], spurious [5] (int64)"""
    if gt.size and int(gt.max()) > 4:
        raise KeyError(int(gt.max()))
    la, ka = B.cc_label((pred_map != 0).astype(np.uint8), conn, False)
    lb, kb = B.cc_label(gt, conn, True)
    if max(int(ka.max()), int(kb.max())) > cap:
        raise ValueError("more components than %d" % cap)
    pred_cls = B.cc_vote(B.cc_stats(la, pred_map, cap), 0, "damage")
    gt_cls = B.cc_vote(B.cc_stats(lb, gt, cap), 0, "all")
    ma, mb = cc_match(la, lb, cap, cap, num, den, mutate)
    loc, conf, spur = np.zeros(3, dtype=np.int64), np.zeros((4, 5), dtype=np.int64), np.zeros(5, dtype=np.int64)
    for n in range(gt.shape[0]):
        for j in range(int(kb[n])):                             # every true building: its partner's class, or 0
            i = int(mb[n, j])
            conf[int(gt_cls[n, j]) - 1, int(pred_cls[n, i - 1]) if i else 0] += 1
            loc[0 if i else 2] += 1
        for i in range(int(ka[n])):                             # every predicted building without a partner
            if ma[n, i, 4] == 0:
                spur[int(pred_cls[n, i])] += 1
                loc[1] += 1
    return dict(pred_labels=la, pred_count=ka, gt_labels=lb, gt_count=kb, match_pred=ma, match_gt=mb, pred_cls=pred_cls,
                gt_cls=gt_cls, loc=loc, confusion=conf, spurious=spur)


# ---- pattern pairs ---------------------------------------------------------------------------------------------------
THRESHOLDS = ((1, 2), (2, 3), (13, 20), (1, 1))
PAIRS = (("squares", "squares>"), ("noise59", "classes59"), ("noise70", "squares"), ("squares", "noise70"),
         ("noise30", "noise30>"), ("ones", "squares"), ("squares", "squares"), ("zeros", "squares"), ("squares", "zeros"))


def shifted(key):
    """one column to the right, column 0 cleared"""
    out = np.zeros_like(key)
    out[:, :, 1:] = key[:, :, :-1]
    return out


def stripes(N, H, W):
    """(A, B) label maps, int32: predicted label 1 is a rectangle of 20 rows whose rows lie 8 on true label 3, 7 on true label 1
    and 5 on true label 2 (40 %, 35 %, 25 %): bit 0 is set in 75 % of its pixels and bit 1 in 65 %, so the bits name label 3,
    which covers less than half.  Predicted label 2, three pixels high, lies inside true label 2 and matches it at no
    threshold above its share of that stripe."""
    assert H >= 26 and W >= 8
    A = np.zeros((N, H, W), dtype=np.int32)
    B_ = np.zeros((N, H, W), dtype=np.int32)
    B_[:, 4:12], B_[:, 12:19], B_[:, 19:24] = 3, 1, 2           # the true stripes run over the whole width
    A[:, 4:24, 3:W - 1] = 1
    A[:, 20:23, 0:2] = 2
    if N > 1:
        A[1], B_[1] = A[1, ::-1, ::-1].copy(), B_[1, ::-1, ::-1].copy()
    return A, B_


def _key(name, pats):
    return shifted(pats[name[:-1]]) if name.endswith(">") else pats[name]


def pair_labels(N, H, W, a_name, b_name):
    """(A, B, K_a, K_b): the labels of the restatement for one pattern pair; the second image of a batch is flipped; B is keyed
    where its pattern has classes"""
    pats = B.patterns(N, H, W)
    out = []
    for name in (a_name, b_name):
        key = _key(name, pats).copy()
        if N > 1:
            key[1] = key[1, ::-1, ::-1]
        lab, k = B.cc_label(key, 8, name.startswith("classes"))
        out.append((lab, int(k.max())))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def all_pairs(N, H, W):
    """name -> (A, B, K_a, K_b), the nine pattern pairs and the stripes"""
    res = {"%s|%s" % p: pair_labels(N, H, W, *p) for p in PAIRS}
    A, B_ = stripes(N, H, W)
    res["stripes"] = (A, B_, 2, 3)
    return res


def cap_choices(ka, kb):
    """room to spare, then half the component count on each side in turn"""
    return ((ka + 3, kb + 3), (max(ka // 2, 1), kb + 3), (ka + 3, max(kb // 2, 1)))


def synthetic_pair(N=2, H=65, W=130):
    """(pred, gt) uint8: the pair of the building-confusion test (a hit, a wrong class, a missed building among noise), with one
    predicted block on empty ground and one predicted block that spans two true buildings"""
    gt = B.noise(N, H, W, 0.3, classes=4)
    gt[:, 10:30, 10:50], gt[:, 10:30, 50:90], gt[:, 40:60, 20:70] = 1, 3, 4
    pred = B.noise(N, H, W, 0.8, classes=4)
    pred[:, 10:30, 10:90], pred[:, 40:60, 20:70] = 3, 0
    gt[:, 32:64, 92:130], pred[:, 31:65, 91:130] = 0, 0          # cleared ground, with a margin on the predicted side
    pred[:, 34:42, 96:110] = 2                                  # a predicted block on empty ground
    gt[:, 46:56, 96:106], gt[:, 46:56, 108:118] = 2, 2          # two true buildings two columns apart ...
    pred[:, 46:56, 96:118] = 2                                  # ... under one predicted block
    gt[:, 58:63, 97:104], pred[:, 58:63, 96:104] = 4, 4         # a clean hit, IoU 35 / 40
    gt[:, 58:63, 110:118], pred[:, 58:63, 110:118] = 3, 1       # a clean hit of the wrong class
    return pred, gt
