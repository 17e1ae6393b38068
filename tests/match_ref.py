"""Reference of ``match_instances`` / ``instance_metrics`` (csrc/match.hip, match.py)
in numpy and Python integers, and the label-map patterns its tests share.

``tables`` builds the dense contingency table c[g][p] of two label maps with one
``np.bincount`` and from it the two tables, the status row and the pair list of
include/unet_hip.h.  ``metrics`` follows the definitions of the scores with
``Fraction`` thresholds and exact integer comparisons; floats appear only in the
final ratios, computed in float64 in id order.
"""
import functools
from fractions import Fraction

import numpy as np
from scipy import ndimage

H0, W0 = 130, 131  # two 64-tiles (four 32-row tiles) plus a remainder per axis, odd width
EPS = 1e-7         # utils.EPS of the package (test_match.py checks that they agree)
THRESHOLDS = tuple(Fraction(10 + k, 20) for k in range(10))  # 0.5, 0.55, ..., 0.95
COLS, STATUS = 4, 5


def _better(a, b):
    """candidates (partner, c, u): higher IoU c / u, then the smaller partner id"""
    l, r = a[1] * b[2], b[1] * a[2]
    return l > r or (l == r and a[0] < b[0])


def tables(gt, pred, max_gt, max_pred):
    """One frame -> dict(gt_table [max_gt][4], pred_table [max_pred][4], status [5], pairs [n_pairs][3] sorted by
    (gt, pred), counted = the pixels that are in range and not background on both sides)."""
    gt = np.asarray(gt).astype(np.int64)
    pred = np.asarray(pred).astype(np.int64)
    assert gt.shape == pred.shape and gt.ndim == 2
    bad = (gt < 0) | (gt > max_gt) | (pred < 0) | (pred > max_pred)
    g = np.where(bad, 0, gt).ravel()
    p = np.where(bad, 0, pred).ravel()
    ng, npd = int(g.max()) + 1, int(p.max()) + 1
    cont = np.bincount(g * npd + p, minlength=ng * npd).reshape(ng, npd)
    gt_area = cont.sum(1)
    pred_area = cont.sum(0)
    gt_area[0] = pred_area[0] = 0  # background is no instance
    gt_table = np.zeros((max_gt, COLS), np.int64)
    pred_table = np.zeros((max_pred, COLS), np.int64)
    pairs = []
    best_g, best_p = {}, {}
    for gi, pi in zip(*np.nonzero(cont[1:, 1:])):
        gi, pi = int(gi) + 1, int(pi) + 1
        c = int(cont[gi, pi])
        u = int(gt_area[gi]) + int(pred_area[pi]) - c
        pairs.append((gi, pi, c))
        if gi not in best_g or _better((pi, c, u), best_g[gi]):
            best_g[gi] = (pi, c, u)
        if pi not in best_p or _better((gi, c, u), best_p[pi]):
            best_p[pi] = (gi, c, u)
    for i in range(1, ng):
        o, c, _ = best_g.get(i, (0, 0, 0))
        gt_table[i - 1] = (gt_area[i], o, c, pred_area[o] if o else 0)
    for i in range(1, npd):
        o, c, _ = best_p.get(i, (0, 0, 0))
        pred_table[i - 1] = (pred_area[i], o, c, gt_area[o] if o else 0)
    status = np.array([np.count_nonzero(gt_area), np.count_nonzero(pred_area), len(pairs), 0, int(bad.sum())], np.int64)
    counted = int(np.count_nonzero((g != 0) | (p != 0)))
    return {"gt_table": gt_table, "pred_table": pred_table, "status": status,
            "pairs": np.array(sorted(pairs), np.int64).reshape(-1, 3), "counted": counted}


def padded_pairs(pairs, max_pairs):
    out = np.zeros((max_pairs, 3), np.int64)
    out[:len(pairs)] = pairs
    return out


def frame_counts(tab, thresholds=THRESHOLDS):
    """Python integers of one frame: tp per threshold, n_gt, n_pred, the matched (c, u) at 0.5, C and U of the AJI,
    and the matches per threshold as (gt, pred) lists."""
    gt_table, pred_table = tab["gt_table"], tab["pred_table"]
    n_gt = sum(1 for r in gt_table if r[0] > 0)
    n_pred = sum(1 for r in pred_table if r[0] > 0)
    matches = []
    for t in thresholds:
        t = Fraction(t).limit_denominator(1000)
        assert t >= Fraction(1, 2)
        m = []
        for i, (area, o, c, oa) in enumerate(gt_table.tolist(), 1):
            if o and c * t.denominator > t.numerator * (area + oa - c):  # IoU > t, decided in integers
                m.append((i, o))
        matches.append(m)
    half = [(c, a + oa - c) for a, o, c, oa in gt_table.tolist() if o and 2 * c > a + oa - c]
    C = U = 0
    used = set()
    for area, o, c, oa in gt_table.tolist():
        if area == 0:
            continue
        if o:
            C += c
            U += area + oa - c
            used.add(o)
        else:
            U += area
    for i, (area, _, _, _) in enumerate(pred_table.tolist(), 1):
        if area > 0 and i not in used:
            U += area
    return {"tp": [len(m) for m in matches], "n_gt": n_gt, "n_pred": n_pred, "half": half, "C": C, "U": U,
            "matches": matches}


def _scores(tp, n_gt, n_pred, half, C, U):
    tp = np.array(tp, np.int64)
    fp, fn = n_pred - tp, n_gt - tp
    precision = np.array([t / (t + f + EPS) for t, f in zip(tp.tolist(), fp.tolist())])
    recall = np.array([t / (t + f + EPS) for t, f in zip(tp.tolist(), fn.tolist())])
    f1 = 2 * precision * recall / (precision + recall + EPS)
    ap = np.array([t / (t + a + b + EPS) for t, a, b in zip(tp.tolist(), fp.tolist(), fn.tolist())])
    s = 0.0
    for c, u in half:
        s += c / u
    k = len(half)
    den = k + 0.5 * (n_pred - k) + 0.5 * (n_gt - k) + EPS
    return {"tp": tp, "fp": fp, "fn": fn, "precision": precision, "recall": recall, "f1": f1, "ap": ap,
            "mean_ap": np.float64(ap.mean()), "pq": np.float64(s / den), "sq": np.float64(s / (k + EPS)),
            "rq": np.float64(k / den), "aji": np.float64(C / U if U else 0.0)}


def metrics(tabs, thresholds=THRESHOLDS):
    """instance_metrics of a list of frames: every entry stacked over the frames, and "pooled"."""
    fc = [frame_counts(t, thresholds) for t in tabs]
    per = [_scores(f["tp"], f["n_gt"], f["n_pred"], f["half"], f["C"], f["U"]) for f in fc]
    out = {k: np.stack([p[k] for p in per]) for k in per[0]}
    out["pooled"] = _scores(np.sum([f["tp"] for f in fc], axis=0), sum(f["n_gt"] for f in fc),
                            sum(f["n_pred"] for f in fc), [h for f in fc for h in f["half"]],
                            sum(f["C"] for f in fc), sum(f["U"] for f in fc))
    return out


# ---- patterns: (gt, pred) int32 -----------------------------------------------------

def _zeros(h=H0, w=W0):
    return np.zeros((h, w), np.int32)


def _disk(a, cy, cx, r, v):
    yy, xx = np.ogrid[:a.shape[0], :a.shape[1]]
    a[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = v


def disks(jit=2, seed=7, h=H0, w=W0):
    """a 20 px grid of disks of radius 3..9; pred: shifted by up to jit px, radius changed by -2..1, 10 % dropped"""
    rng = np.random.default_rng(seed)
    gt, pred = _zeros(h, w), _zeros(h, w)
    k = 0
    for cy in range(10, h, 20):
        for cx in range(10, w, 20):
            k += 1
            r = int(rng.integers(3, 10))
            dy, dx = (int(v) for v in rng.integers(-jit, jit + 1, 2))
            dr = int(rng.integers(-2, 2))
            drop = rng.random() < 0.1
            _disk(gt, cy, cx, r, k)
            if not drop:
                _disk(pred, cy + dy, cx + dx, max(r + dr, 1), k)
    # the pred side numbers its instances on its own
    ids = np.unique(pred[pred > 0])
    lut = np.zeros(k + 1, np.int32)
    lut[ids] = np.arange(1, len(ids) + 1)
    return gt, lut[pred]


def identical(seed=3):
    m = ndimage.binary_opening(np.random.default_rng(seed).random((H0, W0)) < 0.6)
    lab = ndimage.label(m)[0].astype(np.int32)
    return lab, lab.copy()


def disjoint():
    gt, pred = _zeros(), _zeros()
    for k in range(5):
        gt[10 + 22 * k:25 + 22 * k, 5:60] = k + 1
        pred[5 + 22 * k:28 + 22 * k, 62:125] = k + 1
    return gt, pred


def empty_gt():
    return _zeros(), disks()[0]


def empty_pred():
    return disks()[0], _zeros()


def both_empty():
    return _zeros(), _zeros()


def one_to_many():
    """one gt block covered by four preds of different sizes"""
    gt, pred = _zeros(), _zeros()
    gt[30:90, 40:110] = 1
    pred[30:50, 40:70] = 1
    pred[30:50, 70:110] = 2
    pred[50:90, 40:70] = 3
    pred[50:90, 70:110] = 4
    return gt, pred


def many_to_one():
    gt, pred = one_to_many()
    return pred, gt


def tie():
    """a gt of 4 x 8 pixels split by two preds of equal size, and the same with the sides swapped, across a tile
    border: the smaller id wins on both sides"""
    gt, pred = _zeros(), _zeros()
    gt[10:14, 20:28] = 1
    pred[10:14, 20:24] = 5
    pred[10:14, 24:28] = 3
    pred[60:68, 62:66] = 9
    gt[60:64, 62:66] = 4
    gt[64:68, 62:66] = 2
    return gt, pred


def half():
    """IoU exactly 1 / 2: no match at t = 0.5"""
    gt, pred = _zeros(), _zeros()
    gt[70, 63:65] = 1
    pred[70, 64] = 1
    return gt, pred


def all_distinct_tile():
    """32 x 64 with 2048 distinct pairs: more than the LDS table of a tile holds"""
    yy, xx = np.mgrid[:32, :64]
    return (yy + 1).astype(np.int32), (xx + 1).astype(np.int32)


def noise(h=H0, w=W0, seed=11):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 64, (h, w)).astype(np.int32), rng.integers(0, 64, (h, w)).astype(np.int32)


def sparse_ids():
    gt, pred = _zeros(), _zeros()
    for k, v in enumerate((7, 900, 4096)):
        gt[10 + 40 * k:40 + 40 * k, 20:100] = v
        pred[14 + 40 * k:44 + 40 * k, 30 + 10 * k:110] = (4096, 7, 900)[k]
    return gt, pred


def stripes():
    """runs that cross the 64-lane wave boundary and the tile borders"""
    gt, pred = _zeros(), _zeros()
    for k, y in enumerate(range(3, H0 - 6, 9)):
        gt[y:y + 6, 40 + k:100 + k] = k + 1      # horizontal bars across x = 64 (and x = 128 for the last ones)
    for k, x in enumerate(range(2, W0 - 8, 11)):
        pred[20 + k:100 - k, x:x + 8] = k + 1    # vertical bars across y = 32, 64, 96
    return gt, pred


PATTERNS = {
    "disks": disks, "disks0": lambda: disks(0), "identical": identical, "disjoint": disjoint, "empty_gt": empty_gt,
    "empty_pred": empty_pred, "both_empty": both_empty, "one_to_many": one_to_many, "many_to_one": many_to_one,
    "tie": tie, "half": half, "all_distinct_tile": all_distinct_tile, "noise": noise, "sparse_ids": sparse_ids,
    "stripes": stripes,
}
MAX_INSTANCES = 4096   # the default cap of match_instances
MAX_PAIRS = 8 * 4096   # and its default max_pairs


@functools.lru_cache(maxsize=None)
def pattern(name):
    gt, pred = PATTERNS[name]()
    gt.setflags(write=False)
    pred.setflags(write=False)
    return gt, pred


@functools.lru_cache(maxsize=None)
def expected(name, max_gt=MAX_INSTANCES, max_pred=MAX_INSTANCES):
    gt, pred = pattern(name)
    out = tables(gt, pred, max_gt, max_pred)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
