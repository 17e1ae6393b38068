"""References of ``geodesic_grow``, ``watershed`` and ``split_instances``
(csrc/geodesic.hip, geodesic.py) and the patterns their tests share.  Everything is
exact integer arithmetic.

A pixel is free when it is unlabelled and allowed.  A path runs from a free pixel to
a labelled one by steps of the metric, all its pixels but the last free.  Every free
pixel takes the minimum of the key ``(cost, id)`` over such paths.
"""
import heapq

import numpy as np
from scipy import ndimage

import instances_ref as iref

TH, TW = 32, 64  # the tile of a relaxation pass (kGeoTH x kGeoTW)
STEPS = {
    "cityblock": [(-1, 0, 1), (1, 0, 1), (0, -1, 1), (0, 1, 1)],
    "chamfer": [(-1, 0, 3), (1, 0, 3), (0, -1, 3), (0, 1, 3), (-1, -1, 4), (-1, 1, 4), (1, -1, 4), (1, 1, 4)],
}
AXIAL = {"cityblock": 1, "chamfer": 3}
_NOKEY = 1 << 62


def max_cost_of(max_distance, metric):
    """the cost bound of ``max_distance`` pixels; -1 is unlimited"""
    if max_distance is None or np.isinf(max_distance):
        return -1
    return int(np.floor(AXIAL[metric] * np.float64(max_distance)))


def _search(labels, sources, free, metric, max_cost):
    """Dijkstra from the pixels of ``sources`` (bool) with the key cost << 32 | id, relaxing into
    ``free`` pixels only; the flat list of keys (``_NOKEY``: not reached)"""
    H, W = labels.shape
    lab = labels.ravel().tolist()
    fr = free.ravel().tolist()
    key = [_NOKEY] * (H * W)
    heap = []
    for p in np.flatnonzero(sources.ravel()).tolist():
        key[p] = lab[p]
        heap.append((lab[p], p))
    heapq.heapify(heap)
    steps = STEPS[metric]
    while heap:
        k, p = heapq.heappop(heap)
        if k != key[p]:
            continue
        y, x = divmod(p, W)
        for dy, dx, c in steps:
            yy, xx = y + dy, x + dx
            if not (0 <= yy < H and 0 <= xx < W):
                continue
            q = yy * W + xx
            nk = k + (c << 32)
            if fr[q] and nk < key[q] and (max_cost < 0 or (nk >> 32) <= max_cost):
                key[q] = nk
                heapq.heappush(heap, (nk, q))
    return key


def _outputs(key, shape):
    key = np.array(key, np.int64).reshape(shape)
    reached = key != _NOKEY
    return (np.where(reached, key & 0xFFFFFFFF, 0).astype(np.int32),
            np.where(reached, key >> 32, -1).astype(np.int32))


def _free(labels, within, within_value):
    allowed = np.ones(labels.shape, bool) if within is None else iref.foreground(within, within_value)
    return (labels == 0) & allowed


def grow(labels, within=None, within_value=None, metric="cityblock", max_cost=-1):
    """(labels, cost) of unet_geodesic_grow on one frame: one search from all labelled pixels at once"""
    labels = np.asarray(labels, np.int32)
    assert (labels >= 0).all()
    return _outputs(_search(labels, labels != 0, _free(labels, within, within_value), metric, max_cost), labels.shape)


def grow_per_id(labels, within=None, within_value=None, metric="cityblock", max_cost=-1):
    """the same from one single-id search per id, then the minimum (cost, id) per pixel"""
    labels = np.asarray(labels, np.int32)
    free = _free(labels, within, within_value)
    best = np.full(labels.size, _NOKEY, np.int64)
    for i in np.unique(labels[labels > 0]):
        best = np.minimum(best, np.array(_search(labels, labels == i, free, metric, max_cost), np.int64))
    return _outputs(best, labels.shape)


def watershed(relief, markers, mask=None, mask_value=None, metric="cityblock", all_levels=False):
    """flooding by levels on one frame: for every value h of the relief under the mask (or for all
    256 values), ascending, markers <- grow(markers, within = mask & (relief <= h))"""
    relief = np.asarray(relief, np.uint8)
    out = np.asarray(markers, np.int32).copy()
    allowed = np.ones(relief.shape, bool) if mask is None else iref.foreground(mask, mask_value)
    levels = range(256) if all_levels else np.unique(relief[allowed]).tolist()
    for h in levels:
        out = grow(out, allowed & (relief <= h), None, metric)[0]
    return out


def isqrt(a):
    """exact integer floor square root of a non-negative int array"""
    a = np.asarray(a, np.int64)
    r = np.floor(np.sqrt(a.astype(np.float64))).astype(np.int64)
    r = np.where(r * r > a, r - 1, r)
    return np.where((r + 1) * (r + 1) <= a, r + 1, r)


def split(mask, seed_distance, metric="cityblock", connectivity=1, foreground=None):
    """(labels, count, number of seeds) of split_instances on one frame, with scipy"""
    fg = iref.foreground(mask, foreground)
    d2 = np.rint(ndimage.distance_transform_edt(fg) ** 2).astype(np.int64)
    R = int(np.ceil(seed_distance))
    assert 1 <= R <= 255
    seeds, n, _ = iref.label(d2 >= R * R, connectivity)
    relief = np.clip(R - isqrt(d2), 0, 255).astype(np.uint8)
    ws = watershed(relief, seeds, fg, None, metric)
    rest, m, _ = iref.label(fg & (ws == 0), connectivity)
    return (ws + np.where(rest > 0, rest + n, 0)).astype(np.int32), n + m, n


# ---- patterns ---------------------------------------------------------------------

def disc(h, w, cy, cx, r):
    yy, xx = np.mgrid[:h, :w]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r


def touching_discs(h=40, w=80):
    """the fixture of the issue: two discs of radius 13 with centres 20 apart (one blob) and a disc of
    radius 3; seed_distance 10 splits the blob into areas 504 and 487, 9 does not split it"""
    return (disc(h, w, 18, 20, 13) | disc(h, w, 18, 40, 13) | disc(h, w, 30, 70, 3)).astype(np.uint8)


def unequal_discs(h=45, w=70):
    """a large and a small overlapping disc with one marker in each centre: (mask, markers)"""
    m = (disc(h, w, 22, 22, 18) | disc(h, w, 22, 46, 9)).astype(np.uint8)
    mk = np.zeros((h, w), np.int32)
    mk[22, 22], mk[22, 46] = 1, 2
    return m, mk


def ridge(h=40, w=140):
    """(relief, markers): a marker left of a ridge that lies wholly in the first tile; the plain right of
    it, in the other tiles, is at level 0 but is reached only when the ridge floods"""
    relief = np.zeros((h, w), np.uint8)
    relief[:, 60:63] = 100
    markers = np.zeros((h, w), np.int32)
    markers[10, 10] = 6
    return relief, markers


def relief_of(mask, R):
    d2 = np.rint(ndimage.distance_transform_edt(mask != 0) ** 2).astype(np.int64)
    return np.clip(R - isqrt(d2), 0, 255).astype(np.uint8)


def serpentine(h=67, w=131):
    """(labels, within): a corridor one pixel wide that crosses tile borders in every row and comes
    back to tiles it has left, one seed at its start, another id in the middle of its last row"""
    within = iref.serpentine(h, w)
    lab = np.zeros((h, w), np.int32)
    lab[0, 0] = 5
    lab[(h - 1) // 2 * 2, w // 2] = 3
    return lab, within


def u_corridor(h=40, w=70):
    """(labels, within): a U whose arms are two pixels apart, seed 1 at the top of the left arm, seed 2
    half way down the right arm: at that height the left arm is 6 pixels from seed 2 across the gap
    but 27 steps from it round the bend, and 18 from seed 1"""
    within = np.zeros((h, w), np.uint8)
    within[2:36, 10:14] = 1
    within[2:36, 16:20] = 1
    within[32:36, 10:20] = 1
    lab = np.zeros((h, w), np.int32)
    lab[2, 10:14] = 1
    lab[20, 16:20] = 2
    return lab, within


def border_tie(h=40, w=131):
    """two ids in one row, mirrored about column 63, the last of its tile: that column ties, column 62
    is nearer to id 2 and column 64, the first of the next tile, to id 1"""
    lab = np.zeros((h, w), np.int32)
    lab[10, 58] = 2   # 5 left of column 63
    lab[10, 68] = 1   # 5 right of column 63: column 63 ties, the smaller id takes it
    return lab


def corner_tie(h=67, w=131):
    """two ids mirrored about the tile corner (32, 64): the diagonal through the corner ties"""
    lab = np.zeros((h, w), np.int32)
    lab[27, 69] = 2   # up right of the corner pixel (32, 64) by (-5, +5)
    lab[37, 59] = 1   # down left by (+5, -5)
    return lab


def diagonal_gap(h=33, w=65):
    """(labels, within): two rooms that touch only diagonally, at the tile corner"""
    within = np.zeros((h, w), np.uint8)
    within[20:32, 50:64] = 1   # ends at (31, 63)
    within[32:33, 64:65] = 1   # the pixel (32, 64): a diagonal neighbour only
    lab = np.zeros((h, w), np.int32)
    lab[25, 55] = 4
    return lab, within


def wall_with_gap(h=50, w=90):
    """(labels, within): a wall of forbidden pixels with a gap of one pixel, a seed on either side"""
    within = np.ones((h, w), np.uint8) * 7
    within[:, 40] = 0
    within[45, 40] = 7
    lab = np.zeros((h, w), np.int32)
    lab[5, 20] = 1
    lab[5, 42] = 2
    return lab, within


def random_case(rng, h, w, p_label=0.02, p_allowed=0.7, ids=5):
    """(labels, within) with scattered labelled pixels of a few ids and a random allowed set"""
    lab = np.where(rng.random((h, w)) < p_label, rng.integers(1, ids + 1, (h, w)), 0).astype(np.int32)
    within = (rng.random((h, w)) < p_allowed).astype(np.uint8)
    return lab, within


def _open(lab):
    return lab, np.ones(lab.shape, np.uint8)


def _single(h, w, y, x, i):
    lab = np.zeros((h, w), np.int32)
    lab[y, x] = i
    return lab


# name -> (labels, within) of one frame
PATTERN_CASES = {
    "serpentine": serpentine,
    "empty67": lambda: _open(np.zeros((67, 131), np.int32)),
    "single67": lambda: _open(_single(67, 131, 33, 65, 8)),
    "random": lambda: random_case(np.random.default_rng(7), 50, 90),
    "u_corridor": u_corridor,
    "diagonal_gap": diagonal_gap,
    "wall_with_gap": wall_with_gap,
}
