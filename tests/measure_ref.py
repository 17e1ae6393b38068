"""Plain-numpy reference of ``measure_instances`` / ``select_instances``
(csrc/measure.hip) and the label and image patterns their tests share.

Every integer table comes from ``np.add.at`` / ``np.minimum.at`` / ``np.maximum.at``
on int64 (never ``np.bincount(weights=)``, which sums in float64); the edge counts
from four shifted comparisons of the map padded with a sentinel no int32 equals; the
float sums from ``math.fsum`` per id (the correctly rounded sum).
"""
import functools
import math
import os
import sys

import numpy as np
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import instances_ref as iref  # noqa: E402

COLS, STATUS, ICOLS = 13, 3, 4
COLUMNS = ("area", "sum_y", "sum_x", "y0", "x0", "y1", "x1", "sum_yy", "sum_xx", "sum_xy", "edges", "frame_edges",
           "contact_edges")
MAX_INSTANCES = 4096
H0, W0 = iref.H0, iref.W0  # 130 x 131
SENTINEL = np.int64(1) << 40  # outside the frame


def tables(lab, max_instances=MAX_INSTANCES, image=None):
    """{"table" int64 [M][13], "status" int64 [3], "intensity" [M][C][4] or None} of one 2-D frame;
    image: [H][W] or [C][H][W], uint8 / uint16 (int64 table) or float32 (float64 table)"""
    lab = np.asarray(lab)
    assert lab.ndim == 2 and lab.dtype == np.int32
    H, W = lab.shape
    M = max_instances
    valid = (lab >= 1) & (lab <= M)
    yy, xx = np.nonzero(valid)
    y, x = yy.astype(np.int64), xx.astype(np.int64)
    ids = lab[valid].astype(np.int64) - 1  # the same C order as np.nonzero
    tab = np.zeros((M, COLS), np.int64)
    tab[:, 3], tab[:, 4] = H, W
    for col, v in ((0, np.ones_like(y)), (1, y), (2, x), (7, y * y), (8, x * x), (9, y * x)):
        np.add.at(tab[:, col], ids, v)
    np.minimum.at(tab[:, 3], ids, y)
    np.minimum.at(tab[:, 4], ids, x)
    np.maximum.at(tab[:, 5], ids, y + 1)
    np.maximum.at(tab[:, 6], ids, x + 1)
    pad = np.full((H + 2, W + 2), SENTINEL, np.int64)
    pad[1:-1, 1:-1] = lab
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        nb = pad[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx]
        outside = nb == SENTINEL
        differs = nb != lab  # outside the frame differs from everything
        np.add.at(tab[:, 10], ids, differs[valid].astype(np.int64))
        np.add.at(tab[:, 11], ids, outside[valid].astype(np.int64))
        np.add.at(tab[:, 12], ids, (differs & ~outside & (nb != 0))[valid].astype(np.int64))
    present = tab[:, 0] > 0
    tab[~present] = 0
    status = np.array([np.count_nonzero(present), int(np.flatnonzero(present).max()) + 1 if present.any() else 0,
                       np.count_nonzero((lab < 0) | (lab > M))], np.int64)
    inten = None
    if image is not None:
        image = np.asarray(image)
        img = image[None] if image.ndim == 2 else image
        assert img.shape[1:] == lab.shape
        C = img.shape[0]
        if img.dtype == np.float32:
            inten = np.zeros((M, C, ICOLS), np.float64)
            order = np.argsort(ids, kind="stable")
            sid = ids[order]
            starts = np.flatnonzero(np.r_[True, sid[1:] != sid[:-1]]) if len(sid) else np.zeros(0, np.int64)
            ends = np.r_[starts[1:], len(sid)]
            for c in range(C):
                v = img[c][valid].astype(np.float64)[order]
                for s, e in zip(starts, ends):
                    seg = v[s:e]
                    inten[sid[s], c] = (math.fsum(seg), math.fsum(seg * seg), seg.min(), seg.max())
        else:
            assert img.dtype in (np.uint8, np.uint16)
            inten = np.zeros((M, C, ICOLS), np.int64)
            inten[:, :, 2] = np.iinfo(np.int64).max
            for c in range(C):
                v = img[c][valid].astype(np.int64)
                np.add.at(inten[:, c, 0], ids, v)
                np.add.at(inten[:, c, 1], ids, v * v)
                np.minimum.at(inten[:, c, 2], ids, v)
                np.maximum.at(inten[:, c, 3], ids, v)
            inten[~present] = 0
    return {"table": tab, "status": status, "intensity": inten}


def frames(labs, max_instances=MAX_INSTANCES, images=None):
    """the same, stacked over the frames of labs [N][H][W] (images [N][H][W] or [N][C][H][W])"""
    per = [tables(l, max_instances, None if images is None else images[i]) for i, l in enumerate(labs)]
    return {"table": np.stack([p["table"] for p in per]), "status": np.stack([p["status"] for p in per]),
            "intensity": None if images is None else np.stack([p["intensity"] for p in per])}


def select(lab, keep):
    """(relabelled map int32, count, new_ids int32 [M]) of one frame and one keep vector"""
    lab, keep = np.asarray(lab), np.asarray(keep).astype(bool)
    M = keep.shape[0]
    new_ids = np.where(keep, np.cumsum(keep), 0).astype(np.int32)
    lut = np.concatenate([[0], new_ids]).astype(np.int32)
    inside = (lab >= 1) & (lab <= M)
    return np.where(inside, lut[np.clip(lab, 0, M)], 0).astype(np.int32), int(keep.sum()), new_ids


# ---- label patterns -----------------------------------------------------------------

def random_labels(p, h=H0, w=W0, seed=1):
    """scipy's labels of a random mask: many small instances, ids in raster order"""
    return iref.label(iref.random_mask(p, h, w, seed))[0]


def dilated(lab, radius=8):
    """every background pixel within `radius` of an instance takes the nearest one's id (as grow_instances
    does): the instances then span tiles and touch each other"""
    dist, idx = ndimage.distance_transform_edt(lab == 0, return_indices=True)
    grown = lab[idx[0], idx[1]]
    return np.where(dist <= radius, grown, 0).astype(np.int32)


def all_one(h=H0, w=W0):
    return np.ones((h, w), np.int32)


def own_ids():
    """every pixel of one 32 x 64 tile its own id 1..2048: far more ids than the tile's LDS table holds"""
    return np.arange(1, 2049, dtype=np.int32).reshape(32, 64)


def noise(h=H0, w=W0, seed=11, ids=64):
    """per-pixel noise of ids 0..ids-1"""
    return np.random.default_rng(seed).integers(0, ids, (h, w)).astype(np.int32)


def vstripes(width, h=H0, w=W0):
    return (np.arange(w)[None, :] // width + 1 + np.zeros((h, 1), np.int64)).astype(np.int32)


def hstripes(width, h=H0, w=W0):
    return (np.arange(h)[:, None] // width + 1 + np.zeros((1, w), np.int64)).astype(np.int32)


def bars(h=H0, w=W0):
    """bars across the lane-63 / tile borders in x and the row-32 borders in y, two of them abutting"""
    a = np.zeros((h, w), np.int32)
    a[10, 60:70] = 1            # a run across the column-64 border
    a[31:33, 5:9] = 2           # across the row-32 border
    a[40:50, 63] = 3            # on the last lane
    a[40:50, 64] = 4            # on the first lane of the next tile, abutting 3
    a[60:70, 0:w] = 5           # a whole row band, frame to frame
    a[0:h, 100] = 6             # a whole column (crosses 5: the later assignment wins)
    a[h - 1, w - 3:w] = 7       # in the last corner
    return a


def sparse_ids(h=H0, w=W0):
    a = np.zeros((h, w), np.int32)
    a[3:20, 4:30] = 7
    a[20:50, 4:90] = 900        # abuts 7
    a[100:130, 70:131] = 4096   # the cap itself, on the frame
    return a


def out_of_range(h=H0, w=W0):
    """ids above the cap and below 0, as pixels and as neighbours of valid instances"""
    a = np.zeros((h, w), np.int32)
    a[10:20, 10:20] = 5
    a[10:20, 20:25] = MAX_INSTANCES + 1   # right neighbour of 5: contact
    a[20:22, 10:20] = -3                  # below 5: contact
    a[60:70, 60:70] = 2147483647
    a[60:70, 70:80] = 9
    a[0, 0] = -2147483648
    a[0, 1] = 11
    return a


def empty(h=H0, w=W0):
    return np.zeros((h, w), np.int32)


PATTERNS = {
    "random35": lambda: random_labels(0.35), "random55": lambda: random_labels(0.55),
    "random35_grown": lambda: dilated(random_labels(0.35)), "random55_grown": lambda: dilated(random_labels(0.55)),
    # fewer seeds: grown by 8 px they become cells of some hundred pixels that span tiles and touch
    "cells_grown": lambda: dilated(random_labels(0.02, seed=3)),
    "blobs_grown": lambda: dilated(random_labels(0.005, seed=4)),
    "all_one": all_one, "own_ids": own_ids, "noise64": noise, "noise512": lambda: noise(ids=512),
    "vstripes1": lambda: vstripes(1), "vstripes64": lambda: vstripes(64), "hstripes1": lambda: hstripes(1),
    "hstripes64": lambda: hstripes(64), "bars": bars, "sparse_ids": sparse_ids, "out_of_range": out_of_range,
    "empty": empty,
}


@functools.lru_cache(maxsize=None)
def pattern(name):
    a = PATTERNS[name]()
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def expected(name, max_instances=MAX_INSTANCES):
    out = tables(pattern(name), max_instances)
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out


# ---- images ---------------------------------------------------------------------------

def image(dtype, channels=None, h=H0, w=W0, seed=5):
    """uint8 / uint16 noise over the whole range (0 and the largest value are planted), or non-negative
    float32; [h][w] without channels, else [channels][h][w]"""
    rng = np.random.default_rng(seed)
    shape = (h, w) if channels is None else (channels, h, w)
    if dtype == np.float32:
        return (rng.random(shape) * 1000.0).astype(np.float32)
    hi = np.iinfo(dtype).max
    img = rng.integers(0, hi + 1, shape).astype(dtype)
    flat = img.reshape(-1)
    flat[::7] = hi
    flat[3::11] = 0
    return img


def signed_image(h=H0, w=W0, seed=6):
    """float32 with negative values, -0.0 and +0.0"""
    rng = np.random.default_rng(seed)
    img = ((rng.random((h, w)) - 0.5) * 200.0).astype(np.float32)
    flat = img.reshape(-1)
    flat[::5] = -0.0
    flat[2::13] = 0.0
    return img
