"""scipy.ndimage reference of ``label_instances`` (csrc/instances.hip) and the
mask patterns its tests share.  Everything is exact integer arithmetic.

Order of operations: fill holes, then label, then ``min_area``.
"""
import numpy as np
from scipy import ndimage

H0, W0 = 130, 131  # two 64-tiles (four 32-row tiles) plus a remainder per axis, odd width


def foreground(mask, fg=None):
    mask = np.asarray(mask)
    return mask != 0 if fg is None else mask == fg


def fill(fgmask):
    return ndimage.binary_fill_holes(fgmask)


def label(fgmask, connectivity=1, min_area=0, fill_holes=False):
    """(labels int32, count, the mask that was labelled before min_area) of one 2-D frame."""
    fgmask = np.asarray(fgmask, bool)
    if fill_holes:
        fgmask = fill(fgmask)
    st = ndimage.generate_binary_structure(2, connectivity)
    lab, n = ndimage.label(fgmask, structure=st)
    if min_area > 0 and n:
        area = ndimage.sum(np.ones_like(lab), lab, index=np.arange(1, n + 1))
        keep = np.concatenate([[False], area >= min_area])[lab]
        lab, n = ndimage.label(keep, structure=st)
    return lab.astype(np.int32), int(n), fgmask


def stats(lab, n, max_instances):
    """int64 [max_instances][7] = area, sum_y, sum_x, y0, x0, y1, x1; rows >= min(n, max_instances) zero."""
    out = np.zeros((max_instances, 7), np.int64)
    k = min(n, max_instances)
    if k == 0:
        return out
    idx = np.arange(1, k + 1)
    yy, xx = np.mgrid[:lab.shape[0], :lab.shape[1]]
    out[:k, 0] = np.rint(ndimage.sum(np.ones_like(lab), lab, index=idx)).astype(np.int64)
    out[:k, 1] = np.rint(ndimage.sum(yy, lab, index=idx)).astype(np.int64)
    out[:k, 2] = np.rint(ndimage.sum(xx, lab, index=idx)).astype(np.int64)
    for i, sl in enumerate(ndimage.find_objects(lab, max_label=k)):
        out[i, 3:] = (sl[0].start, sl[1].start, sl[0].stop, sl[1].stop)
    return out


# ---- patterns -------------------------------------------------------------------

def empty(h=H0, w=W0):
    return np.zeros((h, w), np.uint8)


def full(h=H0, w=W0):
    return np.ones((h, w), np.uint8)


def corners(h=H0, w=W0):
    m = empty(h, w)
    m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = 1
    return m


def checkerboard(h=H0, w=W0):
    yy, xx = np.mgrid[:h, :w]
    return ((yy + xx) % 2 == 0).astype(np.uint8)


def serpentine(h=H0, w=W0):
    """even rows full, joined alternately at the right and the left end: one component"""
    m = empty(h, w)
    m[0::2] = 1
    for k, y in enumerate(range(1, h - 1, 2)):
        m[y, w - 1 if k % 2 == 0 else 0] = 1
    return m


def comb(h=H0, w=W0):
    """every second column plus the bottom row: the teeth of a tile join only through another tile"""
    m = empty(h, w)
    m[:, 0::2] = 1
    m[-1, :] = 1
    return m


def side_columns(h=H0, w=W0):
    m = empty(h, w)
    m[:, 0] = m[:, -1] = 1
    return m


def random_mask(p, h=H0, w=W0, seed=1):
    return (np.random.default_rng(seed).random((h, w)) < p).astype(np.uint8)


def rings(h=H0, w=W0):
    """rings that straddle tile borders, a hole open to the frame edge, a ring inside a ring's hole"""
    m = empty(h, w)

    def ring(y0, x0, y1, x1):
        m[y0:y1, x0] = m[y0:y1, x1 - 1] = 1
        m[y0, x0:x1] = m[y1 - 1, x0:x1] = 1

    ring(20, 50, 45, 80)      # across the row-32 and column-64 borders
    ring(60, 5, 110, 70)      # outer ring across several tiles ...
    ring(75, 20, 95, 50)      # ... with a ring inside its hole
    ring(100, 100, 128, 131)  # closed, touching the right frame edge with its wall
    m[0:15, 90] = m[14, 90:110] = m[0:15, 109] = 1  # a "U" open to the top edge: not a hole
    m[62, 125:131] = m[70, 125:131] = m[62:71, 125] = 1  # open to the right edge
    return m


PATTERNS = {
    "empty": empty, "full": full, "corners": corners, "checkerboard": checkerboard, "serpentine": serpentine,
    "comb": comb, "side_columns": side_columns,
    "random35": lambda: random_mask(0.35), "random55": lambda: random_mask(0.55), "random62": lambda: random_mask(0.62),
}
