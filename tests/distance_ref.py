"""References of ``distance_transform`` and ``grow_instances`` (csrc/distance.hip)
and the site patterns their tests share.  Everything is exact integer arithmetic.

For every pixel the result is the minimum over the sites of the key
``d2 * 2^31 + flat`` (squared Euclidean distance, then the site's flat index
``y * W + x``): ``dist2`` is the key's upper part, ``nearest`` its lower part.  A
frame without a site gives ``NONE`` and -1.
"""
import numpy as np

import instances_ref as iref

H0, W0 = iref.H0, iref.W0  # 130 x 131
NONE = 2147483647
_SHIFT = 31
_NOKEY = (np.int64(NONE) << _SHIFT) | np.int64(NONE)


def sites_of(mask, fg=None, invert=False):
    """bool sites of a mask as unet_distance_transform defines them (sites = int(invert))"""
    f = iref.foreground(mask, fg)
    return f if invert else ~f


def _split(key):
    d2 = (key >> _SHIFT).astype(np.int64)
    nearest = np.where(key == _NOKEY, -1, key & np.int64(NONE))
    return d2.astype(np.int32), nearest.astype(np.int32)


def brute(site, chunk=4096, count_ties=False):
    """the definition: minimise d2 * 2^31 + flat over all sites, pixels in chunks"""
    site = np.asarray(site, bool)
    H, W = site.shape
    sy, sx = np.nonzero(site)
    sflat = sy.astype(np.int64) * W + sx
    key = np.full(H * W, _NOKEY, np.int64)
    ties = np.zeros(H * W, np.int64)
    if sflat.size:
        py, px = np.divmod(np.arange(H * W, dtype=np.int64), W)
        for a in range(0, H * W, chunk):
            d2 = (py[a:a + chunk, None] - sy[None, :]) ** 2 + (px[a:a + chunk, None] - sx[None, :]) ** 2
            key[a:a + chunk] = ((d2 << _SHIFT) | sflat[None, :]).min(axis=1)
            ties[a:a + chunk] = (d2 == d2.min(axis=1, keepdims=True)).sum(axis=1)
    d2, nearest = _split(key.reshape(H, W))
    return (d2, nearest, ties.reshape(H, W)) if count_ties else (d2, nearest)


def column_offsets(site):
    """(offset of the column's nearest site per pixel, the upper one on a tie; bool 'the column has a site')"""
    site = np.asarray(site, bool)
    H = site.shape[0]
    yy = np.arange(H, dtype=np.int64)[:, None]
    far = np.int64(1) << 20
    up = np.maximum.accumulate(np.where(site, yy, -far), axis=0)
    dn = np.minimum.accumulate(np.where(site, yy, far)[::-1], axis=0)[::-1]
    du, dd = yy - up, dn - yy
    return np.where(du <= dd, -du, dd), site.any(axis=0)


def separable(site):
    """the kernels' form: column offsets, then per row the minimum key over columns"""
    site = np.asarray(site, bool)
    H, W = site.shape
    off, has = column_offsets(site)
    xs = np.arange(W, dtype=np.int64)
    dx2 = (xs[:, None] - xs[None, :]) ** 2
    key = np.full((H, W), _NOKEY, np.int64)
    if has.any():
        cols = xs[has]
        for y in range(H):
            o = off[y, has]
            k = ((o * o)[None, :] + dx2[:, has] << _SHIFT) | ((y + o) * W + cols)[None, :]
            key[y] = k.min(axis=1)
    return _split(key)


def one_row(site):
    """a frame of one row by sorted search, for widths where W x W does not fit"""
    site = np.asarray(site, bool)
    assert site.shape[0] == 1
    W = site.shape[1]
    pos = np.flatnonzero(site[0]).astype(np.int64)
    if pos.size == 0:
        return np.full((1, W), NONE, np.int32), np.full((1, W), -1, np.int32)
    xs = np.arange(W, dtype=np.int64)
    j = np.searchsorted(pos, xs, side="right")          # sites at or left of x: pos[j - 1]
    left = pos[np.clip(j - 1, 0, pos.size - 1)]
    right = pos[np.clip(j, 0, pos.size - 1)]
    dl = np.where(j > 0, xs - left, np.int64(1) << 40)
    dr = np.where(j < pos.size, right - xs, np.int64(1) << 40)
    near = np.where(dl <= dr, left, right)              # the left site has the smaller index
    return (((near - xs) ** 2).astype(np.int32)[None], near.astype(np.int32)[None])


def reference(site):
    """(dist2, nearest) of one frame: the separable form, a sorted search for one long row or column"""
    site = np.asarray(site, bool)
    if site.shape[0] == 1 and site.shape[1] > 4096:
        return one_row(site)
    if site.shape[1] == 1 and site.shape[0] > 4096:  # flat index = row: the transposed row
        d2, nearest = one_row(site.T)
        return np.ascontiguousarray(d2.T), np.ascontiguousarray(nearest.T)
    return separable(site)


def grow(labels, max_d2=-1, within=None, within_value=None, transform=reference):
    """unet_grow_instances of one frame; max_d2 < 0 is unlimited"""
    labels = np.asarray(labels, np.int32)
    d2, nearest = transform(labels != 0)
    ok = nearest >= 0
    if max_d2 >= 0:
        ok &= d2.astype(np.int64) <= max_d2
    if within is not None:
        ok &= iref.foreground(within, within_value)
    taken = labels.ravel()[np.maximum(nearest, 0)]
    return np.where(labels != 0, labels, np.where(ok, taken, 0)).astype(np.int32)


def max_d2_of(max_distance):
    return -1 if max_distance is None else int(np.floor(np.float64(max_distance) ** 2))


# ---- patterns (as site masks: nonzero = site) -------------------------------------

def single(y, x, h=H0, w=W0):
    m = iref.empty(h, w)
    m[y, x] = 1
    return m


def mirrored_columns(h=H0, w=W0):
    """pairs of sites mirrored about the centre column: every pixel of that column is tied"""
    m = iref.empty(h, w)
    c = w // 2
    for y, k in ((10, 3), (64, 40), (120, c)):
        m[y, c - k] = m[y, c + k] = 1
    return m


def mirrored_rows(h=H0, w=W0):
    """pairs of sites mirrored about row (h - 1) // 2: every pixel of that row is tied"""
    m = iref.empty(h, w)
    c = (h - 1) // 2
    for x, k in ((7, 2), (66, 31), (125, c)):
        m[c - k, x] = m[c + k, x] = 1
    return m


PATTERNS = {
    "empty": iref.empty, "full": iref.full,
    "corner_tl": lambda: single(0, 0), "corner_tr": lambda: single(0, W0 - 1),
    "corner_bl": lambda: single(H0 - 1, 0), "corner_br": lambda: single(H0 - 1, W0 - 1),
    "checkerboard": iref.checkerboard, "mirrored_columns": mirrored_columns, "mirrored_rows": mirrored_rows,
    "side_columns": iref.side_columns, "comb": iref.comb, "rings": iref.rings,
    "random02": lambda: iref.random_mask(0.02), "random50": lambda: iref.random_mask(0.5),
    "random98": lambda: iref.random_mask(0.98),
}


def random_labels(p=0.3, h=H0, w=W0, seed=1, connectivity=1):
    """(int32 labels, count) of a random mask, as label_instances numbers them"""
    lab, n, _ = iref.label(iref.random_mask(p, h, w, seed), connectivity)
    return lab, n
