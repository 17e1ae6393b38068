"""References of ``nearest_two_instances``, ``border_weight_map``, ``boundary_targets``
(csrc/weights.hip) and of the per-pixel weights of the softmax cross-entropy
(csrc/softmax_loss.hip), and the label maps their tests share.  The transform is exact
integer arithmetic; the weight map and the loss are float64.

Sites are the pixels with ``labels > 0``.  For every pixel the first site minimises the
key ``d2 * 2^31 + flat`` (squared Euclidean distance, then the site's flat index ``y * W
+ x``) over all sites, the second the same key over the sites whose label differs from
the first's.  ``dist2`` / ``ids`` are ``[2, H, W]``; where there is no such site, or it
lies beyond ``max_d2``, ``NONE`` and 0.
"""
import numpy as np
import torch
import torch.nn.functional as F
from scipy import ndimage

import distance_ref as dref
import instances_ref as iref

H0, W0 = iref.H0, iref.W0  # 130 x 131
NONE = dref.NONE
MAX_DIM = 4096             # UNET_TWO_NEAREST_MAX_DIM
_SHIFT = 31
_NOKEY = (np.int64(NONE) << _SHIFT) | np.int64(NONE)


def _finish(key1, key2, flat_labels, max_d2):
    """(dist2 [2,H,W] int32, ids [2,H,W] int32) from the two minimum keys"""
    d, i = [], []
    for key in (key1, key2):
        none = key == _NOKEY
        d2 = key >> _SHIFT
        if max_d2 >= 0:
            none = none | (d2 > max_d2)
        d.append(np.where(none, NONE, d2).astype(np.int32))
        i.append(np.where(none, 0, flat_labels[np.where(none, 0, key & np.int64(NONE))]).astype(np.int32))
    return np.stack(d), np.stack(i)


def brute(labels, max_d2=-1, chunk=256):
    """the definition: minimise the key over all sites, then over the sites of another label"""
    labels = np.asarray(labels, np.int32)
    H, W = labels.shape
    sy, sx = np.nonzero(labels > 0)
    sflat = sy.astype(np.int64) * W + sx
    slab = labels[sy, sx]
    key1 = np.full(H * W, _NOKEY, np.int64)
    key2 = np.full(H * W, _NOKEY, np.int64)
    if sflat.size:
        py, px = np.divmod(np.arange(H * W, dtype=np.int64), W)
        for a in range(0, H * W, chunk):
            d2 = (py[a:a + chunk, None] - sy[None, :]) ** 2 + (px[a:a + chunk, None] - sx[None, :]) ** 2
            key = (d2 << _SHIFT) | sflat[None, :]
            j = key.argmin(axis=1)
            key1[a:a + chunk] = key[np.arange(len(j)), j]
            other = np.where(slab[None, :] != slab[j][:, None], key, _NOKEY)
            key2[a:a + chunk] = other.min(axis=1)
    return _finish(key1.reshape(H, W), key2.reshape(H, W), labels.ravel(), max_d2)


_FAR = np.int64(1) << 20  # "no site" as a row distance


def _sweep(labels):
    """downward sweep of every column: per pixel the rows to the last site at or above it and its
    label, the rows to the last site with another label and that label (_FAR: none)"""
    H, W = labels.shape
    d1 = np.full(W, _FAR)
    d2 = np.full(W, _FAR)
    l1 = np.zeros(W, np.int64)
    l2 = np.zeros(W, np.int64)
    out = np.empty((4, H, W), np.int64)
    for y in range(H):
        v = labels[y].astype(np.int64)
        d1 = np.minimum(d1 + 1, _FAR)
        d2 = np.minimum(d2 + 1, _FAR)
        site = v > 0
        new = site & (d1 < _FAR) & (v != l1)  # a site with a new label: the old first becomes the second
        d2 = np.where(new, d1, d2)
        l2 = np.where(new, l1, l2)
        l1 = np.where(site, v, l1)
        d1 = np.where(site, 0, d1)
        out[:, y] = d1, l1, d2, l2
    return out


def column_candidates(labels):
    """(o1, l1, o2, l2, has1, has2) per pixel: the row offset and label of c1, the column's nearest
    site (the upper one on a tie), and of c2, the nearest site of the column whose label differs
    from c1's (the upper one on a tie)"""
    labels = np.asarray(labels, np.int32)
    ad1, al1, ad2, al2 = _sweep(labels)
    bd1, bl1, bd2, bl2 = _sweep(labels[::-1])[:, ::-1]
    up1 = ad1 <= bd1
    o1 = np.where(up1, -ad1, bd1)
    l1 = np.where(up1, al1, bl1)
    has1 = np.minimum(ad1, bd1) < _FAR
    af = (ad1 < _FAR) & (al1 != l1)
    bf = (bd1 < _FAR) & (bl1 != l1)
    ud, ul = np.where(af, ad1, ad2), np.where(af, al1, al2)
    dd, dl = np.where(bf, bd1, bd2), np.where(bf, bl1, bl2)
    up2 = ud <= dd
    o2 = np.where(up2, -ud, dd)
    l2 = np.where(up2, ul, dl)
    has2 = has1 & (np.minimum(ud, dd) < _FAR)
    return o1, l1, o2, l2, has1, has2


def separable(labels, max_d2=-1):
    """the kernels' form: two candidates per pixel and column, then per row the minimum key over
    all c1 and the minimum key over all c1 and c2 whose label differs from the winner's"""
    labels = np.asarray(labels, np.int32)
    H, W = labels.shape
    o1, l1, o2, l2, has1, has2 = column_candidates(labels)
    xs = np.arange(W, dtype=np.int64)
    dx2 = (xs[:, None] - xs[None, :]) ** 2
    key1 = np.full((H, W), _NOKEY, np.int64)
    key2 = np.full((H, W), _NOKEY, np.int64)
    for y in range(H):
        k1 = np.where(has1[y][None, :], ((o1[y] * o1[y])[None, :] + dx2 << _SHIFT) | ((y + o1[y]) * W + xs)[None, :],
                      _NOKEY)
        k2 = np.where(has2[y][None, :], ((o2[y] * o2[y])[None, :] + dx2 << _SHIFT) | ((y + o2[y]) * W + xs)[None, :],
                      _NOKEY)
        j = k1.argmin(axis=1)
        key1[y] = k1[xs, j]
        win = np.where(key1[y] == _NOKEY, 0, l1[y][j])
        both = np.concatenate([np.where(l1[y][None, :] != win[:, None], k1, _NOKEY),
                               np.where(l2[y][None, :] != win[:, None], k2, _NOKEY)], axis=1)
        key2[y] = both.min(axis=1)
    return _finish(key1, key2, labels.ravel(), max_d2)


def per_id_edt(labels, max_d2=-1):
    """dist2 [2,H,W] alone: the two smallest of rint(distance_transform_edt(labels != i) ** 2) over the ids i"""
    labels = np.asarray(labels, np.int32)
    a = np.full(labels.shape, NONE, np.int64)
    b = np.full(labels.shape, NONE, np.int64)
    for i in np.unique(labels[labels > 0]):
        d = np.rint(ndimage.distance_transform_edt(labels != i) ** 2).astype(np.int64)
        b = np.minimum(b, np.maximum(a, d))
        a = np.minimum(a, d)
    if max_d2 >= 0:
        a = np.where(a > max_d2, NONE, a)
        b = np.where(b > max_d2, NONE, b)
    return np.stack([a, b]).astype(np.int32)


def one_row(labels, max_d2=-1):
    """a frame of one row by sorted search, for widths where W x 2 W does not fit"""
    labels = np.asarray(labels, np.int32)
    assert labels.shape[0] == 1
    W = labels.shape[1]
    row = labels[0]
    pos = np.flatnonzero(row > 0).astype(np.int64)
    key1 = np.full(W, _NOKEY, np.int64)
    key2 = np.full(W, _NOKEY, np.int64)
    n = pos.size
    if n:
        lab = row[pos].astype(np.int64)
        idx = np.arange(n)
        start = np.maximum.accumulate(np.where(np.r_[True, lab[1:] != lab[:-1]], idx, 0))   # first of the run
        end = np.minimum.accumulate(np.where(np.r_[lab[1:] != lab[:-1], True], idx, n)[::-1])[::-1]  # last
        prev_diff, next_diff = start - 1, end + 1     # nearest site of another label on either side (-1 / n: none)
        far = np.int64(1) << 40
        xs = np.arange(W, dtype=np.int64)
        j = np.searchsorted(pos, xs, side="right") - 1  # the site at or left of x; the one right of x is j + 1
        jl, jr = np.clip(j, 0, n - 1), np.clip(j + 1, 0, n - 1)
        dl = np.where(j >= 0, xs - pos[jl], far)
        dr = np.where(j + 1 < n, pos[jr] - xs, far)
        first = np.where(dl <= dr, jl, jr)              # the left site has the smaller index
        key1 = ((pos[first] - xs) ** 2 << _SHIFT) | pos[first]
        l1 = lab[first]
        cl = np.where((j >= 0) & (lab[jl] != l1), jl, np.where(j >= 0, prev_diff[jl], -1))
        cr = np.where((j + 1 < n) & (lab[jr] != l1), jr, np.where(j + 1 < n, next_diff[jr], n))
        d2l = np.where(cl >= 0, xs - pos[np.clip(cl, 0, n - 1)], far)
        d2r = np.where(cr < n, pos[np.clip(cr, 0, n - 1)] - xs, far)
        second = np.clip(np.where(d2l <= d2r, cl, cr), 0, n - 1)
        key2 = np.where(np.minimum(d2l, d2r) < far, ((pos[second] - xs) ** 2 << _SHIFT) | pos[second], _NOKEY)
    return _finish(key1[None], key2[None], row, max_d2)


def reference(labels, max_d2=-1):
    """(dist2, ids) of one frame: the separable form, a sorted search for one long row or column"""
    labels = np.asarray(labels, np.int32)
    if labels.shape[0] == 1 and labels.shape[1] > 1024:
        return one_row(labels, max_d2)
    if labels.shape[1] == 1 and labels.shape[0] > 1024:  # flat index = row: the transposed row
        d2, ids = one_row(labels.T, max_d2)
        return np.ascontiguousarray(d2.transpose(0, 2, 1)), np.ascontiguousarray(ids.transpose(0, 2, 1))
    return separable(labels, max_d2)


max_d2_of = dref.max_d2_of


def weight_map(labels, w0=10.0, sigma=5.0, max_d2=-1, classes=None, class_weights=None, dist2=None):
    """float64 border weight map of one frame: base + w0 exp(-(d1 + d2)^2 / (2 sigma^2)) on unlabelled
    pixels with a second instance in reach; w0 and sigma as the float32 the C ABI takes"""
    labels = np.asarray(labels, np.int32)
    if dist2 is None:
        dist2 = reference(labels, max_d2)[0]
    w0, sigma = np.float64(np.float32(w0)), np.float64(np.float32(sigma))
    base = np.ones(labels.shape, np.float64)
    if classes is not None:
        cw = np.asarray(class_weights, np.float32).astype(np.float64)
        c = np.asarray(classes).astype(np.int64)
        base = np.where(c < cw.size, cw[np.minimum(c, cw.size - 1)], 0.0)
    on = (labels <= 0) & (dist2[1] != NONE)
    s = np.sqrt(dist2[0].astype(np.float64)) + np.sqrt(dist2[1].astype(np.float64))
    border = np.where(on, w0 * np.exp(-(s * s) / (2.0 * sigma * sigma)), 0.0)
    return base + border


def boundary_targets(labels, connectivity=2):
    """uint8 0 background, 1 interior, 2 boundary (a labelled pixel with a neighbour inside the
    frame of another value), by compares of shifted arrays"""
    labels = np.asarray(labels, np.int32)
    H, W = labels.shape
    diff = np.zeros((H, W), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if (dy == 0 and dx == 0) or (connectivity == 1 and dy != 0 and dx != 0):
                continue
            a = labels[max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)]    # the neighbour
            b = labels[max(-dy, 0):H + min(-dy, 0), max(-dx, 0):W + min(-dx, 0)]  # the pixel
            diff[max(-dy, 0):H + min(-dy, 0), max(-dx, 0):W + min(-dx, 0)] |= a != b
    return np.where(labels <= 0, 0, np.where(diff, 2, 1)).astype(np.uint8)


def weighted_loss(x, y, cw=None, pw=None, ign=-100, alpha=0.5, smooth=1.0, grad=False):
    """float64 on the CPU: ({"ce_num", "w_den"}, {kind: loss}, {kind: dL/dlogits} when grad).
    CE = (F.cross_entropy(x, y, weight=cw, ignore_index=ign, reduction="none") * pw).sum()
         / (cw[y] * pw)[valid].sum(), 0 when the denominator is 0; Dice is unweighted."""
    x, y = x.detach().cpu(), y.detach().cpu().long()
    if y.dim() == 4:
        y = y[:, 0]
    k = x.shape[1]
    valid = (y >= 0) & (y < k) & (y != ign)
    yy = torch.where(valid, y, torch.full_like(y, -100))
    z = x.double().requires_grad_(grad)
    wt = None if cw is None else cw.detach().cpu().double()
    p_w = torch.ones(y.shape, dtype=torch.float64) if pw is None else pw.detach().cpu().double().reshape(y.shape)
    ce_num = (F.cross_entropy(z, yy, weight=wt, ignore_index=-100, reduction="none") * p_w).sum()
    yc = y.clamp(0, k - 1)
    per = p_w if wt is None else wt[yc] * p_w
    w_den = per[valid].sum()
    ce = ce_num / w_den if w_den.item() > 0 else ce_num * 0
    vf = valid.double()
    p = torch.softmax(z, 1)
    oh = F.one_hot(yc, k).permute(0, 3, 1, 2).double() * vf[:, None]
    I, P, Y = (p * oh).sum((0, 2, 3)), (p * vf[:, None]).sum((0, 2, 3)), oh.sum((0, 2, 3))
    dice = 1 - ((2 * I + smooth) / (P + Y + smooth)).mean()
    losses = {0: ce, 1: dice, 2: alpha * ce + (1 - alpha) * dice}
    grads = {}
    if grad:
        for kind, v in losses.items():
            grads[kind] = torch.autograd.grad(v, z, retain_graph=True)[0]
    sums = {"ce_num": ce_num.item(), "w_den": w_den.item(), "valid": int(valid.sum())}
    return sums, {kk: v.item() for kk, v in losses.items()}, grads


# ---- label maps -------------------------------------------------------------------

def _empty(h=H0, w=W0):
    return np.zeros((h, w), np.int32)


def one_instance(h=H0, w=W0):
    m = _empty(h, w)
    m[h // 3:h // 2, w // 4:w // 2] = 5
    return m


def mirrored_columns(h=H0, w=W0):
    """two single-pixel instances mirrored about the centre column: d1 == d2 on every pixel of it"""
    m = _empty(h, w)
    c = w // 2
    m[40, c - 17] = 1
    m[40, c + 17] = 2
    return m


def mirrored_rows(h=H0, w=W0):
    """two single-pixel instances mirrored about row (h - 1) // 2"""
    m = _empty(h, w)
    r = (h - 1) // 2
    m[r - 23, 30] = 2
    m[r + 23, 30] = 1
    return m


def stacked(h=H0, w=W0):
    """two instances in one column and nothing else: the second comes from c2 of that column"""
    m = _empty(h, w)
    m[20:23, 77] = 3
    m[90:94, 77] = 9
    return m


def ring_and_disc(h=H0, w=W0):
    yy, xx = np.mgrid[:h, :w]
    r2 = (yy - h // 2) ** 2 + (xx - w // 2) ** 2
    m = _empty(h, w)
    m[r2 <= 15 ** 2] = 1
    m[(r2 >= 40 ** 2) & (r2 <= 46 ** 2)] = 2
    return m


def own_ids(h=H0, w=W0):
    """every pixel its own id: every candidate has a distinct label"""
    return (np.arange(h * w, dtype=np.int32) + 1).reshape(h, w)


def large_ids(h=H0, w=W0):
    """ids 2^31 - 1 and other non-contiguous large ones; negative values are unlabelled"""
    rng = np.random.default_rng(7)
    pool = np.array([2147483647, 2147483646, 1 << 30, 65536, 65535, 70001, 3], np.int32)
    m = _empty(h, w)
    pick = rng.random((h, w)) < 0.01
    m[pick] = pool[rng.integers(0, pool.size, int(pick.sum()))]
    neg = rng.random((h, w)) < 0.05
    m[neg & ~pick] = -rng.integers(1, 1 << 30, int((neg & ~pick).sum())).astype(np.int32)
    m[5, 5], m[5, 9] = 2147483647, -2147483648
    return m


def touching_edges(h=H0, w=W0):
    """instances touching the frame edge and each other"""
    m = _empty(h, w)
    m[0:10, 0:12] = 1
    m[0:10, 12:30] = 2
    m[h - 6:h, w - 9:w] = 3
    m[50:70, w - 1] = 4
    m[h - 1, 20:60] = 5
    return m


PATTERNS = {
    "none": _empty, "one": one_instance, "mirrored_columns": mirrored_columns, "mirrored_rows": mirrored_rows,
    "stacked": stacked, "ring_and_disc": ring_and_disc, "own_ids": own_ids, "large_ids": large_ids,
    "random02": lambda: dref.random_labels(0.02)[0], "random30": lambda: dref.random_labels(0.3)[0],
}
