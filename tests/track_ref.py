"""Reference of ``link_instances`` (csrc/track.hip, track.py) in numpy and Python
integers on top of ``match_ref.tables`` (imported, not modified), and the label-map
sequences its tests share.

``link`` is the rule of the C header word for word: a frame's instance continues a
track when it and its highest-IoU partner of the frame before choose each other and
their IoU is strictly above ``min_iou``; otherwise it starts a track, with that
partner's track as parent when more than half of it lies on the partner.
"""
import functools
from fractions import Fraction

import numpy as np

import match_ref

H0, W0, T0 = 70, 131, 6   # the main scene: three 32-row tiles and an odd width, 9170 pixels per frame (not a multiple of 4)
COLS, STATUS = 4, 4


def link(stack, min_iou, M, max_tracks):
    """One sequence [T][H][W] -> (tracks [T][H][W], table [max_tracks][4], n_tracks, n_links)."""
    num, den = min_iou.numerator, min_iou.denominator
    out = np.zeros_like(stack); table = np.zeros((max_tracks, 4), np.int64); n = links = 0; prev = {}  # noqa: E702
    for t in range(stack.shape[0]):
        cur = {}; tab = match_ref.tables(stack[t - 1], stack[t], M, M) if t else None  # noqa: E702
        for b in [int(i) for i in np.unique(stack[t]) if 0 < i <= M]:          # ascending
            area = int((stack[t] == b).sum()); trk = par = 0  # noqa: E702
            if t:
                _, a, c, aa = (int(v) for v in tab["pred_table"][b - 1])
                if a and int(tab["gt_table"][a - 1][1]) == b and c * den > num * (aa + area - c):
                    trk = prev[a]; links += 1  # noqa: E702
                elif a and 2 * c > area:
                    par = prev[a]
            if not trk:
                n += 1; trk = n  # noqa: E702
                if trk <= max_tracks: table[trk - 1] = (t, t, par, 0)  # noqa: E701
            if trk <= max_tracks: table[trk - 1][1] = t; table[trk - 1][3] += area  # noqa: E701,E702
            cur[b] = trk; out[t][stack[t] == b] = trk  # noqa: E702
        prev = cur
    return out, table, n, links


def pair_status(stack, M):
    """(dropped, out_of_range) as link_instances reports them: those of match_ref.tables summed over the frame
    pairs; a single frame is matched against itself"""
    T = stack.shape[0]
    pairs = [(stack[t - 1], stack[t]) for t in range(1, T)] or [(stack[0], stack[0])]
    st = [match_ref.tables(g, p, M, M)["status"] for g, p in pairs]
    return int(sum(s[3] for s in st)), int(sum(s[4] for s in st))


def expected(stack, min_iou, M, max_tracks):
    """a batch [B][T][H][W] -> dict(tracks [B][T][H][W], table [B][max_tracks][4], status [B][4])"""
    stack = np.asarray(stack)
    assert stack.ndim == 4
    min_iou = Fraction(min_iou).limit_denominator(1000)
    tracks, table, status = [], [], []
    for s in stack:
        tr, tb, n, links = link(s, min_iou, M, max_tracks)
        tracks.append(tr)
        table.append(tb)
        status.append((n, links) + pair_status(s, M))
    return {"tracks": np.stack(tracks).astype(np.int32), "table": np.stack(table),
            "status": np.array(status, np.int64).reshape(-1, STATUS)}


# ---- sequences: int32 [T][H][W] ---------------------------------------------------------

def _disk(a, cy, cx, r, v):
    yy, xx = np.ogrid[:a.shape[0], :a.shape[1]]
    a[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = v


# the objects of the main scene, by a fixed key; the per-frame ids are perm_t[key]
DRIFT, MOTHER, LEFT, RIGHT, BLINK, LATE, JUMP = range(7)


def scene_objects(t):
    """the disks (key, cy, cx, r) of frame t of the main scene"""
    objs = [(DRIFT, 12, 12 + 3 * t, 8)]                  # a drifting disk
    if t < 3:
        objs.append((MOTHER, 40, 40, 10))                  # a mother of r = 10 ...
    else:                                                  # ... that splits at t = 3 into two r = 6 daughters moving apart
        d = 6 + 2 * (t - 3)
        objs += [(LEFT, 40, 40 - d, 6), (RIGHT, 40, 40 + d, 6)]
    if t != 2:
        objs.append((BLINK, 15, 80, 7))                    # a disk missing in frame 2
    if t >= 4:
        objs.append((LATE, 50, 90, 6))                     # a disk appearing at t = 4
    if 40 + 12 * t + 5 < H0:
        objs.append((JUMP, 40 + 12 * t, 120, 5))           # an r = 5 disk jumping 12 px per frame until it leaves the frame
    return objs


@functools.lru_cache(maxsize=None)
def scene_ids(seed=5):
    """per frame a dict key -> id, drawn from a random permutation of 1..40"""
    rng = np.random.default_rng(seed)
    return tuple({k: int(v) for k, v in enumerate(rng.permutation(40)[:7] + 1)} for _ in range(T0))


@functools.lru_cache(maxsize=None)
def scene(seed=5):
    out = np.zeros((T0, H0, W0), np.int32)
    ids = scene_ids(seed)
    for t in range(T0):
        for key, cy, cx, r in scene_objects(t):
            _disk(out[t], cy, cx, r, ids[t][key])
    out.setflags(write=False)
    return out


def half():
    """a frame pair with IoU exactly 1 / 2: no link at min_iou = 1 / 2, but a parent (the whole of frame 1's instance lies on it)"""
    out = np.zeros((2, 8, 9), np.int32)
    out[0, 3, 2:4] = 1
    out[1, 3, 3] = 1
    return out


def tie():
    """equal daughters: a 4 x 8 block splits into two 4 x 4 halves of ids 5 and 3; both reach IoU 1 / 2 with the
    mother, whose best partner is the smaller id"""
    out = np.zeros((2, 12, 20), np.int32)
    out[0, 4:8, 6:14] = 2
    out[1, 4:8, 6:10] = 5
    out[1, 4:8, 10:14] = 3
    return out


def merge():
    """two cells into one: the merged cell continues the track of the larger one, the other track ends"""
    out = np.zeros((3, 12, 20), np.int32)
    for t in range(2):
        out[t, 4:8, 3:7] = 1
        out[t, 4:8, 8:14] = 2
    out[2, 4:8, 3:14] = 7
    return out


def blocks(T, H, W, seed, max_id=40, empty=()):
    """a field of blocks of 5 x 7 pixels with random ids (a third background) that moves one pixel per frame along
    x, every frame with ids of its own drawn from 1..max_id; a few blocks vanish per frame.  `empty`: frames set to 0"""
    rng = np.random.default_rng(seed)
    gy, gx = (H + 4) // 5, (W + T + 6) // 7
    n = gy * gx
    keys = rng.permutation(n)[:min(n, max_id, 24)]
    field = np.zeros(n, np.int64)
    field[keys] = np.arange(1, len(keys) + 1)
    field = np.where(rng.random(n) < 0.33, 0, field).reshape(gy, gx)
    big = np.kron(field, np.ones((5, 7), np.int64))
    out = np.zeros((T, H, W), np.int32)
    for t in range(T):
        lut = np.zeros(len(keys) + 1, np.int64)
        lut[1:] = rng.permutation(max_id)[:len(keys)] + 1
        lut[1:][rng.random(len(keys)) < 0.15] = 0
        out[t] = lut[big[:H, T - t:T - t + W]]
    for t in empty:
        out[t] = 0
    return out
