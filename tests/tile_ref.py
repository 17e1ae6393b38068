"""float32 numpy restatement of the tiled-inference geometry and blend
(csrc/tile.hip, predict.py), shared by test_predict.py, test_tile_gpu.py and
test_predict_gpu.py.  A helper module, not a conftest.

Square tiles T x T, overlap O, stride S = T - O, 0 <= O <= T/2.  Dihedral
transform d = k + 4 * flip = "np.rot90(a, k), then [::-1] if flip" of the tile
content; the 8-bit mask ``tta`` selects M of them, m = rank among the set bits.
Flat tile index t = ((n M + m) ny + jy) nx + jx.
"""
import numpy as np

MASK_THRESHOLD = np.float32(8.94069742685133e-08)
assert MASK_THRESHOLD.view(np.uint32) == 0x33C00001  # the project's sigmoid > 0.5 rule for non-negative logits


def origins(length, tile, overlap):
    if length <= tile:
        return [-((tile - length) // 2)]
    s = tile - overlap
    n = -(-(length - tile) // s) + 1
    return [j * s for j in range(n - 1)] + [length - tile]


def w1(tile, overlap):
    """int32 [T]: min(i + 1, T - i, O + 1)"""
    i = np.arange(tile)
    return np.minimum(np.minimum(i + 1, tile - i), overlap + 1).astype(np.int32)


def transforms(tta):
    """the selected d, ascending"""
    return [d for d in range(8) if (tta >> d) & 1]


def dihedral(a, d):
    """transform d of the last two (square) axes"""
    a = np.rot90(a, d & 3, axes=(-2, -1))
    return a[..., ::-1, :] if d & 4 else a


def dihedral_inv(a, d):
    if d & 4:
        a = a[..., ::-1, :]
    return np.rot90(a, -(d & 3), axes=(-2, -1))


def src_index(d, tile, y, x):
    """tile position (y, x) of transform d reads footprint position (sy, sx):
    the index map the gather kernel applies on its read side"""
    if d & 4:
        y = tile - 1 - y
    k = d & 3
    if k == 0:
        return y, x
    if k == 1:
        return x, tile - 1 - y
    if k == 2:
        return tile - 1 - y, tile - 1 - x
    return tile - 1 - x, y


def reflect101(i, n):
    """BORDER_REFLECT_101 of an index array into [0, n)"""
    i = np.array(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    while True:
        bad = (i < 0) | (i >= n)
        if not bad.any():
            return i
        i = np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i))


def tile_table(N, H, W, tile, overlap, tta):
    """[(n, d, oy, ox)] in flat order"""
    oys, oxs = origins(H, tile, overlap), origins(W, tile, overlap)
    return [(n, d, oy, ox) for n in range(N) for d in transforms(tta) for oy in oys for ox in oxs]


def gather(image, tile, overlap, tta, first=0, count=None):
    """image [N][H][W] float32 -> tiles [count][T][T] for t in [first, first + count);
    slots past the last tile are zeros"""
    image = np.asarray(image, dtype=np.float32)
    N, H, W = image.shape
    table = tile_table(N, H, W, tile, overlap, tta)
    count = len(table) - first if count is None else count
    out = np.zeros((count, tile, tile), np.float32)
    u = np.arange(tile)
    for s in range(count):
        t = first + s
        if t >= len(table):
            break
        n, d, oy, ox = table[t]
        fp = image[n][np.ix_(reflect101(oy + u, H), reflect101(ox + u, W))]
        out[s] = dihedral(fp, d)
    return out


def _blend(tile_logits, N, K, H, W, tile, overlap, tta, dtype):
    table = tile_table(N, H, W, tile, overlap, tta)
    tl = np.asarray(tile_logits, dtype=np.float32).reshape(len(table), K, tile, tile)
    w = w1(tile, overlap)
    w2 = w[:, None] * w[None, :]  # int32 [T][T], position inside the footprint
    acc = np.zeros((N, K, H, W), dtype)
    mag = np.zeros((N, K, H, W), np.float64)
    ws = np.zeros((N, H, W), np.int32)
    for t, (n, d, oy, ox) in enumerate(table):
        v = dihedral_inv(tl[t], d)  # back in footprint orientation
        y0, y1, x0, x1 = max(oy, 0), min(oy + tile, H), max(ox, 0), min(ox + tile, W)
        fy, fx = slice(y0 - oy, y1 - oy), slice(x0 - ox, x1 - ox)
        wt = w2[fy, fx]
        term = wt.astype(dtype)[None] * v[:, fy, fx].astype(dtype)  # one rounding (fp32)
        acc[n, :, y0:y1, x0:x1] = acc[n, :, y0:y1, x0:x1] + term     # one rounding (fp32)
        mag[n, :, y0:y1, x0:x1] += np.abs(term.astype(np.float64))
        ws[n, y0:y1, x0:x1] += wt
    return acc, ws, mag


def blend(tile_logits, N, K, H, W, tile, overlap, tta):
    """op-for-op fp32: per pixel, over the covering tiles in ascending t,
    acc = acc + (float)w * v from 0; int32 weight sum; acc / (float)wsum"""
    acc, ws, _ = _blend(tile_logits, N, K, H, W, tile, overlap, tta, np.float32)
    return (acc / ws.astype(np.float32)[:, None]).astype(np.float32)


def blend64(tile_logits, N, K, H, W, tile, overlap, tta):
    """(fp64 value of the same formula, sum w |v| / sum w per pixel)"""
    acc, ws, mag = _blend(tile_logits, N, K, H, W, tile, overlap, tta, np.float64)
    den = ws.astype(np.float64)[:, None]
    return acc / den, mag / den


def mask_rule(logits):
    return (np.asarray(logits, np.float32) >= MASK_THRESHOLD).astype(np.uint8)


def labels_rule(logits):
    """argmax over the class axis, lowest class index on ties"""
    return np.argmax(np.asarray(logits), axis=1).astype(np.uint8)
