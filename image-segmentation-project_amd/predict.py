"""Tiled whole-frame inference: ``predict`` runs the tile-sized eval forward over a
sliding window of a frame of ANY size and blends the overlaps on the GPU
(``csrc/tile.hip``: ``unet_tile_gather`` / ``unet_tile_blend``).  No reference
counterpart (the reference predicts at the training size only).

Geometry (the one definition the kernels, ``tile_origins`` and the tests share):
square tiles ``T x T``, overlap ``O``, stride ``S = T - O``, ``0 <= O <= T/2``.
Per axis of length ``L``: ``L <= T`` gives one centred tile at ``-((T - L) // 2)``
whose footprint outside the image is filled by BORDER_REFLECT_101; ``L > T``
gives ``ceil((L - T) / S) + 1`` tiles at ``j S`` and, last, ``L - T`` (nothing is
padded).  A tile position ``(u, v)`` weighs ``w1(u) w1(v)``, ``w1(i) = min(i + 1,
T - i, O + 1)``; the blended logit is ``sum(w v) / sum(w)`` over the covering tiles
in ascending flat tile index ``t = ((n M + m) ny + jy) nx + jx`` (``m`` = rank of
the dihedral transform among the ``M`` selected ones).  The result is
bit-reproducible.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

OUTPUTS = ("logits", "mask", "labels")
# dihedral transform d = k + 4 * flip: np.rot90(a, k), then [::-1] if flip
TTA_FLIPS = (1 << 0) | (1 << 4) | (1 << 6)  # identity, vflip (0, 1), hflip = (2, 1)


def tile_origins(length: int, tile: int, overlap: int) -> list:
    """Tile origins along one axis of ``length`` pixels (module docstring)."""
    length, tile, overlap = int(length), int(tile), int(overlap)
    if length < 1 or tile < 1 or overlap < 0 or 2 * overlap > tile:
        raise ValueError(f"tile_origins: length {length}, tile {tile} must be >= 1 and overlap {overlap} in [0, tile/2]")
    if length <= tile:
        return [-((tile - length) // 2)]
    stride = tile - overlap
    n = -(-(length - tile) // stride) + 1
    return [j * stride for j in range(n - 1)] + [length - tile]


def tta_mask(tta) -> int:
    """The 8-bit transform mask of a ``tta`` argument: False -> identity, True
    -> all 8, ``"flips"`` -> identity + vflip + hflip, an int -> itself, an
    iterable of ``(k, flip)`` pairs -> those transforms."""
    if isinstance(tta, (bool, np.bool_)):
        return 0xFF if tta else 0x01
    if isinstance(tta, str):
        if tta == "flips":
            return TTA_FLIPS
        raise ValueError(f"tta={tta!r}: the only named set is 'flips'")
    if isinstance(tta, (int, np.integer)):
        mask = int(tta)
    else:
        mask = 0
        try:
            for k, flip in tta:
                mask |= 1 << ((int(k) % 4) + (4 if flip else 0))
        except TypeError:
            raise ValueError(f"tta={tta!r}: expected a bool, 'flips', an int mask or (k, flip) pairs") from None
    if not 1 <= mask <= 0xFF:
        raise ValueError(f"tta selects no transform or bits above 0xFF (mask {mask:#x})")
    return mask


def _as_input(images):
    """('u8', frames) for uint8 frames, ('f', tensor [N, H, W]) for float images;
    ValueError on any other rank / dtype.  Touches no GPU."""
    if isinstance(images, (list, tuple)):
        if not len(images):
            raise ValueError("predict: no frames")
        dts = {f.dtype if isinstance(f, torch.Tensor) else np.asarray(f).dtype for f in images}
        if dts not in ({torch.uint8}, {np.dtype(np.uint8)}) or any(np.ndim(f) != 2 for f in images):
            raise ValueError("predict: a list of frames must hold 2-D uint8 frames")
        if len({tuple(np.shape(f)) for f in images}) != 1:
            raise ValueError("predict: the frames of one call share one size")
        return "u8", images
    if isinstance(images, np.ndarray):
        images = torch.from_numpy(np.ascontiguousarray(images))
    if not isinstance(images, torch.Tensor):
        raise ValueError(f"predict: images must be a tensor, an array or a list of frames, got {type(images).__name__}")
    if images.dtype == torch.uint8:
        if images.dim() not in (2, 3):
            raise ValueError(f"predict: uint8 frames must be [N, H, W] or [H, W], got {tuple(images.shape)}")
        if images.numel() == 0:
            raise ValueError("predict: empty frames")
        return "u8", images
    if not images.dtype.is_floating_point:
        raise ValueError(f"predict: images must be float (normalised) or uint8 frames, got {images.dtype}")
    if images.dim() == 4 and images.shape[1] == 1:
        images = images[:, 0]
    elif images.dim() != 3:
        raise ValueError(f"predict: float images must be [N, 1, H, W] or [N, H, W], got {tuple(images.shape)}")
    if images.numel() == 0:
        raise ValueError("predict: empty images")
    return "f", images


def predict(model, images, tile=512, overlap=64, batch_size=16, tta=False, output="logits", normalize=True,
            max_tile_bytes=1 << 30):
    """Segment whole frames of any size with a tile-sized model.

    ``images``: float ``[N, 1, H, W]`` / ``[N, H, W]`` (already normalised), or
    uint8 frames (tensor, array or list), which first go through
    ``preprocess(frames, img_size=(W, H), normalize=normalize)`` at native size.
    ``tta``: see ``tta_mask``.  ``output``: ``"logits"`` (fp32 ``[N, K, H, W]``),
    ``"mask"`` (uint8 ``[N, K, H, W]``, the package's sigmoid > 0.5 rule),
    ``"labels"`` (uint8 ``[N, H, W]`` argmax, ``n_classes >= 2``), or a tuple of
    these (a tuple is returned).

    Runs under ``torch.no_grad()`` with the model in ``eval()`` (its previous
    mode is restored, also on an exception); eager, no host synchronisation.
    Tiles go through the model in flat tile order in batches of exactly
    ``batch_size`` tiles, the tail slots of the last batch zero-filled, so one
    native plan ``(batch_size, tile, tile)`` serves the call.  When the
    tile-logit buffer (the tile count rounded up to whole batches, times
    ``n_classes * tile^2 * 4`` bytes) of all frames would exceed
    ``max_tile_bytes``, frames are processed in groups of the largest number of
    consecutive frames that fits (at least 1); flat order and the zero tail then
    hold per group.
    """
    tile, overlap, batch_size = int(tile), int(overlap), int(batch_size)
    if tile <= 0 or tile % 32 != 0 or tile > _lib.TILE_MAX:
        raise ValueError(f"tile={tile}: a positive multiple of 32 up to {_lib.TILE_MAX}")
    if overlap < 0 or 2 * overlap > tile:
        raise ValueError(f"overlap={overlap} is outside [0, tile/2] (tile={tile})")
    if batch_size < 1:
        raise ValueError(f"batch_size={batch_size} must be >= 1")
    mask_bits = tta_mask(tta)
    single = isinstance(output, str)
    names = (output,) if single else tuple(output)
    if not names or any(o not in OUTPUTS for o in names):
        raise ValueError(f"output={output!r}: choose from {OUTPUTS} (or a tuple of them)")
    K = int(model.n_classes)
    if "labels" in names and K == 1:
        raise ValueError("output 'labels' (argmax over classes) needs n_classes >= 2; use 'mask'")
    kind, images = _as_input(images)

    device = next(model.parameters()).device
    _lib.require_gpu(next(model.parameters()))
    lib = _lib.load()
    if kind == "u8":
        from .dataset import preprocess
        h, w = (images.shape[-2:] if isinstance(images, torch.Tensor) else np.shape(images[0]))
        images = preprocess(images, img_size=(int(w), int(h)), normalize=normalize, device=device)[:, 0]
    x = images.to(device=device, dtype=torch.float32).contiguous()
    N, H, W = x.shape
    st = _lib.stream_handle(device)
    M = bin(mask_bits).count("1")
    per_frame = M * len(tile_origins(H, tile, overlap)) * len(tile_origins(W, tile, overlap))
    tile_bytes = K * tile * tile * 4
    cap_tiles = (int(max_tile_bytes) // tile_bytes) // batch_size * batch_size
    group = max(1, min(N, cap_tiles // per_frame))

    def padded(frames):
        return -(-frames * per_frame // batch_size) * batch_size

    outs = {}
    if "logits" in names:
        outs["logits"] = torch.empty((N, K, H, W), dtype=torch.float32, device=device)
    if "mask" in names:
        outs["mask"] = torch.empty((N, K, H, W), dtype=torch.uint8, device=device)
    if "labels" in names:
        outs["labels"] = torch.empty((N, H, W), dtype=torch.uint8, device=device)
    modes = [(m, m.training) for m in model.modules()]
    model.eval()
    try:
        with torch.no_grad():
            tiles = torch.empty((batch_size, 1, tile, tile), dtype=torch.float32, device=device)
            tl = torch.empty((padded(group), K, tile, tile), dtype=torch.float32, device=device)
            plan = model._plan_for(tiles)
            for f0 in range(0, N, group):
                g = min(group, N - f0)
                xg = x[f0:f0 + g]
                for first in range(0, padded(g), batch_size):
                    _lib.check(lib.unet_tile_gather(xg.data_ptr(), g, H, W, tile, overlap, mask_bits, first,
                                                    batch_size, tiles.data_ptr(), st), "unet_tile_gather")
                    model._run_forward(plan, tiles, training=False, out=tl[first:first + batch_size])
                ptrs = [_lib.ptr(outs[o][f0:f0 + g]) if o in outs else 0 for o in OUTPUTS]
                _lib.check(lib.unet_tile_blend(tl.data_ptr(), g, K, H, W, tile, overlap, mask_bits, *ptrs, st),
                           "unet_tile_blend")
    finally:
        for m, was in modes:
            m.training = was
    return outs[names[0]] if single else tuple(outs[o] for o in names)
