"""Growth along allowed pixels, watershed and splitting of touching cells on the GPU:
``geodesic_grow`` grows the instances of a label map by shortest paths that stay
inside an allowed set, ``watershed`` floods a relief from markers level by level,
and ``split_instances`` splits the merged blobs of a mask with seeds from the
distance map (``csrc/geodesic.hip``: ``unet_geodesic_grow``, ``unet_watershed``).
No reference counterpart; the definitions are those of ``tests/geodesic_ref.py``.

Metrics: ``"cityblock"`` (4 neighbours, a step costs 1) and ``"chamfer"`` (8
neighbours, an axial step costs 3, a diagonal step 4; a diagonal step is allowed
whatever the two axial neighbours are).  Among the ids that reach a pixel at the
least cost the smallest id takes it.  Everything is integer arithmetic; the outputs
are bit-reproducible.

Unlike ``grow_instances`` these calls **synchronise with the host**: relaxation
passes run until one changes nothing, which the host reads back from the current
stream.  They cannot be captured into a graph (inside a capture they raise and
enqueue nothing).  Limits: ``H, W <= 32768`` and ``H * W <= 2^28``.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from ._frames import as_frames, frames_on_gpu, workspace
from .distance import distance_transform
from .instances import label_instances

METRICS = {"cityblock": 0, "chamfer": 1}
_AXIAL = (1, 3)  # cost of an axial step per metric


def _metric(metric):
    if not isinstance(metric, str) or metric not in METRICS:
        raise ValueError(f"metric={metric!r}: 'cityblock' or 'chamfer'")
    return METRICS[metric]


def _frames(x, what, dtypes):
    x = as_frames(x, what, dtypes, _lib.DISTANCE_MAX_DIM)
    H, W = x.shape[-2:]
    if H * W > _lib.GEODESIC_MAX_HW:
        raise ValueError(f"{what}: H * W = {H * W} must be at most 2^28")
    return x


def _allowed(within, within_value, shape, what, name):
    """validated (within tensor or None, value for the C ABI)"""
    if within_value is not None and (within is None or not 0 <= int(within_value) <= 255):
        raise ValueError(f"{name}_value={within_value} needs {name} and must be in 0..255")
    if within is not None:
        within = _frames(within, f"{what}: {name}", (torch.uint8, torch.bool))
        if tuple(within.shape) != tuple(shape):
            raise ValueError(f"{what}: {name} {tuple(within.shape)} and {tuple(shape)} differ")
    return within, (-1 if within_value is None else int(within_value))


def _to(x, dev):
    return None if x is None else frames_on_gpu(x.to(dev) if x.device != dev else x)


def geodesic_grow(labels, within=None, within_value=None, metric="cityblock", max_distance=None,
                  return_distance=False):
    """Grow the instances of a label map along allowed pixels, on the GPU.

    ``labels``: int32, ``[H, W]``, ``[N, H, W]`` or ``[N, K, H, W]``; 0 is
    unlabelled, positive values are ids.  A pixel is free when it is unlabelled
    and allowed: everywhere with ``within=None``, else where ``within`` (uint8 /
    bool of the same shape) is nonzero, or equals ``within_value``.  A free pixel
    takes the id of the labelled pixel that a path of steps of the ``metric``
    through free pixels reaches at the least cost, the smallest id among equal
    costs, when that cost is within ``max_distance`` pixels (cityblock: cost <=
    ``floor(max_distance)``; chamfer: cost <= ``floor(3 * max_distance)``;
    ``None`` or ``inf``: unlimited).  Labelled pixels are copied; pixels without
    such a path stay 0.  Unlike ``grow_instances`` a label never crosses pixels
    that are not allowed.

    Returns int32 labels of the same shape; with ``return_distance=True`` also
    the int32 costs (0 at labelled pixels, -1 where nothing arrived).  The input
    is not modified.  The call synchronises with the host and cannot be captured
    into a graph.
    """
    labels = _frames(labels, "geodesic_grow: labels", (torch.int32,))
    m = _metric(metric)
    if max_distance is None:
        max_cost = -1
    else:
        md = float(max_distance)
        if not md >= 0:
            raise ValueError(f"max_distance={max_distance!r} must be >= 0 or None")
        max_cost = -1 if math.isinf(md) else min(int(math.floor(_AXIAL[m] * md)), (1 << 31) - 1)
    within, wv = _allowed(within, within_value, labels.shape, "geodesic_grow", "within")
    shape = tuple(labels.shape)
    lab = frames_on_gpu(labels)
    dev = lab.device
    w = _to(within, dev)
    lib = _lib.load()
    N, H, W = lab.shape
    with torch.cuda.device(dev):
        out = torch.empty((N, H, W), dtype=torch.int32, device=dev)
        cost = torch.empty((N, H, W), dtype=torch.int32, device=dev) if return_distance else None
        ws, nbytes = workspace(lib, "unet_geodesic_workspace_bytes", dev, N, H, W)
        _lib.check(lib.unet_geodesic_grow(lab.data_ptr(), N, H, W, m, max_cost, _lib.ptr(w), wv, out.data_ptr(),
                                          _lib.ptr(cost), ws.data_ptr(), nbytes, _lib.stream_handle(dev)),
                   "unet_geodesic_grow")
    return (out.reshape(shape), cost.reshape(shape)) if return_distance else out.reshape(shape)


def watershed(relief, markers, mask=None, mask_value=None, metric="cityblock"):
    """Marker watershed of a relief by flooding level by level, on the GPU.

    ``relief``: uint8; ``markers``: int32 of the same shape (0: no marker);
    ``mask``: uint8 / bool of the same shape with the meaning of ``within`` above
    (``None``: everywhere).  For every value ``h`` of the relief under the mask, in
    ascending order, the markers grow as ``geodesic_grow(markers, within=mask &
    (relief <= h), metric=metric)`` does.  Marker pixels keep their id whatever
    relief and mask say; pixels that no marker reaches stay 0.

    Returns int32 labels of the same shape.  The inputs are not modified.  The
    call synchronises with the host (once for the levels, then per level) and
    cannot be captured into a graph.
    """
    relief = _frames(relief, "watershed: relief", (torch.uint8,))
    markers = _frames(markers, "watershed: markers", (torch.int32,))
    if tuple(markers.shape) != tuple(relief.shape):
        raise ValueError(f"watershed: markers {tuple(markers.shape)} and relief {tuple(relief.shape)} differ")
    m = _metric(metric)
    mask, mv = _allowed(mask, mask_value, relief.shape, "watershed", "mask")
    shape = tuple(markers.shape)
    mk = frames_on_gpu(markers)
    dev = mk.device
    r, w = _to(relief, dev), _to(mask, dev)
    lib = _lib.load()
    N, H, W = mk.shape
    with torch.cuda.device(dev):
        out = torch.empty((N, H, W), dtype=torch.int32, device=dev)
        ws, nbytes = workspace(lib, "unet_geodesic_workspace_bytes", dev, N, H, W)
        _lib.check(lib.unet_watershed(r.data_ptr(), mk.data_ptr(), N, H, W, m, _lib.ptr(w), mv, out.data_ptr(),
                                      ws.data_ptr(), nbytes, _lib.stream_handle(dev)), "unet_watershed")
    return out.reshape(shape)


def split_instances(mask, seed_distance, metric="cityblock", connectivity=1, foreground=None, max_instances=4096):
    """Instances of a mask with touching cells split by a watershed, on the GPU.

    ``mask``: uint8, bool or int32 as for ``distance_transform`` (``foreground=c``
    selects a class).  With ``R = ceil(seed_distance)`` (1..255): the seeds are the
    components (``connectivity``) of the pixels at least ``R`` from the
    background, the relief is ``clamp(R - isqrt(d2), 0, 255)`` of the exact squared
    distance ``d2``, and the seeds flood the foreground by ``watershed``.  A blob
    too thin to hold a seed is kept as an instance of its own.

    Returns ``(labels, counts)`` like ``label_instances``.  Ids are ``1..counts``
    per frame: first the seeded instances, in raster order of their seeds, then
    the unseeded blobs in raster order; the order is raster only within each of
    the two groups.  ``counts`` is computed on the device; the watershed inside
    synchronises with the host.
    """
    sd = float(seed_distance)
    if not 0 < sd <= 255:
        raise ValueError(f"seed_distance={seed_distance!r} must be in (0, 255]")
    _metric(metric)
    if connectivity not in (1, 2) or isinstance(connectivity, bool):
        raise ValueError(f"connectivity={connectivity!r}: 1 (4-neighbour) or 2 (8-neighbour)")
    if int(max_instances) < 1:
        raise ValueError(f"max_instances={max_instances} must be >= 1")
    mask = _frames(mask, "split_instances: mask", (torch.uint8, torch.bool, torch.int32))
    R = int(math.ceil(sd))
    d2 = distance_transform(mask, foreground=foreground, squared=True)  # checks foreground; moves a host mask
    mask = mask.to(d2.device)
    fg = (mask != 0) if foreground is None else (mask == int(foreground))
    seeds, n = label_instances(d2 >= R * R, connectivity, max_instances=max_instances)
    root = d2.double().sqrt_().floor_()  # exact: a double holds every int32 and its correctly rounded root
    relief = (R - root).clamp_(0, 255).to(torch.uint8)
    ws = watershed(relief, seeds, mask=fg, metric=metric)
    rest, m = label_instances(fg & (ws == 0), connectivity, max_instances=max_instances)
    labels = ws + torch.where(rest > 0, rest + n[..., None, None], torch.zeros_like(rest))
    return labels, n + m
