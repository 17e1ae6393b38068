"""Distances and growth on the GPU: ``distance_transform`` is an exact Euclidean
distance transform of a mask with the nearest-site (feature) transform, and
``grow_instances`` grows the instances of a label map into their neighbourhood by
nearest label (``csrc/distance.hip``: ``unet_distance_transform``,
``unet_grow_instances``).  No reference counterpart; squared distances equal
``rint(scipy.ndimage.distance_transform_edt(...) ** 2)``.

Among equidistant sites the one with the smallest flat index ``y * W + x`` is the
nearest (scipy leaves that choice unspecified).  Everything up to the optional
square root is integer arithmetic; the outputs are bit-reproducible.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from ._frames import as_frames, frames_on_gpu, workspace

_MASK_DTYPES = (torch.uint8, torch.bool, torch.int32)


def distance_transform(mask, foreground=None, invert=False, squared=False, return_nearest=False):
    """Exact Euclidean distance transform of a mask, on the GPU.

    ``mask``: uint8, bool or int32, tensor or array, ``[H, W]``, ``[N, H, W]`` or
    ``[N, K, H, W]``; leading dimensions are independent frames.  A pixel is
    foreground when it is nonzero, or, with ``foreground=c``, when it equals
    ``c``.  By default every pixel gets its distance to the nearest pixel that
    is not foreground (``scipy.ndimage.distance_transform_edt(fg)``: zero
    outside the foreground); with ``invert=True`` its distance to the nearest
    foreground pixel.

    Returns float32 distances of the mask's shape, ``inf`` in a frame without a
    pixel to measure to; with ``squared=True`` the exact int32 squared distances
    instead (2147483647 in such a frame).  With ``return_nearest=True`` also
    the int32 per-frame flat index ``y * W + x`` of the nearest such pixel (the
    smallest index among equidistant ones, -1 where there is none).  The input
    is not modified and nothing synchronises with the host.
    """
    mask = as_frames(mask, "distance_transform: mask", _MASK_DTYPES, _lib.DISTANCE_MAX_DIM)
    top = 255 if mask.dtype != torch.int32 else (1 << 31) - 1
    if foreground is not None and not 0 <= int(foreground) <= top:
        raise ValueError(f"foreground={foreground} is outside 0..{top}")
    fgv = -1 if foreground is None else int(foreground)
    shape = tuple(mask.shape)
    m = frames_on_gpu(mask)
    lib = _lib.load()
    N, H, W = m.shape
    dev = m.device
    with torch.cuda.device(dev):
        dist2 = torch.empty((N, H, W), dtype=torch.int32, device=dev)
        nearest = torch.empty((N, H, W), dtype=torch.int32, device=dev) if return_nearest else None
        ws, nbytes = workspace(lib, "unet_distance_workspace_bytes", dev, N, H, W)
        _lib.check(lib.unet_distance_transform(m.data_ptr(), int(m.dtype == torch.int32), N, H, W, fgv,
                                               int(bool(invert)), dist2.data_ptr(), _lib.ptr(nearest), ws.data_ptr(),
                                               nbytes, _lib.stream_handle(dev)), "unet_distance_transform")
        if squared:
            out = dist2
        else:  # the one torch op: sqrt in float64 so that the float32 result is correctly rounded
            out = dist2.double().sqrt_().float()
            out.masked_fill_(dist2 == _lib.DISTANCE_NONE, math.inf)
    out = out.reshape(shape)
    return (out, nearest.reshape(shape)) if return_nearest else out


def grow_instances(labels, max_distance=None, within=None, within_value=None):
    """Grow the instances of a label map into the unlabelled pixels, on the GPU.

    ``labels``: int32 (as ``label_instances`` returns them), ``[H, W]``,
    ``[N, H, W]`` or ``[N, K, H, W]``; 0 is unlabelled.  Every unlabelled pixel
    takes the label of the nearest labelled pixel of its frame (Euclidean; the
    smallest flat index among equidistant ones) when that is at most
    ``max_distance`` away (``None``: any distance) and, if ``within`` is given,
    the pixel is allowed there.  ``within``: uint8 / bool of the same shape, a
    pixel is allowed where it is nonzero, or, with ``within_value=c``, where it
    equals ``c`` (``within=predict(..., output="labels"), within_value=2`` for a
    boundary class).  Labelled pixels are copied.  "Nearest" is measured over the
    whole frame, not along allowed pixels (``geodesic_grow`` measures along them).

    Returns int32 labels of the same shape; the set of ids is unchanged (as
    ``skimage.segmentation.expand_labels``).  The input is not modified.
    """
    labels = as_frames(labels, "grow_instances: labels", (torch.int32,), _lib.DISTANCE_MAX_DIM)
    if max_distance is None:
        max_d2 = -1
    else:
        md = float(max_distance)
        if not md >= 0:
            raise ValueError(f"max_distance={max_distance!r} must be >= 0 or None")
        max_d2 = -1 if math.isinf(md) else min(int(math.floor(md * md)), _lib.DISTANCE_NONE)
    if within_value is not None and (within is None or not 0 <= int(within_value) <= 255):
        raise ValueError(f"within_value={within_value} needs within and must be in 0..255")
    if within is not None:
        within = as_frames(within, "grow_instances: within", (torch.uint8, torch.bool), _lib.DISTANCE_MAX_DIM)
        if tuple(within.shape) != tuple(labels.shape):
            raise ValueError(f"grow_instances: within {tuple(within.shape)} and labels {tuple(labels.shape)} differ")
    shape = tuple(labels.shape)
    lab = frames_on_gpu(labels)
    dev = lab.device
    w = None
    if within is not None:
        w = frames_on_gpu(within.to(dev) if within.device != dev else within)
    lib = _lib.load()
    N, H, W = lab.shape
    with torch.cuda.device(dev):
        out = torch.empty((N, H, W), dtype=torch.int32, device=dev)
        ws, nbytes = workspace(lib, "unet_distance_workspace_bytes", dev, N, H, W)
        _lib.check(lib.unet_grow_instances(lab.data_ptr(), N, H, W, max_d2, _lib.ptr(w),
                                           -1 if within_value is None else int(within_value), out.data_ptr(),
                                           ws.data_ptr(), nbytes, _lib.stream_handle(dev)), "unet_grow_instances")
    return out.reshape(shape)
