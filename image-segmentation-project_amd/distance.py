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

import numpy as np
import torch

from . import _lib

_MASK_DTYPES = (torch.uint8, torch.bool, torch.int32)


def _as_frames(x, what, dtypes):
    """Validate an array or tensor of frames; raises ValueError, touches no GPU."""
    names = " / ".join(str(d).replace("torch.", "") for d in dtypes)
    if isinstance(x, np.ndarray):
        if x.dtype not in (np.uint8, np.bool_, np.int32):
            raise ValueError(f"{what} must be {names}, got {x.dtype}")
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{what} must be a tensor or an array, got {type(x).__name__}")
    if x.dtype not in dtypes:
        raise ValueError(f"{what} must be {names}, got {x.dtype}")
    if x.dim() not in (2, 3, 4):
        raise ValueError(f"{what} must be [H, W], [N, H, W] or [N, K, H, W], got {tuple(x.shape)}")
    if x.numel() == 0:
        raise ValueError(f"{what} is empty")
    H, W = x.shape[-2:]
    if H > _lib.DISTANCE_MAX_DIM or W > _lib.DISTANCE_MAX_DIM or H * W >= 1 << 31:
        raise ValueError(f"{what}: H = {H}, W = {W} must be <= {_lib.DISTANCE_MAX_DIM} with H * W below 2^31")
    return x


def _frames_on_gpu(x):
    """[M, H, W] contiguous uint8 / int32 device view or copy of a validated tensor"""
    if not x.is_cuda:
        _lib.require_gpu()
        x = x.cuda()
    _lib.require_gpu(x)
    if x.dtype == torch.bool:
        x = x.view(torch.uint8)
    return x.reshape(-1, x.shape[-2], x.shape[-1]).contiguous()


def _workspace(lib, N, H, W, dev):
    nbytes = int(lib.unet_distance_workspace_bytes(N, H, W))
    if nbytes <= 0:
        _lib.check(1, "unet_distance_workspace_bytes")
    return torch.empty((nbytes,), dtype=torch.uint8, device=dev), nbytes


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
    mask = _as_frames(mask, "distance_transform: mask", _MASK_DTYPES)
    top = 255 if mask.dtype != torch.int32 else (1 << 31) - 1
    if foreground is not None and not 0 <= int(foreground) <= top:
        raise ValueError(f"foreground={foreground} is outside 0..{top}")
    fgv = -1 if foreground is None else int(foreground)
    shape = tuple(mask.shape)
    m = _frames_on_gpu(mask)
    lib = _lib.load()
    N, H, W = m.shape
    dev = m.device
    with torch.cuda.device(dev):
        dist2 = torch.empty((N, H, W), dtype=torch.int32, device=dev)
        nearest = torch.empty((N, H, W), dtype=torch.int32, device=dev) if return_nearest else None
        ws, nbytes = _workspace(lib, N, H, W, dev)
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
    whole frame, not along allowed pixels.

    Returns int32 labels of the same shape; the set of ids is unchanged (as
    ``skimage.segmentation.expand_labels``).  The input is not modified.
    """
    labels = _as_frames(labels, "grow_instances: labels", (torch.int32,))
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
        within = _as_frames(within, "grow_instances: within", (torch.uint8, torch.bool))
        if tuple(within.shape) != tuple(labels.shape):
            raise ValueError(f"grow_instances: within {tuple(within.shape)} and labels {tuple(labels.shape)} differ")
    shape = tuple(labels.shape)
    lab = _frames_on_gpu(labels)
    dev = lab.device
    w = None
    if within is not None:
        w = _frames_on_gpu(within.to(dev) if within.device != dev else within)
    lib = _lib.load()
    N, H, W = lab.shape
    with torch.cuda.device(dev):
        out = torch.empty((N, H, W), dtype=torch.int32, device=dev)
        ws, nbytes = _workspace(lib, N, H, W, dev)
        _lib.check(lib.unet_grow_instances(lab.data_ptr(), N, H, W, max_d2, _lib.ptr(w),
                                           -1 if within_value is None else int(within_value), out.data_ptr(),
                                           ws.data_ptr(), nbytes, _lib.stream_handle(dev)), "unet_grow_instances")
    return out.reshape(shape)
