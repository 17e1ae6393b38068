"""Training targets for touching cells on the GPU (``csrc/weights.hip``):
``nearest_two_instances`` is the exact transform of a label map to the two nearest
distinct instances of every pixel, ``border_weight_map`` the U-Net border weight
map on top of it and ``boundary_targets`` the background / interior / boundary
class map (``unet_two_nearest_instances``, ``unet_border_weights``,
``unet_boundary_targets``).  No reference counterpart; both squared distances are
the two smallest entries of ``rint(scipy.ndimage.distance_transform_edt(labels !=
i) ** 2)`` over the ids ``i``.

Among equidistant pixels of instances the one with the smallest flat index ``y * W
+ x`` is the nearest, as in ``distance_transform``.  Everything up to the weight is
integer arithmetic; the outputs are bit-reproducible.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from ._frames import as_frames, frames_on_gpu, workspace


def _max_d2(max_distance):
    if max_distance is None:
        return -1
    md = float(max_distance)
    if not md >= 0:
        raise ValueError(f"max_distance={max_distance!r} must be >= 0 or None")
    return -1 if math.isinf(md) else min(int(math.floor(md * md)), _lib.DISTANCE_NONE)


def nearest_two_instances(labels, max_distance=None, squared=False, return_ids=False):
    """Distances of every pixel to its two nearest distinct instances, on the GPU.

    ``labels``: int32 (as ``label_instances`` returns them), tensor or array,
    ``[H, W]``, ``[N, H, W]`` or ``[N, K, H, W]`` with ``H, W <= 4096``; leading
    dimensions are independent frames, values ``<= 0`` are unlabelled.  The first
    instance of a pixel is the one of the nearest labelled pixel (Euclidean; the
    smallest flat index among equidistant ones), the second the one of the nearest
    labelled pixel with another id.  With ``max_distance`` an instance further
    away does not count.

    Returns float32 distances with a new axis of length 2 in front of ``H``
    (``[..., 2, H, W]``: nearest, second), ``inf`` where there is no such
    instance; with ``squared=True`` the exact int32 squared distances instead
    (2147483647 for none).  With ``return_ids=True`` also the int32 ids of the two
    instances (0 for none) in the same layout.  A labelled pixel has distance 0
    and its own id first.  The input is not modified and nothing synchronises
    with the host.
    """
    labels = as_frames(labels, "nearest_two_instances: labels", (torch.int32,), _lib.TWO_NEAREST_MAX_DIM)
    max_d2 = _max_d2(max_distance)
    shape = tuple(labels.shape[:-2]) + (2,) + tuple(labels.shape[-2:])
    lab = frames_on_gpu(labels)
    lib = _lib.load()
    N, H, W = lab.shape
    dev = lab.device
    with torch.cuda.device(dev):
        dist2 = torch.empty((N, 2, H, W), dtype=torch.int32, device=dev)
        ids = torch.empty((N, 2, H, W), dtype=torch.int32, device=dev) if return_ids else None
        ws, nbytes = workspace(lib, "unet_two_nearest_workspace_bytes", dev, N, H, W)
        _lib.check(lib.unet_two_nearest_instances(lab.data_ptr(), N, H, W, max_d2, dist2.data_ptr(), _lib.ptr(ids),
                                                  ws.data_ptr(), nbytes, _lib.stream_handle(dev)),
                   "unet_two_nearest_instances")
        if squared:
            out = dist2
        else:  # sqrt in float64 so that the float32 result is correctly rounded
            out = dist2.double().sqrt_().float()
            out.masked_fill_(dist2 == _lib.DISTANCE_NONE, math.inf)
    out = out.reshape(shape)
    return (out, ids.reshape(shape)) if return_ids else out


def border_weight_map(labels, w0=10.0, sigma=5.0, max_distance=None, classes=None, class_weights=None):
    """The U-Net border weight map of a ground-truth instance map, on the GPU.

    ``labels`` as for ``nearest_two_instances``.  Every pixel gets ``base +
    border``: ``border = w0 * exp(-(d1 + d2)^2 / (2 sigma^2))`` on unlabelled
    pixels, with ``d1`` and ``d2`` the distances to the nearest and the second
    nearest instance (0 where there is no second instance, or it is further than
    ``max_distance``), and ``base = class_weights[classes]`` when ``classes``
    (uint8 of the labels' shape, e.g. ``boundary_targets(labels)``) and
    ``class_weights`` (one float per class; a class beyond them weighs 0) are
    given, else 1.  The distances never go to memory; the square roots and the
    exponential are taken in double.

    Returns float32 of the labels' shape, ready as ``pixel_weights`` of
    ``CrossEntropyLoss`` / ``SoftmaxComboLoss``.  With every input on the device
    nothing synchronises with the host.  ``labels``, ``classes`` or
    ``class_weights`` given as a list, an array or a host tensor are copied to
    the GPU first, which blocks the host briefly and cannot be captured into a
    graph: pass device tensors (``class_weights`` as a float32 device tensor) to
    capture the call.
    """
    labels = as_frames(labels, "border_weight_map: labels", (torch.int32,), _lib.TWO_NEAREST_MAX_DIM)
    w0, sigma = float(w0), float(sigma)
    if not (w0 >= 0 and math.isfinite(w0)) or not (sigma > 0 and math.isfinite(sigma)):
        raise ValueError(f"border_weight_map: w0={w0!r} must be finite and >= 0, sigma={sigma!r} finite and > 0")
    max_d2 = _max_d2(max_distance)
    if (classes is None) != (class_weights is None):
        raise ValueError("border_weight_map: classes and class_weights go together")
    cw = None
    if classes is not None:
        classes = as_frames(classes, "border_weight_map: classes", (torch.uint8,))
        if tuple(classes.shape) != tuple(labels.shape):
            raise ValueError(f"border_weight_map: classes {tuple(classes.shape)} and labels {tuple(labels.shape)} "
                             "differ")
        cw = torch.as_tensor(class_weights, dtype=torch.float32).reshape(-1)
        if cw.numel() == 0:
            raise ValueError("border_weight_map: class_weights is empty")
    shape = tuple(labels.shape)
    lab = frames_on_gpu(labels)
    dev = lab.device
    cls = None
    if classes is not None:
        cls = frames_on_gpu(classes.to(dev) if classes.device != dev else classes)
        cw = cw.to(dev).contiguous()
    lib = _lib.load()
    N, H, W = lab.shape
    with torch.cuda.device(dev):
        out = torch.empty((N, H, W), dtype=torch.float32, device=dev)
        ws, nbytes = workspace(lib, "unet_two_nearest_workspace_bytes", dev, N, H, W)
        _lib.check(lib.unet_border_weights(lab.data_ptr(), N, H, W, w0, sigma, max_d2, _lib.ptr(cls), _lib.ptr(cw),
                                           0 if cw is None else cw.numel(), out.data_ptr(), ws.data_ptr(), nbytes,
                                           _lib.stream_handle(dev)), "unet_border_weights")
    return out.reshape(shape)


def boundary_targets(labels, connectivity=2):
    """Background / interior / boundary targets of a ground-truth instance map, on the GPU.

    ``labels``: int32, ``[H, W]``, ``[N, H, W]`` or ``[N, K, H, W]``; values ``<= 0``
    are background.  Returns uint8 of the same shape: 0 background, 2 boundary (a
    labelled pixel with a neighbour inside the frame of another value, background
    or another id; ``connectivity`` 1: 4 neighbours, 2: 8), 1 interior (every
    other labelled pixel).  The class numbers are those ``grow_instances(...,
    within_value=2)`` expects of a boundary class.  Nothing synchronises with the host.
    """
    labels = as_frames(labels, "boundary_targets: labels", (torch.int32,), _lib.DISTANCE_MAX_DIM)
    if connectivity not in (1, 2):
        raise ValueError(f"boundary_targets: connectivity={connectivity!r} must be 1 (4 neighbours) or 2 (8)")
    shape = tuple(labels.shape)
    lab = frames_on_gpu(labels)
    dev = lab.device
    lib = _lib.load()
    N, H, W = lab.shape
    with torch.cuda.device(dev):
        out = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
        _lib.check(lib.unet_boundary_targets(lab.data_ptr(), N, H, W, int(connectivity), out.data_ptr(),
                                             _lib.stream_handle(dev)), "unet_boundary_targets")
    return out.reshape(shape)
