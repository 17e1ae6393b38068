"""Instances from masks on the GPU: ``label_instances`` turns a predicted mask into
numbered objects (``csrc/instances.hip``: ``unet_label_instances``), with optional
hole filling, a minimum area and per-instance statistics.  No reference counterpart;
the definitions are scipy.ndimage's (``label``, ``binary_fill_holes``, ``find_objects``).

Instances of each frame are numbered ``1..count`` in raster order of their first
pixel (ascending minimum flat index), as ``scipy.ndimage.label`` numbers them.  The
order of operations is: fill holes, then label, then ``min_area``.  Everything is
integer arithmetic; the outputs are bit-reproducible.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._frames import as_frames, frames_on_gpu, workspace

STATS_COLUMNS = ("area", "sum_y", "sum_x", "y0", "x0", "y1", "x1")  # the last axis of the stats table
assert len(STATS_COLUMNS) == _lib.INSTANCE_STATS


def _check_args(mask, connectivity, min_area, foreground, max_instances):
    """Validate and return (mask tensor, fg_value); raises ValueError, touches no GPU."""
    if connectivity not in (1, 2) or isinstance(connectivity, bool):
        raise ValueError(f"connectivity={connectivity!r}: 1 (4-neighbour) or 2 (8-neighbour)")
    if int(min_area) < 0:
        raise ValueError(f"min_area={min_area} must be >= 0")
    if int(max_instances) < 1:
        raise ValueError(f"max_instances={max_instances} must be >= 1")
    if foreground is not None and not 0 <= int(foreground) <= 255:
        raise ValueError(f"foreground={foreground} is outside 0..255")
    mask = as_frames(mask, "label_instances: mask", (torch.uint8, torch.bool))
    return mask, (-1 if foreground is None else int(foreground))


def label_instances(mask, connectivity=1, min_area=0, fill_holes=False, foreground=None, max_instances=4096,
                    return_stats=False, return_filled=False):
    """Connected-component instances of a mask, on the GPU.

    ``mask``: uint8 or bool, tensor or array, ``[H, W]``, ``[N, H, W]`` or
    ``[N, K, H, W]``; leading dimensions are independent frames.  A pixel is
    foreground when it is nonzero, or, with ``foreground=c``, when it equals
    ``c`` (``predict(..., output="labels")`` class maps).  ``connectivity``: 1
    (4-neighbour) or 2 (8-neighbour).  ``fill_holes``: first fill the holes
    (4-connected background components that touch no frame edge, as
    ``scipy.ndimage.binary_fill_holes``).  ``min_area``: drop smaller components
    before numbering.

    Returns ``(labels, counts)``: int32 labels of the mask's shape (0 =
    background, ids ``1..count`` per frame in raster order of first pixel) and
    int32 counts of the leading shape; with ``return_stats=True`` also an int64
    table ``[..., max_instances, 7]`` of ``area, sum_y, sum_x, y0, x0, y1, x1``
    (half-open bounding box) for ids up to ``max_instances`` (rows at and beyond
    the count are zero; ``counts`` and the label map are never truncated); with
    ``return_filled=True`` (needs ``fill_holes``) also the uint8 filled mask
    (0 / 1).  The input is not modified and nothing synchronises with the host;
    ``instance_properties`` does.
    """
    mask, fgv = _check_args(mask, connectivity, min_area, foreground, max_instances)
    if return_filled and not fill_holes:
        raise ValueError("return_filled=True needs fill_holes=True")
    min_area, max_instances = int(min_area), int(max_instances)
    shape = tuple(mask.shape)
    lead = shape[:-2]
    m = frames_on_gpu(mask)
    lib = _lib.load()
    N, H, W = m.shape
    dev = m.device
    with torch.cuda.device(dev):
        labels = torch.empty((N, H, W), dtype=torch.int32, device=dev)
        counts = torch.empty((N,), dtype=torch.int32, device=dev)
        stats = torch.empty((N, max_instances, _lib.INSTANCE_STATS), dtype=torch.int64, device=dev) if return_stats else None
        filled = torch.empty((N, H, W), dtype=torch.uint8, device=dev) if return_filled else None
        ws, nbytes = workspace(lib, "unet_instances_workspace_bytes", dev, N, H, W)
        _lib.check(lib.unet_label_instances(m.data_ptr(), N, H, W, fgv, int(connectivity), int(bool(fill_holes)),
                                            min_area, max_instances, labels.data_ptr(), counts.data_ptr(),
                                            _lib.ptr(stats), _lib.ptr(filled), ws.data_ptr(), nbytes,
                                            _lib.stream_handle(dev)), "unet_label_instances")
    out = [labels.reshape(shape), counts.reshape(lead)]
    if return_stats:
        out.append(stats.reshape(lead + (max_instances, _lib.INSTANCE_STATS)))
    if return_filled:
        out.append(filled.reshape(shape))
    return tuple(out)


def instance_properties(stats, counts):
    """Host-side view of a ``label_instances`` stats table (this synchronises).

    Per frame a dict of numpy arrays over its ``min(count, max_instances)``
    instances: ``area`` int64 ``[k]``, ``centroid`` float64 ``[k, 2]`` (y, x =
    sums / area) and ``bbox`` int64 ``[k, 4]`` (y0, x0, y1, x1, half-open).  A
    single frame (``stats`` ``[max_instances, 7]``) gives one dict; leading
    dimensions give nested lists of that shape.
    """
    s = stats.detach().cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats)
    c = counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
    if s.ndim < 2 or s.shape[-1] != _lib.INSTANCE_STATS or s.shape[:-2] != c.shape:
        raise ValueError(f"instance_properties: stats {s.shape} / counts {c.shape} are not a label_instances pair")

    def one(tab, count):
        k = min(int(count), tab.shape[0])
        tab = tab[:k].astype(np.int64)
        area = tab[:, 0]
        centroid = tab[:, 1:3].astype(np.float64) / area[:, None].astype(np.float64)
        return {"area": area.copy(), "centroid": centroid, "bbox": tab[:, 3:7].copy()}

    def walk(tab, cnt):
        if cnt.ndim == 0:
            return one(tab, cnt)
        return [walk(t, k) for t, k in zip(tab, cnt)]

    return walk(s, c)
