"""Measuring instances on the GPU: ``measure_instances`` turns any int32 label map
(and optionally the image it came from) into per-instance tables of area,
coordinate sums up to second order, bounding box, crack-length perimeter, frame
and contact edges and intensities (``csrc/measure.hip``:
``unet_measure_instances``); ``select_instances`` drops instances by a device
mask and renumbers the rest ``1..count`` (``unet_select_instances``);
``region_properties`` is the host view of the tables (the one place that
synchronises).  No reference counterpart; tests/measure_ref.py holds the
definitions as numpy.

Every integer table is a sum, minimum or maximum of integers through integer
atomics and so bit-reproducible.  The one exception are ``sum`` and ``sum_sq`` of
a float32 image: fp64 atomic sums, whose last bits depend on the order of arrival.
"""
from __future__ import annotations

import collections

import numpy as np
import torch

from . import _lib
from ._frames import as_frames, frames_on_gpu, workspace

# the last axis of table, status and intensity
MEASURE_COLUMNS = ("area", "sum_y", "sum_x", "y0", "x0", "y1", "x1", "sum_yy", "sum_xx", "sum_xy", "edges",
                   "frame_edges", "contact_edges")
STATUS_COLUMNS = ("n_present", "max_id", "out_of_range")
INTENSITY_COLUMNS = ("sum", "sum_sq", "min", "max")
assert (len(MEASURE_COLUMNS) == _lib.MEASURE_COLS and len(STATUS_COLUMNS) == _lib.MEASURE_STATUS
        and len(INTENSITY_COLUMNS) == _lib.MEASURE_ICOLS)
MAX_ID = 65535
MAX_DIM = _lib.DISTANCE_MAX_DIM
MAX_HW = _lib.GEODESIC_MAX_HW
MAX_CHANNELS = 4
IMAGE_DTYPES = {torch.uint8: 0, torch.uint16: 1, torch.float32: 2}  # image_dtype of the C ABI
_IMAGE_NUMPY = (np.uint8, np.uint16, np.float32)

InstanceMeasure = collections.namedtuple("InstanceMeasure", ("table", "status", "intensity"))


def _labels(labels, what):
    labels = as_frames(labels, what, (torch.int32,))
    H, W = labels.shape[-2:]
    if H > MAX_DIM or W > MAX_DIM or H * W > MAX_HW:
        raise ValueError(f"{what}: H = {H}, W = {W} must be <= {MAX_DIM} with H * W <= 2^28")
    return labels


def _cap(value, name):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 1 <= int(value) <= MAX_ID:
        raise ValueError(f"{name}={value!r} must be an integer in 1..{MAX_ID}")
    return int(value)


def _image(image, labels):
    """the image as a tensor and its channel count, validated against the labels; touches no GPU"""
    what = "measure_instances: image"
    if isinstance(image, np.ndarray):
        if image.dtype not in _IMAGE_NUMPY:
            raise ValueError(f"{what} must be uint8 / uint16 / float32, got {image.dtype}")
        image = torch.from_numpy(np.ascontiguousarray(image))
    if not isinstance(image, torch.Tensor):
        raise ValueError(f"{what} must be a tensor or an array, got {type(image).__name__}")
    if image.dtype not in IMAGE_DTYPES:
        raise ValueError(f"{what} must be uint8 / uint16 / float32, got {image.dtype}")
    ls, shape = tuple(labels.shape), tuple(image.shape)
    if shape == ls:
        return image, 1
    if len(shape) == len(ls) + 1 and shape[:-3] == ls[:-2] and shape[-2:] == ls[-2:]:
        if not 1 <= shape[-3] <= MAX_CHANNELS:
            raise ValueError(f"{what} {shape} has {shape[-3]} channels; 1..{MAX_CHANNELS} are supported")
        return image, shape[-3]
    raise ValueError(f"{what} {shape} must have the shape of labels {ls} or one axis of channels before H, W")


def measure_instances(labels, image=None, max_instances=4096):
    """Per-instance shape, contact and intensity tables of a label map, on the GPU.

    ``labels``: an int32 label map (of ``label_instances``, ``grow_instances``,
    ``geodesic_grow``, ``watershed``, ``split_instances``, ``select_instances`` or
    a ground truth), tensor or array ``[H, W]``, ``[N, H, W]`` or ``[N, K, H,
    W]``; leading dimensions are independent frames.  0 is background, ids run
    up to ``max_instances`` (1..65535) and need not be compact; a pixel with an
    id below 0 or above ``max_instances`` belongs to no instance (it is counted
    in ``status``) and is, as a neighbour, another nonzero value.  ``H, W <=
    32768`` and ``H * W <= 2^28``, so that every int64 sum is exact.

    Returns ``InstanceMeasure(table, status, intensity)`` of device tensors.
    ``table`` int64 ``[..., max_instances, 13]`` (``MEASURE_COLUMNS``), row ``id -
    1`` over the pixels ``(y, x)`` of value ``id``: ``area``; ``sum_y``, ``sum_x``;
    the half-open box ``y0, x0, y1, x1`` (these seven as the stats of
    ``label_instances``); ``sum_yy``, ``sum_xx``, ``sum_xy``; ``edges``, the pixel
    sides whose other side lies outside the frame or holds a different value
    (the crack-length perimeter); ``frame_edges``, those on the frame's border;
    ``contact_edges``, those whose other side is inside the frame and nonzero
    (contact with another instance).  The row of an id that does not occur is
    zero.  ``status`` int64 ``[..., 3]``: ``n_present``, ``max_id`` (0 if none),
    ``out_of_range`` (pixels).

    ``image`` (optional): uint8, uint16 or float32, of the labels' shape or with
    one axis of ``C <= 4`` channels directly before ``H, W`` (labels ``[N, H, W]``
    take ``[N, C, H, W]``); it is moved to the labels' device if needed.  Then
    ``intensity`` is ``[..., max_instances, C, 4]`` = ``sum, sum_sq, min, max``
    per channel (zero rows for absent ids), int64 with exact sums for integer
    images, float64 for a float32 image; otherwise ``None``.  Float images must
    be finite (not checked); their ``min`` and ``max`` are exact, their ``sum``
    and ``sum_sq`` are fp64 atomic sums: the one output that is not
    bit-reproducible (the last bits depend on the order of arrival).

    The inputs are not modified and nothing synchronises with the host;
    ``region_properties`` does.  Without a GPU the call raises ``RuntimeError``.
    """
    labels = _labels(labels, "measure_instances: labels")
    max_instances = _cap(max_instances, "max_instances")
    C = 0
    if image is not None:
        image, C = _image(image, labels)
    if not labels.is_cuda:
        _lib.require_gpu()
        labels = labels.cuda()
    lead = tuple(labels.shape)[:-2]
    lab = frames_on_gpu(labels)
    lib = _lib.load()
    N, H, W = lab.shape
    dev = lab.device
    img = None
    if image is not None:
        img = image.to(dev).reshape(N, C, H, W).contiguous()
    with torch.cuda.device(dev):
        table = torch.empty((N, max_instances, _lib.MEASURE_COLS), dtype=torch.int64, device=dev)
        status = torch.empty((N, _lib.MEASURE_STATUS), dtype=torch.int64, device=dev)
        intensity = None
        if img is not None:
            intensity = torch.empty((N, max_instances, C, _lib.MEASURE_ICOLS), device=dev,
                                    dtype=torch.float64 if img.dtype == torch.float32 else torch.int64)
        ws, nbytes = workspace(lib, "unet_measure_workspace_bytes", dev, N, H, W, max_instances, C)
        _lib.check(lib.unet_measure_instances(lab.data_ptr(), _lib.ptr(img), IMAGE_DTYPES[img.dtype] if C else 0, C,
                                              N, H, W, max_instances, table.data_ptr(), status.data_ptr(),
                                              _lib.ptr(intensity), ws.data_ptr(), nbytes, _lib.stream_handle(dev)),
                   "unet_measure_instances")
    return InstanceMeasure(table.reshape(lead + (max_instances, _lib.MEASURE_COLS)),
                           status.reshape(lead + (_lib.MEASURE_STATUS,)),
                           None if intensity is None else
                           intensity.reshape(lead + (max_instances, C, _lib.MEASURE_ICOLS)))


def select_instances(labels, keep):
    """Drop instances and renumber the rest ``1..count``, on the GPU.

    ``labels``: an int32 label map as for ``measure_instances``.  ``keep``: a bool
    or uint8 tensor or array ``[..., M]`` with the labels' leading dimensions and
    ``M <= 65535``; entry ``id - 1`` says whether ``id`` survives.  It is
    typically computed with torch ops on the device table::

        m = measure_instances(labels)
        keep = (m.table[..., 0] >= 50) & (m.table[..., 11] == 0)   # at least 50 px, not cut by the frame
        labels2, counts2, new_ids = select_instances(labels, keep)

    Returns ``(labels2, counts2, new_ids)``: ``new_ids`` int32 ``[..., M]``, the
    1-based rank of each kept id among the kept ids in ascending order (which
    keeps the raster order of ``label_instances``) and 0 for a dropped id;
    ``labels2`` int32 of the labels' shape, ``new_ids[id - 1]`` for the ids
    ``1..M`` and 0 for background, dropped ids and ids outside ``1..M``;
    ``counts2`` int32 of the leading shape, the number of kept ids.  An id that
    is kept but absent from the map still takes a rank: pass ``keep & (area >
    0)`` for compact numbering of what is there.  Nothing synchronises.
    """
    labels = _labels(labels, "select_instances: labels")
    if isinstance(keep, np.ndarray):
        if keep.dtype not in (np.bool_, np.uint8):
            raise ValueError(f"select_instances: keep must be bool / uint8, got {keep.dtype}")
        keep = torch.from_numpy(np.ascontiguousarray(keep).reshape(keep.shape))  # a 0-d array stays 0-d
    if not isinstance(keep, torch.Tensor):
        raise ValueError(f"select_instances: keep must be a tensor or an array, got {type(keep).__name__}")
    if keep.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"select_instances: keep must be bool / uint8, got {keep.dtype}")
    lead = tuple(labels.shape)[:-2]
    if keep.dim() != len(lead) + 1 or tuple(keep.shape)[:-1] != lead:
        raise ValueError(f"select_instances: keep {tuple(keep.shape)} must be {lead + ('M',)} for labels "
                         f"{tuple(labels.shape)}")
    M = keep.shape[-1]
    if not 1 <= M <= MAX_ID:
        raise ValueError(f"select_instances: keep has M = {M} entries per frame; 1..{MAX_ID} are supported")
    if not labels.is_cuda:
        _lib.require_gpu()
        labels = labels.cuda()
    shape = tuple(labels.shape)
    lab = frames_on_gpu(labels)
    lib = _lib.load()
    N, H, W = lab.shape
    dev = lab.device
    k = keep.to(dev)
    k = (k.view(torch.uint8) if k.dtype == torch.bool else k).reshape(N, M).contiguous()
    with torch.cuda.device(dev):
        out = torch.empty_like(lab)
        counts = torch.empty((N,), dtype=torch.int32, device=dev)
        new_ids = torch.empty((N, M), dtype=torch.int32, device=dev)
        _lib.check(lib.unet_select_instances(lab.data_ptr(), k.data_ptr(), N, H, W, M, out.data_ptr(),
                                             counts.data_ptr(), new_ids.data_ptr(), _lib.stream_handle(dev)),
                   "unet_select_instances")
    return out.reshape(shape), counts.reshape(lead), new_ids.reshape(lead + (M,))


def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _exact_ratio(num, den):
    """float64 of the exact quotients of two object arrays of Python integers (one rounding each)"""
    return np.array([n / d for n, d in zip(num, den)], dtype=np.float64).reshape(num.shape)


def _frame_properties(tab, inten):
    ids = np.flatnonzero(tab[:, 0] > 0)
    t = tab[ids].astype(np.int64)
    area = t[:, 0]
    a = area.astype(np.float64)
    out = {"ids": (ids + 1).astype(np.int64), "area": area.copy(),
           "centroid": t[:, 1:3].astype(np.float64) / a[:, None], "bbox": t[:, 3:7].copy(),
           "perimeter": t[:, 10].copy(), "frame_edges": t[:, 11].copy(),
           "contact_fraction": t[:, 12].astype(np.float64) / t[:, 10].astype(np.float64),
           "touches_frame": t[:, 11] > 0, "equivalent_diameter": np.sqrt(4.0 * a / np.pi)}
    # area * sum_yy - sum_y^2 reaches 2^28 * 2^58 - 2^86: Python integers, then one division
    A, sy, sx, syy, sxx, sxy = (t[:, k].astype(object) for k in (0, 1, 2, 7, 8, 9))
    num = (A * syy - sy * sy, A * sxx - sx * sx, A * sxy - sy * sx)  # area * (mu_yy, mu_xx, mu_yx)
    out["moments_central"] = np.stack([_exact_ratio(n, A) for n in num], axis=-1).reshape(len(ids), 3)
    A2 = A * A
    c_yy = _exact_ratio(num[0], A2) + 1.0 / 12.0  # a pixel is a unit square: its own second moment is 1 / 12
    c_xx = _exact_ratio(num[1], A2) + 1.0 / 12.0
    c_yx = _exact_ratio(num[2], A2) + 0.0
    mid, dif = 0.5 * (c_yy + c_xx), 0.5 * (c_xx - c_yy)
    rad = np.sqrt(dif * dif + c_yx * c_yx)
    l1, l2 = mid + rad, np.maximum(mid - rad, 0.0)
    out["major_axis_length"] = 4.0 * np.sqrt(l1)
    out["minor_axis_length"] = 4.0 * np.sqrt(l2)
    out["eccentricity"] = np.sqrt(np.maximum(1.0 - l2 / l1, 0.0))
    out["orientation"] = 0.5 * np.arctan2(2.0 * c_yx, c_xx - c_yy)
    if inten is not None:
        v = inten[ids]  # [k, C, 4]
        out["intensity_sum"] = v[..., 0].copy()
        out["intensity_min"] = v[..., 2].copy()
        out["intensity_max"] = v[..., 3].copy()
        if v.dtype.kind == "f":
            mean = v[..., 0] / a[:, None]
            var = np.maximum(v[..., 1] / a[:, None] - mean * mean, 0.0)
        else:
            s, q = v[..., 0].astype(object), v[..., 1].astype(object)
            Ac, A2c = np.broadcast_to(A[:, None], s.shape), np.broadcast_to(A2[:, None], s.shape)
            mean = _exact_ratio(s.ravel(), Ac.ravel()).reshape(s.shape)
            var = _exact_ratio((Ac * q - s * s).ravel(), A2c.ravel()).reshape(s.shape)
        out["intensity_mean"] = mean
        out["intensity_std"] = np.sqrt(var)
    return out


def region_properties(measure):
    """Host-side region properties from a ``measure_instances`` result (this synchronises).

    ``measure``: an ``InstanceMeasure`` or any ``(table, status, intensity)`` /
    ``(table, status)`` of device tensors or host arrays.  Per frame a dict of
    numpy arrays over the ``k`` present ids in ascending order; a single frame
    gives one dict, leading dimensions give nested lists of that shape (as
    ``instance_properties``):

    ``ids``, ``area`` (int64 ``[k]``), ``centroid`` (float64 ``[k, 2]``, y and x),
    ``bbox`` (int64 ``[k, 4]``, half-open ``y0, x0, y1, x1``), ``perimeter`` (the
    crack length ``edges``), ``frame_edges``, ``contact_fraction`` (``contact_edges
    / edges``), ``touches_frame`` (bool), ``equivalent_diameter`` (``sqrt(4 area /
    pi)``), ``moments_central`` (``[k, 3]``: ``mu_yy, mu_xx, mu_yx`` with ``mu_yy =
    sum_yy - sum_y^2 / area``, formed as ``(area * sum_yy - sum_y^2) / area`` in
    exact integers with one division), ``major_axis_length``,
    ``minor_axis_length`` (``4 sqrt(l)`` of the eigenvalues ``l1 >= l2`` of the
    covariance), ``eccentricity`` (``sqrt(1 - l2 / l1)``) and ``orientation``
    (``0.5 atan2(2 c_yx, c_xx - c_yy)``: the angle of the major axis from +x
    towards +y, in ``(-pi/2, pi/2]``).  The covariance is ``mu / area + I / 12``:
    a pixel is taken as a unit square, not a point, and the ``1 / 12`` term is
    this package's choice (a single pixel has both axes ``2 / sqrt(3)``).

    With intensities, per channel (``[k, C]``): ``intensity_sum``,
    ``intensity_mean``, ``intensity_std`` (the population standard deviation;
    for integer images from ``area * sum_sq - sum^2`` in exact integers),
    ``intensity_min``, ``intensity_max``.
    """
    if not isinstance(measure, (tuple, list)) or len(measure) not in (2, 3):
        raise ValueError("region_properties: expected an InstanceMeasure or (table, status[, intensity])")
    table, status = _host(measure[0]), _host(measure[1])
    inten = _host(measure[2]) if len(measure) == 3 and measure[2] is not None else None
    if (table.ndim < 2 or table.shape[-1] != _lib.MEASURE_COLS or table.dtype.kind not in "iu"
            or status.shape != table.shape[:-2] + (_lib.MEASURE_STATUS,)):
        raise ValueError(f"region_properties: table {table.shape} {table.dtype} / status {status.shape} are not a "
                         f"measure_instances result")
    if inten is not None and (inten.ndim != table.ndim + 1 or inten.shape[:-2] != table.shape[:-1]
                              or inten.shape[-1] != _lib.MEASURE_ICOLS or inten.dtype.kind not in "iuf"):
        raise ValueError(f"region_properties: intensity {inten.shape} {inten.dtype} does not belong to table "
                         f"{table.shape}")

    def walk(tab, it):
        if tab.ndim == 2:
            return _frame_properties(tab, it)
        return [walk(t, None if it is None else it[i]) for i, t in enumerate(tab)]

    return walk(table, inten)
