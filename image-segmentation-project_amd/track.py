"""Linking instances across frames on the GPU: ``link_instances`` turns a sequence
of per-frame label maps (a time lapse, or the slices of a z-stack) into the same
maps with one id per track, a lineage table and a status row (``csrc/track.hip``:
``unet_link_instances``, on the tables of ``csrc/match.hip``); ``track_properties``
is the host view of the result (the one place that synchronises).  No reference
counterpart; tests/track_ref.py holds the rule as numpy and Python integers.

Two instances of consecutive frames are linked when each is the other's partner
of highest IoU and that IoU is strictly above ``min_iou``; everything is decided
in integers on the original ids, so every output is bit-reproducible.
"""
from __future__ import annotations

import collections
from fractions import Fraction

import numpy as np
import torch

from . import _lib
from ._frames import as_frames, workspace
from .match import MAX_ID, MAX_PAIRS

TRACK_COLUMNS = ("first", "last", "parent", "volume")  # the last axis of table
TRACK_STATUS = ("n_tracks", "n_links", "dropped", "out_of_range")  # the last axis of status
assert len(TRACK_COLUMNS) == _lib.LINK_COLS and len(TRACK_STATUS) == _lib.LINK_STATUS
MAX_DIM = _lib.DISTANCE_MAX_DIM
MAX_HW = _lib.GEODESIC_MAX_HW
MAX_FRAMES = 65535
MAX_TRACKS = (1 << 31) - 1

InstanceLinks = collections.namedtuple("InstanceLinks", ("tracks", "table", "status"))


def _min_iou(min_iou):
    if isinstance(min_iou, bool) or not isinstance(min_iou, (int, float, Fraction, np.integer, np.floating)):
        raise ValueError(f"min_iou={min_iou!r} must be a number")
    if isinstance(min_iou, np.generic):
        min_iou = min_iou.item()
    try:
        f = Fraction(min_iou).limit_denominator(1000)
    except (ValueError, OverflowError):
        raise ValueError(f"min_iou={min_iou!r} must satisfy 0 <= min_iou < 1") from None
    if not 0 <= f < 1:
        raise ValueError(f"min_iou={min_iou!r} must satisfy 0 <= min_iou < 1")
    return f


def _int_in(value, name, lo, hi):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not lo <= int(value) <= hi:
        raise ValueError(f"{name}={value!r} must be an integer in {lo}..{hi}")
    return int(value)


def link_instances(labels, min_iou=0.25, max_instances=4096, max_tracks=None, max_pairs=None):
    """Track ids for the instances of a sequence of label maps, on the GPU.

    ``labels``: an int32 label map ``[T, H, W]`` or ``[B, T, H, W]``, tensor or
    array; axis ``-3`` is the sequence (time, or z for a stack of 2-D
    segmentations), leading ``B`` are independent sequences.  Within a frame 0
    is background and the ids run up to ``max_instances`` (at most 65535); they
    need not be compact and mean nothing across frames.  ``T == 1`` is valid, ``T
    <= 65535``, ``H, W <= 32768`` and ``H * W <= 2^28``.

    The rule, in integers on the original ids (all ``T - 1`` frame pairs are
    independent): with ``min_iou`` taken as ``Fraction(min_iou)
    .limit_denominator(1000)`` (``0 <= min_iou < 1``), instance ``b`` of frame
    ``t >= 1`` and its partner ``a`` of highest IoU in frame ``t - 1`` (as
    ``match_instances(pred=frame t, gt=frame t - 1)`` defines it, ties to the
    smaller id; intersection ``I``, areas ``A_a``, ``A_b``):

    * ``b`` continues the track of ``a`` iff ``a`` exists, the best partner of
      ``a`` in frame ``t`` is ``b`` and the IoU is strictly above ``min_iou`` (an
      IoU equal to it is no link; with ``min_iou=0`` every mutually best
      overlapping pair links);
    * otherwise ``b`` starts a track, whose ``parent`` is the track of ``a`` iff
      ``a`` exists and ``2 * I > A_b`` (more than half of ``b`` lies on ``a``),
      else 0.

    Every instance of frame 0 starts a track without a parent.  In a division the
    daughter that is the mother's best partner may continue the mother's track
    and the other daughter gets it as parent.  There is no gap closing: a cell
    absent for one frame comes back as a new track.  Tracks are numbered
    ``1..n_tracks`` in the order (first frame, original id), so the result is a
    pure function of the input.

    Returns ``InstanceLinks(tracks, table, status)`` of device tensors:
    ``tracks`` int32 of the shape of ``labels`` (the track id of every pixel
    with an id in ``1..max_instances``, 0 elsewhere); ``table`` int64 ``[B,
    max_tracks, 4]`` (``TRACK_COLUMNS``; no ``B`` axis for a 3-D input), row
    ``track - 1`` = ``first, last`` (frame indices), ``parent`` (a track id or
    0), ``volume`` (the sum of the areas over the frames), zero rows for absent
    tracks; ``status`` int64 ``[B, 4]`` (``TRACK_STATUS``): ``n_tracks`` is the
    true count and ``tracks`` carries the true ids even above ``max_tracks``
    (default ``4 * max_instances``), only the table ends at ``max_tracks`` rows,
    so ``n_tracks > max_tracks`` is the overflow signal; ``n_links`` the
    instances that continue a track; ``dropped`` and ``out_of_range`` those of
    ``match_instances`` summed over the frame pairs (``max_pairs`` as there,
    default ``8 * max_instances``).  When one of the two is nonzero only
    ``status`` is specified; ``track_properties`` checks them.

    ``labels`` is not modified and nothing synchronises with the host.  Without
    a GPU the call raises ``RuntimeError``.
    """
    what = "link_instances: labels"
    labels = as_frames(labels, what, (torch.int32,))
    if labels.dim() not in (3, 4):
        raise ValueError(f"{what} must be [T, H, W] or [B, T, H, W], got {tuple(labels.shape)}")
    T, H, W = labels.shape[-3:]
    if H > MAX_DIM or W > MAX_DIM or H * W > MAX_HW:
        raise ValueError(f"{what}: H = {H}, W = {W} must be <= {MAX_DIM} with H * W <= 2^28")
    if T > MAX_FRAMES:
        raise ValueError(f"{what}: T = {T} must be <= {MAX_FRAMES}")
    frac = _min_iou(min_iou)
    max_instances = _int_in(max_instances, "max_instances", 1, MAX_ID)
    if max_pairs is None:
        max_pairs = 8 * max_instances
    max_pairs = _int_in(max_pairs, "max_pairs", 1, MAX_PAIRS)
    if max_tracks is None:
        max_tracks = 4 * max_instances
    max_tracks = _int_in(max_tracks, "max_tracks", 1, MAX_TRACKS)
    if T * min(max_instances, H * W) > MAX_TRACKS:
        raise ValueError(f"{what}: T * min(max_instances, H * W) = {T * min(max_instances, H * W)} track ids do "
                         f"not fit int32")
    if not labels.is_cuda:
        _lib.require_gpu()
        labels = labels.cuda()
    _lib.require_gpu(labels)
    shape = tuple(labels.shape)
    lab = labels.reshape(-1, T, H, W).contiguous()
    B = lab.shape[0]
    lib = _lib.load()
    dev = lab.device
    with torch.cuda.device(dev):
        tracks = torch.empty_like(lab)
        table = torch.empty((B, max_tracks, _lib.LINK_COLS), dtype=torch.int64, device=dev)
        status = torch.empty((B, _lib.LINK_STATUS), dtype=torch.int64, device=dev)
        ws, nbytes = workspace(lib, "unet_link_workspace_bytes", dev, B, T, max_instances, max_pairs)
        _lib.check(lib.unet_link_instances(lab.data_ptr(), B, T, H, W, max_instances, max_pairs, max_tracks,
                                           frac.numerator, frac.denominator, tracks.data_ptr(), table.data_ptr(),
                                           status.data_ptr(), ws.data_ptr(), nbytes, _lib.stream_handle(dev)),
                   "unet_link_instances")
    if len(shape) == 3:
        table = table[0]
    return InstanceLinks(tracks.reshape(shape), table, status)


def _host(x):
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return a.astype(np.int64, copy=False)


def track_properties(links):
    """The lineage of a ``link_instances`` result as host arrays (this synchronises).

    ``links``: an ``InstanceLinks`` (or any ``(tracks, table, status)``; only
    ``table`` and ``status`` are read) of device tensors or host arrays.

    Returns a dict; under every key a list with one entry per sequence (the
    entry itself for the result of a 3-D input, whose table has no ``B`` axis):
    over the ``n_tracks`` present tracks the int64 arrays ``track``
    (``1..n_tracks``), ``first``, ``last``, ``parent``, ``length`` (``last -
    first + 1``) and ``volume``; ``children``, a list of arrays (the tracks whose
    ``parent`` is this track, ascending); and ``ctc``, the ``[n, 4]`` array ``L B E
    P`` of the Cell Tracking Challenge's ``res_track.txt`` (label, first frame,
    last frame, parent).  Unlike the challenge's convention, in which both
    daughters of a division are new tracks, the daughter that is the mother's
    best partner above ``min_iou`` continues the mother's track here and only the
    other one names it as parent: a parent's ``E`` may therefore lie after its
    child's ``B``.

    Raises ``RuntimeError`` when the result is incomplete: ``dropped`` or
    ``out_of_range`` nonzero, or ``n_tracks`` above the table's ``max_tracks``.
    """
    table, status = _host(links[1]), _host(links[2])
    if (status.ndim != 2 or status.shape[1] != _lib.LINK_STATUS or table.ndim not in (2, 3)
            or table.shape[-1] != _lib.LINK_COLS):
        raise ValueError(f"track_properties: table {table.shape} / status {status.shape} are not a link_instances "
                         f"result")
    single = table.ndim == 2
    if single:
        table = table[None]
    if table.shape[0] != status.shape[0]:
        raise ValueError(f"track_properties: table {table.shape} and status {status.shape} differ in sequences")
    if status[:, 2].any():
        raise RuntimeError(f"track_properties: {int(status[:, 2].sum())} pixels found no room in a pair table "
                           f"(status.dropped): call link_instances with a larger max_pairs")
    if status[:, 3].any():
        raise RuntimeError(f"track_properties: {int(status[:, 3].sum())} pixels carry an id below 0 or above the "
                           f"cap (status.out_of_range): call link_instances with a larger max_instances")
    max_tracks = table.shape[1]
    if (status[:, 0] > max_tracks).any():
        raise RuntimeError(f"track_properties: {int(status[:, 0].max())} tracks but the table has {max_tracks} rows "
                           f"(status.n_tracks): call link_instances with a larger max_tracks")
    keys = ("track", "first", "last", "parent", "length", "volume", "children", "ctc")
    out = {k: [] for k in keys}
    for b in range(table.shape[0]):
        n = int(status[b, 0])
        first, last, parent, volume = (np.array(table[b, :n, k]) for k in range(4))
        track = np.arange(1, n + 1, dtype=np.int64)
        order = np.argsort(parent, kind="stable")
        lo = np.searchsorted(parent[order], track, side="left")
        hi = np.searchsorted(parent[order], track, side="right")
        out["track"].append(track)
        out["first"].append(first)
        out["last"].append(last)
        out["parent"].append(parent)
        out["length"].append(last - first + 1)
        out["volume"].append(volume)
        out["children"].append([track[order[i:j]] for i, j in zip(lo, hi)])
        out["ctc"].append(np.stack([track, first, last, parent], axis=1))
    return {k: v[0] for k, v in out.items()} if single else out
