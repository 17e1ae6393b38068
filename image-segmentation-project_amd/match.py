"""Scoring instances on the GPU: ``match_instances`` matches the instances of a
predicted label map to those of a ground truth (``csrc/match.hip``:
``unet_match_instances``) and ``instance_metrics`` turns the tables into the
DSB-2018 average precision over IoU thresholds, F1, panoptic quality and the
aggregated Jaccard index.  No reference counterpart; tests/match_ref.py holds the
definitions as numpy and Python integers.

The tables are integer counts from integer atomics, and every IoU comparison is a
comparison of integer products: the outputs are bit-reproducible.
"""
from __future__ import annotations

import collections
from fractions import Fraction

import numpy as np
import torch

from . import _lib
from ._frames import as_frames, frames_on_gpu, workspace
from .utils import EPS

MATCH_COLUMNS = ("area", "partner", "intersection", "partner_area")  # the last axis of both tables
STATUS_COLUMNS = ("n_gt", "n_pred", "n_pairs", "dropped", "out_of_range")  # the last axis of status
assert len(MATCH_COLUMNS) == _lib.MATCH_COLS and len(STATUS_COLUMNS) == _lib.MATCH_STATUS
MAX_ID = 65535
MAX_PAIRS = 1 << 24
DEFAULT_THRESHOLDS = tuple(Fraction(10 + k, 20) for k in range(10))  # 0.5, 0.55, ..., 0.95

InstanceMatch = collections.namedtuple("InstanceMatch", ("gt_table", "pred_table", "status"))
InstanceMatchPairs = collections.namedtuple("InstanceMatch", ("gt_table", "pred_table", "status", "pairs"))


def match_instances(pred, gt, max_instances=4096, max_pairs=None, return_pairs=False):
    """IoU tables of predicted instances against a ground truth, on the GPU.

    ``pred`` and ``gt``: int32 label maps (as ``label_instances`` and
    ``grow_instances`` return them), tensors or arrays of equal shape ``[H, W]``,
    ``[N, H, W]`` or ``[N, K, H, W]``; leading dimensions are independent frames.
    0 is background; ids run up to ``max_instances`` (at most 65535) on both
    sides and need not be compact.  ``max_pairs`` (default ``8 *
    max_instances``, at most 2^24) sizes the pair table of a frame: the smallest
    power of two ``>= 2 * max_pairs`` entries for the overlapping (gt, pred)
    pairs and one entry per instance that also touches background.

    Returns ``InstanceMatch(gt_table, pred_table, status)`` of device int64
    tensors: ``gt_table`` ``[..., max_instances, 4]``, row ``id - 1`` = ``area,
    partner, intersection, partner_area`` where ``partner`` is the id of the
    other map that overlaps with the highest IoU (the smaller id among equal
    IoUs; all three 0 for an absent id or one that overlaps nothing);
    ``pred_table`` the same for the predicted ids; ``status`` ``[..., 5]`` =
    ``n_gt, n_pred, n_pairs, dropped, out_of_range``.  ``dropped`` (pixels whose
    pair found no room: raise ``max_pairs``) and ``out_of_range`` (pixels with an
    id below 0 or above ``max_instances``) are 0 when the tables describe the
    maps exactly; ``instance_metrics`` checks them.  With ``return_pairs=True``
    also ``pairs`` ``[..., max_pairs, 3]``: ``gt, pred, intersection`` of the
    ``n_pairs`` overlapping pairs, sorted by ``(gt, pred)``, zero rows after
    them.  The inputs are not modified and nothing synchronises with the host;
    ``instance_metrics`` does.
    """
    pred = as_frames(pred, "match_instances: pred", (torch.int32,))
    gt = as_frames(gt, "match_instances: gt", (torch.int32,))
    if tuple(pred.shape) != tuple(gt.shape):
        raise ValueError(f"match_instances: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ")
    if isinstance(max_instances, bool) or not 1 <= int(max_instances) <= MAX_ID:
        raise ValueError(f"max_instances={max_instances!r} must be in 1..{MAX_ID}")
    max_instances = int(max_instances)
    if max_pairs is None:
        max_pairs = 8 * max_instances
    if isinstance(max_pairs, bool) or not 1 <= int(max_pairs) <= MAX_PAIRS:
        raise ValueError(f"max_pairs={max_pairs!r} must be in 1..{MAX_PAIRS}")
    max_pairs = int(max_pairs)
    if not pred.is_cuda and not gt.is_cuda:
        _lib.require_gpu()
        pred, gt = pred.cuda(), gt.cuda()
    elif pred.device != gt.device:
        pred, gt = (pred.to(gt.device), gt) if gt.is_cuda else (pred, gt.to(pred.device))
    lead = tuple(gt.shape)[:-2]
    p, g = frames_on_gpu(pred), frames_on_gpu(gt)
    lib = _lib.load()
    N, H, W = g.shape
    dev = g.device
    with torch.cuda.device(dev):
        gt_table = torch.empty((N, max_instances, _lib.MATCH_COLS), dtype=torch.int64, device=dev)
        pred_table = torch.empty((N, max_instances, _lib.MATCH_COLS), dtype=torch.int64, device=dev)
        status = torch.empty((N, _lib.MATCH_STATUS), dtype=torch.int64, device=dev)
        pairs = torch.empty((N, max_pairs, 3), dtype=torch.int64, device=dev) if return_pairs else None
        ws, nbytes = workspace(lib, "unet_match_workspace_bytes", dev, N, max_instances, max_instances, max_pairs)
        _lib.check(lib.unet_match_instances(g.data_ptr(), p.data_ptr(), N, H, W, max_instances, max_instances,
                                            max_pairs, gt_table.data_ptr(), pred_table.data_ptr(), status.data_ptr(),
                                            _lib.ptr(pairs), ws.data_ptr(), nbytes, _lib.stream_handle(dev)),
                   "unet_match_instances")
        if return_pairs:
            # the kernel appends in arrival order: one sort of gt << 16 | pred (zero rows last) fixes the order
            key = (pairs[..., 0] << 16) | pairs[..., 1]
            key = torch.where(key == 0, torch.full_like(key, 1 << 62), key)
            order = torch.sort(key, dim=1).indices
            pairs = torch.gather(pairs, 1, order[..., None].expand(-1, -1, 3))
    out = [gt_table.reshape(lead + (max_instances, _lib.MATCH_COLS)),
           pred_table.reshape(lead + (max_instances, _lib.MATCH_COLS)), status.reshape(lead + (_lib.MATCH_STATUS,))]
    if return_pairs:
        return InstanceMatchPairs(*out, pairs.reshape(lead + (max_pairs, 3)))
    return InstanceMatch(*out)


def _threshold(t):
    f = t if isinstance(t, Fraction) else Fraction(float(t)).limit_denominator(1000)
    if f < Fraction(1, 2):
        raise ValueError(f"instance_metrics: threshold {t!r} must be >= 0.5: below it an instance can match more "
                         f"than once")
    return f


def _host(x):
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return a.astype(np.int64, copy=False)


def _scores(tp, fp, fn, sum_iou, c, u):
    """tp, fp, fn int64 [..., T]; sum_iou float64 [4, ...]: at 0.5 the sum of the matched IoUs, tp, fp, fn;
    c, u int64 [...]: the sums of the aggregated Jaccard index"""
    tp_f, fp_f, fn_f = tp.astype(np.float64), fp.astype(np.float64), fn.astype(np.float64)
    precision = tp_f / (tp_f + fp_f + EPS)
    recall = tp_f / (tp_f + fn_f + EPS)
    out = {"tp": tp, "fp": fp, "fn": fn, "precision": precision, "recall": recall,
           "f1": 2 * precision * recall / (precision + recall + EPS), "ap": tp_f / (tp_f + fp_f + fn_f + EPS)}
    out["mean_ap"] = out["ap"].mean(axis=-1)
    tp5, fp5, fn5 = sum_iou[1], sum_iou[2], sum_iou[3]
    den = tp5 + 0.5 * fp5 + 0.5 * fn5 + EPS
    out["pq"] = sum_iou[0] / den
    out["sq"] = sum_iou[0] / (tp5 + EPS)
    out["rq"] = tp5 / den
    uf = u.astype(np.float64)
    out["aji"] = np.where(u > 0, c.astype(np.float64) / np.where(u > 0, uf, 1.0), 0.0)
    return out


def instance_metrics(match, thresholds=DEFAULT_THRESHOLDS):
    """Instance scores from a ``match_instances`` result (this synchronises).

    ``match``: an ``InstanceMatch`` (or any ``(gt_table, pred_table, status,
    ...)``) of device tensors or host arrays.  ``thresholds``: IoU thresholds of
    at least 0.5, each taken as ``Fraction(t).limit_denominator(1000)``; a gt
    instance is a true positive at ``t`` when the IoU with its partner is
    strictly above ``t`` (decided in integers).  From 0.5 on such a match is
    unique and is both sides' best partner; a threshold below 0.5 raises
    ``ValueError``.

    Returns a dict of numpy arrays of the leading (frame) shape: ``tp``, ``fp``,
    ``fn`` (int64 ``[..., T]``), ``precision``, ``recall``, ``f1`` and ``ap = tp /
    (tp + fp + fn)`` (``[..., T]``), ``mean_ap`` (the mean over the thresholds),
    ``pq``, ``sq``, ``rq`` (panoptic, segmentation and recognition quality at
    0.5: the sum of the matched IoUs over ``tp + fp / 2 + fn / 2``, over ``tp``,
    and their ratio) and ``aji`` (the aggregated Jaccard index, an exact integer
    ratio; 0 where both maps are empty); under ``"pooled"`` the same from the
    counts summed over all frames.  The count ratios add the package's ``EPS``
    to the denominator as ``calculate_metrics`` does, so an empty frame scores 0.
    Raises ``RuntimeError`` when the tables are incomplete (``dropped`` or
    ``out_of_range`` nonzero).
    """
    ths = [_threshold(t) for t in thresholds]
    if not ths:
        raise ValueError("instance_metrics: no thresholds")
    gt_table, pred_table, status = _host(match[0]), _host(match[1]), _host(match[2])
    if (gt_table.ndim < 2 or gt_table.shape[-1] != _lib.MATCH_COLS or pred_table.ndim != gt_table.ndim
            or pred_table.shape[-1] != _lib.MATCH_COLS or status.shape[-1:] != (_lib.MATCH_STATUS,)
            or not gt_table.shape[:-2] == pred_table.shape[:-2] == status.shape[:-1]):
        raise ValueError(f"instance_metrics: gt_table {gt_table.shape} / pred_table {pred_table.shape} / status "
                         f"{status.shape} are not a match_instances result")
    lead = status.shape[:-1]
    if status[..., 3].any():
        raise RuntimeError(f"instance_metrics: {int(status[..., 3].sum())} pixels found no room in the pair table "
                           f"(status.dropped): call match_instances with a larger max_pairs")
    if status[..., 4].any():
        raise RuntimeError(f"instance_metrics: {int(status[..., 4].sum())} pixels carry an id below 0 or above the "
                           f"cap (status.out_of_range): call match_instances with a larger max_instances")
    G, P = gt_table.shape[-2], pred_table.shape[-2]
    gtab = gt_table.reshape(-1, G, _lib.MATCH_COLS)
    ptab = pred_table.reshape(-1, P, _lib.MATCH_COLS)
    F, T = gtab.shape[0], len(ths)
    tp = np.zeros((F, T), np.int64)
    n_gt = np.zeros(F, np.int64)
    n_pred = np.zeros(F, np.int64)
    five = np.zeros((4, F), np.float64)  # at 0.5: sum of matched IoUs, tp, fp, fn
    cc = np.zeros(F, np.int64)
    uu = np.zeros(F, np.int64)
    for f in range(F):
        area, partner, inter, parea = (gtab[f, :, k] for k in range(4))
        n_gt[f] = np.count_nonzero(area)
        n_pred[f] = np.count_nonzero(ptab[f, :, 0])
        has = partner > 0
        c, u = inter[has], (area + parea - inter)[has]
        for k, t in enumerate(ths):
            tp[f, k] = np.count_nonzero(c * t.denominator > t.numerator * u)
        m5 = 2 * c > u
        five[0, f] = float(np.sum(c[m5].astype(np.float64) / u[m5].astype(np.float64)))
        five[1, f] = np.count_nonzero(m5)
        # aggregated Jaccard index: every gt with its best partner, then the preds that are nobody's best partner
        used = np.zeros(P + 1, bool)
        used[partner[has]] = True
        cc[f] = int(c.sum())
        uu[f] = int(u.sum()) + int(area[~has].sum()) + int(ptab[f, :, 0][~used[1:]].sum())
    fp, fn = n_pred[:, None] - tp, n_gt[:, None] - tp
    five[2], five[3] = n_pred - five[1], n_gt - five[1]
    out = _scores(tp, fp, fn, five, cc, uu)
    out = {k: v.reshape(lead + v.shape[1:]) for k, v in out.items()}
    out["pooled"] = _scores(tp.sum(0), fp.sum(0), fn.sum(0), five.sum(1), cc.sum(), uu.sum())
    out["pooled"] = {k: np.asarray(v) for k, v in out["pooled"].items()}
    out["thresholds"] = np.array([float(t) for t in ths])
    return out
