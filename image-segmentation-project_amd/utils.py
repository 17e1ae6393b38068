"""Metrics and helpers of the training loop (/root/reference/utils.py:120-190).

``calculate_metrics`` keeps the reference aggregation exactly: foreground
counts pooled over the whole batch from ``pred > 0.5``, then precision /
recall / f1 / iou / accuracy with eps 1e-7 in Python floats (so an empty
prediction on an empty mask gives IoU 0, utils.py:142).  The counts come from
one HIP reduction (exact fp64 sums) and ONE device->host copy instead of the
reference's four ``.item()`` syncs.
"""
from __future__ import annotations

import torch

from . import _lib

EPS = 1e-7


def metrics_from_counts(tp: float, fp: float, fn: float, tn: float) -> dict:
    """utils.py:135-151 formula on already-reduced counts."""
    precision = tp / (tp + fp + EPS)
    recall = tp / (tp + fn + EPS)
    f1 = 2 * precision * recall / (precision + recall + EPS)
    iou = tp / (tp + fp + fn + EPS)
    accuracy = (tp + tn) / (tp + tn + fp + fn + EPS)
    return {"precision": precision, "recall": recall, "f1": f1, "iou": iou, "accuracy": accuracy}


def mask_counts(values, target, from_logits: bool):
    """Device fp64 tensor [8]; [4:8] = tp, fp, fn, tn (no host sync)."""
    _lib.require_gpu(values, target)
    v = values.contiguous().float()
    t = target.to(device=v.device, dtype=torch.float32).contiguous()
    sums, scratch = _lib.loss_buffers(v.device)
    _lib.check(_lib.load().unet_mask_metrics(v.data_ptr(), t.data_ptr(), v.numel(), 0 if from_logits else 1,
                                             sums.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                             _lib.stream_handle(v.device)), "unet_mask_metrics")
    return sums


def calculate_metrics(pred, target) -> dict:
    """utils.py:120-151: ``pred`` are probabilities (sigmoid outputs)."""
    c = mask_counts(pred, target, from_logits=False)[4:8].tolist()
    return metrics_from_counts(*c)


def calculate_metrics_from_logits(logits, target) -> dict:
    """Same as ``calculate_metrics(torch.sigmoid(logits), target)`` with the mask
    decided bit-exactly as the reference's fp32 CPU sigmoid does."""
    c = mask_counts(logits, target, from_logits=True)[4:8].tolist()
    return metrics_from_counts(*c)


def _per_class(values, target, from_logits: bool) -> list:
    if values.dim() != 4 or tuple(values.shape) != tuple(target.shape):
        raise ValueError(f"expected [N,K,H,W] values and target of one shape, got {tuple(values.shape)} "
                         f"and {tuple(target.shape)}")
    out = []
    for k in range(values.shape[1]):
        c = mask_counts(values[:, k].contiguous(), target[:, k].contiguous(), from_logits)[4:8].tolist()
        out.append(metrics_from_counts(*c))
    return out


def calculate_metrics_per_class(pred, target) -> list:
    """``calculate_metrics`` of every channel of ``[N,K,H,W]`` probabilities: a
    list of K dicts (the same exact counts, one reduction per channel)."""
    return _per_class(pred, target, from_logits=False)


def calculate_metrics_per_class_from_logits(logits, target) -> list:
    """``calculate_metrics_from_logits`` of every channel of ``[N,K,H,W]`` logits."""
    return _per_class(logits, target, from_logits=True)


def confusion_matrix(logits, labels, ignore_index=-100):
    """Device int64 ``[K,K]`` (row = true class, column = argmax of the logits,
    lowest index on ties) of ``[N,K,H,W]`` logits and an integer label map
    ``[N,H,W]`` / ``[N,1,H,W]``; labels equal to ``ignore_index`` or outside
    ``[0,K)`` are not counted.  One HIP pass, exact integer counts, no host sync."""
    from .losses import softmax_inputs
    n, k, hw, labels = softmax_inputs(logits, labels)
    _lib.require_gpu(logits)
    x = logits.detach().contiguous().float()
    y = labels.to(x.device).contiguous()
    _, scratch = _lib.softmax_buffers(x.device)
    cm = torch.empty((k, k), dtype=torch.int64, device=x.device)
    _lib.check(_lib.load().unet_confusion_matrix(x.data_ptr(), y.data_ptr(), _lib.LABEL_DTYPES[y.dtype], n, k, hw,
                                                 int(ignore_index), cm.data_ptr(), scratch.data_ptr(),
                                                 scratch.numel(), _lib.stream_handle(x.device)),
               "unet_confusion_matrix")
    return cm


def metrics_from_confusion(cm) -> dict:
    """Metrics of a ``[K,K]`` confusion matrix (row = truth, column = prediction),
    in Python floats on the host.  Per class one-vs-rest with the formulas of
    ``metrics_from_counts``; ``precision`` / ``recall`` / ``f1`` are their macro
    means, ``iou`` is the mean IoU over the classes that occur in the truth or
    the prediction (tp + fp + fn > 0; 0.0 when there is none), ``accuracy`` is
    trace / total; the per-class lists are under ``"per_class"``."""
    rows = cm.detach().cpu().tolist() if isinstance(cm, torch.Tensor) else [list(r) for r in cm]
    k = len(rows)
    if k == 0 or any(len(r) != k for r in rows):
        raise ValueError("metrics_from_confusion needs a square [K,K] matrix")
    total = sum(sum(r) for r in rows)
    per = {"precision": [], "recall": [], "f1": [], "iou": []}
    present = []
    for c in range(k):
        tp = rows[c][c]
        fp = sum(rows[r][c] for r in range(k)) - tp
        fn = sum(rows[c]) - tp
        m = metrics_from_counts(tp, fp, fn, total - tp - fp - fn)
        for name in per:
            per[name].append(m[name])
        if tp + fp + fn > 0:
            present.append(m["iou"])
    out = {name: sum(per[name]) / k for name in ("precision", "recall", "f1")}
    out["iou"] = sum(present) / len(present) if present else 0.0
    out["accuracy"] = sum(rows[c][c] for c in range(k)) / (total + EPS)
    out["per_class"] = per
    return out


def calculate_multiclass_metrics(logits, labels, ignore_index=-100) -> dict:
    """``metrics_from_confusion(confusion_matrix(...))``: argmax metrics of
    mutually exclusive classes (one device->host copy of K*K counts)."""
    return metrics_from_confusion(confusion_matrix(logits, labels, ignore_index))


def get_device():
    """utils.py:153-167 — the ROCm GPU when present (torch's 'cuda' device)."""
    if torch.cuda.is_available():
        print("Using CUDA device")
        return torch.device("cuda")
    print("Using CPU")
    return torch.device("cpu")


class EarlyStopping:
    """utils.py:174-190 — stop after ``patience`` non-improving steps."""

    def __init__(self, patience=10, min_delta=0.001):
        self.patience = patience
        self.min_delta = min_delta
        self.counter = 0
        self.best_score = None
        self.early_stop = False

    def step(self, current_score):
        improved = self.best_score is None or current_score > self.best_score + self.min_delta
        if improved:
            self.best_score = current_score
            self.counter = 0
        else:
            self.counter += 1
            self.early_stop = self.early_stop or self.counter >= self.patience
        return self.early_stop
