"""Pixel-wise segmentation losses on MI355X (hot-path subset of
/root/reference/losses.py).

``BCELoss`` (:31-37), ``DiceLoss`` (:13-28, one global Dice over the whole
batch, smooth=1) and ``ComboLoss`` (:161-171, alpha*BCE + (1-alpha)*Dice) run as
one fused HIP reduction (BCE terms, sum sigma*y, sum sigma, sum y in fp64) plus
a fused gradient kernel.  ``get_loss_function`` (:345-403) keeps the registry
behaviour: default 'combo', unknown names print a warning and fall back to
ComboLoss.  The reference's other fourteen losses (``_NOT_ON_PATH``) are outside
the hot path and raise ``NotImplementedError``.

Those three treat the K output channels as independent sigmoid planes.  For
mutually exclusive classes (one integer label per pixel, which the reference
does not have) ``CrossEntropyLoss``, ``SoftmaxDiceLoss`` and
``SoftmaxComboLoss`` run a softmax over the channels: one fused pass over the
fp32 NCHW logits for all sums, one for the gradient (csrc/softmax_loss.hip).
Registry names: 'ce', 'softmax_dice', 'softmax_combo'.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib

BCE, DICE, COMBO = 0, 1, 2


class _FusedLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, kind, alpha, smooth):
        _lib.require_gpu(logits, target)
        lib = _lib.load()
        x = logits.contiguous().float()
        t = target.to(device=x.device, dtype=torch.float32).contiguous()
        if x.numel() != t.numel():
            raise ValueError(f"logits {tuple(x.shape)} and target {tuple(t.shape)} differ in size")
        sums, scratch = _lib.loss_buffers(x.device)
        out = torch.empty((), dtype=torch.float32, device=x.device)
        _lib.check(lib.unet_loss_forward(x.data_ptr(), t.data_ptr(), x.numel(), kind, float(alpha), float(smooth),
                                         sums.data_ptr(), scratch.data_ptr(), scratch.numel(), out.data_ptr(),
                                         _lib.stream_handle(x.device)),
                   "unet_loss_forward")
        ctx.save_for_backward(x, t, sums)
        ctx.cfg = (kind, float(alpha), float(smooth))
        ctx.in_shape = logits.shape
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, t, sums = ctx.saved_tensors
        kind, alpha, smooth = ctx.cfg
        g = grad_out.contiguous().float()
        dl = torch.empty_like(x)
        _lib.check(_lib.load().unet_loss_backward(x.data_ptr(), t.data_ptr(), x.numel(), kind, alpha, smooth,
                                                  sums.data_ptr(), g.data_ptr(), dl.data_ptr(),
                                                  _lib.stream_handle(x.device)), "unet_loss_backward")
        return dl.view(ctx.in_shape), None, None, None, None


class DiceLoss(nn.Module):
    """losses.py:13-28 — 1 - (2*sum(sigma*y) + smooth) / (sum sigma + sum y + smooth)."""

    def __init__(self, smooth=1.0):
        super().__init__()
        self.smooth = smooth

    def forward(self, pred, target):
        return _FusedLoss.apply(pred, target, DICE, 0.0, self.smooth)


class BCELoss(nn.Module):
    """losses.py:31-37 — F.binary_cross_entropy_with_logits, mean reduction."""

    def forward(self, pred, target):
        return _FusedLoss.apply(pred, target, BCE, 1.0, 1.0)


class ComboLoss(nn.Module):
    """losses.py:161-171 — alpha * BCE + (1 - alpha) * Dice."""

    def __init__(self, alpha=0.5, smooth=1.0):
        super().__init__()
        self.alpha = alpha
        self.smooth = smooth

    def forward(self, pred, target):
        return _FusedLoss.apply(pred, target, COMBO, self.alpha, self.smooth)


def softmax_inputs(logits, labels):
    """Validate ``[N,K,H,W]`` float logits against an integer label map
    ``[N,H,W]`` (or ``[N,1,H,W]``) and return ``(N, K, HW, labels [N,H,W])``.
    Raises ``ValueError``; runs before any GPU is touched."""
    if not isinstance(logits, torch.Tensor) or not isinstance(labels, torch.Tensor):
        raise ValueError("logits and labels must be tensors")
    if logits.dim() != 4 or not logits.is_floating_point():
        raise ValueError(f"expected float logits [N,K,H,W], got {logits.dtype} {tuple(logits.shape)}")
    n, k, h, w = logits.shape
    if k < 2 or k > _lib.SOFTMAX_MAX_CLASSES:
        raise ValueError(f"softmax losses / metrics need 2..{_lib.SOFTMAX_MAX_CLASSES} classes, got K = {k} "
                         "(a single channel is the sigmoid path: bce / dice / combo)")
    if labels.dtype not in _lib.LABEL_DTYPES:
        raise ValueError(f"labels must be an integer class map of dtype uint8, int32 or int64, got {labels.dtype} "
                         "(float [N,K,H,W] planes are the sigmoid path: bce / dice / combo)")
    if labels.dim() == 4 and labels.shape[1] == 1:
        labels = labels[:, 0]
    if tuple(labels.shape) != (n, h, w):
        raise ValueError(f"labels {tuple(labels.shape)} do not match logits {tuple(logits.shape)}: expected "
                         f"[{n},{h},{w}] or [{n},1,{h},{w}]")
    if n == 0 or h * w == 0:
        raise ValueError(f"empty logits {tuple(logits.shape)}")
    return n, k, h * w, labels


def pixel_weight_input(pixel_weights, n, h, w):
    """Validate per-pixel loss weights (a float tensor ``[N,H,W]`` or ``[N,1,H,W]``)
    against the logits' shape and return them as ``[N,H,W]``.  Raises
    ``ValueError``; runs before any GPU is touched."""
    if not isinstance(pixel_weights, torch.Tensor) or not pixel_weights.is_floating_point():
        raise ValueError("pixel_weights must be a float tensor [N,H,W] or [N,1,H,W]")
    if pixel_weights.dim() == 4 and pixel_weights.shape[1] == 1:
        pixel_weights = pixel_weights[:, 0]
    if tuple(pixel_weights.shape) != (n, h, w):
        raise ValueError(f"pixel_weights {tuple(pixel_weights.shape)} do not match the logits: expected "
                         f"[{n},{h},{w}] or [{n},1,{h},{w}]")
    return pixel_weights


def _class_weights(weight, k):
    if weight is None:
        return None
    w = torch.as_tensor(weight, dtype=torch.float32).reshape(-1)
    if k is not None and w.numel() != k:
        raise ValueError(f"class weights have {w.numel()} entries, the logits have K = {k} classes")
    return w


class _SoftmaxLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, weight, kind, alpha, smooth, ignore_index, pixel_weights=None):
        n, k, hw, labels = softmax_inputs(logits, labels)
        weight = _class_weights(weight, k)
        if pixel_weights is not None:
            if kind == DICE:
                raise ValueError("pixel weights apply to the cross-entropy term; SoftmaxDiceLoss takes none")
            pixel_weights = pixel_weight_input(pixel_weights, n, logits.shape[2], logits.shape[3])
        _lib.require_gpu(logits)
        lib = _lib.load()
        x = logits.contiguous().float()
        y = labels.to(x.device).contiguous()
        w = None if weight is None else weight.to(x.device).contiguous()
        sums, scratch = _lib.softmax_buffers(x.device)
        out = torch.empty((), dtype=torch.float32, device=x.device)
        if pixel_weights is None:
            pw = None
            _lib.check(lib.unet_softmax_loss_forward(
                x.data_ptr(), y.data_ptr(), _lib.LABEL_DTYPES[y.dtype], n, k, hw, _lib.ptr(w), int(ignore_index),
                kind, float(alpha), float(smooth), sums.data_ptr(), scratch.data_ptr(), scratch.numel(),
                out.data_ptr(), _lib.stream_handle(x.device)), "unet_softmax_loss_forward")
        else:
            pw = pixel_weights.detach().to(x.device).contiguous().float()
            _lib.check(lib.unet_softmax_loss_forward_pw(
                x.data_ptr(), y.data_ptr(), _lib.LABEL_DTYPES[y.dtype], n, k, hw, _lib.ptr(w), pw.data_ptr(),
                int(ignore_index), kind, float(alpha), float(smooth), sums.data_ptr(), scratch.data_ptr(),
                scratch.numel(), out.data_ptr(), _lib.stream_handle(x.device)), "unet_softmax_loss_forward_pw")
        # the tensors of backward in a fixed order: x, y, sums, then the class weights and the pixel weights if any
        ctx.save_for_backward(x, y, sums, *([] if w is None else [w]), *([] if pw is None else [pw]))
        ctx.has = (w is not None, pw is not None)
        ctx.cfg = (n, k, hw, kind, float(alpha), float(smooth), int(ignore_index))
        ctx.in_shape, ctx.in_dtype = logits.shape, logits.dtype
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, y, sums, *rest = ctx.saved_tensors
        w = rest.pop(0) if ctx.has[0] else None
        pw = rest.pop(0) if ctx.has[1] else None
        n, k, hw, kind, alpha, smooth, ignore_index = ctx.cfg
        g = grad_out.contiguous().float()
        dl = torch.empty_like(x)
        if pw is None:
            _lib.check(_lib.load().unet_softmax_loss_backward(
                x.data_ptr(), y.data_ptr(), _lib.LABEL_DTYPES[y.dtype], n, k, hw, _lib.ptr(w),
                ignore_index, kind, alpha, smooth, sums.data_ptr(), g.data_ptr(), dl.data_ptr(),
                _lib.stream_handle(x.device)), "unet_softmax_loss_backward")
        else:
            _lib.check(_lib.load().unet_softmax_loss_backward_pw(
                x.data_ptr(), y.data_ptr(), _lib.LABEL_DTYPES[y.dtype], n, k, hw, _lib.ptr(w), pw.data_ptr(),
                ignore_index, kind, alpha, smooth, sums.data_ptr(), g.data_ptr(), dl.data_ptr(),
                _lib.stream_handle(x.device)), "unet_softmax_loss_backward_pw")
        return dl.view(ctx.in_shape).to(ctx.in_dtype), None, None, None, None, None, None, None


class _SoftmaxModule(nn.Module):
    """Shared state of the softmax losses: class weights live in a buffer (they
    follow ``.to(device)``; one left on the host is moved once, on first use)."""
    kind = BCE

    def __init__(self, alpha, smooth, weight, ignore_index):
        super().__init__()
        self.alpha = alpha
        self.smooth = smooth
        self.ignore_index = int(ignore_index)
        self.register_buffer("weight", _class_weights(weight, None))

    def forward(self, pred, target, pixel_weights=None):
        """``pixel_weights``: a float tensor ``[N,H,W]`` or ``[N,1,H,W]`` (finite, >= 0; moved to
        the logits' device), or ``None``.  A valid pixel then weighs ``weight[y] * pixel_weights[p]``
        in the cross-entropy term (numerator, denominator and gradient); the Dice term is unweighted."""
        if self.weight is not None and isinstance(pred, torch.Tensor) and self.weight.device != pred.device:
            self.weight = self.weight.to(pred.device)
        if pixel_weights is not None and self.kind == DICE:
            raise ValueError("pixel weights apply to the cross-entropy term; SoftmaxDiceLoss takes none")
        return _SoftmaxLoss.apply(pred, target, self.weight, self.kind, self.alpha, self.smooth, self.ignore_index,
                                  pixel_weights)


class CrossEntropyLoss(_SoftmaxModule):
    """``F.cross_entropy(logits, labels, weight, ignore_index, reduction='mean')``
    on ``[N,K,H,W]`` logits and an integer label map ``[N,H,W]`` / ``[N,1,H,W]``
    (uint8, int32 or int64).  With no valid pixel the loss and its gradient are
    0 where torch gives NaN."""
    kind = BCE

    def __init__(self, weight=None, ignore_index=-100):
        super().__init__(1.0, 1.0, weight, ignore_index)


class SoftmaxDiceLoss(_SoftmaxModule):
    """1 - mean_k (2 I_k + smooth) / (P_k + Y_k + smooth) on softmax
    probabilities: one global Dice per class over the valid pixels of the batch
    (the multi-class form of ``DiceLoss``); absent classes count in the mean."""
    kind = DICE

    def __init__(self, smooth=1.0, ignore_index=-100):
        super().__init__(0.0, smooth, None, ignore_index)


class SoftmaxComboLoss(_SoftmaxModule):
    """alpha * CrossEntropyLoss + (1 - alpha) * SoftmaxDiceLoss from one pass."""
    kind = COMBO

    def __init__(self, alpha=0.5, smooth=1.0, weight=None, ignore_index=-100):
        super().__init__(alpha, smooth, weight, ignore_index)


_NOT_ON_PATH = ("weighted_bce", "balanced_bce", "focal", "triple_combo", "tversky", "tversky_balanced",
                "tversky_recall", "focal_tversky", "sensitivity_specificity", "log_cosh_dice",
                "exponential_logarithmic", "distance_map_bce", "hausdorff", "boundary")


def get_loss_function(config):
    """losses.py:345-403: build the criterion named by ``config['loss_fn']``."""
    name = config.get("loss_fn", "combo")
    if name == "dice":
        return DiceLoss(smooth=config.get("smooth", 1.0))
    if name == "bce":
        return BCELoss()
    if name == "combo":
        return ComboLoss(alpha=config.get("loss_alpha", 0.5))
    if name == "ce":
        return CrossEntropyLoss(weight=config.get("class_weights"), ignore_index=config.get("ignore_index", -100))
    if name == "softmax_dice":
        return SoftmaxDiceLoss(smooth=config.get("smooth", 1.0), ignore_index=config.get("ignore_index", -100))
    if name == "softmax_combo":
        return SoftmaxComboLoss(alpha=config.get("loss_alpha", 0.5), smooth=config.get("smooth", 1.0),
                                weight=config.get("class_weights"), ignore_index=config.get("ignore_index", -100))
    if name in _NOT_ON_PATH:
        raise NotImplementedError(f"loss '{name}' is outside the MI355X hot path (SURVEY.md §2 row 2)")
    print(f"Warning: Unknown loss function '{name}', defaulting to ComboLoss")
    return ComboLoss(alpha=config.get("loss_alpha", 0.5))
