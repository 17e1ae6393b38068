"""What the label-map ops (``instances``, ``distance``, ``match``) share: validation
of an array or tensor of frames, its ``[M, H, W]`` device view and the workspace of
one call."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

_NUMPY = {torch.uint8: np.uint8, torch.bool: np.bool_, torch.int32: np.int32}


def as_frames(x, what, dtypes, max_dim=None):
    """Validate an array or tensor of frames (``[H, W]``, ``[N, H, W]`` or ``[N, K, H, W]``,
    not empty, ``H * W`` below 2^31, ``H`` and ``W`` at most ``max_dim`` when given) and
    return it as a tensor; raises ValueError, touches no GPU."""
    names = " / ".join(str(d).replace("torch.", "") for d in dtypes)
    if isinstance(x, np.ndarray):
        if x.dtype not in [_NUMPY[d] for d in dtypes]:
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
    if max_dim is not None and (H > max_dim or W > max_dim or H * W >= 1 << 31):
        raise ValueError(f"{what}: H = {H}, W = {W} must be <= {max_dim} with H * W below 2^31")
    if H * W >= 1 << 31:
        raise ValueError(f"{what}: H * W = {H * W} must be below 2^31")
    return x


def frames_on_gpu(x):
    """[M, H, W] contiguous device view or copy of a validated tensor (bool viewed as uint8)"""
    if not x.is_cuda:
        _lib.require_gpu()
        x = x.cuda()
    _lib.require_gpu(x)
    if x.dtype == torch.bool:
        x = x.view(torch.uint8)
    return x.reshape(-1, x.shape[-2], x.shape[-1]).contiguous()


def workspace(lib, sizer_name, dev, *dims):
    """(uint8 tensor, nbytes) of the size ``lib.<sizer_name>(*dims)`` asks for"""
    nbytes = int(getattr(lib, sizer_name)(*dims))
    if nbytes <= 0:
        _lib.check(1, sizer_name)
    return torch.empty((nbytes,), dtype=torch.uint8, device=dev), nbytes
