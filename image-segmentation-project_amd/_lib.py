"""ctypes binding of libunet_hip.so (the C ABI declared in include/unet_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` (``make -C csrc``).
There is no CPU fallback: if the library or a ROCm GPU is missing, every op
raises ``RuntimeError``.
"""
from __future__ import annotations

import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# UNET_HIP_LIB: an alternative in-tree build for A/B measurements (scripts/)
LIB_PATH = os.environ.get("UNET_HIP_LIB") or os.path.join(_HERE, "libunet_hip.so")
LOSS_SCRATCH_LEN = 8 * 256  # UNET_LOSS_SCRATCH_LEN (include/unet_hip.h): per-block partials of the loss sums
# softmax loss / confusion matrix geometry (UNET_SOFTMAX_* of include/unet_hip.h)
SOFTMAX_MAX_CLASSES = 16
SOFTMAX_SUMS_LEN = 52
SOFTMAX_MAX_BLOCKS = 1024
SOFTMAX_THREADS = 256
SOFTMAX_SCRATCH_LEN = SOFTMAX_SUMS_LEN * SOFTMAX_MAX_BLOCKS
TILE_MAX = 1024  # UNET_TILE_MAX: largest tile of unet_tile_gather / unet_tile_blend
INSTANCE_STATS = 7  # UNET_INSTANCE_STATS: area, sum_y, sum_x, y0, x0, y1, x1
DISTANCE_NONE = 2147483647  # UNET_DISTANCE_NONE: dist2 of a frame without a site
DISTANCE_MAX_DIM = 32768  # UNET_DISTANCE_MAX_DIM: largest H and W of the distance transform
GEODESIC_MAX_HW = 1 << 28  # UNET_GEODESIC_MAX_HW: largest H * W of geodesic growth / watershed (int32 chamfer costs)
TWO_NEAREST_MAX_DIM = 4096  # UNET_TWO_NEAREST_MAX_DIM: largest H and W of the two-nearest transform / border weights
MATCH_COLS = 4  # UNET_MATCH_COLS: area, partner, intersection, partner_area
MATCH_STATUS = 5  # UNET_MATCH_STATUS: n_gt, n_pred, n_pairs, dropped, out_of_range
MEASURE_COLS = 13  # UNET_MEASURE_COLS: area, sums, box, second-order sums, edges, frame_edges, contact_edges
MEASURE_STATUS = 3  # UNET_MEASURE_STATUS: n_present, max_id, out_of_range
MEASURE_ICOLS = 4  # UNET_MEASURE_ICOLS: sum, sum_sq, min, max
LINK_COLS = 4  # UNET_LINK_COLS: first, last, parent, volume
LINK_STATUS = 4  # UNET_LINK_STATUS: n_tracks, n_links, dropped, out_of_range
LINK_BLOCK = 1024  # UNET_LINK_BLOCK: ids per chunk of the resolve pass
LINK_LDS_IDS = 8191  # UNET_LINK_LDS_IDS: largest max_instances whose LUT row the relabel pass keeps in LDS

_lib = None

c_int, c_int64, c_float, c_double, c_void_p, c_char_p = (
    ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_void_p, ctypes.c_char_p)


class UnetConfig(ctypes.Structure):
    _fields_ = [("N", c_int), ("H", c_int), ("W", c_int), ("width", c_int), ("n_classes", c_int),
                ("bn_eps", c_float), ("bn_momentum", c_float), ("attention", c_int), ("backbone", c_int),
                ("fp8", c_int)]


class ConvExArgs(ctypes.Structure):
    """unet_conv_ex_args (include/unet_hip.h): one conv launch with the whole
    epilogue; zero / null fields are off.  size is filled in here."""
    _fields_ = ([(n, c_int) for n in (
        "size", "mode", "chunk_major", "grid_cap", "N", "H", "W", "C", "P", "Q", "Cout", "R", "S", "stride", "pad",
        "ldx", "ldy", "ldadd", "ldact", "ldyraw", "ldyraw2", "ldx2", "C2", "ldysplit", "csplit", "ldyds", "relu")]
                + [("eps", c_float)]
                + [(n, c_void_p) for n in (
                    "x", "w", "y", "bias", "addend", "stats", "act", "yraw", "mean", "invstd", "yraw2", "mean2",
                    "invstd2", "bsums", "bsums2", "x2", "w2", "ysplit", "gamma", "beta", "running_mean",
                    "running_var", "wds", "yds", "stats_ds")])

    def __init__(self, **kw):
        super().__init__(**kw)
        self.size = ctypes.sizeof(ConvExArgs)


class AttGateOpArgs(ctypes.Structure):
    """unet_att_gate_args (include/unet_hip.h): one pass of the attention gate
    as a single op.  size is filled in here."""
    _fields_ = ([(n, c_int) for n in (
        "size", "pass_", "training", "Fi", "Fl", "lds", "ldx", "ldxatt", "lddxatt", "lddxpsi", "lddS", "ldyraw",
        "ldyraw2")]
                + [("eps", c_float), ("momentum", c_float), ("npix", c_int64)]
                + [(n, c_void_p) for n in (
                    "s", "psi_w", "psi_b", "p", "psi", "dbnp", "pst", "pbs", "save", "gamma", "beta", "run_mean",
                    "run_var", "nbt", "x", "xatt", "dxatt", "dxpsi", "dS", "gpsi_w", "ggamma", "gbeta", "gpsi_acc",
                    "yraw", "yraw2", "mean", "invstd", "mean2", "invstd2", "bsums", "bsums2")])

    def __init__(self, **kw):
        super().__init__(**kw)
        self.size = ctypes.sizeof(AttGateOpArgs)


class ChAttOpArgs(ctypes.Structure):
    """unet_ch_att_args (include/unet_hip.h): one pass of the channel attention
    as a single op.  size is filled in here."""
    _fields_ = ([(n, c_int) for n in (
        "size", "pass_", "N", "C", "Cr", "ldy", "ldo", "lddo2", "lddo", "ldact", "ldyraw")]
                + [("HW", c_int64)]
                + [(n, c_void_p) for n in (
                    "y", "out", "psum", "pkey", "w1", "w2", "am", "h", "gate", "dout2", "dgate", "dam", "gw1", "gw2",
                    "gw_acc", "dout", "act", "yraw", "mean", "invstd", "bsums")])

    def __init__(self, **kw):
        super().__init__(**kw)
        self.size = ctypes.sizeof(ChAttOpArgs)


# name -> (restype, argtypes); every exported symbol of include/unet_hip.h
SIGNATURES = {
    "unet_last_error": (c_char_p, []),
    "unet_version": (c_char_p, []),
    "unet_plan_create": (c_int, [ctypes.POINTER(UnetConfig), ctypes.POINTER(c_void_p)]),
    "unet_plan_destroy": (None, [c_void_p]),
    "unet_plan_workspace_bytes": (c_int64, [c_void_p]),
    "unet_plan_num_params": (c_int, [c_void_p]),
    "unet_plan_param_name": (c_int, [c_void_p, c_int, ctypes.c_char_p, c_int]),
    "unet_plan_param_shape": (c_int, [c_void_p, c_int, ctypes.POINTER(c_int64)]),
    "unet_plan_param_offset": (c_int64, [c_void_p, c_int]),
    "unet_plan_grad_numel": (c_int64, [c_void_p]),
    "unet_plan_num_bn": (c_int, [c_void_p]),
    "unet_plan_num_buckets": (c_int, [c_void_p]),
    "unet_plan_bucket_range": (c_int, [c_void_p, c_int, ctypes.POINTER(c_int64), ctypes.POINTER(c_int64)]),
    "unet_plan_flops": (c_double, [c_void_p, c_int]),
    "unet_plan_num_tensors": (c_int, [c_void_p]),
    "unet_plan_tensor_info": (c_int, [c_void_p, c_int, ctypes.c_char_p, c_int, ctypes.POINTER(c_int64)]),
    "unet_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "unet_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "unet_bucket_wait": (c_int, [c_void_p, c_int, c_void_p]),
    "unet_plan_use_bucket_events": (c_int, [c_void_p, c_int]),
    "unet_profile_enable": (c_int, [c_void_p, c_int]),
    "unet_timing_enable": (c_int, [c_void_p, c_int]),
    "unet_timing_read": (c_int64, [c_void_p, c_void_p, c_int64, ctypes.c_char_p, c_int64]),
    "unet_profile_report": (c_int, [c_void_p, ctypes.c_char_p, c_int64]),
    "unet_loss_forward": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_float, c_float, c_void_p, c_void_p,
                                  c_int64, c_void_p, c_void_p]),
    "unet_loss_backward": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_float, c_float, c_void_p, c_void_p,
                                   c_void_p, c_void_p]),
    "unet_mask_metrics": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_int64, c_void_p]),
    "unet_softmax_loss_forward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_int, c_int,
                                          c_float, c_float, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "unet_softmax_loss_backward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_int, c_int,
                                           c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "unet_softmax_loss_forward_pw": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_void_p,
                                             c_int, c_int, c_float, c_float, c_void_p, c_void_p, c_int64, c_void_p,
                                             c_void_p]),
    "unet_softmax_loss_backward_pw": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_void_p,
                                              c_int, c_int, c_float, c_float, c_void_p, c_void_p, c_void_p,
                                              c_void_p]),
    "unet_confusion_matrix": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int64, c_int, c_void_p, c_void_p,
                                      c_int64, c_void_p]),
    "unet_adam_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float,
                               c_float, c_float, c_int, c_void_p]),
    "unet_allreduce_unique_id": (c_int, [c_void_p]),
    "unet_allreduce_init": (c_int, [c_void_p, c_int, c_int, ctypes.POINTER(c_void_p)]),
    "unet_allreduce_destroy": (None, [c_void_p]),
    "unet_allreduce_bucket": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "unet_allreduce_mean": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "unet_grad_to_bf16": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "unet_grad_from_bf16": (c_int, [c_void_p, c_void_p, c_int64, c_float, c_void_p]),
    "unet_conv_fwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p]
                      + [c_int] * 12 + [c_void_p]),
    "unet_conv_ex": (c_int, [ctypes.POINTER(ConvExArgs), c_void_p]),
    "unet_last_kernel_tag": (c_char_p, []),
    "unet_att_gate_op": (c_int, [ctypes.POINTER(AttGateOpArgs), c_void_p]),
    "unet_ch_att_op": (c_int, [ctypes.POINTER(ChAttOpArgs), c_void_p]),
    "unet_conv_wgrad": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p] + [c_int] * 12 + [c_void_p]),
    "unet_conv3x3_fl": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p,
                                c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                c_void_p, c_void_p, c_void_p] + [c_int] * 7 + [c_void_p]),
    "unet_convt2x2": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int,
                              c_void_p, c_void_p, c_void_p, c_void_p] + [c_int] * 7 + [c_void_p]),
    "unet_f8_quantize": (c_int, [c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p, c_int, c_void_p]),
    "unet_f8_pack_weight": (c_int, [c_void_p] + [c_int] * 4 + [c_void_p, c_void_p, c_int, c_void_p]),
    "unet_f8_roll": (c_int, [c_void_p, c_int, c_void_p]),
    "unet_conv_fwd_f8": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                 c_int, c_void_p] + [c_int] * 11 + [c_void_p]),
    "unet_conv_wgrad_slab": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int64]
                             + [c_int] * 12 + [c_void_p]),
    "unet_convt_wgrad_slab": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int64]
                              + [c_int] * 5 + [c_void_p]),
    "unet_set_conv_config": (c_int, [c_int]),
    "unet_pack_weight": (c_int, [c_void_p, c_void_p] + [c_int] * 5 + [c_void_p]),
    "unet_unpack_grad": (c_int, [c_void_p, c_void_p] + [c_int] * 5 + [c_void_p]),
    "unet_bn_forward": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p]),
    "unet_bn_backward": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "unet_warp_affine_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                    c_void_p]),
    "unet_filter2d_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "unet_resize_area_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
    "unet_mask_prep": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
    "unet_normalize_microscopy": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "unet_rot90_vflip_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "unet_tile_grid": (c_int, [c_int] * 4 + [ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "unet_tile_gather": (c_int, [c_void_p] + [c_int] * 5 + [ctypes.c_uint, c_int64, c_int64, c_void_p, c_void_p]),
    "unet_tile_blend": (c_int, [c_void_p] + [c_int] * 6 + [ctypes.c_uint, c_void_p, c_void_p, c_void_p, c_void_p]),
    "unet_instances_workspace_bytes": (c_int64, [c_int] * 3),
    "unet_label_instances": (c_int, [c_void_p] + [c_int] * 8 + [c_void_p] * 5 + [c_int64, c_void_p]),
    "unet_distance_workspace_bytes": (c_int64, [c_int] * 3),
    "unet_distance_transform": (c_int, [c_void_p] + [c_int] * 6 + [c_void_p] * 3 + [c_int64, c_void_p]),
    "unet_grow_instances": (c_int, [c_void_p] + [c_int] * 3 + [c_int64, c_void_p, c_int, c_void_p, c_void_p, c_int64,
                                                                c_void_p]),
    "unet_geodesic_workspace_bytes": (c_int64, [c_int] * 3),
    "unet_geodesic_grow": (c_int, [c_void_p] + [c_int] * 4 + [c_int64, c_void_p, c_int] + [c_void_p] * 3
                           + [c_int64, c_void_p]),
    "unet_watershed": (c_int, [c_void_p] * 2 + [c_int] * 4 + [c_void_p, c_int] + [c_void_p] * 2 + [c_int64, c_void_p]),
    "unet_geodesic_last_counts": (c_int, [c_void_p] * 3),
    "unet_two_nearest_workspace_bytes": (c_int64, [c_int] * 3),
    "unet_two_nearest_instances": (c_int, [c_void_p] + [c_int] * 3 + [c_int64] + [c_void_p] * 3 + [c_int64, c_void_p]),
    "unet_border_weights": (c_int, [c_void_p] + [c_int] * 3 + [c_float, c_float, c_int64, c_void_p, c_void_p, c_int,
                                                                c_void_p, c_void_p, c_int64, c_void_p]),
    "unet_boundary_targets": (c_int, [c_void_p] + [c_int] * 4 + [c_void_p, c_void_p]),
    "unet_match_workspace_bytes": (c_int64, [c_int] * 4),
    "unet_match_instances": (c_int, [c_void_p, c_void_p] + [c_int] * 6 + [c_void_p] * 5 + [c_int64, c_void_p]),
    "unet_measure_workspace_bytes": (c_int64, [c_int] * 5),
    "unet_measure_instances": (c_int, [c_void_p, c_void_p] + [c_int] * 6 + [c_void_p] * 4 + [c_int64, c_void_p]),
    "unet_select_instances": (c_int, [c_void_p, c_void_p] + [c_int] * 4 + [c_void_p] * 4),
    "unet_link_workspace_bytes": (c_int64, [c_int] * 4),
    "unet_link_instances": (c_int, [c_void_p] + [c_int] * 9 + [c_void_p] * 4 + [c_int64, c_void_p]),
    "unet_maxpool_fwd": (c_int,[c_void_p, c_int, c_void_p, c_void_p] + [c_int] * 4 + [c_void_p]),
    "unet_maxpool_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p] + [c_int] * 4 + [c_void_p]),
}


def load(path: str = LIB_PATH):
    """Load (once) and type the shared library.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RuntimeError(
            f"libunet_hip.so not found at {path}: build it with `python -c 'import __graft_entry__ as g; "
            f"g.build()'` (make -C image-segmentation-project_amd/csrc). There is no CPU fallback.")
    lib = ctypes.CDLL(path)
    alt = path != os.path.join(_HERE, "libunet_hip.so")
    for name, (res, args) in SIGNATURES.items():
        if alt and not hasattr(lib, name):
            continue  # an older A/B build (UNET_HIP_LIB) without this entry point
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().unet_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def require_gpu(*tensors):
    """The product path has no CPU fallback: fail loudly."""
    if not torch.cuda.is_available():
        raise RuntimeError("libunet_hip needs a ROCm GPU (MI355X / gfx950); no CPU fallback exists")
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("libunet_hip ops take device tensors; call .to('cuda') first")


def stream_handle(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def loss_buffers(device):
    """(sums [8], scratch [LOSS_SCRATCH_LEN]) fp64 device buffers of one
    unet_loss_forward / unet_mask_metrics call (one allocation)."""
    buf = torch.empty(8 + LOSS_SCRATCH_LEN, dtype=torch.float64, device=device)
    return buf[:8], buf[8:]


def softmax_buffers(device):
    """(sums [SOFTMAX_SUMS_LEN], scratch [SOFTMAX_SCRATCH_LEN]) fp64 device buffers
    of one unet_softmax_loss_forward / unet_confusion_matrix call (one allocation)."""
    buf = torch.empty(SOFTMAX_SUMS_LEN + SOFTMAX_SCRATCH_LEN, dtype=torch.float64, device=device)
    return buf[:SOFTMAX_SUMS_LEN], buf[SOFTMAX_SUMS_LEN:]


# label dtypes the softmax kernels read as they are -> label_dtype of the C ABI
LABEL_DTYPES = {torch.uint8: 0, torch.int32: 1, torch.int64: 2}


def ptr(t) -> int:
    return 0 if t is None else t.data_ptr()
