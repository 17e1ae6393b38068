"""``unet_label_instances`` as a single op through the C ABI and ``label_instances``
on top of it, against scipy.ndimage (tests/instances_ref.py).  Every comparison is
exact integer equality.

The 520 x 515 serpentine (one component whose chain crosses every tile many times)
takes 77 microseconds per ``label_instances`` call on an MI355X (profiles/instances.md).
"""
import functools
import importlib
import os
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import instances_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

CAP = 4096  # the default max_instances


def _lib():
    mod = importlib.import_module("image-segmentation-project_amd._lib")
    return mod, mod.load()


@functools.lru_cache(maxsize=None)
def _pattern(name):
    m = ref.PATTERNS[name]()
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _expected(name, connectivity, min_area=0, fill_holes=False):
    lab, n, fm = ref.label(_pattern(name), connectivity, min_area, fill_holes)
    st = ref.stats(lab, n, CAP)
    for a in (lab, st, fm):
        a.setflags(write=False)
    return lab, n, st, fm


def _abi(mask, connectivity=1, min_area=0, fill_holes=False, fg=-1, cap=CAP, want_filled=False):
    """one C ABI call on frames [N][H][W]; the workspace and every output start as 0xFF bytes"""
    _, lib = _lib()
    m = torch.from_numpy(np.array(mask)).cuda()  # a writable, contiguous copy
    N, H, W = m.shape
    nbytes = lib.unet_instances_workspace_bytes(N, H, W)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    labels = torch.full((N, H, W), -1, dtype=torch.int32, device="cuda")
    counts = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    stats = torch.full((N, cap, 7), -1, dtype=torch.int64, device="cuda")
    filled = torch.full((N, H, W), 0xFF, dtype=torch.uint8, device="cuda") if want_filled else None
    rc = lib.unet_label_instances(m.data_ptr(), N, H, W, fg, connectivity, int(fill_holes), min_area, cap,
                                  labels.data_ptr(), counts.data_ptr(), stats.data_ptr(),
                                  0 if filled is None else filled.data_ptr(), ws.data_ptr(), nbytes,
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.unet_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(m.cpu().numpy(), mask)  # the input is untouched
    return (labels.cpu().numpy(), counts.cpu().numpy(), stats.cpu().numpy(),
            None if filled is None else filled.cpu().numpy())


def _same(got_labels, got_count, got_stats, lab, n, st):
    assert int(got_count) == n
    assert got_labels.dtype == np.int32 and np.array_equal(got_labels, lab)
    assert np.array_equal(got_stats, st)


@pytest.mark.parametrize("connectivity", [1, 2])
@pytest.mark.parametrize("name", list(ref.PATTERNS))
def test_abi_single_op(name, connectivity):
    lab, n, st, _ = _expected(name, connectivity)
    labels, counts, stats, _ = _abi(_pattern(name)[None], connectivity)
    _same(labels[0], counts[0], stats[0], lab, n, st)
    if name == "checkerboard":
        assert n == (8515 if connectivity == 1 else 1)
    if n > CAP:  # truncation: the count and the label map are complete, the table holds ids <= CAP
        assert labels.max() == n and np.all(stats[0, :CAP, 0] > 0)


@pytest.mark.parametrize("connectivity", [1, 2])
@pytest.mark.parametrize("name", list(ref.PATTERNS))
def test_label_instances(pkg, cuda, name, connectivity):
    lab, n, st, _ = _expected(name, connectivity)
    labels, counts, stats = pkg.label_instances(torch.from_numpy(np.array(_pattern(name))).to(cuda),
                                                connectivity=connectivity, return_stats=True)
    assert labels.dtype == torch.int32 and counts.dtype == torch.int32 and stats.dtype == torch.int64
    assert labels.shape == lab.shape and counts.shape == () and stats.shape == (CAP, 7)
    _same(labels.cpu().numpy(), counts.item(), stats.cpu().numpy(), lab, n, st)
    two = pkg.label_instances(np.array(_pattern(name)), connectivity=connectivity)  # a host array is moved to the GPU
    assert len(two) == 2 and np.array_equal(two[0].cpu().numpy(), lab) and int(two[1]) == n


@pytest.mark.parametrize("connectivity", [1, 2])
@pytest.mark.parametrize("shape", [(1, 1), (1, 200), (200, 1), (63, 65), (64, 64), (32, 64), (33, 128)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_shapes(shape, connectivity):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    for m in (np.ones(shape, np.uint8), (rng.random(shape) < 0.55).astype(np.uint8)):
        lab, n, _ = ref.label(m, connectivity)
        labels, counts, stats, _ = _abi(m[None], connectivity, cap=64)
        _same(labels[0], counts[0], stats[0], lab, n, ref.stats(lab, n, 64))


@pytest.mark.parametrize("connectivity", [1, 2])
def test_frames_are_isolated(pkg, cuda, connectivity):
    frames = np.stack([ref.random_mask(0.55, seed=5), ref.comb(), ref.random_mask(0.35, seed=6)])
    frames[:, 0, :] = 1   # last row of frame n and first row of frame n + 1 are foreground:
    frames[:, -1, :] = 1  # flat-index neighbours across the frame boundary must not join
    labels, counts, stats = pkg.label_instances(torch.from_numpy(frames).to(cuda), connectivity=connectivity,
                                                return_stats=True, max_instances=512)
    assert counts.shape == (3,) and stats.shape == (3, 512, 7)
    for i in range(3):
        lab, n, _ = ref.label(frames[i], connectivity)
        _same(labels[i].cpu().numpy(), counts[i].item(), stats[i].cpu().numpy(), lab, n, ref.stats(lab, n, 512))
        assert lab[0, 0] == 1  # labels restart at 1 in every frame


def test_long_chain_serpentine():
    m = ref.serpentine(520, 515)
    lab, n, _ = ref.label(m, 1)
    assert n == 1
    labels, counts, stats, _ = _abi(m[None], 1, cap=4)
    _same(labels[0], counts[0], stats[0], lab, n, ref.stats(lab, n, 4))


@pytest.mark.parametrize("connectivity", [1, 2])
def test_min_area(connectivity):
    lab, n, st, _ = _expected("random55", connectivity, 5)
    assert 0 < n < _expected("random55", connectivity)[1]
    labels, counts, stats, _ = _abi(_pattern("random55")[None], connectivity, min_area=5)
    _same(labels[0], counts[0], stats[0], lab, n, st)
    assert stats[0, :n, 0].min() >= 5
    labels, counts, stats, _ = _abi(_pattern("random55")[None], connectivity, min_area=130 * 131 + 1)
    assert counts[0] == 0 and not labels.any() and not stats.any()


@pytest.mark.parametrize("connectivity", [1, 2])
@pytest.mark.parametrize("name", ["rings", "random62"])
def test_fill_holes(name, connectivity):
    m = ref.rings() if name == "rings" else _pattern(name)
    lab, n, fm = ref.label(m, connectivity, fill_holes=True)
    assert fm.sum() > (m != 0).sum()  # the pattern has holes
    labels, counts, stats, filled = _abi(m[None], connectivity, fill_holes=True, want_filled=True)
    assert np.array_equal(filled[0], fm.astype(np.uint8))
    _same(labels[0], counts[0], stats[0], lab, n, ref.stats(lab, n, CAP))
    if name == "rings":
        assert filled[0, 80, 30] == 1 and filled[0, 5, 100] == 0 and filled[0, 66, 128] == 0
    # without the optional output, and together with min_area (fill, then label, then min_area)
    lab5, n5, _ = ref.label(m, connectivity, min_area=5, fill_holes=True)
    labels, counts, stats, _ = _abi(m[None], connectivity, fill_holes=True, min_area=5)
    _same(labels[0], counts[0], stats[0], lab5, n5, ref.stats(lab5, n5, CAP))


def test_foreground_value(pkg, cuda):
    cls = np.random.default_rng(11).integers(0, 4, (2, 70, 90)).astype(np.uint8)
    labels, counts, stats, filled = pkg.label_instances(torch.from_numpy(cls).to(cuda), foreground=2, connectivity=2,
                                                        fill_holes=True, return_stats=True, return_filled=True,
                                                        max_instances=256)
    for i in range(2):
        lab, n, fm = ref.label(cls[i] == 2, 2, fill_holes=True)
        _same(labels[i].cpu().numpy(), counts[i].item(), stats[i].cpu().numpy(), lab, n, ref.stats(lab, n, 256))
        assert np.array_equal(filled[i].cpu().numpy(), fm.astype(np.uint8))
    labels, counts = pkg.label_instances(cls, foreground=0)
    for i in range(2):
        lab, n, _ = ref.label(cls[i] == 0, 1)
        assert np.array_equal(labels[i].cpu().numpy(), lab) and counts[i].item() == n


def test_instance_properties(pkg, cuda):
    m = _pattern("random55")
    lab, n, st, _ = _expected("random55", 1)
    _, counts, stats = pkg.label_instances(torch.from_numpy(np.array(m)).to(cuda), return_stats=True)
    props = pkg.instance_properties(stats, counts)
    assert np.array_equal(props["area"], st[:n, 0]) and np.array_equal(props["bbox"], st[:n, 3:])
    com = np.array(ndimage.center_of_mass(np.ones_like(lab), lab, np.arange(1, n + 1)))
    assert np.allclose(props["centroid"], com, rtol=0, atol=1e-9)
    assert stats[n:].count_nonzero().item() == 0


def test_input_handling(pkg, cuda):
    rng = np.random.default_rng(12)
    base = (rng.random((2, 3, 70, 2 * 45)) < 0.5)
    # bool, [N, K, H, W], non-contiguous (every second column)
    t = torch.from_numpy(base).to(cuda)
    view = t[..., ::2]
    assert not view.is_contiguous()
    before = t.clone()
    labels, counts, stats = pkg.label_instances(view, connectivity=2, return_stats=True, max_instances=128)
    again = pkg.label_instances(view, connectivity=2, return_stats=True, max_instances=128)
    assert torch.equal(t, before)
    assert labels.shape == (2, 3, 70, 45) and counts.shape == (2, 3) and stats.shape == (2, 3, 128, 7)
    assert all(torch.equal(a, b) for a, b in zip((labels, counts, stats), again))
    for i in range(2):
        for k in range(3):
            lab, n, _ = ref.label(base[i, k, :, ::2], 2)
            _same(labels[i, k].cpu().numpy(), counts[i, k].item(), stats[i, k].cpu().numpy(), lab, n,
                  ref.stats(lab, n, 128))
    # [H, W] uint8 with values other than 0 / 1
    m2 = (base[0, 0] * 200).astype(np.uint8)
    labels, counts = pkg.label_instances(torch.from_numpy(m2).to(cuda))
    lab, n, _ = ref.label(m2, 1)
    assert labels.shape == m2.shape and counts.shape == () and counts.item() == n
    assert np.array_equal(labels.cpu().numpy(), lab)


def test_short_workspace_is_an_error():
    _, lib = _lib()
    m = torch.zeros((1, 40, 40), dtype=torch.uint8, device="cuda")
    labels = torch.full((1, 40, 40), -7, dtype=torch.int32, device="cuda")
    counts = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    nbytes = lib.unet_instances_workspace_bytes(1, 40, 40)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    rc = lib.unet_label_instances(m.data_ptr(), 1, 40, 40, -1, 1, 0, 0, 16, labels.data_ptr(), counts.data_ptr(), 0, 0,
                                  ws.data_ptr(), nbytes - 1, st)
    assert rc != 0 and b"workspace" in lib.unet_last_error()
    rc = lib.unet_label_instances(m.data_ptr(), 1, 40, 40, -1, 3, 0, 0, 16, labels.data_ptr(), counts.data_ptr(), 0, 0,
                                  ws.data_ptr(), nbytes, st)
    assert rc != 0 and b"connectivity" in lib.unet_last_error()
    torch.cuda.synchronize()
    assert (labels == -7).all() and counts.item() == -7  # nothing was launched


def test_predict_then_label(pkg, cuda):
    torch.manual_seed(0)
    model = pkg.UNetWithBackbone(pretrained=False, use_attention=False).to(cuda)
    frame = torch.randn(1, 1, 96, 80, device=cuda)
    mask = pkg.predict(model, frame, tile=64, overlap=16, output="mask")
    assert mask.dtype == torch.uint8 and mask.shape == (1, 1, 96, 80)
    labels, counts, stats = pkg.label_instances(mask, return_stats=True, max_instances=1024)
    lab, n, _ = ref.label(mask[0, 0].cpu().numpy(), 1)
    _same(labels[0, 0].cpu().numpy(), counts[0, 0].item(), stats[0, 0].cpu().numpy(), lab, n,
          ref.stats(lab, n, 1024))
