"""Instance matching without a GPU: the argument checks of ``match_instances`` (which
run before anything touches the GPU), the refusal to fall back to the CPU, the C ABI
table and workspace size, ``instance_metrics`` on the host tables of
tests/match_ref.py against that reference's metrics, and the reference's own claims."""
import importlib
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_ref as ref  # noqa: E402

INT_KEYS = ("tp", "fp", "fn")
FLOAT_KEYS = ("precision", "recall", "f1", "ap", "mean_ap", "pq", "sq", "rq", "aji")
# both sides sum at most 4096 terms of [0, 1] in float64: 4096 * 2^-53 = 4.5e-13
FLOAT_TOL = 1e-12


def _lib():
    return importlib.import_module("image-segmentation-project_amd._lib")


GOOD = np.zeros((8, 9), np.int32)

BAD_LABELS = [
    (np.zeros((8, 9), np.uint8), "u8-array"), (np.zeros((8, 9), np.int64), "i64-array"),
    (np.zeros((8, 9), np.float32), "f32-array"), (torch.zeros((8, 9), dtype=torch.int64), "i64-tensor"),
    (torch.zeros((8, 9), dtype=torch.bool), "bool-tensor"), (np.zeros((9,), np.int32), "rank1"),
    (np.zeros((1, 1, 1, 8, 9), np.int32), "rank5"), (np.zeros((0, 8, 9), np.int32), "empty-n"),
    (torch.zeros((2, 0, 9), dtype=torch.int32), "empty-h"), ([[0, 1], [1, 0]], "list"),
    (torch.zeros((1, 1), dtype=torch.int32).expand(1 << 16, 1 << 15), "HW>=2^31"),  # no storage behind it
]


@pytest.mark.parametrize("labels", [m for m, _ in BAD_LABELS], ids=[i for _, i in BAD_LABELS])
def test_bad_labels_raise_value_error(pkg, labels):
    with pytest.raises(ValueError):
        pkg.match_instances(labels, labels)
    with pytest.raises(ValueError):
        pkg.match_instances(GOOD, labels)
    with pytest.raises(ValueError):
        pkg.match_instances(labels, GOOD)


@pytest.mark.parametrize("kw", [
    dict(max_instances=0), dict(max_instances=65536), dict(max_instances=-1), dict(max_instances=True),
    dict(max_pairs=0), dict(max_pairs=(1 << 24) + 1), dict(max_pairs=-5),
], ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_bad_caps_raise_value_error(pkg, kw):
    with pytest.raises(ValueError):
        pkg.match_instances(GOOD, GOOD, **kw)


def test_shape_mismatch_raises_value_error(pkg):
    for other in (np.zeros((8, 8), np.int32), np.zeros((1, 8, 9), np.int32), np.zeros((9, 8), np.int32)):
        with pytest.raises(ValueError):
            pkg.match_instances(GOOD, other)


def test_no_cpu_fallback(pkg):
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the refusal cannot be shown")
    with pytest.raises(RuntimeError):
        pkg.match_instances(GOOD, GOOD)
    with pytest.raises(RuntimeError):
        pkg.match_instances(torch.zeros((2, 8, 9), dtype=torch.int32), torch.zeros((2, 8, 9), dtype=torch.int32),
                            max_instances=16, return_pairs=True)


def test_signatures_and_exports(pkg):
    mod = _lib()
    res, args = mod.SIGNATURES["unet_match_instances"]
    assert res is mod.c_int and len(args) == 15 and args[-2] is mod.c_int64 and args[2:8] == [mod.c_int] * 6
    assert mod.SIGNATURES["unet_match_workspace_bytes"] == (mod.c_int64, [mod.c_int] * 4)
    assert mod.MATCH_COLS == ref.COLS == 4 and mod.MATCH_STATUS == ref.STATUS == 5
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                            "unet_hip.h")).read()
    assert "#define UNET_MATCH_COLS 4" in hdr and "#define UNET_MATCH_STATUS 5" in hdr
    lib = mod.load()
    for name in ("unet_match_workspace_bytes", "unet_match_instances"):
        assert hasattr(lib, name)
    assert callable(pkg.match_instances) and callable(pkg.instance_metrics)
    assert pkg.InstanceMatch._fields == ("gt_table", "pred_table", "status")
    alias = importlib.import_module("image_segmentation_project_amd")
    assert alias.match_instances is pkg.match_instances and alias.instance_metrics is pkg.instance_metrics
    utils = importlib.import_module("image-segmentation-project_amd.utils")
    assert utils.EPS == ref.EPS


def test_workspace_bytes_positive_and_growing(pkg):
    lib = _lib().load()
    base = (1, 512, 512, 4096)
    b0 = lib.unet_match_workspace_bytes(*base)
    assert b0 > 0
    # the pair table: 8 bytes per slot, slots = the smallest power of two >= 2 max_pairs
    assert b0 >= 8 * 8192
    for k, bigger in enumerate((3, 4096, 4096, 4097)):
        args = list(base)
        args[k] = bigger
        assert lib.unet_match_workspace_bytes(*args) > b0, k
    assert lib.unet_match_workspace_bytes(1, 512, 512, 4097) >= 8 * 16384
    assert lib.unet_match_workspace_bytes(1, 1, 1, 1) > 0
    assert lib.unet_match_workspace_bytes(2, 65535, 65535, 1 << 24) > 2 * 8 * (1 << 25)
    for bad in ((0, 8, 8, 8), (-1, 8, 8, 8), (1, 0, 8, 8), (1, 65536, 8, 8), (1, 8, 0, 8), (1, 8, 65536, 8),
                (1, 8, 8, 0), (1, 8, 8, (1 << 24) + 1)):
        assert lib.unet_match_workspace_bytes(*bad) == 0
        assert b"unet_match_workspace_bytes" in lib.unet_last_error()


def test_abi_rejects_bad_arguments_before_any_launch(pkg):
    """null buffers stand in for device memory: every call must fail before it touches them"""
    lib = _lib().load()
    need = lib.unet_match_workspace_bytes(1, 16, 16, 64)
    P = 0x1000  # never dereferenced
    names = ("gt", "pred", "N", "H", "W", "max_gt", "max_pred", "max_pairs", "gt_table", "pred_table", "status",
             "pairs", "ws", "bytes", "stream")
    good = dict(gt=P, pred=P, N=1, H=8, W=9, max_gt=16, max_pred=16, max_pairs=64, gt_table=P, pred_table=P,
                status=P, pairs=None, ws=P, bytes=need, stream=None)
    call = lambda **k: lib.unet_match_instances(*[{**good, **k}[n] for n in names])  # noqa: E731
    for kw, word in ((dict(gt=None), b"null"), (dict(pred=None), b"null"), (dict(gt_table=None), b"null"),
                     (dict(pred_table=None), b"null"), (dict(status=None), b"null"), (dict(N=0), b"positive"),
                     (dict(H=0), b"positive"), (dict(W=-3), b"positive"), (dict(H=1 << 16, W=1 << 15), b"2^31"),
                     (dict(max_gt=0), b"max_gt"), (dict(max_gt=65536), b"max_gt"), (dict(max_pred=0), b"max_pred"),
                     (dict(max_pred=65536), b"max_pred"), (dict(max_pairs=0), b"max_pairs"),
                     (dict(max_pairs=(1 << 24) + 1), b"max_pairs"), (dict(ws=None), b"workspace"),
                     (dict(bytes=need - 1), b"workspace")):
        assert call(**kw) != 0, kw
        err = lib.unet_last_error()
        assert b"unet_match_instances" in err and word in err, (kw, err)


# ---- instance_metrics on host tables ------------------------------------------------

def _match_of(names):
    tabs = [ref.expected(n) for n in names]
    return tabs, tuple(np.stack([t[k] for t in tabs]) for k in ("gt_table", "pred_table", "status"))


def _same_metrics(got, want, lead):
    for k in INT_KEYS:
        assert got[k].dtype == np.int64 and got[k].shape == lead + (10,)
        assert np.array_equal(got[k], want[k]), k
        assert np.array_equal(got["pooled"][k], want["pooled"][k]), k
    for k in FLOAT_KEYS:
        assert got[k].dtype == np.float64 and got[k].shape == want[k].shape, k
        assert np.all(np.abs(got[k] - want[k]) <= FLOAT_TOL), (k, got[k], want[k])
        assert np.all(np.abs(got["pooled"][k] - want["pooled"][k]) <= FLOAT_TOL), k
        assert np.all(np.isfinite(got[k]))


def test_instance_metrics_equals_the_reference(pkg):
    names = list(ref.PATTERNS)
    tabs, match = _match_of(names)
    got = pkg.instance_metrics(match)
    want = ref.metrics(tabs)
    tp = want["tp"][names.index("disks")].tolist()
    assert len(set(tp)) > 3 and tp[0] > 0 and tp == sorted(tp, reverse=True)  # the pattern exercises the thresholds
    _same_metrics(got, want, (len(names),))
    # one frame without a leading shape, and an InstanceMatch of tensors
    one = pkg.instance_metrics(pkg.InstanceMatch(*(torch.from_numpy(np.array(m[0])) for m in match)))
    for k in INT_KEYS + FLOAT_KEYS:
        assert one[k].shape == got[k].shape[1:] and np.array_equal(one[k], got[k][0])
    # a leading shape of [2, K]
    k2 = len(names) // 2 * 2
    two = pkg.instance_metrics(tuple(m[:k2].reshape((2, k2 // 2) + m.shape[1:]) for m in match))
    assert two["tp"].shape == (2, k2 // 2, 10) and two["aji"].shape == (2, k2 // 2)
    assert np.array_equal(two["tp"].reshape(k2, 10), got["tp"][:k2])
    # other thresholds: Fraction(t).limit_denominator(1000)
    ths = (0.5, 0.7, Fraction(2, 3), 0.999)
    got = pkg.instance_metrics(match, thresholds=ths)
    want = ref.metrics(tabs, ths)
    assert np.array_equal(got["tp"], want["tp"]) and got["tp"].shape == (len(names), 4)
    assert np.all(np.abs(got["mean_ap"] - want["mean_ap"]) <= FLOAT_TOL)


def test_instance_metrics_on_special_frames(pkg):
    for name in ("both_empty", "empty_gt", "empty_pred", "disjoint"):
        tabs, match = _match_of([name])
        got = pkg.instance_metrics(match)
        for k in FLOAT_KEYS:
            assert np.all(got[k] == 0.0), (name, k)
        assert not got["tp"].any()
    tabs, match = _match_of(["identical"])
    got = pkg.instance_metrics(match)
    n = int(match[2][0, 0])
    assert n > 5 and np.all(got["tp"] == n) and not got["fp"].any() and not got["fn"].any()
    assert got["aji"][0] == 1.0 and abs(got["pq"][0] - 1.0) < 1e-7 and abs(got["mean_ap"][0] - 1.0) < 1e-7
    tabs, match = _match_of(["half"])  # IoU exactly 1 / 2 is no match at 0.5
    got = pkg.instance_metrics(match)
    assert not got["tp"].any() and got["fp"][0, 0] == 1 and got["fn"][0, 0] == 1 and got["aji"][0] == 0.5
    assert pkg.instance_metrics(match, thresholds=(Fraction(1, 2),))["tp"][0, 0] == 0


def test_instance_metrics_refuses_bad_input(pkg):
    _, match = _match_of(["disks", "tie"])
    for t in (0.49, 0.0, -1, Fraction(499, 1000)):
        with pytest.raises(ValueError):
            pkg.instance_metrics(match, thresholds=(0.5, t))
    with pytest.raises(ValueError):
        pkg.instance_metrics(match, thresholds=())
    with pytest.raises(ValueError):
        pkg.instance_metrics((match[0], match[1][0], match[2]))
    status = np.array(match[2])
    status[1, 3] = 17
    with pytest.raises(RuntimeError, match="max_pairs"):
        pkg.instance_metrics((match[0], match[1], status))
    status = np.array(match[2])
    status[0, 4] = 1
    with pytest.raises(RuntimeError, match="max_instances"):
        pkg.instance_metrics((match[0], match[1], status))


# ---- the reference's own claims -------------------------------------------------------

def test_reference_tables_are_consistent():
    for name in ref.PATTERNS:
        gt, pred = ref.pattern(name)
        e = ref.expected(name)
        assert e["status"][4] == 0 and e["status"][3] == 0
        assert e["status"][2] == len(e["pairs"]) <= ref.MAX_PAIRS  # the default max_pairs has room for every pattern
        ids, area = np.unique(gt[gt > 0], return_counts=True)
        assert np.array_equal(np.flatnonzero(e["gt_table"][:, 0]) + 1, ids)
        assert np.array_equal(e["gt_table"][ids - 1, 0], area)
        ids, area = np.unique(pred[pred > 0], return_counts=True)
        assert np.array_equal(np.flatnonzero(e["pred_table"][:, 0]) + 1, ids)
        assert np.array_equal(e["pred_table"][ids - 1, 0], area)
        assert e["pairs"][:, 2].sum() == np.count_nonzero((gt > 0) & (pred > 0))
        assert e["counted"] == np.count_nonzero((gt > 0) | (pred > 0))
    assert ref.expected("all_distinct_tile")["status"][2] == 2048
    assert 3000 < ref.expected("noise")["status"][2] <= 63 * 63  # far more than one tile's LDS table holds


def test_reference_ties_go_to_the_smaller_id():
    e = ref.expected("tie")
    assert e["gt_table"][0].tolist() == [32, 3, 16, 16]     # gt 1: preds 5 and 3 at IoU 1 / 2 each
    assert e["pred_table"][8].tolist() == [32, 2, 16, 16]   # pred 9: gts 4 and 2
    assert e["pred_table"][4].tolist() == [16, 1, 16, 32] and e["gt_table"][3].tolist() == [16, 9, 16, 32]


def test_reference_matches_are_unique_and_mutual():
    for name in ref.PATTERNS:
        e = ref.expected(name)
        fc = ref.frame_counts(e)
        for m in fc["matches"]:
            gs, ps = [g for g, _ in m], [p for _, p in m]
            assert len(set(gs)) == len(gs) and len(set(ps)) == len(ps)  # no instance has two matches
            for g, p in m:  # a match is both sides' best partner
                assert e["gt_table"][g - 1, 1] == p and e["pred_table"][p - 1, 1] == g
        # and no pair above 0.5 is missed by looking at the gt side's best partner only
        area_g, area_p = e["gt_table"][:, 0], e["pred_table"][:, 0]
        above = [(g, p) for g, p, c in e["pairs"].tolist() if 2 * c > area_g[g - 1] + area_p[p - 1] - c]
        assert sorted(above) == sorted(fc["matches"][0])
    assert ref.frame_counts(ref.expected("noise"))["tp"][0] == 0


def test_reference_aji():
    fc = ref.frame_counts(ref.expected("identical"))
    assert fc["C"] == fc["U"] > 0
    assert ref.metrics([ref.expected("identical")])["aji"][0] == 1.0
    fc = ref.frame_counts(ref.expected("disjoint"))
    assert fc["C"] == 0 and fc["U"] > 0
    assert ref.metrics([ref.expected("disjoint")])["aji"][0] == 0.0
    gt, pred = ref.pattern("one_to_many")  # the three preds that are not the best partner count into U whole
    fc = ref.frame_counts(ref.expected("one_to_many"))
    assert fc["C"] == 40 * 40 and fc["U"] == 60 * 70 + (600 + 800 + 1200) and fc["tp"][0] == 0
    assert ref.metrics([ref.expected("both_empty")])["aji"][0] == 0.0


def test_reference_out_of_range_pixels_take_no_part():
    gt, pred = (np.array(a) for a in ref.pattern("disks"))
    clean = ref.tables(np.where(gt > 20, 0, gt), np.where(gt > 20, 0, pred), 20, 4096)
    dirty = ref.tables(gt, pred, 20, 4096)
    assert dirty["status"][4] == np.count_nonzero(gt > 20) > 0
    for k in ("gt_table", "pred_table", "pairs"):
        assert np.array_equal(clean[k], dirty[k])
