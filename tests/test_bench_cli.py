"""bench.py's command line: a plain run times the steps and nothing else,
--full adds the parity / roofline / CPU-baseline legs, --dump-outputs writes
the last timed step's logits and loss.

Tolerances: the dumped loss is the fused BCE kernel's fp32 mean over the
dumped fp32 logits (fp32 per thread, fp64 above, 2*64*64 elements), the check
recomputes it in fp64 from the same logits: relative 1e-5 covers the fp32
per-element rounding (2^-24 each) and the fp32 result with room to spare.
"""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
BATCH, SIZE = 2, 64


@pytest.fixture(scope="module")
def bench():
    return importlib.import_module("bench")  # conftest.py puts the repository root on sys.path


def test_dump_outputs_small_arrays_whole(bench, tmp_path):
    a = torch.arange(24, dtype=torch.bfloat16).reshape(2, 3, 4)
    b = torch.tensor(0.25, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "d"), {"a": a, "b": b})
    ra, rb = np.load(tmp_path / "d" / "a.npy"), np.load(tmp_path / "d" / "b.npy")
    assert ra.dtype == np.float32 and ra.shape == (2, 3, 4) and np.array_equal(ra, a.float().numpy())
    assert rb.dtype == np.float64 and rb.shape == () and rb == 0.25


def test_dump_outputs_samples_within_budget(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 64 << 10)
    big = torch.arange(100_000, dtype=torch.float32)
    small = torch.ones(5)
    for d in ("d1", "d2"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small}, rank=1, world=2)
    files = sorted(os.listdir(tmp_path / "d1"))
    assert files == ["big.rank1.npy", "small.rank1.npy"]
    # both ranks' files together stay inside the budget
    assert 2 * sum(os.path.getsize(tmp_path / "d1" / f) for f in files) <= 64 << 10
    s1, s2 = np.load(tmp_path / "d1" / files[0]), np.load(tmp_path / "d2" / files[0])
    assert np.array_equal(s1, s2)  # the same sample every run
    assert 1000 < s1.size < big.numel() and np.all(np.diff(s1) >= 0)  # values are their own sorted indices
    assert np.array_equal(np.load(tmp_path / "d1" / files[1]), small.numpy())


def test_bench_inputs_are_seeded(pkg):
    a, b = pkg.synthetic_cells(BATCH, SIZE, SIZE, seed=1234), pkg.synthetic_cells(BATCH, SIZE, SIZE, seed=1234)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _run(*extra):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--batch", str(BATCH), "--size", str(SIZE), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=REPO, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_outputs(cuda, pkg, tmp_path):
    import oracle
    out = tmp_path / "dump"
    line = _run("--dump-outputs", str(out))
    print(line)
    for k in KEYS:
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "images/sec" and line["dtype"] == "bf16"
    assert line["higher_is_better"] is True and line["ms_per_step"] > 0
    # value and ms_per_step are the same wall time (both rounded to 3 decimals)
    assert line["value"] == pytest.approx(BATCH * 1e3 / line["ms_per_step"], rel=1e-2)
    # nothing that takes a run of its own
    assert line["roofline"] is None and line["miou_step0"] is None and line["miou_ref"] is None
    assert "cpu_baseline" not in line
    assert sorted(os.listdir(out)) == ["logits.npy", "loss.npy"]
    logits, loss = np.load(out / "logits.npy"), np.load(out / "loss.npy")
    assert logits.dtype == np.float32 and logits.shape == (BATCH, 1, SIZE, SIZE) and np.isfinite(logits).all()
    assert loss.dtype == np.float32 and loss.shape == ()
    # logits and loss belong to the same step: BCE of the dumped logits on the seeded masks
    masks = torch.from_numpy(pkg.synthetic_cells(BATCH, SIZE, SIZE, seed=1234)[1]).double()
    want = oracle.bce_with_logits(torch.from_numpy(logits).double(), masks).item()
    print(f"dumped loss {float(loss):.8f} vs BCE of dumped logits {want:.8f}")
    assert abs(float(loss) - want) <= 1e-5 * abs(want)


@pytest.mark.gpu
def test_full_run_keeps_parity_roofline_and_cpu_baseline(cuda):
    line = _run("--full", "--cpu-steps", "1")
    print(line)
    for k in KEYS:
        assert k in line, k
    assert line["steps"] == 3
    # the parity leg ran (its bound is test_miou_parity_gpu.py's business, at sizes where one pixel is < 1e-3)
    assert None not in (line["miou_step0"], line["miou_ref"], line["miou_abs_diff"])
    roof = line["roofline"]
    assert roof["kernel"] and roof["achieved"] > 0 and roof["launches_per_step"] > 0 and roof["step_tflops"] > 0
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["unit"] == "images/sec"
