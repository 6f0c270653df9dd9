"""bench.py's command line: a plain run prints the headline line (and --dump-outputs) without the legs after the timed
steps; --full adds them, each one still switchable off with its --no-* flag."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "final_loss")
LEGS = ("fwd_bwd_only", "host_only_ms_per_step", "roofline", "roofline_kernels", "fp32_path", "bf16_path", "fp16_path",
        "cpu_baseline")
# a small shape: the command line is under test here, not the C2 workload
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "4", "--layers", "2"]


def test_full_is_off_by_default(monkeypatch):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "2"])
    args = bench.parse()
    assert not args.full and (args.steps, args.warmup) == (4, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cpu-baseline", "--no-roofline", "--no-alt-leg"])
    args = bench.parse()
    assert args.full and args.no_cpu_baseline and args.no_roofline and args.no_alt_leg and not args.no_fp32_leg


def _bench(args, tmp_path, timeout=300):
    r = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, os.path.join(ROOT, "bench.py"), *args],
                       cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-4000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_without_legs(gpu, tmp_path):
    out = _bench(SMALL + ["--dump-outputs", str(tmp_path / "dump")], tmp_path)
    assert all(k in out for k in HEADLINE), sorted(out)
    assert out["metric"] == "samples/sec fwd+bwd" and out["unit"] == "samples/s" and out["higher_is_better"] is True
    assert out["dtype"] == "fp16" and (out["steps"], out["warmup"]) == (2, 1)
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert abs(out["value"] - 4 * 1e3 / out["ms_per_step"]) < 1e-2 * out["value"]
    assert not [k for k in LEGS if k in out], sorted(out)
    for name, shape in out["dump_outputs"]["arrays"].items():
        a = np.load(str(tmp_path / "dump" / (name + ".npy")))
        assert list(a.shape) == shape and np.isfinite(a).all(), name


@pytest.mark.gpu
def test_full_run_adds_the_legs_it_is_not_told_to_skip(gpu, tmp_path):
    out = _bench(SMALL + ["--full", "--no-cpu-baseline", "--no-roofline", "--no-alt-leg", "--no-fp32-leg"], tmp_path)
    assert all(k in out for k in HEADLINE), sorted(out)
    assert out["fwd_bwd_only"]["ms_per_step_per_rank"] > 0
    assert isinstance(out["host_only_ms_per_step"], float) and out["host_only_ms_per_step"] > 0
    assert not [k for k in ("roofline", "roofline_kernels", "fp32_path", "bf16_path", "cpu_baseline") if k in out], sorted(out)
