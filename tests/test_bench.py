"""bench.py's command line: a plain run times the steps alone and prints the
result line; --dump-outputs writes what the timed steps computed; --full adds
the other measurements.  One small configuration (C2: 100k -> 100k), one
process per mode.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("whole_icp", "roofline", "compute_roofline", "setup_ms", "sequence_scan_ms", "cpu_baseline")


def run_bench(*extra, steps=3):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c2",
                        "--steps", str(steps), "--warmup", "2", "--device-warmup", "0", *extra],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_options_are_declared():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True)
    assert p.returncode == 0
    for opt in ("--gpus", "--steps", "--warmup", "--dump-outputs", "--full"):
        assert opt in p.stdout


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    out = tmp_path_factory.mktemp("plain")
    return run_bench("--dump-outputs", str(out)), out


@pytest.fixture(scope="module")
def full(tmp_path_factory):
    out = tmp_path_factory.mktemp("full")
    return run_bench("--full", "--cpu-iters", "5", "--no-cpu-baseline", "--dump-outputs", str(out)), out


@pytest.mark.gpu
def test_plain_run_and_dump(plain):
    r, out = plain
    for k in HEADLINE:
        assert k in r
    assert r["steps"] == 3 and r["warmup"] == 2 and r["dtype"] == "f32" and r["higher_is_better"] is True
    assert r["ms_per_step"] > 0 and r["value"] == pytest.approx(100_000 * 3 / (3 * r["ms_per_step"] * 1e-3))
    assert len(r["timed_iterations"]["levels"]) == 3
    assert not [k for k in FULL_ONLY if k in r]
    assert sorted(os.listdir(out)) == ["T.npy", "last_step.npy"]
    T = np.load(out / "T.npy")
    assert T.dtype == np.float32 and T.shape == (4, 4)
    np.testing.assert_array_equal(T[3], [0, 0, 0, 1])
    np.testing.assert_allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-5)
    assert np.abs(T - np.eye(4)).max() > 1e-3  # (the reading starts away from the reference)
    last = np.load(out / "last_step.npy")
    assert last.dtype == np.float64 and last[0] == 5 and last[1] == r["kept_pairs_last_iter"]


@pytest.mark.gpu
def test_full_run_adds_the_other_measurements(plain, full):
    r, out = full
    for k in HEADLINE + FULL_ONLY:
        assert k in r
    assert r["whole_icp"]["iterations"] == 5 and r["cpu_baseline"] is None
    assert r["roofline"]["avg_launch_ms"] > 0
    # the same inputs and the same timed steps in both runs: the same outputs
    for name in ("T.npy", "last_step.npy"):
        np.testing.assert_array_equal(np.load(out / name), np.load(plain[1] / name))


@pytest.mark.gpu
def test_more_steps_than_the_diagnostics_ring(tmp_path):
    """A long run (the library's per-iteration diagnostics look back 1024
    iterations) times all its steps and reports the last ones' diagnostics."""
    r = run_bench("--dump-outputs", str(tmp_path), steps=1030)
    assert r["steps"] == 1030 and r["ms_per_step"] > 0
    assert len(r["timed_iterations"]["levels"]) == 1024
    assert np.load(tmp_path / "last_step.npy")[0] == 1032
