"""bench.py's two modes: a plain run prints the headline line only, `--full` adds the roofline passes (and, at the default
shape, config.secondary and the CPU baseline)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*args, timeout=600):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_help_names_full():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr
    assert "--full" in p.stdout


@pytest.mark.gpu
def test_bench_plain_run_is_headline_only(tmp_path):
    d = _bench("--points", "256", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path))
    for k in HEADLINE:
        assert k in d, k
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["steps"] == 2 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["dtype"] == "f64"
    assert "roofline" not in d and "cpu_baseline" not in d
    assert not any(k.startswith(("phase_ms", "device_pass", "secondary")) for k in d["config"])
    assert sorted(os.listdir(tmp_path)) == ["R.npy", "T.npy"]


@pytest.mark.gpu
def test_bench_full_adds_roofline():
    d = _bench("--full", "--points", "256", "--steps", "1", "--warmup", "0", "--no-cpu-baseline")
    for k in HEADLINE:
        assert k in d, k
    r = d["roofline"]
    assert r["kernel"] == "k_layer_native<4, 15>" and r["launches"] > 0 and r["achieved"] > 0
    assert d["config"]["device_pass_ms (run() only, HIP events)"] > 0
    assert set(d["config"]["phase_ms (one extra untimed pass with syncs)"]) == {"h2d", "optics", "run", "gather_d2h"}
    assert "cpu_baseline" not in d
