"""bench.py end to end on the GPU: a plain run measures the headline and nothing else; --full adds the passes that run after
the timed region."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "hbm_leg", "collective", "secondary", "cpu_baseline")


def run_bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "UNETDC_DP_FORCE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", *extra],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_reports_the_headline_only(tmp_path):
    d = run_bench("--dump-outputs", str(tmp_path))
    assert all(k in d for k in CONTRACT)
    assert d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["step_ms"]["n"] == 3
    assert not [k for k in FULL_ONLY if k in d]
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in d["dumped_outputs"]["arrays"])


def test_full_run_adds_the_instrumented_legs():
    d = run_bench("--full", "--no-cpu-baseline", "--no-secondary")
    assert all(k in d for k in CONTRACT)
    assert d["roofline"]["achieved"] > 0 and d["roofline"]["kernel"]
    assert d["hbm_leg"]["entries"] and d["hbm_leg"]["achieved"] > 0
    assert "secondary" not in d and "cpu_baseline" not in d
