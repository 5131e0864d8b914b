"""bench.py's plain run (`--gpus 1 --steps N --warmup W`) measures the headline and nothing else (the diagnostic legs are behind
`--full`), and spends at most 30 s outside its warm-up and timed steps."""
import json
import os
import subprocess
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                 "dtype", "data", "config", "frame"}


def test_bench_plain_run_is_headline_only():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "VV_DIST_FORCE", "VV_BENCH_STUB")}
    steps, warmup = 2, 1
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                       env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-1500:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-1500:]
    j = json.loads(lines[0])
    assert set(j) == HEADLINE_KEYS, sorted(set(j) ^ HEADLINE_KEYS)
    assert (j["metric"], j["unit"], j["higher_is_better"], j["dtype"]) == ("audio-sec/s", "audio-sec/s", True, "bf16")
    assert (j["n_gpus"], j["steps"], j["warmup"]) == (1, steps, warmup) and j["value"] > 0 and j["ms_per_step"] > 0
    outside = wall - (steps + warmup) * j["ms_per_step"] / 1e3
    assert outside < 30.0, (round(wall, 2), j["ms_per_step"], r.stderr[-1500:])
