"""GPU (one MI355X): bench.py's own contract on a small workload.  A plain run prints ONE line whose `ms_per_step` prices the
`--steps` it was given and leaves out the legs that only `--full` runs; `--dump-outputs DIR` writes the last timed step's
logits (float32), and with the same workload arguments a second run -- `--full` this time -- dumps the same logits."""
from __future__ import annotations

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
FULL_ONLY = {"cpu_baseline", "fp32_exact_reads_per_s", "pcie_inclusive_reads_per_s", "p50_host_visible_latency_ms"}


def _bench(*args: str) -> dict:
    cmd = [sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--batch", "8", "--bases", "2100", "--steps", "3", "--warmup", "1",
           *args]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_and_full_runs_dump_the_same_logits(tmp_path, built_lib):
    plain = _bench("--dump-outputs", str(tmp_path / "plain"))
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["unit"] == "reads/s" and plain["higher_is_better"] is True
    assert abs(plain["value"] - 8 * 3 / (plain["ms_per_step"] * 3e-3)) < 1e-6 * plain["value"]
    assert plain["dtype"] in ("fp16c", "fp16x3", "fp32") and "reads/sec" in plain["metric"]
    assert not FULL_ONLY & set(plain), sorted(FULL_ONLY & set(plain))
    a = np.load(tmp_path / "plain" / "logits.npy")
    assert a.dtype == np.float32 and a.shape == (8, 2) and np.isfinite(a).all()

    full = _bench("--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full"))
    assert full["fp32_exact_reads_per_s"] > 0 and full["pcie_inclusive_reads_per_s"] > 0 and full["p50_host_visible_latency_ms"] > 0
    b = np.load(tmp_path / "full" / "logits.npy")
    np.testing.assert_allclose(b, a, rtol=0, atol=1e-6)
