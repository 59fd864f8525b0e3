"""GPU suite, early on purpose (fresh child processes; this process has not touched the GPU yet): a plain bench.py run does the
headline measurement only, and --dump-outputs writes what its last timed step returned -- the same arrays from run to run and
the same arrays that a --full run verifies against the oracle and the exact HIP path."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
BENCH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py")
ARGS = ["--gpus", "1", "--rows", "200000", "--queries", "300", "--k", "10", "--steps", "4", "--warmup", "1"]


def run_bench(extra, out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, BENCH] + ARGS + extra + ["--dump-outputs", str(out_dir)], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, p.stderr.decode("utf-8", "replace")[-3000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), np.load(out_dir / "ids.npy"), np.load(out_dir / "distances.npy")


def test_plain_bench_times_its_steps_and_dumps_the_last_one(tmp_path):
    d, ids, dist = run_bench([], tmp_path / "a")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in d
    assert d["steps"] == 4 and d["step_ms_hip_events"]["n"] == 4 and d["roofline"]["launches_timed"] == 4
    assert d["value"] > 0 and d["ms_per_step"] > 0
    for key in ("verified", "cpu_baseline", "pcie_inclusive", "vendor_stack", "hbm_bound_configs", "query_latency", "embed"):
        assert key not in d, f"a plain run computed {key}"
    assert ids.dtype == np.float64 and dist.dtype == np.float64
    assert ids.shape == (300, 10) and dist.shape == (300, 10)
    assert np.array_equal(ids, np.round(ids)) and ids.min() >= 0 and ids.max() < 200000
    assert np.all(np.diff(dist, axis=1) >= 0)

    _, ids2, dist2 = run_bench([], tmp_path / "b")
    assert np.array_equal(ids, ids2) and np.array_equal(dist, dist2)

    f, ids3, dist3 = run_bench(["--full", "--no-embed", "--no-cpu-baseline", "--no-side-configs"], tmp_path / "c")
    assert f["verified"]["equals_exact_hip_path"] and f["verified"]["equals_oracle_scan_of_slice"]
    assert np.array_equal(ids, ids3) and np.array_equal(dist, dist3)
