"""A plain `python bench.py` run sets up, warms up, times its steps, writes --dump-outputs and prints the line; whatever
else the benchmark measures or checks (roofline, golden hashes, extra legs, CPU baseline, the other configs) runs only
with --full."""

import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(args, timeout):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)


@pytest.mark.timeout(120)
def test_stages_needs_full():
    """--stages prints the profiled pass that only --full runs: without it, a usage error before anything touches the GPU."""
    run = run_bench(["--stages"], timeout=100)
    assert run.returncode == 2 and "--full" in run.stderr, run.stderr[-2000:]


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_plain_run_is_the_headline_alone(tmp_path):
    run = run_bench(["--gpus", "1", "--layers", "2", "--rows", "768", "--cols", "768", "--steps", "2", "--warmup", "1",
                     "--dump-outputs", str(tmp_path)], timeout=280)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, run.stdout
    got = json.loads(lines[0])
    assert got["full"] is False
    assert got["value"] > 0 and got["ms_per_step"] > 0 and (got["steps"], got["warmup"]) == (2, 1)
    assert got["unit"] == "Mweights/s" and got["higher_is_better"] is True and got["dtype"] == "f64"
    assert got["layer_errors"]["layers"] == 2 and got["layer_errors"]["all_finite"]
    for key in ("roofline", "cpu_baseline", "latency_ms_single_layer", "asymmetric_H", "hessian_accumulate", "local_search", "golden"):
        assert got[key] is None, key
    assert "configs" not in got and "rccl" not in got
    assert got["summary"]["golden_ok"] is None
    assert got["dump_outputs"]["bytes"] > 0 and "layer_errors.npy" in os.listdir(tmp_path)
