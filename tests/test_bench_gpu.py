"""GPU: what a plain `bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` run prints and writes -- exactly K timed steps,
the headline keys, no leg of --full, and the last timed step's outputs, identical between two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
NAMES = ("losses", "params", "grads", "bn_running_stats")


def _plain_run(out_dir, K=4, W=2):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(K), "--warmup", str(W), "--dump-outputs", str(out_dir)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    from splice_amd import synth
    n_params = sum(v.size for v in synth.generator_params(1, 0.02).values())
    dumps = []
    for run in range(2):
        out = _plain_run(tmp_path / f"run{run}")
        assert out["metric"] == "opt_steps_per_sec" and out["unit"] == "steps/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
        t = out["config"]["timing"]
        assert out["steps"] == 4 and out["warmup"] == 2 and t["blocks"] == 1 and t["steps_per_block"] == 4
        assert abs(out["value"] * out["ms_per_step"] - 1e3) < 1.0                 # steps/s and ms per step of the same 4 steps
        assert out["roofline"] is None and out["north_star"] is None and out["cpu_baseline"] is None
        assert out["config"]["outputs"]["last_step"] == 5
        arrays = {n: np.load(tmp_path / f"run{run}" / f"{n}.npy") for n in NAMES}
        assert sorted(os.listdir(tmp_path / f"run{run}")) == sorted(n + ".npy" for n in NAMES)
        assert sum(a.nbytes for a in arrays.values()) <= 64e6
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
        assert arrays["losses"].shape == (1, 8) and arrays["losses"][0, 0] > 0
        assert arrays["params"].shape == (1, n_params) and arrays["grads"].shape == (1, n_params)
        assert abs(arrays["losses"][0, 0] - out["config"]["last_loss"]) <= 1e-4 * abs(out["config"]["last_loss"]) + 1e-5
        dumps.append(arrays)
    for n in NAMES:   # seeded inputs and weights, deterministic kernels: the same bits
        assert np.array_equal(dumps[0][n], dumps[1][n]), n
