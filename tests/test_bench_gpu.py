"""bench.py's plain run, the command every change is timed with: one JSON line with the headline
fields and none of the ``--full`` figures, and ``--dump-outputs DIR`` writing what the last timed
step handed its caller (loss, parameters after the optimiser step, gradients) as float32 arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_plain_run_prints_the_headline_line_and_dumps_the_last_step(cuda, tmp_path):
    sys.path.insert(0, ROOT)
    import bench

    out_dir = tmp_path / "outputs"
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "bench.py"), "--gpus",
           "1", "--steps", "3", "--warmup", "1", "--batch", "1", "--size", "32",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["unit"] == "volumes/s" and d["higher_is_better"] is True and d["dtype"]
    assert d["metric"].startswith("volumes/sec") and d["steps"] == 3 and d["warmup"] == 1
    # value: volumes over the timed steps; ms_per_step: one timed step
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    for k in ("roofline", "cpu_baseline", "fp32_mfma", "secondary", "streams", "step_record"):
        assert k not in d, k

    assert sorted(os.listdir(out_dir)) == ["gradients.npy", "loss.npy", "parameters.npy"]
    loss = np.load(out_dir / "loss.npy")
    assert loss.dtype == np.float32 and float(loss) == d["final_loss"]
    params, grads = np.load(out_dir / "parameters.npy"), np.load(out_dir / "gradients.npy")
    assert params.dtype == grads.dtype == np.float32
    assert params.shape == grads.shape == (bench.DUMP_MAX_VALUES,)       # 8.3 M parameters: sampled
    assert np.isfinite(params).all() and np.isfinite(grads).all() and np.abs(grads).max() > 0
    assert sum(os.path.getsize(out_dir / f) for f in os.listdir(out_dir)) <= 64 * 10**6
