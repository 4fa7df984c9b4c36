"""PicaiEval.compute() on two ranks (tests/picai_worker.py): 2 gloo ranks on the one card, each with
half of the fixture cases; both report the mean of the two ranks' values (Lightning's sync_dist)."""
import math
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_two_rank_compute_is_the_mean_over_ranks(cuda, tmp_path):
    import torch

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, ADELL_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tests", "picai_worker.py"), str(tmp_path)]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    res = [torch.load(tmp_path / f"rank{r}.pt") for r in range(2)]
    for k, key in enumerate(("AP", "R", "AUC")):
        a, b = res[0]["local"][k], res[1]["local"][k]
        want = (a + b) / 2
        for r in range(2):
            got = res[r]["values"][key]
            assert (math.isnan(got) and math.isnan(want)) or abs(got - want) < 1e-12, (r, key, got, want)
    assert res[0]["local"] != res[1]["local"]
