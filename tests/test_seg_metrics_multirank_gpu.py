"""Metric ``compute()`` on two ranks (tests/seg_metrics_worker.py): 2 gloo ranks on the one card,
each updating its shard; both ranks report the value one process computes over every shard
(torchmetrics' sync_dist), and keep their local counts."""
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_two_rank_compute_equals_single_process(cuda, tmp_path):
    import torch

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import seg_metrics_worker as w

    ms = w.build(cuda)
    rows = w.shards(cuda)
    for row in rows:
        for shard in row:
            w.update(ms, *shard)
    want = {k: float(m.compute()) for k, m in ms.items()}
    per_rank = []
    for r in range(2):
        mr = w.build(cuda)
        for row in rows:
            w.update(mr, *row[r])
        per_rank.append({k: m.state.cpu() for k, m in mr.items()})

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, ADELL_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tests", "seg_metrics_worker.py"), str(tmp_path)]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    for r in range(2):
        res = torch.load(tmp_path / f"rank{r}.pt")
        assert res["values"] == want, (r, res["values"], want)
        for k in want:
            assert torch.equal(res["local"][k], per_rank[r][k]), (r, k)
            assert torch.equal(res["after"][k], res["local"][k]), (r, k)     # local counts kept
    # the shards differ: a rank alone would report something else
    assert not all(torch.equal(per_rank[0][k], per_rank[1][k]) for k in want)
