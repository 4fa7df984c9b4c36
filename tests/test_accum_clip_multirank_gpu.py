"""Gradient accumulation with clipping on two ranks (tests/accum_clip_worker.py): 2 gloo ranks on
the one card, GradSync's bucketed exchange from backward hooks (sent by the last micro-batch of a
window only), accumulate_grad_batches=2 and gradient_clip_val on. Every rank ends with the
parameters of one process stepping on the concatenated micro-batches (torch DDP + Lightning
semantics: entrypoints/segmentation/train.py:799-819), both ranks bit for bit alike."""
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_two_rank_accumulation_with_clipping_equals_single_process(cuda, tmp_path):
    import torch

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import accum_clip_worker as w
    import ddp_worker

    # the clip value: a tenth of the unclipped norm of the first window
    runner, _ = w.run(ddp_worker.build(cuda), w.micro_batches(cuda)[:2], 1e30)
    clip = 0.1 * float(runner.last_grad_norm)
    runner, params = w.run(ddp_worker.build(cuda), w.micro_batches(cuda), clip)
    assert not runner.sync.overlap and runner.optimizer_steps == 2

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, ADELL_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tests", "accum_clip_worker.py"), str(tmp_path), repr(clip)]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    res = [torch.load(tmp_path / f"rank{r}.pt") for r in range(2)]
    for r in range(2):
        assert abs(res[r]["norm"] - float(runner.last_grad_norm)) <= 1e-4 * float(runner.last_grad_norm)
        for k, p in params.items():
            assert torch.allclose(res[r]["params"][k], p, rtol=1e-4, atol=2e-6), k
    for k in params:
        assert torch.equal(res[0]["params"][k], res[1]["params"][k]), k
    # the toy: `a` had a gradient in micro-batch 1 only and is still stepped (mean over ranks / 2)
    x1 = (torch.arange(8, dtype=torch.float32) * 1 + torch.arange(8, dtype=torch.float32) * 2) / 2
    for r in range(2):
        assert torch.allclose(res[r]["toy"]["a"], 2.0 - 0.5 * x1 / 2)
        assert torch.allclose(res[r]["toy"]["b"], 3.0 - 0.5 * (x1 + 1.0) / 2)
