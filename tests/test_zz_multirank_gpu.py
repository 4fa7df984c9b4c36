"""The N > 1 code path of bench.py on the GPU box: two ranks launched exactly as the driver
launches them (torch.distributed.run, one process per rank), sharing the one card and exchanging
gradients over gloo (RCCL needs one GPU per rank; `ADELL_DIST_BACKEND` / `ADELL_SINGLE_GPU_REHEARSAL`
exist for this rehearsal only). Checks the contract fields of the single JSON line rank 0 prints."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_two_rank_bench_prints_one_contract_line(cuda):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, ADELL_DIST_BACKEND="gloo", ADELL_SINGLE_GPU_REHEARSAL="1",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--batch", "1", "--size", "32", "--full"]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]          # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["warmup"] == 1 and d["scaling"] == "weak"
    assert d["config"]["parallelism"] == "dp2" and d["config"]["per_gpu_batch"] == 1
    assert "cpu_baseline" not in d                      # rank 0 at N = 1 only
    # whole-job throughput: both ranks' volumes over the slowest rank's time
    assert abs(d["value"] - 2 * 1 * 2 / (2 * d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert d["roofline"]["frac"] > 0 and d["final_loss"] == d["final_loss"]
    # the line explains its own exchange: exposed wait, bucket sizes, issue times against backward
    ex = d["gradient_exchange"]
    assert ex["overlap"] and ex["steps_profiled"] == 3 and ex["backend"] == "gloo"
    assert ex["exposed_comm_ms"] is not None and ex["exposed_comm_ms"] >= 0
    assert ex["exposed_comm_host_ms"] >= 0 and 0 <= ex["exposed_share_of_step"] < 1
    assert len(ex["bucket_mb"]) == len(ex["issue_before_backward_end_ms"]) >= 1
    assert abs(sum(ex["bucket_mb"]) - ex["gradient_mb"]) < 1e-2 and ex["gradient_mb"] > 30   # 33 MB
    assert all(v is not None for v in ex["issue_before_backward_end_ms"])


@pytest.mark.gpu
def test_two_rank_unet_equals_single_process_batch(cuda, tmp_path):
    """The real small U-Net on two ranks (one fixture item each, bucketed all-reduce issued from
    backward hooks, 1/world folded into the optimiser) == one process on the batch of two: the
    averaged first-step gradients and the parameters after two SGD-Nesterov steps. Reference
    semantics: torch DDP under entrypoints/segmentation/train.py:799-819."""
    import numpy as np
    import torch

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ddp_worker

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, ADELL_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tests", "ddp_worker.py"), str(tmp_path)]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    res = [torch.load(tmp_path / f"rank{r}.pt") for r in range(2)]
    g = np.load(os.path.join(ROOT, "tests", "golden", "unet3d_cfg2_small.npz"))
    net = ddp_worker.build(cuda)
    batch = {"image": torch.from_numpy(g["x"]).to(cuda), "mask": torch.from_numpy(g["y"]).to(cuda)}
    grads, params, sync = ddp_worker.run(net, batch, 2)
    assert not sync.overlap                      # world size 1: no hooks, no collectives
    scale = float(grads.abs().max())
    for r in range(2):
        assert float((res[r]["grads"] - grads).abs().max()) < 2e-5 * scale
        for k, p in params.items():
            assert torch.allclose(res[r]["params"][k], p, rtol=1e-4, atol=2e-6), k
    for k in params:
        assert torch.equal(res[0]["params"][k], res[1]["params"][k]), k


@pytest.mark.gpu
def test_single_rank_rccl_overlap_path(cuda, tmp_path):
    """RCCL itself (backend "nccl", one rank on the one card) under the overlapped GradSync path:
    hooks -> gather launch -> async all-reduce on the collective stream -> wait -> fused SGD. Two
    steps of the small U-Net must reproduce the no-exchange run bit for bit; two backward passes in
    one step must give twice the single-pass gradient (tests/rccl_worker.py)."""
    import torch

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1",
               LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tests", "rccl_worker.py"),
           str(tmp_path)]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    res = torch.load(tmp_path / "rccl.pt")
    assert res["losses"] == res["plain_losses"]
    for k, p in res["plain"].items():
        assert torch.equal(res["params"][k], p), k
    scale = float(res["once"].abs().max())
    assert float((res["twice"] - 2.0 * res["once"]).abs().max()) <= 1e-6 * scale
    # the same network under torch DistributedDataParallel (Lightning's strategy="ddp"): no weight
    # gradient leaves the main stream (DDP's Reducer reads it from a C++ hook the moment the node
    # returns), and the steps are bit-identical with the side stream switched off
    l_on, p_on, calls_on = res["ddp_on"]
    l_off, p_off, calls_off = res["ddp_off"]
    assert calls_on == 0 and calls_off == 0
    assert l_on == l_off
    for k, p in p_off.items():
        assert torch.equal(p_on[k], p), k
