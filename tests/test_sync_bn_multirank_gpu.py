"""Synchronised batch norm on two ranks (tests/sync_bn_worker.py): 2 gloo ranks on the one card.
W ranks of B items with synchronised batch norm and a per-item loss step like one process on all
W * B items with ordinary batch norm (torch.nn.SyncBatchNorm as Lightning's sync_batchnorm=True
uses it: entrypoints/ssl/train_3d.py:349)."""
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _excess(a, b, rtol=1e-4, atol=2e-6):
    """max |a - b| / (atol + rtol |b|): <= 1 is within the multirank tolerance."""
    return float(((a.double() - b.double()).abs() / (atol + rtol * b.double().abs())).max())


@pytest.mark.gpu
def test_two_rank_sync_batchnorm_equals_single_process(cuda, tmp_path):
    import torch

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sync_bn_worker as w

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, ADELL_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tests", "sync_bn_worker.py"), str(tmp_path)]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    res = [torch.load(tmp_path / f"rank{r}.pt") for r in range(2)]

    # --- U-Net, one item per rank, StepRunner(sync_batchnorm=True) == one process on both items
    net = w.build_unet(cuda)
    p0 = w.state(net)[0]
    w.steps(net, w.unet_batch(cuda), 2)
    params, buffers = w.state(net)
    assert buffers and all(int(buffers[k]) == 2 for k in buffers if k.endswith("num_batches_tracked"))
    for r in range(2):
        p_sync, b_sync = res[r]["unet_sync"]
        for k, p in params.items():
            assert _excess(p_sync[k], p) <= 1.0, k
        for k, b in buffers.items():
            assert _excess(b_sync[k], b) <= 1.0, k
    for i in range(2):
        for k in res[0]["unet_sync"][i]:
            assert torch.equal(res[0]["unet_sync"][i][k], res[1]["unet_sync"][i][k]), k
    # without synchronisation each rank normalises its one item: the running statistics land far
    # outside the tolerance, and the two steps' parameter updates differ by far more than the
    # synchronised ones do
    def update_err(got):
        num = max(float(((got[k] - p0[k]) - (p - p0[k])).abs().max()) for k, p in params.items())
        return num / max(float((p - p0[k]).abs().max()) for k, p in params.items())

    for r in range(2):
        p_plain, b_plain = res[r]["unet_plain"]
        worst = max([_excess(p_plain[k], p) for k, p in params.items()]
                    + [_excess(b_plain[k], b) for k, b in buffers.items()
                       if not k.endswith("num_batches_tracked")])
        assert worst > 100.0, worst
        e_sync, e_plain = update_err(res[r]["unet_sync"][0]), update_err(p_plain)
        assert e_plain > 10.0 * e_sync, (e_sync, e_plain)

    # --- SSL ResNet converted by torch's converter: each rank's rows of the 4-item forward
    net = w.build_ssl(cuda)
    rep, proj = w.ssl_forward(net, w.ssl_batch(cuda))
    for r in range(2):
        rep_r, proj_r = res[r]["ssl_forward"]
        rows = slice(2 * r, 2 * r + 2)
        assert torch.allclose(rep_r, rep[rows], rtol=1e-4, atol=1e-5), float((rep_r - rep[rows]).abs().max())
        assert torch.allclose(proj_r, proj[rows], rtol=1e-4, atol=1e-5), float((proj_r - proj[rows]).abs().max())
    # after two steps: parameters and batch-norm buffers bit-identical across ranks
    for i in range(2):
        assert res[0]["ssl_steps"][i]
        for k in res[0]["ssl_steps"][i]:
            assert torch.equal(res[0]["ssl_steps"][i][k], res[1]["ssl_steps"][i][k]), k
