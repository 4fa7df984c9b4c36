"""Rank program of tests/test_sync_bn_multirank_gpu.py (not a test module): synchronised batch norm
on two ranks.

* the small 3-D U-Net of tests/ddp_worker.py with batch norm, one fixture item per rank, two steps
  of StepRunner(sync_batchnorm=True) -- and the same with sync_batchnorm=False;
* the batch-norm ResNet of the SSL hand-off as SelfSLResNetPL (vicreg), two items per rank,
  converted by torch's own SyncBatchNorm.convert_sync_batchnorm (what Lightning runs): the
  forward outputs of this rank's items, then two training steps.

Parameters and batch-norm buffers are saved per rank."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def build_unet(device):
    """ddp_worker.build with norm_type="batch"; the by-name fill also wrote the running statistics,
    which start from torch's defaults again."""
    from adell_mri_amd.modules.activations import activation_factory
    from adell_mri_amd.modules.segmentation.losses import (CompoundLoss, binary_focal_loss,
                                                           binary_generalized_dice_loss)
    from adell_mri_amd.modules.segmentation.pl import UNetPL
    from cases import UNET_CASES
    from oracle.weights import tensor_for

    kw = dict(UNET_CASES["unet3d_cfg2_small"])
    kw["activation_fn"] = activation_factory[kw["activation_fn"]]
    kw["dropout_param"] = 0.0
    kw["norm_type"] = "batch"
    loss = CompoundLoss([(binary_generalized_dice_loss, {"smooth": 1e-5, "eps": 1e-6}),
                         (binary_focal_loss, {"gamma": 1.0, "eps": 1e-6})])
    net = UNetPL(image_key="image", label_key="mask", learning_rate=5e-2, weight_decay=5e-3,
                 loss_fn=loss, **kw)
    net.load_state_dict({k: torch.from_numpy(tensor_for(k, v.shape))
                         for k, v in net.state_dict().items()})
    for m in net.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.reset_running_stats()
    return net.to(device).train()


def unet_batch(device, rank=None):
    g = np.load(os.path.join(ROOT, "tests", "golden", "unet3d_cfg2_small.npz"))
    sl = slice(None) if rank is None else slice(rank, rank + 1)
    return {"image": torch.from_numpy(g["x"])[sl].to(device),
            "mask": torch.from_numpy(g["y"])[sl].to(device)}


def build_ssl(device):
    from adell_mri_amd.modules.layers.adn_fn import get_adn_fn
    from adell_mri_amd.modules.self_supervised.pl import SelfSLResNetPL

    torch.manual_seed(0)
    net = SelfSLResNetPL(
        aug_image_key_1="a", aug_image_key_2="b", ssl_method="vicreg", stop_gradient=False,
        ema=None, learning_rate=1e-3, weight_decay=5e-3, optimizer_eps=1e-8, batch_size=2,
        backbone_args=dict(spatial_dim=3, in_channels=2,
                           structure=[[8, 8, 5, 1], [16, 16, 3, 1], [32, 32, 3, 1]],
                           maxpool_structure=[[2, 2, 1], [2, 2, 2], [2, 2, 2]],
                           adn_fn=get_adn_fn(3, "batch", "swish", 0.0)),
        projection_head_args=dict(in_channels=32, structure=[16, 8],
                                  adn_fn=get_adn_fn(1, "batch", "swish", 0.0)),
        prediction_head_args=dict(in_channels=8, structure=[16, 8],
                                  adn_fn=get_adn_fn(1, "batch", "swish", 0.0)))
    return net.to(device).train()


def ssl_batch(device, rank=None):
    """Two items per rank; rank=None: all four (the single-process equivalent)."""
    g = torch.Generator().manual_seed(99)
    a, b = torch.rand((4, 2, 32, 32, 32), generator=g), torch.rand((4, 2, 32, 32, 32), generator=g)
    sl = slice(None) if rank is None else slice(2 * rank, 2 * rank + 2)
    return {"a": a[sl].to(device), "b": b[sl].to(device)}


def ssl_forward(net, batch):
    """The outputs the test compares (train mode: the statistics are the batch's)."""
    rep = net(batch["a"], ret="representation")
    proj = net(batch["a"], ret="projection")
    return rep.detach().cpu(), proj.detach().cpu()


def state(net):
    return ({k: p.detach().cpu().clone() for k, p in net.named_parameters()},
            {k: b.detach().cpu().clone() for k, b in net.named_buffers()
             if k.endswith(("running_mean", "running_var", "num_batches_tracked"))})


def steps(net, batch, n, **kw):
    from adell_mri_amd.trainer import StepRunner

    runner = StepRunner(net, **kw)
    for _ in range(n):
        runner.train_step(batch)
    torch.cuda.synchronize()
    return runner


def main():
    from adell_mri_amd.parallel import init_distributed

    out = sys.argv[1]
    rank, world, _ = init_distributed()
    assert world == 2
    device = torch.device("cuda", 0)    # both ranks share the one card (gloo)
    torch.cuda.set_device(device)
    res = {}

    net = build_unet(device)
    steps(net, unet_batch(device, rank), 2, sync_batchnorm=True)
    res["unet_sync"] = state(net)
    net = build_unet(device)
    steps(net, unet_batch(device, rank), 2, sync_batchnorm=False)
    res["unet_plain"] = state(net)

    net = torch.nn.SyncBatchNorm.convert_sync_batchnorm(build_ssl(device))
    batch = ssl_batch(device, rank)
    res["ssl_forward"] = ssl_forward(net, batch)
    steps(net, batch, 2)
    res["ssl_steps"] = state(net)

    torch.save(res, os.path.join(out, f"rank{rank}.pt"))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
