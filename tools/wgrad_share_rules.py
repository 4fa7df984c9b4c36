"""Which side-stream conv weight gradients should carry the share hint (ops.conv3d_bwd_weight(share=)):
blocks of steps of the bench workload alternate between rules inside ONE process on ONE box, as
tools/ab_step.py does for a switch. A rule decides per launch from (input channels, output channels,
input voxels per item); where it says yes the launch gets ADELL_WGRAD_SHARE_ALWAYS, "auto" passes
ADELL_WGRAD_SHARE_AUTO everywhere (the default step), "none" no hint (the parent's launches).
usage: wgrad_share_rules.py [rounds=4] [steps per block=8] [rule ...]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from adell_mri_amd import ops  # noqa: E402
from adell_mri_amd.parallel import GradSync  # noqa: E402
from adell_mri_amd.trainer import StepRunner  # noqa: E402

FULL = 128 ** 3
RULES = {
    "none": lambda cin, cout, vox: False,
    "auto": None,
    "all": lambda cin, cout, vox: True,
    "full": lambda cin, cout, vox: vox >= FULL,
    "low": lambda cin, cout, vox: vox < FULL,
    "l1": lambda cin, cout, vox: vox == 64 ** 3,
    "l01": lambda cin, cout, vox: vox >= 64 ** 3,
    "wide": lambda cin, cout, vox: cin > 32 or cout > 32,
    "c32": lambda cin, cout, vox: cin <= 32 and cout <= 32,
    "fullwide": lambda cin, cout, vox: vox >= FULL and (cin > 32 or cout > 32),
    "fullcin": lambda cin, cout, vox: vox >= FULL and cin > 32,
    "fullwide_l1": lambda cin, cout, vox: (vox >= FULL and (cin > 32 or cout > 32)) or vox == 64 ** 3,
}
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 4
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 8
names = sys.argv[3:] or ["none", "auto", "all", "full", "low"]
state = {"rule": RULES["none"]}
real = ops.conv3d_bwd_weight


def hinted(x0, dy, *a, share=False, x1=None, **k):
    if share and state["rule"] is not None:     # (only launches the step would hint: the side stream's)
        cin = x0.shape[1] + (0 if x1 is None else x1.shape[1])
        share = 2 if state["rule"](cin, dy.shape[1], x0.shape[2] * x0.shape[3] * x0.shape[4]) else False
    return real(x0, dy, *a, share=share, x1=x1, **k)


ops.conv3d_bwd_weight = hinted
dev = torch.device("cuda:0")
net, _ = bench.build_module(dev, bench.CONFIG)
net.train()
opt = net.configure_optimizers()["optimizer"]
runner = StepRunner(net, opt, GradSync(opt))
batch = bench.synthetic_batch(int(net.batch_size), (128, 128, 128), dev, 42)
for _ in range(6):
    runner.train_step(batch)
torch.cuda.synchronize()
res = {n: [] for n in names}
for r in range(rounds):
    for n in names:
        state["rule"] = RULES[n]
        runner.train_step(batch)          # settle
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            runner.train_step(batch)
        e1.record()
        torch.cuda.synchronize()
        res[n].append(round(e0.elapsed_time(e1) / steps, 3))
for n in names:
    print(json.dumps({"rule": n, "median_ms_per_step": statistics.median(res[n]), "blocks": res[n]}),
          flush=True)
