"""Generate the SWIN-UNet fixtures of tests/swin_window_cases.py from the REAL reference (build host
only; the reference tree does not travel to the GPU machine): windows of more than 64 tokens and
heads wider than 32, which the reference runs through F.scaled_dot_product_attention
(linear_blocks.py:358-417).

Each case goes through oracle.make_golden.gen_unet with ``_cls="swin"``, so the fp64 gradients of
the same network are stored beside the fp32 ones (tests/test_swin.py explains why). gen_unet writes
one archive per case; it is re-packed here into files below the repository's 1 MiB limit for a
committed file:
  <name>.npz         x, y, logits, loss, param_keys, param_shapes
  <name>.gradN.npz   "grad:<param>" (the reference's fp32 gradient) and "grad64:<param>" (its fp64
                     gradient), whole parameters per file, as many files as the limit asks for
prob, dice and focal of gen_unet's archive are not kept: no test of these cases reads them.

    python tools/make_golden_swin_windows.py
"""
import glob
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

import oracle.make_golden as mg  # noqa: E402
from swin_window_cases import SWIN_WINDOW_CASES  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
LIMIT = 1000 * 1024        # bytes per committed file, with a margin below 1 MiB
HEAD = ("x", "y", "logits", "loss", "param_keys", "param_shapes")


def _size(arrays):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "a.npz")
        np.savez_compressed(path, **arrays)
        return os.path.getsize(path)


def repack(name, g):
    for old in glob.glob(os.path.join(GOLD, name + ".grad*.npz")):
        os.remove(old)
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **{k: g[k] for k in HEAD})
    parts, cur = [], {}
    for k in [str(k) for k in g["param_keys"]]:
        if ("grad:" + k) not in g.files:
            continue
        new = {"grad:" + k: g["grad:" + k], "grad64:" + k: g["grad64:" + k]}
        if cur and _size({**cur, **new}) > LIMIT:
            parts.append(cur)
            cur = {}
        cur.update(new)
    parts.append(cur)
    for i, part in enumerate(parts):
        np.savez_compressed(os.path.join(GOLD, f"{name}.grad{i}.npz"), **part)
    sizes = [os.path.getsize(p) for p in sorted(glob.glob(os.path.join(GOLD, name + ".*npz")))]
    assert max(sizes) <= 1024 * 1024, sizes
    print(name, "files", sizes)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        mg.OUT = tmp
        for name, (kw, shape) in SWIN_WINDOW_CASES.items():
            mg.gen_unet(name, dict(kw, _cls="swin"), shape, "uniform")
            repack(name, np.load(os.path.join(tmp, name + ".npz")))


if __name__ == "__main__":
    main()
