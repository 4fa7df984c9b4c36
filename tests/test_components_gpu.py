"""ops.label_components (csrc/components.hip) against the numpy restatement of
scipy.ndimage.label(x, np.ones((3, 3, 3))) in tests/picai_ref.py: labels and counts equal as
integers, and a second run bitwise identical."""
import os
import sys

import numpy as np
import pytest
import torch

from adell_mri_amd import ops

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import picai_ref  # noqa: E402


def _check(mask, cuda, threshold=None, values=None):
    x = torch.from_numpy(values if values is not None else mask.astype(np.float32)).to(cuda)
    lab, n = ops.label_components(x, threshold)
    lab2, n2 = ops.label_components(x, threshold)
    torch.cuda.synchronize()
    lab, n = lab.cpu().numpy(), n.cpu().numpy()
    assert torch.equal(lab2.cpu(), torch.from_numpy(lab)) and n2.cpu().numpy().tolist() == n.tolist()
    masks = mask.reshape((-1,) + mask.shape[-3:])
    labs = lab.reshape((-1,) + mask.shape[-3:])
    ns = n.reshape(-1)
    for i, m in enumerate(masks):
        want, wn = picai_ref.label(m)
        assert int(ns[i]) == wn, (i, int(ns[i]), wn)
        assert np.array_equal(labs[i], want), i
    return ns


@pytest.mark.parametrize("density", [0.05, 0.3, 0.5, 0.9])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 77), (1, 50, 1), (40, 1, 1), (17, 33, 65),
                                   (9, 17, 33), (8, 16, 32), (2, 19, 40, 70)])
def test_random_masks(cuda, shape, density):
    rng = np.random.default_rng(abs(hash((shape, density))) % 2 ** 32)
    _check(rng.random(shape) < density, cuda)


@pytest.mark.parametrize("density", [0.05, 0.3, 0.5, 0.9])
def test_128_cubed(cuda, density):
    rng = np.random.default_rng(int(density * 100))
    _check(rng.random((128, 128, 128)) < density, cuda)


def test_all_zero_and_all_one(cuda):
    for shape in [(1, 1, 1), (17, 33, 65), (64, 64, 64)]:
        assert _check(np.zeros(shape, bool), cuda).tolist() == [0]
        assert _check(np.ones(shape, bool), cuda).tolist() == [1]


def test_diagonal_chains(cuda):
    m = np.zeros((40, 40, 70), bool)
    for k in range(40):
        m[k, k, k] = True                  # corner-only chain across tiles
        m[k, 39 - k, 60] = True            # edge-only chain
    m[5, 0, 65:70:2] = True                # isolated voxels
    assert _check(m, cuda).tolist() == [5]


def test_serpentine_crosses_every_tile(cuda):
    D, H, W = 20, 36, 70
    m = np.zeros((D, H, W), bool)
    for z in range(0, D, 2):
        for y in range(0, H, 2):
            m[z, y, :] = True                                  # a row
            if y + 2 < H:
                m[z, y + 1, W - 1 if (y // 2) % 2 == 0 else 0] = True   # its turn
        if z + 1 < D:
            m[z + 1, 0, 0] = True                              # the step to the next plane
    assert _check(m, cuda).tolist() == [1]


def test_lattice_maximises_the_count(cuda):
    m = np.zeros((33, 34, 67), bool)
    m[::2, ::2, ::2] = True
    ns = _check(m, cuda)
    assert int(ns[0]) == 17 * 17 * 34


def test_threshold_and_batches(cuda):
    rng = np.random.default_rng(5)
    v = rng.random((3, 2, 12, 20, 36)).astype(np.float32)
    ns = _check(v > np.float32(0.6), cuda, threshold=0.6, values=v)
    assert len(ns) == 6
    lab, n = ops.label_components(torch.from_numpy(v).to(cuda), 0.6)
    assert lab.shape == v.shape and lab.dtype == torch.int32 and n.shape == (3, 2)


def test_rejects_2d_and_cpu(cuda):
    with pytest.raises(Exception, match="3-D"):
        ops.label_components(torch.zeros((4, 4), device=cuda))
    with pytest.raises(Exception, match="CPU"):
        ops.label_components(torch.zeros((4, 4, 4)))
