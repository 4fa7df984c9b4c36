"""StepRunner(gradient_clip_val, gradient_clip_algorithm, accumulate_grad_batches): Lightning's
argument checks (entrypoints/segmentation/train.py:807,811; assemble_args.py:386-392), on a
CPU-resident model -- nothing is launched before they raise."""
import pytest
import torch

from adell_mri_amd.trainer import StepRunner


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(4))

    def training_step(self, batch, idx):
        return (self.w * batch).sum()


def test_negative_clip_value_raises():
    with pytest.raises(ValueError, match="gradient_clip_val"):
        StepRunner(_Tiny(), torch.optim.SGD(_Tiny().parameters(), lr=0.1), gradient_clip_val=-1.0)


@pytest.mark.parametrize("n", [0, -2, 1.5])
def test_accumulate_grad_batches_below_one_raises(n):
    with pytest.raises(ValueError, match="accumulate_grad_batches"):
        StepRunner(_Tiny(), torch.optim.SGD(_Tiny().parameters(), lr=0.1), accumulate_grad_batches=n)


def test_clip_by_value_is_not_implemented():
    with pytest.raises(NotImplementedError, match="value"):
        StepRunner(_Tiny(), torch.optim.SGD(_Tiny().parameters(), lr=0.1), gradient_clip_val=1.0,
                   gradient_clip_algorithm="value")
    with pytest.raises(ValueError):
        StepRunner(_Tiny(), torch.optim.SGD(_Tiny().parameters(), lr=0.1), gradient_clip_val=1.0,
                   gradient_clip_algorithm="bogus")


def test_clipping_and_accumulation_need_a_fused_optimizer():
    m = _Tiny()
    with pytest.raises(TypeError, match="fused"):
        StepRunner(m, torch.optim.SGD(m.parameters(), lr=0.1), gradient_clip_val=1.0)
    with pytest.raises(TypeError, match="fused"):
        StepRunner(m, torch.optim.SGD(m.parameters(), lr=0.1), accumulate_grad_batches=2)


def test_defaults_and_off_values_keep_todays_runner():
    m = _Tiny()
    for off in (None, 0, 0.0):
        r = StepRunner(m, torch.optim.SGD(m.parameters(), lr=0.1), gradient_clip_val=off)
        assert r.gradient_clip_val is None and r.accumulate_grad_batches == 1
        assert r.optimizer_steps == 0 and r.step_idx == 0 and r.last_grad_norm is None
        assert not r.flush()
