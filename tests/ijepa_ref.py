"""fp64 torch restatement of what csrc/ijepa.hip computes and of the part of I-JEPA's training step
that follows the encoders (adell_mri/modules/self_supervised/jepa.py, ``IJEPAPL.step``): plain
indexing, ``cat``, ``expand``, ``layer_norm`` and ``SmoothL1Loss``. tests/test_ijepa.py pins it to the
reference's own results in tests/golden/ijepa_step.npz; the GPU tests compare the kernels to it."""
import numpy as np
import torch
import torch.nn.functional as F


def _d(t):
    return torch.as_tensor(np.asarray(t) if not isinstance(t, torch.Tensor) else t).double()


def _idx(rows):
    return torch.as_tensor(np.asarray(rows).astype(np.int64))


def gather(x, rows):
    """x[:, rows]"""
    return _d(x)[:, _idx(rows)]


def predictor_input(e, pos, mask, ctx, tgt):
    """IJEPAPredictor.forward between ``predictor_embed_`` and ``predictor_``."""
    e, pos, mask = _d(e), _d(pos), _d(mask)
    x = e + pos[:, _idx(ctx), :]
    mask_tokens = (mask + pos[:, _idx(tgt), :]).expand(e.shape[0], -1, -1)
    return torch.cat([x, mask_tokens], dim=1)


def targets(h, rows):
    """``layer_norm(h)[:, rows]`` for each row set (the rows carry the ``skip_n`` offset)."""
    h = _d(h)
    h = F.layer_norm(h, (h.shape[-1],))
    return [h[:, _idx(r)] for r in rows]


def block_loss(pred, h, rows):
    """SmoothL1Loss()(pred, layer_norm(h, (E,))[:, rows])"""
    return torch.nn.SmoothL1Loss()(_d(pred), targets(h, [rows])[0])


def step_loss(predictions, h, rows):
    """``IJEPAPL.calculate_loss`` on the predictions and the targets ``forward_training`` takes
    from the teacher's raw output h."""
    return torch.stack([torch.nn.SmoothL1Loss()(_d(p), t)
                        for p, t in zip(predictions, targets(h, rows))]).mean()


def sample_mask_indices(masker, n_patches, n_masked_patches):
    """``IJEPA._sample_mask_indices`` on a masker: context blocks first, then the target blocks."""
    context_coords = masker.sample_patches(n_patches)
    context_idx = np.unique(np.concatenate(
        [masker.retrieve_patch(c) for c in context_coords])).astype(np.int64)
    target_coords = masker.sample_patches(n_masked_patches)
    target_idx = [np.setdiff1d(masker.retrieve_patch(c).astype(np.int64), context_idx)
                  for c in target_coords]
    return context_idx, target_idx      # empty blocks NOT dropped: the caller sees which were
