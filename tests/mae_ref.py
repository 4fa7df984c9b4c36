"""fp64 torch restatement of what csrc/mae.hip computes and of the masked autoencoder's plumbing
(adell_mri/modules/self_supervised/autoencoders.py: ``random_masking``, the un-shuffle of
``ViTMaskedAutoEncoder.forward``, its view / permute "image", ``MSELoss``): plain ``argsort``,
``gather``, ``repeat``, ``cat``. tests/test_mae.py pins it to the reference's own results in
tests/golden/mae_step.npz; the GPU tests compare the kernels to it."""
import numpy as np
import torch


def _d(t):
    return torch.as_tensor(np.asarray(t) if not isinstance(t, torch.Tensor) else t).double()


def _idx(ids):
    return torch.as_tensor(np.asarray(ids).astype(np.int64))


def len_keep(L, mask_ratio):
    return int(L * (1 - mask_ratio))


def masking_ids(noise, mask_ratio):
    """(ids_shuffle, ids_restore, mask) of ``random_masking`` for the noise [N, L] it drew."""
    noise = torch.as_tensor(np.asarray(noise))
    N, L = noise.shape
    ids_shuffle = torch.argsort(noise, dim=1, stable=True)
    ids_restore = torch.argsort(ids_shuffle, dim=1, stable=True)
    mask = torch.ones([N, L])
    mask[:, :len_keep(L, mask_ratio)] = 0
    return ids_shuffle.numpy(), ids_restore.numpy(), torch.gather(mask, 1, ids_restore).numpy()


def keep(x, ids_shuffle, K):
    """torch.gather(x, 1, ids_keep) with ids_keep = ids_shuffle[:, :K]"""
    x = _d(x)
    ids_keep = _idx(ids_shuffle)[:, :K]
    return torch.gather(x, 1, ids_keep.unsqueeze(-1).repeat(1, 1, x.shape[2]))


def restore(enc, mask_token, scale, pos, ids_shuffle):
    """``ViTMaskedAutoEncoder.forward`` between the encoder and the decoder."""
    enc, mask_token, scale, pos = _d(enc), _d(mask_token), _d(scale), _d(pos)
    ids_restore = torch.argsort(_idx(ids_shuffle), dim=1, stable=True)
    mask_tokens = scale * mask_token.reshape(1, 1, -1).repeat(
        enc.shape[0], ids_restore.shape[1] - enc.shape[1], 1)
    full = torch.cat([enc, mask_tokens], dim=1)
    out = torch.gather(full, 1, ids_restore.unsqueeze(-1).expand(-1, -1, full.shape[2]))
    return out + pos


def to_image(pred, image_shape):
    """pred [B, L, P * C] -> view(B, L, P, C).permute(0, 3, 1, 2).view(B, C, H, W): the patch axes
    ph, pw of the reference's five-axis view stay adjacent and in order, so they are one axis here."""
    B, C, H, W = image_shape
    L = pred.shape[1]
    return pred.reshape(B, L, -1, C).permute(0, 3, 1, 2).contiguous().view(B, C, H, W)


def loss(pred, x):
    """MSELoss()(image(pred), x) over the whole image."""
    x = _d(x)
    return torch.nn.MSELoss()(to_image(_d(pred), tuple(x.shape)), x)
