"""fp64 restatements of the semi-supervised losses, in the tests' own words (torch on the CPU, autograd
for the gradients), used where no fixture fits: sizes spanning several blocks, NaN inputs, the cosine
with a zero vector. tests/test_semisl_losses.py holds them against the fixtures of the real reference.

The cosine is the installed torch's ``F.cosine_similarity(a, b, dim, eps=1e-8)`` restated:
``sum(a b) / (max(|a|, eps) max(|b|, eps))``, each norm clamped on its own, so a zero vector has
cosine 0 with everything and passes the gradient ``b / (eps max(|b|, eps))``."""
import torch

COS_EPS = 1e-8


def cosine(a, b, dim):
    # (vector_norm, whose gradient at a zero vector is 0 where sqrt's would be infinite)
    na = torch.linalg.vector_norm(a, 2, dim, keepdim=True).clamp_min(COS_EPS)
    nb = torch.linalg.vector_norm(b, 2, dim, keepdim=True).clamp_min(COS_EPS)
    return ((a / na) * (b / nb)).sum(dim)


def _f64(t):
    return t.detach().cpu().double()


def anchor_loss(x, a1, a2, temperature):
    """[B] fp64: sum_v (xlogy(q, q) - q p), p / q the softmax over an item's voxels of the cosines / T
    with the first / second anchors (kl_div with a probability as its input, as the reference)."""
    x, a1, a2 = x.flatten(2), a1.flatten(2), a2.flatten(2)
    p = torch.softmax(cosine(x, a1, 1) / temperature, 1)
    q = torch.softmax(cosine(x, a2, 1) / temperature, 1)
    return (torch.xlogy(q, q) - q * p).sum(-1)


def anchor_loss_and_grads(x, a1, a2, r, temperature, anchor_grad=True):
    """(loss [B], dx, da1, da2) in fp64 of fp32 tensors, for the objective sum(loss r)."""
    x, a1, a2 = (_f64(t).requires_grad_(True) for t in (x, a1, a2))
    loss = anchor_loss(x, a1, a2, temperature)
    (loss * _f64(r)).sum().backward()
    return loss.detach(), x.grad, a1.grad if anchor_grad else None, a2.grad if anchor_grad else None


def nn_loss(x, y, past, past_class, temperature, chunk=4096):
    """0-d fp64: the mean over the voxels whose ratio is not NaN of S / O (a NaN term counting 0 in
    either sum), walked in chunks of voxels so that the [chunk, Q] products stay small."""
    B, C = x.shape[:2]
    rows = x.flatten(2).permute(0, 2, 1).reshape(-1, C)
    K = y.shape[1]
    labels = y.flatten(2).permute(0, 2, 1).reshape(-1, K)
    ratios = []
    for at in range(0, rows.shape[0], chunk):
        xs, ys = rows[at:at + chunk], labels[at:at + chunk]
        d = 1 - cosine(xs[:, None, :], past[None, :, :], -1)
        m = ys[:, past_class.long()]
        same = torch.exp(-d * m / temperature).nansum(-1)
        other = torch.exp(-d * (1 - m) / temperature).nansum(-1)
        ratios.append(same / other)
    return torch.nanmean(torch.cat(ratios))


def nn_loss_and_grad(x, y, past, past_class, temperature):
    x = _f64(x).requires_grad_(True)
    loss = nn_loss(x, _f64(y), _f64(past), past_class.detach().cpu(), temperature)
    loss.backward()
    return loss.detach(), x.grad


def pseudo_label_ce(pred, proba, threshold, weight=None, label_smoothing=0.0, reduction="mean"):
    """fp64: -sum_k w_k t_k log_softmax_k per voxel with t = (proba > threshold) (1 - ls) + ls / K, the
    comparison made in fp32 as torch compares an fp32 tensor with a number; "mean" divides by B V."""
    K = pred.shape[1]
    t = (proba.float() > threshold).to(pred.dtype) * (1 - label_smoothing) + label_smoothing / K
    shape = [1, K] + [1] * (pred.dim() - 2)
    w = torch.ones(K, dtype=pred.dtype) if weight is None else torch.as_tensor(weight, dtype=pred.dtype)
    per_voxel = -(w.reshape(shape) * t * torch.log_softmax(pred, 1)).sum(1)
    if reduction == "none":
        return per_voxel
    return per_voxel.sum() if reduction == "sum" else per_voxel.sum() / per_voxel.numel()


def pseudo_label_ce_and_grad(pred, proba, threshold, **kw):
    pred = _f64(pred).requires_grad_(True)
    loss = pseudo_label_ce(pred, proba.detach().cpu(), threshold, **kw)
    loss.backward()
    return loss.detach(), pred.grad
