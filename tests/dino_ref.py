"""Plain-torch restatement of the DINO loss (both teacher modes), the centre update and the head,
evaluated in whatever dtype the inputs carry (the tests feed fp64). Pinned to the reference by
tests/golden/dino_loss.npz (tests/test_dino.py); the reference for shapes too large to store."""
import torch


def sk_scores(x, t2, iterations=3, world_size=1):
    """DinoLoss.sinkhorn_knopp_teacher (losses/dino.py:156-193), one rank."""
    x = x.flatten(end_dim=-2)
    Q = torch.exp(x / t2).t()
    B = Q.shape[1] * world_size
    K = Q.shape[0]
    Q = Q / Q.sum()
    for _ in range(iterations):
        Q = Q / Q.sum(dim=1, keepdim=True)
        Q = Q / K
        Q = Q / Q.sum(dim=0, keepdim=True)
        Q = Q / B
    return (Q * B).t()


def teacher_scores(b, centers, t2, method="center", sk_iterations=3):
    if method == "center":
        return torch.softmax((b - centers) / t2, dim=-1)
    return sk_scores(b.detach(), t2, sk_iterations)


def dino_loss(a, b, centers, t1, t2, method="center", sk_iterations=3):
    """DinoLoss.forward (losses/dino.py:195-217)."""
    p_t = teacher_scores(b, centers, t2, method, sk_iterations).flatten(end_dim=-2)
    log_s = torch.log_softmax(a / t1, dim=-1).flatten(end_dim=-2)
    return (p_t * log_s).sum(-1).neg().mean()


def center_sum(x):
    if x.dim() > 2:
        x = x.flatten(end_dim=-2)
    return x.sum(0, keepdim=True), len(x)


def center_apply(centers, batch_sum, rows, m, world_size=1):
    """DinoLoss.apply_center_update (losses/dino.py:77-98)."""
    return centers * m + batch_sum.reshape(-1) / (rows * world_size) * (1 - m)


def l2_normalize(x, eps=1e-12):
    return x / x.norm(2, dim=-1, keepdim=True).clamp_min(eps)


def weight_norm_linear(x, g, v):
    """Linear under torch's weight_norm (dim 0): weight = g * v / ||v_row||."""
    w = g.reshape(-1, 1) * v / v.norm(2, dim=1, keepdim=True)
    return x @ w.t()
