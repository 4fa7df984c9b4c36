"""fp64 numpy restatement of every kernel of csrc/diffusion.hip: what the GPU tests compare against,
and what tests/test_diffusion.py pins to the recorded outputs of the real reference
(tools/make_diffusion_golden.py) at fp64 round-off."""
import math

import numpy as np

STEP_KINDS = ("ddpm", "ddim", "alpha_deblending")


def timestep_embedding(t, channels, max_period=10000):
    """``get_timestep_embedding``: t [G] -> [G, channels]; cos half, sin half, zero pad."""
    t = np.asarray(t, np.float64).reshape(-1)
    half = channels // 2
    k = np.arange(half, dtype=np.float64)
    freqs = np.exp(-math.log(max_period) * k / max(half, 1))
    args = t[:, None] * freqs[None, :]
    emb = np.concatenate([np.cos(args), np.sin(args)], -1)
    if channels % 2 == 1:
        emb = np.pad(emb, ((0, 0), (0, 1)))
    return emb


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def silu(x):
    return x * sigmoid(x)


def silu_grad(x):
    s = sigmoid(x)
    return s * (1.0 + x * (1.0 - s))


PARAM_KEYS = ("class_to_channels.weight", "class_to_channels.bias", "op.1.weight", "op.1.bias",
              "op.2.weight", "op.2.bias", "op.4.weight", "op.4.bias")


def eca_gates(emb, p, eps=1e-5):
    """Pre-sigmoid logits [G, C] of one site from the embedding rows [G, T]; ``p``: the eight
    parameters in PARAM_KEYS order. Also returns what the backward needs."""
    w0, b0, w1, b1, lg, lb, w2, b2 = (np.asarray(v, np.float64) for v in p)
    h0 = emb @ w0.T + b0
    a0 = silu(h0)
    h1 = a0 @ w1.T + b1
    mean = h1.mean(-1, keepdims=True)
    var = ((h1 - mean) ** 2).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = (h1 - mean) * rstd
    h2 = xhat * lg + lb
    a2 = silu(h2)
    z = a2 @ w2.T + b2
    return z, (emb, h0, a0, xhat, rstd, h2, a2)


def eca_gates_backward(gz, p, saved):
    """(the eight parameter gradients, the gradient of the embedding rows)."""
    w0, b0, w1, b1, lg, lb, w2, b2 = (np.asarray(v, np.float64) for v in p)
    emb, h0, a0, xhat, rstd, h2, a2 = saved
    gz = np.asarray(gz, np.float64)
    dw2, db2 = gz.T @ a2, gz.sum(0)
    dh2 = (gz @ w2) * silu_grad(h2)
    dlg, dlb = (dh2 * xhat).sum(0), dh2.sum(0)
    dxh = dh2 * lg
    dh1 = rstd * (dxh - dxh.mean(-1, keepdims=True) - xhat * (dxh * xhat).mean(-1, keepdims=True))
    dw1, db1 = dh1.T @ a0, dh1.sum(0)
    dh0 = (dh1 @ w1) * silu_grad(h0)
    dw0, db0 = dh0.T @ emb, dh0.sum(0)
    return (dw0, db0, dw1, db1, dlg, dlb, dw2, db2), dh0 @ w0


def eca_apply(x, z):
    """x [N, C, *spatial] times sigmoid(z [Ng, C]), Ng in {1, N}."""
    x = np.asarray(x, np.float64)
    s = sigmoid(np.asarray(z, np.float64))
    return x * s.reshape(s.shape + (1,) * (x.ndim - 2))


def eca_apply_backward(x, z, dy):
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    s = sigmoid(np.asarray(z, np.float64))
    dx = dy * s.reshape(s.shape + (1,) * (x.ndim - 2))
    ds = (dy * x).reshape(x.shape[0], x.shape[1], -1).sum(-1)
    if s.shape[0] == 1:
        ds = ds.sum(0, keepdims=True)
    return dx, ds * s * (1.0 - s)


def noise_images(x, eps, alpha_bar, t):
    """Items whose t is outside the table are NaN."""
    x, eps = np.asarray(x, np.float64), np.asarray(eps, np.float64)
    ab = np.asarray(alpha_bar, np.float64)
    t = np.asarray(t).reshape(-1)
    ok = (t >= 0) & (t < ab.shape[0])
    a = np.where(ok, ab[np.where(ok, t, 0)], np.nan).reshape((-1,) + (1,) * (x.ndim - 1))
    return np.sqrt(a) * x + np.sqrt(1.0 - a) * eps


def reverse_step(kind, x, eps, t, tables, noise=None, eps_uncond=None, scale=0.0, eta=1.0, clip=True):
    """``ddpm_reverse_step`` / ``ddim_reverse_step`` / ``alpha_deblending_step`` in fp64, the guidance
    blend in front. ``tables``: "beta", "alpha", "alpha_bar"."""
    x, e = np.asarray(x, np.float64), np.asarray(eps, np.float64)
    if eps_uncond is not None:
        u = np.asarray(eps_uncond, np.float64)
        e = u + scale * (e - u)
    ab = float(tables["alpha_bar"][t])
    abp = float(tables["alpha_bar"][t - 1]) if t > 0 else 1.0
    beta, alpha = float(tables["beta"][t]), float(tables["alpha"][t])
    if kind == "ddpm":
        bb = 1.0 - ab
        x0 = (x - math.sqrt(bb) * e) / math.sqrt(ab)
        if clip:
            x0 = np.clip(x0, -1.0, 1.0)
        out = math.sqrt(abp) * beta / bb * x0 + math.sqrt(alpha) * (1.0 - abp) / bb * x
        if t > 0 and eta > 0:
            out = out + np.asarray(noise, np.float64) * math.sqrt((1.0 - abp) / (1.0 - ab) * beta) * eta
        return out
    if kind == "ddim":
        var = math.sqrt((1.0 - abp) / (1.0 - ab)) * math.sqrt(1.0 - ab / abp) * eta
        x0 = (x - math.sqrt(1.0 - ab) * e) / math.sqrt(ab)
        out = math.sqrt(abp) * x0 + math.sqrt(max(1.0 - abp - var ** 2, 0.0)) * e
        if var != 0.0:
            out = out + np.asarray(noise, np.float64) * var
        return out
    if kind == "alpha_deblending":
        return x + (ab - abp) * e
    raise ValueError(kind)


def mse(pred, target):
    d = np.asarray(pred, np.float64) - np.asarray(target, np.float64)
    return float((d * d).mean()), 2.0 * d / d.size
