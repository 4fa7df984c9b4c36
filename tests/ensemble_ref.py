"""fp64 numpy restatements of the ensemble and Gaussian-process kernels (csrc/ensemble.hip), this
project's own; tests/test_ensemble.py pins them to the real reference's fp64 intermediates
(tests/golden/ensemble_kernels.npz)."""
import numpy as np


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def layer_norm(x, gamma, beta, eps=1e-5):
    """(x^, xt = (x - mean) rstd, rstd): torch.nn.LayerNorm over the last axis (biased variance)."""
    x = _f64(x)
    mean = x.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x - mean) ** 2).mean(-1, keepdims=True) + eps)
    xt = (x - mean) * rstd
    return xt * _f64(gamma) + _f64(beta), xt, rstd


def gp_phi(x, W, b, weights, scale, gamma=None, beta=None, eps=1e-5):
    """(phi [N, r], logits [N, o]): phi = scale cos(b - x^ W^T), logits = phi weights^T."""
    xh = _f64(x) if gamma is None else layer_norm(x, gamma, beta, eps)[0]
    z = _f64(b).reshape(1, -1) - xh @ _f64(W).reshape(-1, xh.shape[1]).T
    phi = scale * np.cos(z)
    return phi, (None if weights is None else phi @ _f64(weights).T)


def gp_phi_bwd(x, W, b, weights, scale, dlogits, dphi, gamma=None, beta=None, eps=1e-5):
    """{"dx", "dgamma", "dbeta", "dweights"} from the gradients of logits and / or phi."""
    x, W2 = _f64(x), _f64(W).reshape(-1, np.shape(x)[1])
    if gamma is None:
        xh, xt, rstd = x, None, None
    else:
        xh, xt, rstd = layer_norm(x, gamma, beta, eps)
    z = _f64(b).reshape(1, -1) - xh @ W2.T
    phi = scale * np.cos(z)
    g = np.zeros_like(phi)
    out = {"dgamma": None, "dbeta": None, "dweights": None}
    if dlogits is not None:
        g = g + _f64(dlogits) @ _f64(weights)
        out["dweights"] = _f64(dlogits).T @ phi
    if dphi is not None:
        g = g + _f64(dphi)
    dxh = (scale * np.sin(z) * g) @ W2          # d cos(z) = -sin(z) dz and dz / dx^ = -W
    if gamma is None:
        out["dx"] = dxh
        return out
    out["dgamma"], out["dbeta"] = (dxh * xt).sum(0), dxh.sum(0)
    gg = dxh * _f64(gamma)
    out["dx"] = rstd * (gg - gg.mean(-1, keepdims=True) - xt * (gg * xt).mean(-1, keepdims=True))
    return out


def curvature(prob):
    """p (1 - p) of a vector, or its sum over the last axis of a matrix."""
    p = _f64(prob)
    c = p * (1.0 - p)
    return c if c.ndim == 1 else c.sum(-1)


def precision_update(P, phi, prob, use_momentum=False, m=0.999):
    """The new precision [r, r]: P + U, or m P + (1 - m) U, U = sum_n c_n phi_n phi_n^T."""
    phi = _f64(phi)
    U = np.einsum("n,ni,nj->ij", curvature(prob), phi, phi)
    P = _f64(P).reshape(U.shape)
    return m * P + (1.0 - m) * U if use_momentum else P + U


def covariance(P):
    P = _f64(P)
    return np.linalg.inv(P + 1e-6 * np.eye(P.shape[-1]))


def variance(phi, cov):
    phi = _f64(phi)
    return np.einsum("ni,ij,nj->n", phi, _f64(cov).reshape(phi.shape[1], phi.shape[1]), phi)


def sample(mean, var, eps):
    """(samples [S, N, o], mean over S, unbiased std over S; S = 1: NaN)."""
    s = _f64(mean)[None] + np.sqrt(np.maximum(_f64(var), 0.0))[None, :, None] * _f64(eps)
    with np.errstate(invalid="ignore", divide="ignore"):
        std = s.std(0, ddof=1) if s.shape[0] > 1 else np.full(s.shape[1:], np.nan)
    return s, s.mean(0), std


def pool(members):
    """(out [B, sum C], arg [B, sum C]): per member the maximum over the flattened space (lowest
    index on a tie: numpy's argmax), a vector copied; concatenated."""
    outs, args = [], []
    for m in members:
        m = _f64(m)
        flat = m.reshape(m.shape[0], m.shape[1], -1)
        a = flat.argmax(-1)
        outs.append(np.take_along_axis(flat, a[..., None], -1)[..., 0])
        args.append(a)
    return np.concatenate(outs, 1), np.concatenate(args, 1).astype(np.int32)


def pool_bwd(members, g):
    """The members' gradients: g scattered to the arg-max."""
    _, arg = pool(members)
    out, off = [], 0
    for m in members:
        C = m.shape[1]
        flat = np.zeros((m.shape[0], C, int(np.prod(m.shape[2:]))))
        np.put_along_axis(flat, arg[:, off:off + C, None].astype(np.int64),
                          _f64(g)[:, off:off + C, None], -1)
        out.append(flat.reshape(m.shape))
        off += C
    return out


def average(logits):
    """sigmoid (one column) or softmax over axis 1 of the members' mean."""
    mean = sum(_f64(x) for x in logits) / len(logits)
    if mean.shape[1] == 1:
        return 1.0 / (1.0 + np.exp(-mean))
    e = np.exp(mean - mean.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def average_bwd(logits, dy):
    """Every member's gradient (they are equal)."""
    y, dy = average(logits), _f64(dy)
    dm = y * (1.0 - y) * dy if y.shape[1] == 1 else y * (dy - (y * dy).sum(1, keepdims=True))
    return dm / len(logits)
