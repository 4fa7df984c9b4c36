"""fp64 restatement of torch's ``_SpectralNorm`` forward and of its gradient, in numpy. ``u`` and
``v`` are rounded to fp32 where torch stores them (its buffers), and the rounded values are what every
later product uses."""
import numpy as np


def to_matrix(w, dim):
    """[h, outer * inner] with ``dim`` in front (a copy)."""
    w = np.moveaxis(np.asarray(w), dim, 0)
    return w.reshape(w.shape[0], -1)


def from_matrix(m, shape, dim):
    rest = [s for i, s in enumerate(shape) if i != dim]
    return np.moveaxis(m.reshape([shape[dim]] + rest), 0, dim)


def normalize(x, eps):
    return x / max(float(np.sqrt(np.sum(x * x))), eps)


def forward(W, u, v, n, eps, dim, training):
    """(W_sn fp64, u fp32, v fp32, sigma fp64) of one access."""
    M = to_matrix(W, dim).astype(np.float64)
    u = np.asarray(u, dtype=np.float32).copy()
    v = np.asarray(v, dtype=np.float32).copy()
    if training:
        for _ in range(n):
            u = normalize(M @ v.astype(np.float64), eps).astype(np.float32)
            v = normalize(M.T @ u.astype(np.float64), eps).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        sigma = float(u.astype(np.float64) @ (M @ v.astype(np.float64)))
        return np.asarray(W, dtype=np.float64) / sigma, u, v, sigma


def backward(G, W_sn, u, v, sigma, dim):
    """dL/dW = (G - <G, W_sn> u v^T) / sigma with u and v as constants, in the weight's layout."""
    G = np.asarray(G, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = float(np.sum(G * W_sn))
        outer = np.outer(u.astype(np.float64), v.astype(np.float64))
        return (G - s * from_matrix(outer, G.shape, dim)) / sigma
