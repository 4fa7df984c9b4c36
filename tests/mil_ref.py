"""fp64 numpy restatements of the kernels of csrc/mil.hip, forward and backward: the volume-to-slices
copy, the gated-attention pooling and the slice tokens. tests/test_mil.py pins them to the reference's
recorded intermediates (tests/golden/mil_step_*.npz); tests/test_mil_gpu.py checks the kernels against
them."""
import numpy as np


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def volume_to_slices(x):
    """[B, C, H, W, S] -> [B * S, C, H, W] ("b c h w s -> (b s) c h w")."""
    x = np.asarray(x)
    B, C, H, W, S = x.shape
    return np.ascontiguousarray(x.transpose(0, 4, 1, 2, 3)).reshape(B * S, C, H, W)


def slices_to_volume(y, S):
    y = np.asarray(y)
    BS, C, H, W = y.shape
    return np.ascontiguousarray(y.reshape(BS // S, S, C, H, W).transpose(0, 2, 3, 4, 1))


def sigmoid(x):
    x = _f64(x)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def softmax(x, axis):
    x = _f64(x)
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def attention(hv, hu, w, b):
    """(A [B, S, 1], gate [B, S, N]) with score = sum_n w tanh(hv) sigmoid(hu) + b."""
    hv, hu, w, b = _f64(hv), _f64(hu), _f64(w).reshape(-1), _f64(b).reshape(-1)
    gate = np.tanh(hv) * sigmoid(hu)
    score = gate @ w + b[0]
    return softmax(score, 1)[..., None], gate


def products(feat, A, mode):
    """What is reduced over the slices: feat A, or softmax_F(feat) A."""
    feat = _f64(feat)
    return (softmax(feat, -1) if mode == "vocabulary" else feat) * A


def pool(feat, A, mode):
    """(pooled [B, F], arg-max [B, F] for "max" else None); A [B, S, 1]."""
    prod = products(feat, _f64(A), mode)
    if mode == "max":
        return prod.max(1), prod.argmax(1)      # numpy's argmax: the first maximal index
    return prod.sum(1), None


def gated_pool(feat, hv=None, hu=None, w=None, b=None, mode="mean"):
    """(pooled, A, arg); without gate inputs A = 1 / S."""
    lead = feat if feat is not None else hv
    B, S = lead.shape[:2]
    A = np.full((B, S, 1), 1.0 / S) if hv is None else attention(hv, hu, w, b)[0]
    if feat is None:
        return None, A, None
    pooled, arg = pool(feat, A, mode)
    return pooled, A, arg


def gated_pool_bwd(feat, hv, hu, w, b, mode, g, gA=None):
    """dict of dfeat, dhv, dhu, dw, db and dscore [B, S, 1] (the gate's only with gate inputs) from the gradient g [B, F]
    of pooled and gA [B, S, 1] (or None) of A."""
    feat, g = _f64(feat), _f64(g)
    pooled, A, arg = gated_pool(feat, hv, hu, w, b, mode)
    out = {}
    dA = np.zeros_like(A) if gA is None else _f64(gA).reshape(A.shape).copy()
    if feat is not None:
        B, S, F = feat.shape
        if mode == "mean":
            out["dfeat"] = g[:, None, :] * A
            dA += (g[:, None, :] * feat).sum(-1, keepdims=True)
        elif mode == "max":
            hit = arg[:, None, :] == np.arange(S)[None, :, None]
            out["dfeat"] = np.where(hit, g[:, None, :] * A, 0.0)
            dA += np.where(hit, g[:, None, :] * feat, 0.0).sum(-1, keepdims=True)
        else:
            p = softmax(feat, -1)
            q = (g[:, None, :] * p).sum(-1, keepdims=True)
            out["dfeat"] = p * A * (g[:, None, :] - q)
            dA += q
    if hv is None:
        return out
    hv, hu, w = _f64(hv), _f64(hu), _f64(w).reshape(-1)
    dscore = A * (dA - (A * dA).sum(1, keepdims=True))          # [B, S, 1]
    t, sg = np.tanh(hv), sigmoid(hu)
    out["dhv"] = dscore * w * sg * (1.0 - t * t)
    out["dhu"] = dscore * w * t * sg * (1.0 - sg)
    out["dw"] = (dscore * t * sg).sum((0, 1))
    out["db"] = dscore.sum().reshape(1)
    out["dscore"] = dscore
    return out


def slice_tokens(x, pos=None, class_token=None):
    """[B, S (+ 1), E]: row 0 the class token, row (1 +) s = x[b, s] + pos[s]."""
    x = np.asarray(x)
    out = x if pos is None else x + np.asarray(pos).reshape(1, -1, 1)
    if class_token is not None:
        ct = np.broadcast_to(np.asarray(class_token).reshape(1, 1, -1), (x.shape[0], 1, x.shape[2]))
        out = np.concatenate([ct, out], 1)
    return out


def slice_tokens_bwd(dout, has_class_token):
    """(dx, dpos [1, S, 1], dclass_token [1, 1, E] or None)."""
    dout = _f64(dout)
    ct = int(bool(has_class_token))
    dx = dout[:, ct:]
    dpos = dx.sum((0, 2)).reshape(1, -1, 1)
    dcls = dout[:, :1].sum(0, keepdims=True) if ct else None
    return dx, dpos, dcls
