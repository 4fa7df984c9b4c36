"""fp64 restatements of the batch-ensemble arithmetic in plain torch (test infrastructure): the three
kernels' results and gradients, and the four forward modes of the layers around a given body.
Pinned to the real reference by tests/test_batch_ensemble.py (tests/golden/batch_ensemble_layers.npz)."""
import numpy as np
import torch


def _t(a):
    return a.detach().double().cpu() if isinstance(a, torch.Tensor) else torch.as_tensor(
        np.asarray(a), dtype=torch.float64)


def _rows(table, x):
    """[B or K B, C] rows as [., C, 1, ...] against ``x``."""
    return table.reshape(table.shape + (1,) * (x.dim() - 2))


def wrap(idx, n):
    """Host indices as torch indexing reads them: negative entries wrap; out of range raises."""
    idx = np.asarray(idx, dtype=np.int64)
    if ((idx < -n) | (idx >= n)).any():
        raise IndexError("index out of range")
    return np.where(idx < 0, idx + n, idx)


def be_scale(x, table, idx=None):
    """y[b] = x[b] table[idx[b]]; ``idx`` None: row 0 for every item."""
    x, table = _t(x), _t(table)
    idx = np.zeros(x.shape[0], dtype=np.int64) if idx is None else wrap(idx, table.shape[0])
    return x * _rows(table[idx], x)


def be_scale_backward(x, table, idx, dy):
    """(dx, dtable): dtable[m] sums dy x over the voxels of the items that drew m; others 0."""
    x, table, dy = _t(x), _t(table), _t(dy)
    idx = np.zeros(x.shape[0], dtype=np.int64) if idx is None else wrap(idx, table.shape[0])
    dx = dy * _rows(table[idx], x)
    per_item = (dy * x).flatten(2).sum(-1) if x.dim() > 2 else dy * x
    dtable = torch.zeros_like(table)
    for b, m in enumerate(idx):
        dtable[m] += per_item[b]
    return dx, dtable


def _expand(x, pre, m0, m1):
    return torch.cat([x * _rows(pre[m][None], x) for m in range(m0, m1)])


def _mean(y, post, m0, m1, n, acc):
    B = y.shape[0] // (m1 - m0)
    out = torch.zeros_like(y[:B]) if acc is None else acc
    for m in range(m0, m1):
        out = out + y[(m - m0) * B:(m - m0 + 1) * B] * _rows(post[m][None], y)
    return out / n if m1 == n else out


def members_expand(x, pre, m0, m1):
    """out[(m - m0) B + b] = x[b] pre[m] for m0 <= m < m1."""
    return _expand(_t(x), _t(pre), m0, m1)


def members_mean(y, post, m0, m1, n, acc=None):
    """acc + sum_m post[m] y[(m - m0) B + b], divided by n in the call whose m1 == n."""
    return _mean(_t(y), _t(post), m0, m1, n, None if acc is None else _t(acc))


def members_expand_backward(x, pre, m0, m1, dy):
    """(dx, dpre [n, C]) of ``members_expand``."""
    x, pre = _t(x).requires_grad_(True), _t(pre).requires_grad_(True)
    (_expand(x, pre, m0, m1) * _t(dy)).sum().backward()
    return x.grad, pre.grad


def members_mean_backward(y, post, m0, m1, n, dout, acc=None):
    """(dy, dpost [n, C], dacc or None) of ``members_mean``."""
    y, post = _t(y).requires_grad_(True), _t(post).requires_grad_(True)
    acc = None if acc is None else _t(acc).requires_grad_(True)
    (_mean(y, post, m0, m1, n, acc) * _t(dout)).sum().backward()
    return y.grad, post.grad, None if acc is None else acc.grad


def layer_forward(x, pre, post, mod, training, idx=None, drawn=None):
    """The four modes of batch_ensemble.py around ``mod`` (a callable on fp64 tensors), on tensors that
    may carry autograd. ``idx``: an int or one member per item; ``drawn``: the members a training
    forward drew; neither: the mean over all members."""
    n = pre.shape[0]
    if idx is not None or training:
        if idx is None:
            members = wrap(drawn, n)
        elif isinstance(idx, int):
            members = wrap([idx] * x.shape[0], n)
        else:
            members = wrap(idx, n)
        h = mod(x * _rows(pre[members], x))
        return h * _rows(post[members], h)
    outs = []
    for m in range(n):
        h = mod(x * _rows(pre[m][None], x))
        outs.append(h * _rows(post[m][None], h))
    return torch.stack(outs).mean(0)
