"""fp64 restatements for the deconfounded-classification tests, in the tests' own words (torch on the
CPU, autograd for the gradients).

The correlation loss is the wrapper's expression (pl.py:2396-2407) with ONE rule of its own: the
gradient of ``sqrt`` at an exactly zero argument is taken as 0. The reference's ``sqrt`` has an
infinite derivative there, which makes the gradient of a feature column that is constant over the
batch NaN (a dead ReLU channel after the global max-pool; from there the NaN reaches every parameter
of the extractor: tools/make_deconfounded_golden.py checks and prints it). With the rule such a column
has ``r = 0`` with every partner and an exact 0 gradient; wherever the reference's gradient is finite
the two agree. For ``0 < |a| |b| < 1e-8`` the expression is followed as written: the denominator is
the constant 1e-8 and the gradient flows through the numerator only. Clamp gradients are torch's
(passed where ``min <= x <= max``)."""
import numpy as np
import torch


class _Sqrt0(torch.autograd.Function):
    """sqrt whose derivative at exactly 0 is 0."""

    @staticmethod
    def forward(ctx, x):
        y = x.sqrt()
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return torch.where(y > 0, g / (2 * torch.where(y > 0, y, torch.ones_like(y))),
                           torch.zeros_like(g))


def correlation_loss(features, n_conf, sqrt=_Sqrt0.apply):
    """The loss as a 0-d fp64 tensor of ``features`` (an fp64 tensor, possibly requiring a gradient).
    ``sqrt=torch.sqrt`` is the reference's expression to the letter."""
    conf_f = features[:, :n_conf, None]
    deconf_f = features[:, None, n_conf:]
    conf_f_norm = conf_f - conf_f.mean(0, keepdim=True)
    deconf_f_norm = deconf_f - deconf_f.mean(0, keepdim=True)
    n = (conf_f_norm * deconf_f_norm).sum(0)
    d = torch.multiply(sqrt(conf_f_norm.square().sum(0)),
                       sqrt(deconf_f_norm.square().sum(0))).clamp(min=1e-8)
    return torch.clamp(n / d, -1.0, 1.0).square().mean()


def correlation_loss_and_grad(x, n_conf, sqrt=_Sqrt0.apply):
    """(loss, gradient [B, F]) in fp64 from an array."""
    t = torch.from_numpy(np.asarray(x, dtype=np.float64)).requires_grad_(True)
    loss = correlation_loss(t, n_conf, sqrt)
    loss.backward()
    return float(loss.detach()), t.grad.numpy()


def _cross_entropy(z, y):
    """Mean cross entropy of logits [B, K] against labels [B]; an item whose label is outside
    [0, K) is NaN, and so are the mean and the item's gradient; the label is never used as an
    index."""
    K = z.shape[1]
    ok = (y >= 0) & (y < K)
    lse = torch.logsumexp(z, 1)
    picked = z.gather(1, torch.where(ok, y, torch.zeros_like(y))[:, None])[:, 0]
    item = (lse - picked) * torch.where(ok, torch.ones_like(lse), torch.full_like(lse, float("nan")))
    return item.mean()


def heads_losses(x, n_conf, cat, labels, cont, target, conf_mult=1.0):
    """``(cat_loss | None, cont_loss | None, grads)`` in fp64: ``cat`` a list of ``(W, b)`` arrays,
    ``labels`` int64 [H, B], ``cont`` ``(W, b)`` or None with ``target`` [B, n_cont]. ``grads``:
    ``{"x": [B, F], "W0": ..., "b0": ..., "Wc": ..., "bc": ...}`` of ``cat_loss + cont_loss``
    (upstream gradients ``g_cat`` / ``g_cont`` = 1)."""
    as64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64)).requires_grad_(True)  # noqa: E731
    xt = as64(x)
    conf = xt[:, :n_conf]
    leaves, cat_loss, cont_loss = {"x": xt}, None, None
    if cat:
        total = 0.0
        for h, (W, b) in enumerate(cat):
            Wt, bt = as64(W), as64(b)
            leaves[f"W{h}"], leaves[f"b{h}"] = Wt, bt
            total = total + _cross_entropy(conf @ Wt.T + bt, torch.from_numpy(labels[h])) / len(cat)
        cat_loss = total * conf_mult
    if cont is not None:
        Wt, bt = as64(cont[0]), as64(cont[1])
        leaves["Wc"], leaves["bc"] = Wt, bt
        pred = conf @ Wt.T + bt
        cont_loss = (pred - torch.from_numpy(np.asarray(target, dtype=np.float64))).square().mean() \
            * conf_mult
    sum(v for v in (cat_loss, cont_loss) if v is not None).backward()
    grads = {k: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape)))
             for k, v in leaves.items()}
    return (None if cat_loss is None else float(cat_loss.detach()),
            None if cont_loss is None else float(cont_loss.detach()), grads)


def rel(got, ref):
    """The largest difference over the largest reference magnitude (the SUM_BOUND metric)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-300))
