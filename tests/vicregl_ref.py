"""Plain-torch restatement of the local VICReg loss (VICRegLocalLoss of the reference,
self_supervised/losses/vicreg.py:168-404) for the tests, written from its description: it runs in
the dtype of its inputs (fp64 for references, fp32 on a device for timings) and needs nothing but
torch.

What it keeps of the reference, as written: the gamma LARGEST entries of each T x T distance matrix
are selected, only the ROW index i of a selected pair (i, j) is used and it indexes BOTH views, and
the gathered [B gamma, C] rows give (var + cov / gamma + inv) / gamma of the VICReg terms.

What it fixes, like the kernel (csrc/vicregl.hip): ties are broken by (distance descending, flat
index i T + j ascending), and the matrix of direction (X2, X1) being the transpose of the one of
(X1, X2), one ranking per kind serves both directions (rows for one, columns for the other).
"""
import torch

ALPHA = 0.9


def tokens(X):
    """[B, C, *spatial] -> [B, T, C]."""
    return X.flatten(2).transpose(1, 2)


def grid_coords(spatial, box):
    """[B, T, ndim]: the token grid mapped into the boxes (lo..., hi...), grid * (hi - lo) + lo."""
    ndim = len(spatial)
    grid = torch.stack([g.flatten() for g in torch.meshgrid(
        *[torch.arange(int(s), device=box.device) for s in spatial], indexing="ij")], 1).to(box.dtype)
    lo, hi = box[:, None, :ndim], box[:, None, ndim:]
    return grid[None] * (hi - lo) + lo


def sq_dists(a, b):
    """[B, T, T] squared Euclidean distances of the rows of a and b [B, T, C], in the difference
    form, the channels added in order (identical rows give exactly equal entries)."""
    d = torch.zeros((a.shape[0], a.shape[1], b.shape[1]), dtype=a.dtype, device=a.device)
    for c in range(a.shape[2]):
        d += (a[:, :, None, c] - b[:, None, :, c]) ** 2
    return d


def top_pairs(d2, gamma):
    """int64 [B, gamma, 2]: the (i, j) of the gamma largest entries, (value descending, flat index
    ascending)."""
    T = d2.shape[-1]
    order = torch.sort(-d2.flatten(1), dim=1, stable=True).indices[:, :gamma]
    return torch.stack([torch.div(order, T, rounding_mode="floor"), order % T], -1)


def boundary_gap(d2, gamma):
    """Per item the relative gap between the gamma-th and the (gamma + 1)-th largest DISTANCE (the
    selection is pinned against an error of the distances only when this dwarfs that error); inf
    when every pair is selected."""
    v = torch.sort(d2.flatten(1).sqrt(), dim=1, descending=True).values
    if v.shape[1] <= gamma:
        return torch.full((v.shape[0],), float("inf"), dtype=v.dtype)
    return (v[:, gamma - 1] - v[:, gamma]) / v[:, gamma - 1]


def vicreg_terms(x1, x2, min_var=1.0, eps=1e-4):
    """(var, cov, inv) of two [R, D] matrices, unweighted (vicreg.py:60-136)."""
    def hinge(x):
        return torch.relu(min_var - torch.sqrt(x.var(0) + eps)).mean()

    def cov(x):
        xc = x - x.mean(0)
        c = (xc.T @ xc) / (x.shape[0] - 1)
        off = c - torch.diag(torch.diag(c))
        return (off ** 2).sum() / x.shape[1]

    inv = ((x1 - x2) ** 2).sum() / x1.numel()
    return (hinge(x1) + hinge(x2)) / 2, (cov(x1) + cov(x2)) / 2, inv


def gather_rows(t, rows):
    """t [B, T, C], rows [B, gamma] -> [B gamma, C]."""
    B = t.shape[0]
    return t[torch.arange(B, device=t.device)[:, None], rows].reshape(-1, t.shape[2])


def local_term(ta, tb, rows, gamma, min_var=1.0, eps=1e-4):
    var, cov, inv = vicreg_terms(gather_rows(ta, rows), gather_rows(tb, rows), min_var, eps)
    return (var + cov / gamma + inv) / gamma


def vicregl_loss(X1, X2, box1, box2, gamma=10, min_var=1.0, eps=1e-4, lam=25.0, mu=25.0, nu=0.1,
                 rank="exact"):
    """((lam inv alpha, mu var alpha, nu cov alpha, local), location pairs, feature pairs).
    rank="exact": the deterministic order above; rank="cdist": torch.cdist + torch.topk, the
    reference's own calls (for timings: its tie order is torch's)."""
    assert X1.shape == X2.shape
    t1, t2 = tokens(X1), tokens(X2)
    c1, c2 = grid_coords(X1.shape[2:], box1.to(X1.dtype)), grid_coords(X1.shape[2:], box2.to(X1.dtype))
    var, cov, inv = vicreg_terms(X1.flatten(2).mean(-1), X2.flatten(2).mean(-1), min_var, eps)
    local, picked = 0.0, []
    for a, b in ((c1, c2), (t1, t2)):
        with torch.no_grad():
            if rank == "exact":
                pairs = top_pairs(sq_dists(a, b), gamma)
            else:
                d = torch.cdist(a, b, p=2)
                idx = torch.topk(d.flatten(1), gamma, 1).indices
                T = d.shape[-1]
                pairs = torch.stack([torch.div(idx, T, rounding_mode="floor"), idx % T], -1)
        picked.append(pairs)
        local = local + (local_term(t1, t2, pairs[..., 0], gamma, min_var, eps) * (1 - ALPHA)
                         + local_term(t2, t1, pairs[..., 1], gamma, min_var, eps) * (1 - ALPHA)) / 2
    return (lam * inv * ALPHA, mu * var * ALPHA, nu * cov * ALPHA, local), picked[0], picked[1]
