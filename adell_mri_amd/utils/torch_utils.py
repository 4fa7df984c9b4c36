"""State-dict helpers of the reference's ``utils/torch_utils.py``."""
import torch


def calculate_sn_weights(state_dict):
    """Replaces, in place, every spectral-norm triple ``<p>.parametrizations.<name>.original`` /
    ``.0._u`` / ``.0._v`` of ``state_dict`` by the normalised weight ``original / (u^T W v)`` under
    ``<p>.<name>``, and returns the dict; keys without both vectors are left alone.

    One deviation from the reference, on purpose: it views every weight as ``[size(0), -1]``, which
    fails -- or silently uses the wrong matrix when Cin == Cout -- for a transposed convolution,
    whose ``_u`` has ``size(1)`` entries. Here the matrix is chosen by the lengths of ``_u`` and
    ``_v``: dimension 0 in front when they fit it, else the first dimension that fits."""
    keys = list(state_dict.keys())
    stems = [k[:-len(".original")] for k in keys if k.endswith(".original")]
    stems = [s for s in stems if s + ".0._u" in state_dict and s + ".0._v" in state_dict]
    for stem in stems:
        w = state_dict[stem + ".original"]
        u, v = state_dict[stem + ".0._u"], state_dict[stem + ".0._v"]
        dim = None
        for d in range(w.dim()):
            if w.size(d) == u.numel() and w.numel() == u.numel() * v.numel():
                dim = d
                break
        if dim is None:
            raise ValueError(f"calculate_sn_weights: {stem}: u [{u.numel()}] and v [{v.numel()}] fit no "
                             f"dimension of the weight {tuple(w.shape)}")
        mat = w if dim == 0 else w.permute(dim, *[d for d in range(w.dim()) if d != dim])
        sigma = torch.dot(u, torch.mv(mat.reshape(mat.size(0), -1), v))
        state_dict[stem.replace(".parametrizations", "")] = w / sigma
        for k in (stem + ".original", stem + ".0._u", stem + ".0._v"):
            del state_dict[k]
    return state_dict
