"""What the diffusion tests and tools/make_diffusion_golden.py share: the case tables, the
deterministic inputs of every kernel case (fp32-representable, so every side reads the same numbers)
and the two fixture networks."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the project's bounds for these kinds of quantity (tests/test_mil_gpu.py)
SUM_BOUND = 5e-5                  # of the largest reference magnitude: kernel outputs and gradients
STEP_TOL = dict(loss=1e-4, grad=5e-3, param=(2e-4, 2e-6))
STEP_LR, STEP_EPS, STEP_WD = 1e-4, 1e-2, 0.05

# ---- gate logits -------------------------------------------------------------------------------------
GATE_WIDTHS = (1, 5, 33, 130)          # the sites of one call
GATE_RECORDED = (1, 5, 33)             # the widths whose fp64 outputs the fixture keeps
# (t_dim, G, with a class embedding, kind of t)
GATE_CASES = [(T, G, c, "fraction") for T in (1, 7, 32) for G in (1, 3) for c in (False, True)]
GATE_CASES.append((32, 3, True, "integer"))       # t an integer near 1000
GATE_CASES.append((7, 1, True, "one_t"))          # one timestep, three class rows (sample's call)


def gate_name(case):
    T, G, c, kind = case
    return f"T{T}_G{G}_{'cls' if c else 'nocls'}_{kind}"


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def gate_inputs(case):
    """t [Gt], cls [Ng, T] or None, per width the eight parameters (tests/diffusion_ref.PARAM_KEYS
    order) and the gradient gz [Ng, C] that arrives on the logits."""
    T, G, with_cls, kind = case
    rng = np.random.default_rng(1000 + 7 * T + G + (100 if with_cls else 0) + len(kind))
    if kind == "integer":
        t = _f32(np.array([999.0, 1000.0, 987.0])[:G])
    else:
        t = _f32(rng.uniform(0.02, 0.98, size=1 if kind == "one_t" else G))
    Ng = 3 if kind == "one_t" else G
    cls = _f32(rng.normal(0, 0.7, size=(Ng, T))) if with_cls else None
    sites = []
    for C in GATE_WIDTHS:
        def u(shape, fan):
            return _f32(rng.uniform(-1, 1, size=shape) * 1.5 / np.sqrt(fan))
        p = (u((C, T), T), u((C,), 4), u((C, C), C), u((C,), 4), _f32(1.0 + rng.uniform(-0.3, 0.3, C)),
             u((C,), 4), u((C, C), C), u((C,), 4))
        sites.append((p, _f32(rng.normal(0, 1, size=(Ng, C)))))
    return t, cls, sites


def rel_err(got, ref, floor=0.0):
    """max |got - ref| over the largest magnitude of ref (at least ``floor``)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), floor, 1e-300))


def site_grad_err(got, ref):
    """Worst error of a site's gradient tensors, each relative to its own largest magnitude but
    to no less than a tenth of the site's largest gradient (a one-channel site's LayerNorm output
    is its beta: the gradients in front of it are mathematically zero and the reference's values
    are rounding noise, the floor of cases.grad_rel_err for such biases)."""
    floor = 1e-1 * max(float(np.abs(r).max()) for r in ref)
    return max(rel_err(g, r, floor) for g, r in zip(got, ref))


# ---- gate apply -------------------------------------------------------------------------------------
APPLY_SHAPES = [(1, 1, 1, 1, 1), (2, 3, 5, 7, 3), (3, 130, 2, 3, 5), (2, 16, 16, 16, 8), (2, 6, 5, 7)]


def apply_inputs(shape, one_row):
    rng = np.random.default_rng(int(np.prod(shape)) * 2 + int(one_row) + 17 * len(shape))
    x = _f32(rng.normal(0, 1, size=shape))
    dy = _f32(rng.normal(0, 1, size=shape))
    z = _f32(rng.normal(0, 2, size=(1 if one_row else shape[0], shape[1])))
    return x, z, dy


# ---- noising and reverse steps --------------------------------------------------------------------
PROCESS_STEPS = 50
PROCESS_SHAPE = (3, 2, 5, 6, 3)
# (kind, t, eta, guidance)
STEP_CASES = [(k, t, eta, g) for k in ("ddpm", "ddim", "alpha_deblending") for t in (0, 1, 23)
              for eta in (0.0, 1.0) for g in (False, True)]


def step_name(case):
    k, t, eta, g = case
    return f"{k}_t{t}_eta{int(eta)}_{'guided' if g else 'plain'}"


def process_inputs(seed=5):
    """x, eps, eps_uncond, noise of PROCESS_SHAPE and the timesteps of the noising case."""
    rng = np.random.default_rng(seed)
    x = _f32(rng.uniform(-1, 1, size=PROCESS_SHAPE))
    eps = _f32(rng.normal(0, 1, size=PROCESS_SHAPE))
    eps_u = _f32(rng.normal(0, 1, size=PROCESS_SHAPE))
    noise = _f32(rng.normal(0, 1, size=PROCESS_SHAPE))
    return x, eps, eps_u, noise, np.array([0, 23, 49], np.int64)


GUIDANCE_SCALE = 3.0
MSE_SIZES = (1, 63, 64 * 1024 + 1)

# ---- the fixture networks ----------------------------------------------------------------------------
NET_STEPS = 50           # noise_steps of the networks' Diffusion
NETS = {
    "net3d": dict(
        kwargs=dict(t_dim=32, classifier_free_guidance=True, classifier_classes=3,
                    spatial_dimensions=3, in_channels=1, depth=[8, 16, 32],
                    strides=[[2, 2, 2], [2, 2, 1], [2, 2, 1]], kernel_sizes=[3, 3, 3],
                    conv_type="resnet", link_type="conv", upscale_type="transpose",
                    norm_type="instance", padding=1, dropout_param=0.0),
        shape=(2, 1, 16, 16, 8), cls=[0, 2], img_size=(16, 16, 8)),
    "net2d": dict(
        kwargs=dict(t_dim=7, classifier_free_guidance=False, spatial_dimensions=2, in_channels=2,
                    depth=[8, 16, 32], strides=[2, 2, 2], kernel_sizes=[3, 3, 3],
                    conv_type="regular", link_type="identity", upscale_type="transpose",
                    norm_type="instance", padding=1, dropout_param=0.0),
        shape=(2, 2, 16, 16), cls=None, img_size=(16, 16)),
}
NET_TIMESTEPS = ([7, 31], [44, 2], [19, 25])       # training step 1, step 2, validation
SAMPLE_STEPS = 6         # noise_steps of the sampling chains (on net3d, with guidance)
SAMPLE_CLS = [2, 1]


def net_kwargs(name, activation_factory):
    kw = {k: (list(v) if isinstance(v, list) else v) for k, v in NETS[name]["kwargs"].items()}
    kw["activation_fn"] = activation_factory["swish"]
    return kw


def net_inputs(name):
    """The image batch and the three noise tensors (step 1, step 2, validation)."""
    shape = NETS[name]["shape"]
    rng = np.random.default_rng(31 + len(shape))
    grids = np.meshgrid(*[np.arange(float(s)) for s in shape[2:]], indexing="ij")
    x = np.stack([np.stack([np.sin((b + 1) * 0.37 * grids[0] + c) * np.cos((b + 2) * 0.23 * grids[1])
                            for c in range(shape[1])]) for b in range(shape[0])])
    x = _f32(0.8 * x + 0.1 * rng.uniform(-1, 1, size=shape))
    eps = [_f32(rng.normal(0, 1, size=shape)) for _ in range(3)]
    return x, eps


def fill(state_dict, gain):
    from oracle.weights import fill_state_dict

    return fill_state_dict(state_dict, gain=gain, norm_weight_offset=1.0)


class Gold:
    """One fixture file (``files`` and items: what cases.grad_rel_err reads), keys optionally
    behind a prefix."""

    def __init__(self, fname, prefix=""):
        self._g = np.load(os.path.join(GOLD, fname), allow_pickle=False)
        self._p = prefix
        self.files = [k[len(prefix):] for k in self._g.files if k.startswith(prefix)]

    def __getitem__(self, k):
        return self._g[self._p + k]

    def __contains__(self, k):
        return (self._p + k) in self._g.files
