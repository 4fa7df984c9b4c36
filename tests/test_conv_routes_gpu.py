"""functional.conv3d launches what its route functions say: for one small shape per forward and
backward-data route the kernel families recorded by ops.KernelTimer are the ones conv3d_route /
conv3d_dgrad_route / conv3d_wgrad_route predict, and y, dx, dw (db) are bit for bit what the same
ops.* front-ends return when they are called directly with the same operands (every family here
is run-to-run bit-stable: fixed fold orders, no atomics in the results)."""
import pytest
import torch

from adell_mri_amd import functional as HF
from adell_mri_amd import ops

pytestmark = pytest.mark.gpu

IGEMM, IGEMM32 = "adell_conv_igemm_f16_kernel", "adell_conv_igemm_kernel"
# route -> (kernel family of the _timed call in ops.py, kind in its tag); None: no timed launch
FWD = {"conv1_small": "adell_conv1_small_kernel", "cin_small": "adell_cin_small_kernel",
       "cinfold": "adell_cinfold_kernel", "fold": IGEMM, "igemm": IGEMM}
DGRAD = {"conv1_lowrank": None, "conv1_small": ("adell_conv1_small_kernel", "dgrad"),
         "cinfold": ("adell_cinfold_kernel", "dgrad"), "cin_small": ("adell_cin_small_kernel", "dgrad"),
         "cin_small_flipped": ("adell_cin_small_kernel", "fwd"),     # the forward kernel on dy
         "s2_fused": ("adell_dgrad_s2_fused_kernel", "dgrad"), "s2_classes": (IGEMM, "dgrad"),
         "igemm_adn": (IGEMM, "dgrad"), "igemm": (IGEMM, "dgrad"), None: None}
WGRAD = {"conv1_small": "adell_conv1_small_kernel", "cinfold_f16x3": "adell_cinfold_kernel",
         "cinfold_fp32": "adell_cinfold_kernel", "igemm_f16x3": "adell_conv_wgrad_f16_kernel",
         "igemm_fp32": "adell_conv_wgrad_kernel", "bias_only": None, None: None}

S1, S2, P0, P1, K1, K3 = (1, 1, 1), (2, 2, 2), (0, 0, 0), (1, 1, 1), (1, 1, 1), (3, 3, 3)
V8, V16 = (8, 8, 8), (16, 16, 16)


def _case(name, N, C0, C1, Cout, k, stride, pad, size, routes, **kw):
    return pytest.param(dict(N=N, C0=C0, C1=C1, Cout=Cout, k=k, stride=stride, pad=pad, size=size,
                             routes=routes, **kw), id=name)


CASES = [  # routes: (forward, backward-data, weight gradient), written by hand
    _case("conv1_small", 2, 16, 0, 2, K1, S1, P0, V8, ("conv1_small",) * 3),
    _case("conv1_small_two_sources", 1, 8, 8, 2, K1, S1, P0, V8, ("conv1_small",) * 3),
    _case("conv1_lowrank", 2, 16, 0, 2, K1, S1, P0, V8,
          ("conv1_small", "conv1_lowrank", "conv1_small"), site=True),
    _case("cin_small", 2, 2, 0, 4, K3, S1, P1, V8, ("cin_small", "cin_small", "igemm_f16x3")),
    _case("cin_small_flipped", 1, 2, 0, 2, K3, S1, P1, V8,
          ("cin_small", "cin_small_flipped", "igemm_f16x3")),
    _case("cinfold", 2, 2, 0, 32, K3, S1, P1, V8, ("cinfold", "cinfold", "cinfold_f16x3")),
    _case("cinfold_parked_gradient", 1, 2, 0, 32, K3, S1, P1, V8,
          ("cinfold", "cinfold", "cinfold_f16x3"), carry=True),       # the add is a pass of its own
    _case("cinfold_dx_refused", 1, 2, 0, 6, K3, S1, P1, V8, ("cinfold", "igemm", "cinfold_f16x3")),
    _case("fold", 1, 2, 0, 8, (1, 3, 3), S1, (0, 1, 1), V8, ("fold", "igemm", "igemm_f16x3")),
    _case("igemm_two_sources", 1, 16, 16, 16, K3, S1, P1, V8, ("igemm", "igemm", "igemm_f16x3")),
    _case("igemm_parked_gradient", 2, 16, 0, 16, K3, S1, P1, V8, ("igemm", "igemm", "igemm_f16x3"),
          carry=True),                                                # the add rides in the epilogue
    _case("igemm_no_dx", 1, 16, 0, 16, K3, S1, P1, V8, ("igemm", None, "igemm_f16x3"), need0=False),
    _case("igemm_fp32", 1, 16, 0, 16, K3, S1, P1, V8, ("igemm", "igemm", "igemm_fp32"),
          precision="fp32"),
    _case("s2_fused", 1, 32, 0, 32, K3, S2, P1, V16, ("igemm", "s2_fused", "igemm_f16x3"),
          fwd_family="adell_fwd_s2_fused_kernel"),     # (ops.conv3d_fwd's own one-launch kernel)
    _case("s2_fused_parked_gradient", 1, 32, 0, 32, K3, S2, P1, V16,
          ("igemm", "s2_fused", "igemm_f16x3"), fwd_family="adell_fwd_s2_fused_kernel", carry=True),
    _case("s2_classes", 1, 16, 0, 48, K3, S2, P1, (8, 12, 20),
          ("igemm", "s2_classes", "igemm_f16x3"), flags=("s2class_always",)),
    _case("s2_plain", 1, 16, 0, 48, K3, S2, P1, (8, 12, 20), ("igemm", "igemm", "igemm_f16x3")),
    _case("igemm_adn", 2, 32, 0, 32, K3, S1, P1, V16, ("igemm", "igemm_adn", "igemm_f16x3"),
          site=True),
]


def _direct(c, x0, x1, w, b, dy, site, parked, routes):
    """The same kernels through ops.*: (y, dx0, dx1, dw, db)."""
    fwd, dgrad, wgrad = routes
    C0, C1, k, st, pad, size = c["C0"], c["C1"], c["k"], c["stride"], c["pad"], tuple(c["size"])
    f16x3 = HF.CONV_PRECISION == "f16x3"
    amax = torch.zeros(2, dtype=torch.int32, device=x0.device) if fwd == "igemm" and f16x3 else None
    dx0 = dx1 = dy_amax = None
    if fwd == "conv1_small":
        y = ops.conv1_small_fwd(x0, x1, w, b)
    elif fwd == "cin_small":
        y, _ = ops.conv_cin_small_fwd(x0, w, b, pad, True)
    elif fwd == "cinfold":
        y, _ = ops.conv_cinfold_fwd(x0, w, b, pad, True, f16x3=f16x3)
    elif fwd == "fold":
        y, _ = ops.conv3d_fwd(ops.fold_x_taps(x0, k[2], pad[2]), HF._packed_folded(w), b, c["Cout"],
                              (k[0], k[1], 1), st, (pad[0], pad[1], 0), want_stats=True)
    else:
        y, _ = ops.conv3d_fwd(x0, HF._packed(w, 0), b, c["Cout"], k, st, pad, x1=x1,
                              want_stats=True, amax=None if amax is None else amax[0:1])
    if amax is not None and dgrad is not None:
        dy_amax = amax[1:2]
    if dgrad == "conv1_lowrank":
        dx0 = ops.norm_act_bwd_lowrank(site.x, dy, w, site.mean, site.rstd, site.act,
                                       act_p=site.act_p, drop_p=site.drop_p)
    elif dgrad == "conv1_small":
        dx0, dx1 = ops.conv1_small_bwd_data(dy, w, size, C0, C1)
    elif dgrad == "cinfold":
        dx0 = ops.conv_cinfold_bwd_data(dy, w, size, pad, f16x3=f16x3)
        dx0 = dx0 if parked is None else dx0 + parked
    elif dgrad == "cin_small":
        dx0 = ops.conv_cin_small_bwd_data(dy, w, size, pad)
    elif dgrad == "cin_small_flipped":
        wt = w.transpose(0, 1).flip(2, 3, 4).contiguous()
        dx0, _ = ops.conv_cin_small_fwd(dy, wt, None, tuple(kk - 1 - p for kk, p in zip(k, pad)),
                                        False)
    elif dgrad == "s2_fused":
        dx0 = ops.conv3d_bwd_data_s2_fused(dy, HF._packed(w, 1), size, amax=dy_amax, add0=parked)
    elif dgrad == "s2_classes":
        dx0 = ops.conv3d_bwd_data_s2(dy, HF._packed_s2_classes(w, pad), size, C0, pad,
                                     amax=dy_amax, add0=parked)
    elif dgrad == "igemm_adn":
        nt = ops.conv3d_bwd_data_adn_ntiles(size, c["N"], C0, C1, c["Cout"], k, st, pad)
        dt, _, part = ops.conv3d_bwd_data_adn(dy, HF._packed(w, 1), size, C0, C1, k, st, pad, nt,
                                              site0=site, amax=dy_amax, add0=parked)
        dx0 = ops.norm_act_bwd_from_dt(site.x, dt, site.mean, site.rstd, part, 0)
    elif dgrad == "igemm":
        dx0, dx1 = ops.conv3d_bwd_data(dy, HF._packed(w, 1), size, C0, C1, k, st, pad,
                                       amax=dy_amax, add0=parked if f16x3 and C1 == 0 else None)
        if parked is not None and not (f16x3 and C1 == 0):
            dx0 = dx0 + parked
    if wgrad == "conv1_small":
        dw, db = ops.conv1_small_bwd_weight(x0, x1, dy, True)
    elif wgrad.startswith("cinfold"):
        dw, db = ops.conv_cinfold_bwd_weight(x0, dy, pad, True, f16x3=wgrad == "cinfold_f16x3")
    else:
        dw, db = ops.conv3d_bwd_weight(x0, dy, k, st, pad, x1=x1, want_db=True,
                                       f16x3=wgrad == "igemm_f16x3",
                                       x_amax=None if amax is None else amax[0:1], dy_amax=dy_amax)
    return y, dx0, dx1, dw.view(w.shape), db


class _SiteCopy:
    """The fields of an AdnSite (its backward clears them)."""

    def __init__(self, s):
        self.x, self.mean, self.rstd, self.mask = s.x, s.mean, s.rstd, s.mask
        self.drop_p, self.act, self.act_p = s.drop_p, s.act, s.act_p


@pytest.mark.parametrize("c", CASES)
def test_conv3d_runs_the_routed_kernels_bit_for_bit(cuda, monkeypatch, c):
    monkeypatch.setattr(HF, "CONV_PRECISION", c.get("precision", "f16x3"))
    for f in c.get("flags", ()):
        monkeypatch.setitem(HF.FLAGS, f, True)
    N, C0, C1, Cout, k, st, pad = (c[n] for n in ("N", "C0", "C1", "Cout", "k", "stride", "pad"))
    need0 = c.get("need0", True)
    g = torch.Generator().manual_seed(C0 + 3 * C1 + 7 * Cout)
    rnd = lambda *s: torch.randn(*s, generator=g).to(cuda)       # noqa: E731
    src = ops.ndhwc(rnd(N, C0, *c["size"])).requires_grad_(need0)
    x1 = ops.ndhwc(rnd(N, C1, *c["size"])).requires_grad_(True) if C1 else None
    w = (rnd(Cout, C0 + C1, *k) * 0.1).requires_grad_(True)
    b = rnd(Cout).requires_grad_(True)
    parked = ops.ndhwc(rnd(N, C0, *c["size"])) if c.get("carry") else None
    out_size = ops.conv_out_size(c["size"], k, st, pad)
    dy = ops.ndhwc(rnd(N, Cout, *out_size))

    site = None
    x0 = src
    if c.get("site"):       # a single-use norm -> activation site in front (test_adn_fused_gpu.py)
        x0 = HF.single_use(HF.norm_drop_act(src, norm="instance", act="swish", drop_p=0.0,
                                            training=True))
        site = _SiteCopy(x0._adell_site)
        if C0 == 32:
            assert ops.conv3d_bwd_data_adn_ntiles(c["size"], N, C0, C1, Cout, k, st, pad) > 0
    carry = None
    if parked is not None:
        carry = HF.GradCarry()
        carry.grad = parked

    shapes = ((N, C0, *c["size"]), (Cout, C0 + C1, *k))
    fwd = HF.conv3d_route(*shapes, st, pad, C1 or None, has_carry=carry is not None)
    dgrad = HF.conv3d_dgrad_route(fwd, *shapes, st, pad, C1, need0=need0, need1=True,
                                  has_x1=bool(C1), has_add0=carry is not None,
                                  sites=site is not None and fwd == "igemm",
                                  lowrank=site is not None and fwd == "conv1_small")
    wgrad = HF.conv3d_wgrad_route(fwd, True, True)
    assert (fwd, dgrad, wgrad) == c["routes"]

    timer = ops.KernelTimer()
    monkeypatch.setattr(ops, "KERNEL_TIMER", timer)
    y = HF.conv3d(x0, w, b, st, pad, x1=x1, carry_in=carry)
    (y * dy).sum().backward()
    monkeypatch.setattr(ops, "KERNEL_TIMER", None)
    conv_families = set(FWD.values()) | {IGEMM32, "adell_fwd_s2_fused_kernel",
                                         "adell_dgrad_s2_fused_kernel",
                                         "adell_conv_wgrad_f16_kernel", "adell_conv_wgrad_kernel"}
    got = [(r[0], r[4].split()[0]) for r in timer.records if r[0] in conv_families]
    igemm = IGEMM if c.get("precision", "f16x3") == "f16x3" else IGEMM32
    want = [(c.get("fwd_family", FWD[fwd]), "fwd"), DGRAD[dgrad], (WGRAD[wgrad], "wgrad")]
    want = [(igemm if fam == IGEMM else fam, kind) for fam, kind in (p for p in want if p)]
    assert got == want        # (the site's own backward is not a conv family)

    with torch.no_grad():
        ry, rdx0, rdx1, rdw, rdb = _direct(c, x0.detach(), x1, w.detach(), b.detach(), dy, site,
                                           parked, (fwd, dgrad, wgrad))
    assert torch.equal(y.detach(), ry)
    assert torch.equal(w.grad, rdw) and torch.equal(b.grad, rdb)
    if need0:
        assert torch.equal(src.grad, rdx0)
    else:
        assert src.grad is None
    if x1 is not None:
        assert torch.equal(x1.grad, rdx1)
    if carry is not None:
        assert carry.grad is None       # taken


GEMM = {"adell_gemm_f32_kernel", "adell_gemm_f16x3_kernel"}


def test_pointwise_conv_takes_the_linear_gemms_bit_for_bit(cuda, monkeypatch):
    """64 -> 8 1x1x1: conv3d runs the Linear layer's three GEMMs and nothing of the conv families,
    with results equal to functional.linear on the voxel rows; a residual, a gradient carry or the
    switch keep it on the implicit-GEMM conv kernels."""
    monkeypatch.setattr(HF, "CONV_PRECISION", "f16x3")
    monkeypatch.setitem(HF.FLAGS, "no_pointwise_gemm", False)
    g = torch.Generator().manual_seed(64)
    N, C, Cout, size = 2, 64, 8, V8
    x0 = ops.ndhwc(torch.randn(N, C, *size, generator=g).to(cuda))
    w0 = (torch.randn(Cout, C, 1, 1, 1, generator=g) * 0.1).to(cuda)
    b0 = torch.randn(Cout, generator=g).to(cuda)
    dy = ops.ndhwc(torch.randn(N, Cout, *size, generator=g).to(cuda))
    assert HF.conv3d_route(x0.shape, w0.shape, S1, P0) == "pointwise_gemm"

    def run(fn):
        x, w, b = (t.clone().requires_grad_(True) for t in (x0, w0, b0))
        x = ops.ndhwc(x.detach()).requires_grad_(True)
        timer = ops.KernelTimer()
        monkeypatch.setattr(ops, "KERNEL_TIMER", timer)
        y = fn(x, w, b)
        (y * dy).sum().backward()
        monkeypatch.setattr(ops, "KERNEL_TIMER", None)
        return [r[0] for r in timer.records], y.detach(), x.grad, w.grad, b.grad

    names, y, dx, dw, db = run(lambda x, w, b: HF.conv3d(x, w, b, 1, 0))
    assert len(names) == 3 and set(names) <= GEMM          # forward, dX, dW

    def as_linear(x, w, b):
        rows = HF.linear(x.permute(0, 2, 3, 4, 1).reshape(-1, C), w.view(Cout, C), b)
        return rows.view(N, *size, Cout).permute(0, 4, 1, 2, 3)

    _, ry, rdx, rdw, rdb = run(as_linear)
    assert torch.equal(y, ry) and torch.equal(dx, rdx)
    assert torch.equal(dw, rdw) and torch.equal(db, rdb)

    # what keeps it a conv: the routed families are those of the "igemm" route
    conv = [IGEMM, IGEMM, "adell_conv_wgrad_f16_kernel"]
    res = ops.ndhwc(torch.randn(N, Cout, *size, generator=g).to(cuda))
    parked = ops.ndhwc(torch.randn(N, C, *size, generator=g).to(cuda))

    def with_carry(x, w, b):
        carry = HF.GradCarry()
        carry.grad = parked
        return HF.conv3d(x, w, b, 1, 0, carry_in=carry)

    names, _, dxc, _, _ = run(with_carry)
    assert names == conv
    assert float((dxc - (dx + parked)).abs().max()) <= 2e-5 * float(dxc.abs().max())   # carry taken
    for kw in ({"carry_out": HF.GradCarry()}, {"carry_x0": HF.GradCarry()},
               {"carry_cat": HF.GradCarry()}, {"residual": res}):
        names, yk, _, _, _ = run(lambda x, w, b: HF.conv3d(x, w, b, 1, 0, **kw))
        assert names == conv, kw
        want = y + res if "residual" in kw else y
        assert float((yk - want).abs().max()) <= 2e-5 * float(want.abs().max())
    monkeypatch.setitem(HF.FLAGS, "no_pointwise_gemm", True)
    names, yk, _, _, _ = run(lambda x, w, b: HF.conv3d(x, w, b, 1, 0))
    assert names == conv
    assert float((yk - y).abs().max()) <= 2e-5 * float(y.abs().max())
