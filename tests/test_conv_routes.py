"""The routing decisions of functional.conv3d -- conv3d_route (forward), conv3d_dgrad_route
(backward-data), conv3d_wgrad_route (weight gradient) -- and conv_transpose3d_route, on the host:
shapes and flags in, a route name out, no GPU. The expected names are written down by hand from the
route lists in DESIGN.md ("Conv dispatch"), one row per condition that decides."""
import pytest

from adell_mri_amd import functional as HF
from adell_mri_amd import ops

S1, S2, P0, P1 = (1, 1, 1), (2, 2, 2), (0, 0, 0), (1, 1, 1)
V8, V16, V128 = (8, 8, 8), (16, 16, 16), (128, 128, 128)


def _case(name, C0, Cout, k, stride, pad, size, fwd, dgrad, wgrad="igemm_f16x3", N=1, C1=None,
          flags=(), precision="f16x3", **dgrad_kw):
    return pytest.param(dict(C0=C0, Cout=Cout, k=k, stride=stride, pad=pad, size=size, fwd=fwd,
                             dgrad=dgrad, wgrad=wgrad, N=N, C1=C1, flags=flags,
                             precision=precision, dgrad_kw=dgrad_kw), id=name)


K1, K3 = (1, 1, 1), (3, 3, 3)
CASES = [
    # the logits head
    _case("16to2_1x1x1", 16, 2, K1, S1, P0, V8, "conv1_small", "conv1_small", "conv1_small"),
    _case("16to2_1x1x1_lowrank_site", 16, 2, K1, S1, P0, V8, "conv1_small", "conv1_lowrank",
          "conv1_small", lowrank=True),
    _case("16to2_1x1x1_lowrank_site_no_dx", 16, 2, K1, S1, P0, V8, "conv1_small", None,
          "conv1_small", lowrank=True, need0=False),
    _case("8+8to2_1x1x1_second_source_only", 8, 2, K1, S1, P0, V8, "conv1_small", "conv1_small",
          "conv1_small", C1=8, need0=False, need1=True),
    # a wide 1x1x1 conv is a Linear layer; behind the switch it is an ordinary conv
    _case("64to8_1x1x1", 64, 8, K1, S1, P0, V8, "pointwise_gemm", None, None),
    _case("64to8_1x1x1_no_pointwise_gemm", 64, 8, K1, S1, P0, V8, "igemm", "igemm",
          flags=("no_pointwise_gemm",)),
    # narrow inputs
    _case("2to2_3x3x3", 2, 2, K3, S1, P1, V8, "cin_small", "cin_small_flipped"),
    _case("2to2_3x3x3_pad0_shrinks", 2, 2, K3, S1, P0, V8, "cin_small", "igemm"),
    _case("2to4_3x3x3", 2, 4, K3, S1, P1, V8, "cin_small", "cin_small"),
    _case("2to32_3x3x3", 2, 32, K3, S1, P1, V8, "cinfold", "cinfold", "cinfold_f16x3"),
    _case("2to32_3x3x3_wgrad_switch", 2, 32, K3, S1, P1, V8, "cinfold", "cinfold", "cinfold_fp32",
          flags=("no_cinfold_wgrad_f16",)),
    _case("2to32_3x3x3_fp32", 2, 32, K3, S1, P1, V8, "cinfold", "cinfold", "cinfold_fp32",
          precision="fp32"),
    _case("2to6_3x3x3_dx_refused_cout_mod4", 2, 6, K3, S1, P1, V8, "cinfold", "igemm",
          "cinfold_f16x3"),
    _case("2to72_3x3x3_dx_refused_cout_gt64", 2, 72, K3, S1, P1, V8, "cinfold", "igemm",
          "cinfold_f16x3"),
    _case("2to8_k133", 2, 8, (1, 3, 3), S1, (0, 1, 1), V8, "fold", "igemm"),
    _case("2to8_k133_no_fold", 2, 8, (1, 3, 3), S1, (0, 1, 1), V8, "igemm", "igemm",
          flags=("no_fold",)),
    _case("2to8_k133_fp32_never_folds", 2, 8, (1, 3, 3), S1, (0, 1, 1), V8, "igemm", "igemm",
          "igemm_fp32", precision="fp32"),
    _case("2to32_3x3x3_no_cinfold", 2, 32, K3, S1, P1, V8, "fold", "igemm",
          flags=("ops.no_cinfold",)),
    # the implicit-GEMM kernels
    _case("16+16to16_3x3x3", 16, 16, K3, S1, P1, V8, "igemm", "igemm", C1=16, need1=True),
    _case("16+16to16_3x3x3_second_source_only", 16, 16, K3, S1, P1, V8, "igemm", "igemm", C1=16,
          need0=False, need1=True),
    _case("16to16_3x3x3_no_dx", 16, 16, K3, S1, P1, V8, "igemm", None, need0=False),
    _case("16to16_3x3x3_fp32", 16, 16, K3, S1, P1, V8, "igemm", "igemm", "igemm_fp32",
          precision="fp32"),
    # stride 2: the one-launch 32 -> 32 kernel, the parity classes, the plain kernel
    _case("32to32_s2_16", 32, 32, K3, S2, P1, V16, "igemm", "s2_fused"),
    _case("32to32_s2_16_no_s2fused", 32, 32, K3, S2, P1, V16, "igemm", "igemm",
          flags=("ops.no_s2fused",)),
    _case("32to32_s2_16_fused_precedes_classes", 32, 32, K3, S2, P1, V16, "igemm", "s2_fused",
          flags=("s2class_always",)),
    _case("32to32_s2_16_classes_always", 32, 32, K3, S2, P1, V16, "igemm", "s2_classes",
          flags=("ops.no_s2fused", "s2class_always")),
    _case("32to32_s2_16_fp32", 32, 32, K3, S2, P1, V16, "igemm", "igemm", "igemm_fp32",
          precision="fp32"),
    _case("16to48_s2_8x12x20", 16, 48, K3, S2, P1, (8, 12, 20), "igemm", "igemm"),
    _case("16to48_s2_8x12x20_classes_always", 16, 48, K3, S2, P1, (8, 12, 20), "igemm",
          "s2_classes", flags=("s2class_always",)),
    _case("16to48_s2_8x12x20_never_wins", 16, 48, K3, S2, P1, (8, 12, 20), "igemm", "igemm",
          flags=("s2class_always", "no_s2class")),
    _case("16to48_s2_odd_extent", 16, 48, K3, S2, P1, (8, 12, 21), "igemm", "igemm",
          flags=("s2class_always",)),
    _case("32to32_s2_128_fused_precedes_threshold", 32, 32, K3, S2, P1, V128, "igemm", "s2_fused"),
    _case("16to16_s2_128_threshold", 16, 16, K3, S2, P1, V128, "igemm", "s2_classes"),
    _case("16to16_s2_64_below_threshold", 16, 16, K3, S2, P1, (64, 64, 64), "igemm", "igemm"),
    _case("16to16_s2_64_batch4_reaches_threshold", 16, 16, K3, S2, P1, (64, 64, 64), "igemm",
          "s2_classes", N=4),
    _case("16to16_s2_128_never", 16, 16, K3, S2, P1, V128, "igemm", "igemm",
          flags=("no_s2class",)),
    _case("16to16_s2_128_fp32", 16, 16, K3, S2, P1, V128, "igemm", "igemm", "igemm_fp32",
          precision="fp32"),
    _case("16to16_s2_128_parked_gradient", 16, 16, K3, S2, P1, V128, "igemm", "s2_classes",
          has_add0=True),
    # single-use ADN sites in front
    _case("32to32_sites", 32, 32, K3, S1, P1, V16, "igemm", "igemm_adn", sites=True),
    _case("32to32_sites_parked_gradient", 32, 32, K3, S1, P1, V16, "igemm", "igemm_adn", sites=True,
          has_add0=True),
    _case("32+32to64_sites", 32, 64, K3, S1, P1, V16, "igemm", "igemm_adn", C1=32, sites=True,
          need1=True),
    _case("32+32to64_sites_parked_gradient", 32, 64, K3, S1, P1, V16, "igemm", "igemm", C1=32,
          sites=True, need1=True, has_add0=True),
    _case("32+32to64_sites_second_source_unwanted", 32, 64, K3, S1, P1, V16, "igemm", "igemm",
          C1=32, sites=True, need1=False),
    _case("32to32_sites_no_dx", 32, 32, K3, S1, P1, V16, "igemm", None, sites=True, need0=False),
    _case("32to32_sites_fp32", 32, 32, K3, S1, P1, V16, "igemm", "igemm", "igemm_fp32", sites=True,
          precision="fp32"),
    _case("32to32_s2_16_sites_fused_precedes", 32, 32, K3, S2, P1, V16, "igemm", "s2_fused",
          sites=True),
]


@pytest.fixture
def switches(monkeypatch):
    """Sets dispatch flags and the conv precision for one test; both are restored afterwards."""
    def set_(flags, precision):
        for f in flags:
            table, key = (ops.FLAGS, f[4:]) if f.startswith("ops.") else (HF.FLAGS, f)
            monkeypatch.setitem(table, key, True)
        monkeypatch.setattr(HF, "CONV_PRECISION", precision)
    for table, keys in ((HF.FLAGS, ("no_pointwise_gemm", "no_fold", "s2class_always", "no_s2class",
                                    "no_cinfold_wgrad_f16")),
                        (ops.FLAGS, ("no_cinfold", "no_s2fused", "no_cin_small", "cin_small_all"))):
        for key in keys:
            monkeypatch.setitem(table, key, False)     # (whatever the environment asked for)
    return set_


@pytest.mark.parametrize("c", CASES)
def test_routes(switches, c):
    switches(c["flags"], c["precision"])
    C1 = c["C1"]
    x0 = (c["N"], c["C0"], *c["size"])
    w = (c["Cout"], c["C0"] + (C1 or 0), *c["k"])
    fwd = HF.conv3d_route(x0, w, c["stride"], c["pad"], C1)
    assert fwd == c["fwd"]
    if fwd == "pointwise_gemm":
        return      # a Linear layer from here on
    kw = dict(need0=True, need1=False, has_x1=C1 is not None, has_add0=False, sites=False,
              lowrank=False)
    kw.update(c["dgrad_kw"])
    assert HF.conv3d_dgrad_route(fwd, x0, w, c["stride"], c["pad"], C1 or 0, **kw) == c["dgrad"]
    assert HF.conv3d_wgrad_route(fwd, True, False) == c["wgrad"]
    assert HF.conv3d_wgrad_route(fwd, True, True) == c["wgrad"]


def test_forward_route_conditions_outside_the_shapes(switches):
    switches((), "f16x3")
    x, w = (1, 64, 8, 8, 8), (8, 64, 1, 1, 1)
    assert HF.conv3d_route(x, w, S1, P0) == "pointwise_gemm"
    # a residual, a gradient carry, a second source or split-row input keep it a conv
    assert HF.conv3d_route(x, w, S1, P0, has_residual=True) == "igemm"
    assert HF.conv3d_route(x, w, S1, P0, has_carry=True) == "igemm"
    assert HF.conv3d_route(x, w, S1, P0, has_rows=True) == "igemm"
    assert HF.conv3d_route((1, 32, 8, 8, 8), w, S1, P0, C1=32) == "igemm"
    assert HF.conv3d_route(x, w, S2, P0) == "igemm"
    assert HF.conv3d_route((1, 7, 8, 8, 8), (64, 7, 1, 1, 1), S1, P0) == "igemm"     # min side < 8
    # every narrow route refuses a residual; the fold takes one
    assert HF.conv3d_route((1, 16, 8, 8, 8), (2, 16, 1, 1, 1), S1, P0, has_residual=True) == "igemm"
    assert HF.conv3d_route((1, 2, 8, 8, 8), (2, 2, 3, 3, 3), S1, P1, has_residual=True) == "fold"
    assert HF.conv3d_route((1, 2, 8, 8, 8), (32, 2, 3, 3, 3), S1, P1, has_residual=True) == "fold"
    # a 2-D weight (a Linear layer run as a conv) goes to the implicit-GEMM kernels
    assert HF.conv3d_route((1, 16, 4, 4, 4), (24, 16), S1, P0) == "igemm"
    assert HF.conv3d_dgrad_route("igemm", (1, 16, 4, 4, 4), (24, 16), S1, P0) == "igemm"


def test_weight_gradient_routes_without_a_weight_gradient(switches):
    switches((), "f16x3")
    for fwd in ("cin_small", "cinfold", "fold", "igemm"):
        assert HF.conv3d_wgrad_route(fwd, False, True) == "bias_only"
        assert HF.conv3d_wgrad_route(fwd, False, False) is None
    # the logits head's kernel yields the bias gradient too
    assert HF.conv3d_wgrad_route("conv1_small", False, True) == "conv1_small"
    assert HF.conv3d_wgrad_route("conv1_small", False, False) is None


def test_transposed_conv_routes(monkeypatch):
    monkeypatch.setitem(ops.FLAGS, "no_convt_k2", False)
    w = (32, 32, 2, 2, 2)
    assert HF.conv_transpose3d_route((1, 32, 32, 32, 32), w) == "k2"        # 32 K voxels
    assert HF.conv_transpose3d_route((1, 32, 16, 16, 16), w) == "igemm"     # fewer
    assert HF.conv_transpose3d_route((1, 32, 32, 32, 32), (32, 32, 2, 2, 1)) == "k2"
    assert HF.conv_transpose3d_route((1, 32, 32, 32, 32), (32, 16, 2, 2, 1)) == "igemm"
    assert HF.conv_transpose3d_route((1, 24, 32, 32, 32), (24, 32, 2, 2, 2)) == "igemm"
    assert HF.conv_transpose3d_route((1, 32, 32, 32, 32), (32, 32, 1, 2, 2)) == "igemm"
    monkeypatch.setitem(ops.FLAGS, "no_convt_k2", True)
    assert HF.conv_transpose3d_route((1, 32, 32, 32, 32), w) == "igemm"
