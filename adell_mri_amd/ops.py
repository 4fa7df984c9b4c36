"""Raw (non-autograd) Python front-ends of the HIP kernels.

Activations are torch CUDA tensors of logical shape ``[N, C, D, H, W]`` whose
memory is dense NDHWC (``torch.channels_last_3d``); ``ndhwc()`` / ``new_act()``
are the only places that care about strides. Everything is enqueued on
``torch.cuda.current_stream()``; PyTorch only provides memory and streams.
"""
import collections
import ctypes
import functools
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import ACT_IDS, AdellHipError, ConvDesc, NormActDesc, check


class KernelTimer:
    """Per-launch HIP-event timing of the MFMA kernels (bench.py's roofline leg).

    Events are recorded on ``torch.cuda.current_stream()``, the stream the kernels
    are enqueued on; nothing synchronises until ``summary()`` is read.
    """

    def __init__(self, only=None):
        self.records = []
        self._agg = None
        self.only = None if only is None else set(only)  # kernel families to time (None: all)
        # an event pair costs ~6 us of stream idle time per launch (measured: rocprofv3 timeline,
        # DESIGN.md 8); bench.py switches the timer off for the steps it does not sample
        self.active = True

    def start(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def stop(self, name, flops, e0, tag=None, nbytes=0.0, kernels=1):
        """``kernels``: device launches of the named kernel behind this call (8 for the
        parity-class backward-data), so that ms / launches is a per-kernel average."""
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        self.records.append((name, float(flops), e0, e1, tag, float(nbytes), int(kernels)))

    def by_tag(self):
        """{(kernel, tag): {flops, ms, launches, tflops}} -- per-layer view (tools/)."""
        torch.cuda.synchronize()
        agg = {}
        for name, flops, e0, e1, tag, _nb, _k in self.records:
            a = agg.setdefault((name, tag), [0.0, 0.0, 0])
            a[0] += flops
            a[1] += e0.elapsed_time(e1)
            a[2] += 1
        return {k: {"flops": v[0], "ms": v[1], "launches": v[2],
                    "tflops": v[0] / max(v[1], 1e-9) / 1e9} for k, v in agg.items()}

    def summary(self):
        if self._agg is None:
            torch.cuda.synchronize()
            agg = {}
            for name, flops, e0, e1, _tag, nb, k in self.records:
                a = agg.setdefault(name, [0.0, 0.0, 0, 0.0])
                a[0] += flops
                a[1] += e0.elapsed_time(e1)
                a[2] += k
                a[3] += nb
            self._agg = {k: {"flops": v[0], "ms": v[1], "launches": v[2],
                             "tflops": v[0] / max(v[1], 1e-9) / 1e9,
                             "algorithmic_bytes": v[3]} for k, v in agg.items()}
        return self._agg

    def dominant(self):
        """The kernel family with the most time among those that carry FLOPs (the HBM-bound
        families are recorded with flops = 0 and reported through their bytes)."""
        s = {k: v for k, v in self.summary().items() if v["flops"] > 0}
        if not s:
            return None
        name = max(s, key=lambda k: s[k]["ms"])
        return name, s[name]["flops"], s[name]["ms"], s[name]["launches"]

    def share(self, name, total_ms):
        return self.summary()[name]["ms"] / max(total_ms, 1e-9)


KERNEL_TIMER = None
# dispatch switches for A/B tests (read from the environment once at import)
FLAGS = {"no_cinfold": bool(os.environ.get("ADELL_NO_CINFOLD")),
         "no_convt_k2": bool(os.environ.get("ADELL_NO_CONVT_K2")),
         "no_grad_carry": bool(os.environ.get("ADELL_NO_GRAD_CARRY")),
         "no_skip_fork": bool(os.environ.get("ADELL_NO_SKIP_FORK")),
         "no_s2fused": bool(os.environ.get("ADELL_NO_S2FUSED")),
         # Linear layers on the f16x3 GEMM (1.2-2x the fp32-MFMA GEMM per launch) when both output
         # sides are >= 64: measured per step (bench.py secondary, alternating runs on one box) UNETR
         # 22.6 -> 21.8 ms, VICReg ConvNeXt 27.7 -> 24.8 ms, SWIN-UNet 198 -> 197.5 ms; with every
         # size SWIN's narrow projections (24 ... 48 wide) lose 1 % (round 3; round 5: 32-wide layers
         # over >= 64 k rows are streaming problems and take it too, gemm_f16x3_ok). ADELL_GEMM_F16X3=0: fp32-MFMA
         # GEMMs everywhere; =1: every applicable size (ADELL_GEMM_F16X3_MIN_K / _MIN_MN: knobs).
         "gemm_f16x3": os.environ.get("ADELL_GEMM_F16X3", "auto") != "0",
         "gemm_f16x3_min_k": int(os.environ.get("ADELL_GEMM_F16X3_MIN_K", "0")),
         "gemm_f16x3_min_mn": int(os.environ.get(
             "ADELL_GEMM_F16X3_MIN_MN", "64" if os.environ.get("ADELL_GEMM_F16X3", "auto") == "auto" else "0")),
         "no_cin_small": bool(os.environ.get("ADELL_NO_CIN_SMALL")),
         "cin_small_all": bool(os.environ.get("ADELL_CIN_SMALL_ALL"))}
NORM_ACT_FAMILY = "adell_norm_act_kernels"   # norm -> dropout -> activation, forward + backward


def _timed(name, flops, fn, tag=None, nbytes=0.0, kernels=1):
    t = KERNEL_TIMER
    if t is None or not t.active or (t.only is not None and name not in t.only):
        return fn()
    e0 = t.start()
    rc = fn()
    t.stop(name, flops, e0, tag() if callable(tag) else tag, nbytes, kernels)
    return rc


def _conv_bytes(d, residual=False):
    """Algorithmic HBM bytes of one conv launch (any direction): the input volume(s), the
    output volume (+ residual) and the weights, each touched once, fp32."""
    vin = d.N * d.D * d.H * d.W * (d.C0 + d.C1)
    vout = d.N * d.Do * d.Ho * d.Wo * d.Cout
    w = d.Cout * (d.C0 + d.C1) * d.KD * d.KH * d.KW
    return 4.0 * (vin + vout * (2 if residual else 1) + w)


def _conv_tag(d, kind):
    return lambda: (f"{kind} {d.C0 + d.C1}->{d.Cout} in {d.D}x{d.H}x{d.W} k{d.KD}{d.KH}{d.KW} "
                    f"s{d.SD}{d.SH}{d.SW}")


def _conv_flops(d):
    return 2.0 * d.N * d.Do * d.Ho * d.Wo * d.Cout * (d.C0 + d.C1) * d.KD * d.KH * d.KW


def _triple(v):
    if isinstance(v, (int,)):
        return (int(v),) * 3
    v = tuple(int(i) for i in v)
    if len(v) == 1:
        return v * 3
    assert len(v) == 3, v
    return v


_raw_stream = (None if os.environ.get("ADELL_TORCH_STREAM_API")
               else getattr(torch._C, "_cuda_getCurrentRawStream", None))


def _stream():
    """The current HIP stream of the current device as a raw handle (the private fast path
    when this torch build has it: ~0.3 us instead of ~10 us per launch)."""
    if _raw_stream is not None:
        return ctypes.c_void_p(_raw_stream(torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_CHECK_DENSE = bool(os.environ.get("ADELL_CHECK_DENSE"))


def _ptr(t):
    """Device address of ``t``. The kernels index dense memory (row-major, or NDHWC for 5-D / NHWC
    for 4-D activations). Always checked: an expanded view (a stride-0 dimension of size > 1) raises
    -- a kernel would read ``numel`` elements from a storage that holds fewer (the masked-attention
    backward at batch 1 did, round 4). With ADELL_CHECK_DENSE=1 (tests/conftest.py sets it) every
    other non-dense layout -- a slice with gaps, a permuted view -- raises too."""
    if t is None:
        return None
    st = t.stride()
    if 0 in st:
        for s, n in zip(st, t.shape):
            if s == 0 and n > 1:
                raise _lib.AdellHipError(f"expanded (stride-0) tensor handed to a kernel: shape "
                                         f"{tuple(t.shape)}, strides {st}")
    if _CHECK_DENSE and not (t.is_contiguous()
                             or (t.dim() == 5 and t.is_contiguous(memory_format=torch.channels_last_3d))
                             or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last))):
        raise _lib.AdellHipError(f"non-dense tensor handed to a kernel: shape {tuple(t.shape)}, "
                                 f"strides {st}")
    return ctypes.c_void_p(t.data_ptr())


def _require_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.AdellHipError(
                "adell_mri_amd kernels run on MI355X only: got a CPU tensor (no CPU fallback)")
        if t is not None and t.dtype != torch.float32:
            raise _lib.AdellHipError(f"adell_mri_amd kernels are fp32; got {t.dtype}")


def rng_advance(delta, set_value=False):
    """The library's replay counter of the dropout offsets (adell_rng_advance): add ``delta`` to the
    device word every dropout kernel adds to its offset argument, or set it. Stream-ordered; the
    last node of a captured training step (trainer.StepRunner.enable_graph)."""
    check(_lib.lib().adell_rng_advance(int(delta) & 0xFFFFFFFF, 1 if set_value else 0, _stream()))


def ndhwc(x):
    """Return a tensor sharing x's logical NCDHW shape whose memory is dense NDHWC."""
    if x.dim() != 5:
        raise _lib.AdellHipError(f"expected a 5-D [N,C,D,H,W] tensor, got {tuple(x.shape)}")
    # (the common case returns x itself: two permutes + a contiguity check cost 3.3 us of host time
    # per call, ~200 calls per UNETR step)
    if x.is_contiguous(memory_format=torch.channels_last_3d):
        return x
    xp = x.permute(0, 2, 3, 4, 1)
    if not xp.is_contiguous():
        xp = xp.contiguous()
    return xp.permute(0, 4, 1, 2, 3)


def bn_running_update(mean, rstd, running_mean, running_var, num_batches_tracked, count, eps,
                      momentum):
    """torch.nn.BatchNorm running statistics in training, in place, from the batch (mean, rstd) of
    stats_finalize(per_item=False) over ``count`` elements per channel (csrc/norm_act.hip)."""
    _require_cuda(mean, rstd, running_mean, running_var)
    nbt = num_batches_tracked
    if nbt is not None and (not nbt.is_cuda or nbt.dtype != torch.int64):
        raise _lib.AdellHipError("num_batches_tracked must be an int64 device tensor")
    check(_lib.lib().adell_bn_running_update(
        _ptr(mean), _ptr(rstd), _ptr(running_mean), _ptr(running_var),
        None if nbt is None else ctypes.c_void_p(nbt.data_ptr()), int(mean.numel()), int(count),
        float(eps), -1.0 if momentum is None else float(momentum), _stream()))


def window_ndhwc(x, out_size, offset):
    """out[n, :, d, h, w] = x[n, :, d + od, h + oh, w + ow] where that voxel exists, zeros elsewhere
    (csrc/layout.hip): ``x`` a dense-NDHWC [N, C, D, H, W] tensor; returns a dense-NDHWC tensor of the
    spatial size ``out_size``. Crop (positive offsets) and its gradient (negative offsets)."""
    _require_cuda(x)
    N, C, D, H, W = x.shape
    Do, Ho, Wo = (int(v) for v in out_size)
    out = new_act(N, C, Do, Ho, Wo, x.device)
    check(_lib.lib().adell_window_ndhwc(_ptr(x), _ptr(out), N, C, D, H, W, Do, Ho, Wo,
                                        int(offset[0]), int(offset[1]), int(offset[2]), _stream()))
    return out


def new_act(N, C, D, H, W, device):
    return torch.empty((N, D, H, W, C), device=device, dtype=torch.float32).permute(0, 4, 1, 2, 3)


def conv_out_size(size, k, s, p):
    return tuple((d + 2 * pp - kk) // ss + 1 for d, kk, ss, pp in zip(size, k, s, p))


def make_conv_desc(N, size, C0, C1, Cout, k, s, p):
    k, s, p = _triple(k), _triple(s), _triple(p)
    o = conv_out_size(size, k, s, p)
    return ConvDesc(N, *size, C0, C1, Cout, *k, *s, *p, *o)


def pack_weight(w, mode):
    """mode 0/1: conv weight [Cout,Cin,k,k,k]; mode 2/3: convT weight [Cin,Cout,2,2,2]."""
    _require_cuda(w)
    w = w.contiguous()
    out = torch.empty(w.numel(), device=w.device, dtype=torch.float32)
    d0, d1, kd, kh, kw = w.shape
    check(_lib.lib().adell_pack_weight(_ptr(w), _ptr(out), mode, d0, d1, kd, kh, kw, _stream()))
    return out


class SplitWeight:
    """Weights packed for the f16x3 kernel: fp16 hi/lo tiles + the scale-undo scalar."""

    __slots__ = ("halfs", "scale")

    def __init__(self, halfs, scale):
        self.halfs, self.scale = halfs, scale


def pack_weight_f16x3(w, mode):
    """mode 0: forward operand, mode 1: backward-data operand, of a conv weight
    [Cout, Cin, kD, kH, kW]."""
    _require_cuda(w)
    w = w.contiguous()
    d0, d1, kd, kh, kw = w.shape
    nbytes = _lib.lib().adell_pack_weight_f16x3_bytes(mode, d0, d1, kd * kh * kw)
    if nbytes < 0:
        check(int(nbytes))
    halfs = torch.empty(nbytes // 2, device=w.device, dtype=torch.float16)
    scale = torch.empty(d0 if mode == 0 else d1, device=w.device, dtype=torch.float32)
    check(_lib.lib().adell_pack_weight_f16x3(_ptr(w), _ptr(halfs), _ptr(scale), mode, d0, d1, kd,
                                             kh, kw, _stream()))
    return SplitWeight(halfs, scale)


def pack_weight_f16x3_multi(table, entries, total_blocks):
    """table: int64 [entries, 8] device tensor (see adell_pack_weight_f16x3_multi)."""
    if not (table.is_cuda and table.dtype == torch.int64 and table.is_contiguous()):
        raise AdellHipError("pack_weight_f16x3_multi: table must be a contiguous int64 CUDA tensor")
    check(_lib.lib().adell_pack_weight_f16x3_multi(_ptr(table), int(entries), int(total_blocks),
                                                   _stream()))


# conv launches that had to convert a split-row source back to fp32 (a plan that cannot stage rows)
ROWS_FALLBACKS = [0]


def _splitk_workspace(d, backward, device):
    """(workspace tensor or None, bytes) for the split-K path of the small (8^3 - 16^3) layers."""
    nbytes = _lib.lib().adell_conv3d_splitk_workspace(ctypes.byref(d), backward)
    if nbytes <= 0:
        return None, 0
    return _workspace(nbytes, device), nbytes


# launch plan of an f16x3 conv (adell_conv3d_f16x3_plan): config (8 = the 16-channel z-ring kernel),
# brick voxels, columns per tile, log2 brick extents, K shares (1 = no split-K), LDS bytes
ConvPlan = collections.namedtuple("ConvPlan", "cfg BM BN lTX lTY lTZ shares lds")


def conv3d_plan(N, in_size, C0, C1, Cout, kernel, stride, padding, backward_data=False):
    """The launch plan conv3d_fwd (or conv3d_bwd_data) would run on the f16x3 kernel; None when
    that kernel refuses the problem. Host only: no GPU needed."""
    d = make_conv_desc(N, tuple(in_size), C0, C1, Cout, kernel, stride, padding)
    out = (ctypes.c_int * 8)()
    rc = _lib.lib().adell_conv3d_f16x3_plan(ctypes.byref(d), int(bool(backward_data)), out)
    if rc == _lib.E_UNSUPPORTED:
        return None
    check(rc)
    return ConvPlan(*out)


def convtranspose3d_plan(N, in_size, Cin, Cout, factors=(2, 2, 2)):
    """The same for convtranspose3d_fwd on the f16x3 kernel (its backward-data is the
    kernel = stride conv3d_plan)."""
    out = (ctypes.c_int * 8)()
    rc = _lib.lib().adell_convtranspose3d_f16x3_plan(N, *in_size, Cin, Cout, *factors, out)
    if rc == _lib.E_UNSUPPORTED:
        return None
    check(rc)
    return ConvPlan(*out)


def conv3d_fwd(x0, w_packed, bias, Cout, kernel, stride, padding, x1=None, residual=None,
               want_stats=False, amax=None, rows0=None, rows1=None):
    """y = conv(cat(x0, x1)) + bias + residual ; optional (sum, sumsq) partials.
    ``w_packed``: fp32 GEMM-B tensor (exact fp32 MFMA) or a SplitWeight (f16x3 MFMA).
    ``rows0`` / ``rows1`` (SplitRows): that source holds split rows; a launch plan that cannot
    stage rows gets the fp32 tensor back first (rows_to_f32: one extra pass, counted in
    ROWS_FALLBACKS)."""
    split = isinstance(w_packed, SplitWeight)
    if rows0 is not None or rows1 is not None:
        N_, C0_ = x0.shape[:2]
        C1_ = 0 if x1 is None else x1.shape[1]
        if not (split and conv3d_rows_ok(N_, tuple(x0.shape[2:]), C0_, C1_, Cout, kernel, stride,
                                         padding)):
            ROWS_FALLBACKS[0] += 1
            if rows0 is not None:
                x0, rows0 = rows_to_f32(x0, rows0), None
            if rows1 is not None:
                x1, rows1 = rows_to_f32(x1, rows1), None
    if not split:
        _require_cuda(w_packed)
    _require_cuda(x0, x1, bias, residual)
    x0 = ndhwc(x0)
    N, C0, D, H, W = x0.shape
    C1 = 0
    if x1 is not None:
        x1 = ndhwc(x1)
        assert x1.shape[0] == N and tuple(x1.shape[2:]) == (D, H, W)
        C1 = x1.shape[1]
    d = make_conv_desc(N, (D, H, W), C0, C1, Cout, kernel, stride, padding)
    y = new_act(N, Cout, d.Do, d.Ho, d.Wo, x0.device)
    if residual is not None:
        residual = ndhwc(residual)
        assert tuple(residual.shape) == tuple(y.shape)
    part = None
    # the 32 -> 32 stride-2 downsampling layer: one persistent launch (csrc/conv_fwd_s2.hip)
    s2fused = (split and x1 is None and residual is None and not FLAGS["no_s2fused"]
               and bool(_lib.lib().adell_conv3d_fwd_s2_fused_applicable(ctypes.byref(d))))
    if rows0 is not None or rows1 is not None:
        s2fused = False
    if want_stats:
        fn = (_lib.lib().adell_conv3d_fwd_s2_fused_ntiles if s2fused
              else _lib.lib().adell_conv3d_fwd_ntiles_f16x3 if (rows0 is not None or rows1 is not None)
              else _lib.lib().adell_conv3d_fwd_ntiles_f16x3_ws if split
              else _lib.lib().adell_conv3d_fwd_ntiles)
        nt = fn(ctypes.byref(d))
        if nt < 0:
            check(nt)
        part = torch.empty((N, nt, Cout, 2), device=x0.device, dtype=torch.float32)
    rows = 0 if part is None else part.shape[1]    # checked by the library against its launch plan
    if rows0 is not None or rows1 is not None:
        check(_timed("adell_conv_igemm_f16_kernel", _conv_flops(d),
                     lambda: _lib.lib().adell_conv3d_fwd_f16x3_rows(
                         ctypes.byref(d), _ptr(x0), None if rows0 is None else _ptr(rows0.xk),
                         _ptr(x1), None if rows1 is None else _ptr(rows1.xk),
                         _ptr(w_packed.halfs), _ptr(w_packed.scale), _ptr(bias), _ptr(residual),
                         _ptr(y), _ptr(part), rows, _ptr(amax), _stream()), _conv_tag(d, "fwd"),
                     _conv_bytes(d, residual is not None)))
        return y, part
    if s2fused:
        check(_timed("adell_fwd_s2_fused_kernel", _conv_flops(d),
                     lambda: _lib.lib().adell_conv3d_fwd_s2_fused(
                         ctypes.byref(d), _ptr(x0), _ptr(w_packed.halfs), _ptr(w_packed.scale),
                         _ptr(bias), _ptr(y), _ptr(part), rows, _ptr(amax), _stream()),
                     _conv_tag(d, "fwd"), _conv_bytes(d)))
    elif split:
        ws, wsb = _splitk_workspace(d, 0, x0.device)
        check(_timed("adell_conv_igemm_f16_kernel", _conv_flops(d),
                     lambda: _lib.lib().adell_conv3d_fwd_f16x3_ws(
                         ctypes.byref(d), _ptr(x0), _ptr(x1), _ptr(w_packed.halfs),
                         _ptr(w_packed.scale), _ptr(bias), _ptr(residual), _ptr(y), _ptr(part),
                         rows, _ptr(amax), _ptr(ws), wsb, _stream()), _conv_tag(d, "fwd"),
                     _conv_bytes(d, residual is not None)))
    else:
        check(_timed("adell_conv_igemm_kernel", _conv_flops(d), lambda: _lib.lib().adell_conv3d_fwd(
            ctypes.byref(d), _ptr(x0), _ptr(x1), _ptr(w_packed), _ptr(bias), _ptr(residual),
            _ptr(y), _ptr(part), rows, _stream()), _conv_tag(d, "fwd"),
            _conv_bytes(d, residual is not None)))
    return y, part


# ---- convolutions with Cin <= 4 (the 2-channel input block): canonical weights, vector ALU ----
def conv_cin_small_ok(weight, x0, x1, stride, padding, residual):
    if residual is not None or x1 is not None or weight.dim() != 5 or x0.shape[1] > 4:
        return False
    if FLAGS["no_cin_small"]:
        return False
    k = tuple(weight.shape[2:])
    # measured at 128^3 (tools/bench_layers.py): 2 -> 2 0.21 ms here vs 0.34 ms on the MFMA path,
    # but 2 -> 32 is slower here (the vector ALU does 1728 FMAs per voxel): narrow outputs only
    if weight.shape[0] > 4 and not FLAGS["cin_small_all"]:
        return False
    return k[0] in (1, 3) and k[1:] == (3, 3) and tuple(stride) == (1, 1, 1)


def conv_cin_small_fwd(x, weight, bias, padding, want_stats):
    _require_cuda(x, weight, bias)
    x = ndhwc(x)
    N, Cin, D, H, W = x.shape
    Cout = weight.shape[0]
    d = make_conv_desc(N, (D, H, W), Cin, 0, Cout, tuple(weight.shape[2:]), 1, padding)
    y = new_act(N, Cout, d.Do, d.Ho, d.Wo, x.device)
    part = None
    wc = weight.contiguous()   # bound to a local: must outlive the launch
    if want_stats:
        nt = _lib.lib().adell_conv_cin_small_ntiles(ctypes.byref(d))
        if nt < 0:
            check(nt)
        part = torch.empty((N, nt, Cout, 2), device=x.device, dtype=torch.float32)
    check(_timed("adell_cin_small_kernel", _conv_flops(d),
                 lambda: _lib.lib().adell_conv_cin_small_fwd(
                     ctypes.byref(d), _ptr(x), _ptr(wc), _ptr(bias), _ptr(y),
                     _ptr(part), 0 if part is None else part.shape[1], _stream()),
                 _conv_tag(d, "fwd"), _conv_bytes(d)))
    return y, part


def conv_cin_small_bwd_data(dy, weight, in_size, padding):
    dy = ndhwc(dy)
    N, Cout = dy.shape[:2]
    Cin = weight.shape[1]
    d = make_conv_desc(N, tuple(in_size), Cin, 0, Cout, tuple(weight.shape[2:]), 1, padding)
    assert (d.Do, d.Ho, d.Wo) == tuple(dy.shape[2:])
    dx = new_act(N, Cin, *in_size, dy.device)
    wc = weight.contiguous()
    check(_timed("adell_cin_small_kernel", _conv_flops(d),
                 lambda: _lib.lib().adell_conv_cin_small_bwd_data(
                     ctypes.byref(d), _ptr(dy), _ptr(wc), _ptr(dx), _stream()),
                 _conv_tag(d, "dgrad"), _conv_bytes(d)))
    return dx


# ---- 3x3x3 stride-1 conv with 1..4 input channels and a wide output: K = 27 Cin GEMM per brick ---
def conv_cinfold_ok(weight, x0, x1, stride, padding, residual):
    """True when the im2col-GEMM kernels (csrc/conv_cinfold.hip) take this conv: they replace the
    x-tap fold + 16-channel MFMA chunk (forward) and the vector-ALU weight gradient."""
    if residual is not None or x1 is not None or weight.dim() != 5 or x0.dim() != 5:
        return False
    if FLAGS.get("no_cinfold") or x0.shape[1] > 4 or weight.shape[0] <= 4:
        return False
    return (tuple(weight.shape[2:]) == (3, 3, 3) and tuple(stride) == (1, 1, 1)
            and all(0 <= p <= 1 for p in padding))


def conv_cinfold_fwd(x, weight, bias, padding, want_stats, f16x3=False):
    """``f16x3``: the split-f16 MFMA kernel (two input channels) instead of the exact fp32 one."""
    _require_cuda(x, weight, bias)
    x = ndhwc(x)
    N, Cin, D, H, W = x.shape
    Cout = weight.shape[0]
    d = make_conv_desc(N, (D, H, W), Cin, 0, Cout, 3, 1, padding)
    y = new_act(N, Cout, d.Do, d.Ho, d.Wo, x.device)
    part = None
    wc = weight.contiguous()   # bound to a local: must outlive the launch
    if want_stats:
        nt = _lib.lib().adell_conv_cinfold_ntiles(ctypes.byref(d))
        if nt < 0:
            check(nt)
        part = torch.empty((N, nt, Cout, 2), device=x.device, dtype=torch.float32)
    fn = _lib.lib().adell_conv_cinfold_fwd_f16x3 if f16x3 else _lib.lib().adell_conv_cinfold_fwd
    check(_timed("adell_cinfold_kernel", _conv_flops(d),
                 lambda: fn(ctypes.byref(d), _ptr(x), _ptr(wc), _ptr(bias), _ptr(y), _ptr(part),
                            0 if part is None else part.shape[1], _stream()),
                 _conv_tag(d, "fwd"), _conv_bytes(d)))
    return y, part


def conv_cinfold_bwd_weight(x, dy, padding, want_db, f16x3=False):
    """(dw [Cout, Cin, 3, 3, 3], db or None). ``f16x3``: the split-f16 MFMA kernel (bound by the one
    pass over dy) instead of the exact fp32-MFMA one."""
    _require_cuda(x, dy)
    x, dy = ndhwc(x), ndhwc(dy)
    N, Cin, D, H, W = x.shape
    Cout = dy.shape[1]
    d = make_conv_desc(N, (D, H, W), Cin, 0, Cout, 3, 1, padding)
    assert (d.Do, d.Ho, d.Wo) == tuple(dy.shape[2:])
    nbytes = _lib.lib().adell_conv_cinfold_wgrad_workspace(ctypes.byref(d))
    check(min(nbytes, 0))
    ws = _workspace(nbytes, x.device)
    dw = torch.empty((Cout, Cin, 3, 3, 3), device=x.device, dtype=torch.float32)
    db = torch.empty(Cout, device=x.device, dtype=torch.float32) if want_db else None
    fn = (_lib.lib().adell_conv_cinfold_bwd_weight_f16x3 if f16x3
          else _lib.lib().adell_conv_cinfold_bwd_weight)
    check(_timed("adell_cinfold_kernel", _conv_flops(d),
                 lambda: fn(ctypes.byref(d), _ptr(x), _ptr(dy), _ptr(dw), _ptr(db), _ptr(ws),
                            ws.numel() * 4, _stream()), _conv_tag(d, "wgrad"), _conv_bytes(d)))
    return dw, db


def conv_cinfold_bwd_data(dy, weight, in_size, padding, f16x3=False):
    """dx [N, Cin, *in_size] of a narrow-input conv, or None when the kernel does not take the
    shape (Cout > 64 or not a multiple of 4: the caller falls to the implicit-GEMM kernel)."""
    _require_cuda(dy, weight)
    dy = ndhwc(dy)
    N, Cout = dy.shape[:2]
    Cin = weight.shape[1]
    d = make_conv_desc(N, tuple(in_size), Cin, 0, Cout, 3, 1, padding)
    assert (d.Do, d.Ho, d.Wo) == tuple(dy.shape[2:])
    if not _lib.lib().adell_conv_cinfold_dx_applicable(ctypes.byref(d)):
        return None
    dx = new_act(N, Cin, *in_size, dy.device)
    wc = weight.contiguous()
    fn = (_lib.lib().adell_conv_cinfold_bwd_data_f16x3 if f16x3
          else _lib.lib().adell_conv_cinfold_bwd_data)
    check(_timed("adell_cinfold_kernel", _conv_flops(d),
                 lambda: fn(ctypes.byref(d), _ptr(dy), _ptr(wc), _ptr(dx), _stream()),
                 _conv_tag(d, "dgrad"), _conv_bytes(d)))
    return dx


# ---- 1x1x1 convolution with Cout <= 4 (logits head): canonical weights, one pass each way ----
def conv1_small_ok(weight, Cin, stride, padding, residual):
    return (residual is None and weight.dim() == 5 and tuple(weight.shape[2:]) == (1, 1, 1)
            and weight.shape[0] <= 4 and Cin <= 512 and tuple(stride) == (1, 1, 1)
            and tuple(padding) == (0, 0, 0))


def _conv1_desc(N, size, C0, C1, Cout):
    return make_conv_desc(N, tuple(size), C0, C1, Cout, (1, 1, 1), (1, 1, 1), (0, 0, 0))


def conv1_small_fwd(x0, x1, weight, bias):
    _require_cuda(x0, x1, weight, bias)
    x0 = ndhwc(x0)
    N, C0, D, H, W = x0.shape
    C1 = 0
    if x1 is not None:
        x1 = ndhwc(x1)
        C1 = x1.shape[1]
    Cout = weight.shape[0]
    d = _conv1_desc(N, (D, H, W), C0, C1, Cout)
    y = new_act(N, Cout, D, H, W, x0.device)
    wc = weight.contiguous()
    check(_timed("adell_conv1_small_kernel", _conv_flops(d),
                 lambda: _lib.lib().adell_conv1_small_fwd(ctypes.byref(d), _ptr(x0), _ptr(x1),
                                                          _ptr(wc), _ptr(bias),
                                                          _ptr(y), _stream()),
                 _conv_tag(d, "fwd"), _conv_bytes(d)))
    return y


def conv1_small_bwd_data(dy, weight, in_size, C0, C1):
    dy = ndhwc(dy)
    N, Cout = dy.shape[:2]
    d = _conv1_desc(N, in_size, C0, C1, Cout)
    dx0 = new_act(N, C0, *in_size, dy.device)
    dx1 = new_act(N, C1, *in_size, dy.device) if C1 > 0 else None
    wc = weight.contiguous()
    check(_timed("adell_conv1_small_kernel", _conv_flops(d),
                 lambda: _lib.lib().adell_conv1_small_bwd_data(ctypes.byref(d), _ptr(dy),
                                                               _ptr(wc),
                                                               _ptr(dx0), _ptr(dx1), _stream()),
                 _conv_tag(d, "dgrad"), _conv_bytes(d)))
    return dx0, dx1


def conv1_small_bwd_weight(x0, x1, dy, want_db):
    x0, dy = ndhwc(x0), ndhwc(dy)
    N, C0, D, H, W = x0.shape
    C1 = 0
    if x1 is not None:
        x1 = ndhwc(x1)
        C1 = x1.shape[1]
    Cout = dy.shape[1]
    d = _conv1_desc(N, (D, H, W), C0, C1, Cout)
    ws = _workspace(_lib.lib().adell_conv1_small_wgrad_workspace(ctypes.byref(d)), x0.device)
    dw = torch.empty((Cout, C0 + C1, 1, 1, 1), device=x0.device, dtype=torch.float32)
    db = torch.empty((Cout,), device=x0.device, dtype=torch.float32) if want_db else None
    check(_timed("adell_conv1_small_kernel", _conv_flops(d),
                 lambda: _lib.lib().adell_conv1_small_bwd_weight(
                     ctypes.byref(d), _ptr(x0), _ptr(x1), _ptr(dy), _ptr(dw), _ptr(db), _ptr(ws),
                     ws.numel() * 4, _stream()), _conv_tag(d, "wgrad"), _conv_bytes(d)))
    return dw, db


def conv3d_bwd_data(dy, w_packed_bwd, in_size, C0, C1, kernel, stride, padding, amax=None,
                    add0=None):
    """``add0``: a tensor of dx0's shape added to it inside the kernel epilogue (f16x3 path, one
    destination); the caller adds it itself when this returns it unused (third value)."""
    split = isinstance(w_packed_bwd, SplitWeight)
    if add0 is not None and split and C1 == 0:
        _require_cuda(dy, add0)
        dy, add0 = ndhwc(dy), ndhwc(add0)
        N, Cout = dy.shape[:2]
        d = make_conv_desc(N, tuple(in_size), C0, 0, Cout, kernel, stride, padding)
        dx0 = new_act(N, C0, *in_size, dy.device)
        ws, wsb = _splitk_workspace(d, 1, dy.device)
        check(_timed("adell_conv_igemm_f16_kernel", _conv_flops(d),
                     lambda: _lib.lib().adell_conv3d_bwd_data_f16x3_add(
                         ctypes.byref(d), _ptr(dy), _ptr(w_packed_bwd.halfs),
                         _ptr(w_packed_bwd.scale), _ptr(add0), _ptr(dx0), _ptr(amax), _ptr(ws), wsb,
                         _stream()), _conv_tag(d, "dgrad"), _conv_bytes(d, True)))
        return dx0, None
    _require_cuda(dy)
    dy = ndhwc(dy)
    N, Cout = dy.shape[:2]
    d = make_conv_desc(N, tuple(in_size), C0, C1, Cout, kernel, stride, padding)
    assert (d.Do, d.Ho, d.Wo) == tuple(dy.shape[2:])
    dx0 = new_act(N, C0, *in_size, dy.device)
    dx1 = new_act(N, C1, *in_size, dy.device) if C1 > 0 else None
    if split:
        ws, wsb = _splitk_workspace(d, 1, dy.device)
        check(_timed("adell_conv_igemm_f16_kernel", _conv_flops(d),
                     lambda: _lib.lib().adell_conv3d_bwd_data_f16x3_ws(
                         ctypes.byref(d), _ptr(dy), _ptr(w_packed_bwd.halfs),
                         _ptr(w_packed_bwd.scale), _ptr(dx0), _ptr(dx1), _ptr(amax), _ptr(ws), wsb,
                         _stream()), _conv_tag(d, "dgrad"), _conv_bytes(d)))
    else:
        check(_timed("adell_conv_igemm_kernel", _conv_flops(d),
                     lambda: _lib.lib().adell_conv3d_bwd_data(
                         ctypes.byref(d), _ptr(dy), _ptr(w_packed_bwd), _ptr(dx0), _ptr(dx1),
                         _stream()), _conv_tag(d, "dgrad"), _conv_bytes(d)))
    return dx0, dx1


def plan_epoch():
    """The library's launch-plan epoch (adell_plan_epoch): changes with every adell_set_tuning flip;
    row counts taken from the *_ntiles queries are valid within one epoch."""
    return int(_lib.lib().adell_plan_epoch())


def conv3d_bwd_data_adn_ntiles(in_size, N, C0, C1, Cout, kernel, stride, padding):
    """Bricks per batch item when the backward-data of this conv takes the fused ADN epilogue
    (adell_conv3d_bwd_data_f16x3_adn), else 0."""
    d = make_conv_desc(N, tuple(in_size), C0, C1, Cout, kernel, stride, padding)
    return int(_lib.lib().adell_conv3d_bwd_data_f16x3_adn_ntiles(ctypes.byref(d)))


def _adn_site_struct(site):
    if site is None:
        return None
    return _lib.AdnSite(_ptr(site.x), _ptr(site.mean), _ptr(site.rstd), _ptr(site.mask),
                        float(site.drop_p), float(site.act_p), ACT_IDS[site.act])


def conv3d_bwd_data_adn(dy, w_packed_bwd, in_size, C0, C1, kernel, stride, padding, ntiles,
                        site0=None, site1=None, amax=None, add0=None):
    """Backward-data whose destinations are gradients of the outputs of norm -> dropout ->
    activation sites (``site0`` for dx0, ``site1`` for dx1; objects with x, mean, rstd, mask,
    drop_p, act, act_p): returns (dt0 or dx0, dt1 or dx1, partials [N, ntiles, C0 + C1, 2])."""
    _require_cuda(dy, add0)
    dy = ndhwc(dy)
    N, Cout = dy.shape[:2]
    d = make_conv_desc(N, tuple(in_size), C0, C1, Cout, kernel, stride, padding)
    assert (d.Do, d.Ho, d.Wo) == tuple(dy.shape[2:])
    if add0 is not None:
        add0 = ndhwc(add0)
    dx0 = new_act(N, C0, *in_size, dy.device)
    dx1 = new_act(N, C1, *in_size, dy.device) if C1 > 0 else None
    part = torch.empty((N, ntiles, C0 + C1, 2), device=dy.device, dtype=torch.float32)
    s0, s1 = _adn_site_struct(site0), _adn_site_struct(site1)
    extra = sum(4.0 * t.numel() for t, s in ((dx0, site0), (dx1, site1)) if s is not None)
    check(_timed("adell_conv_igemm_f16_kernel", _conv_flops(d),
                 lambda: _lib.lib().adell_conv3d_bwd_data_f16x3_adn(
                     ctypes.byref(d), _ptr(dy), _ptr(w_packed_bwd.halfs), _ptr(w_packed_bwd.scale),
                     _ptr(add0), _ptr(dx0), _ptr(dx1), _ptr(amax),
                     None if s0 is None else ctypes.byref(s0),
                     None if s1 is None else ctypes.byref(s1), _ptr(part), int(ntiles),
                     _stream()),
                 _conv_tag(d, "dgrad"), _conv_bytes(d, add0 is not None) + extra))
    return dx0, dx1, part


def conv3d_bwd_data_s2(dy, class_weights, in_size, C0, padding, amax=None, add0=None):
    """Backward-data of a stride-2 k = 3 conv by parity classes; ``class_weights``: 8 SplitWeights
    (c = 4 pz + 2 py + px) of the sub-kernels packed with mode 1. ``add0`` (dX-shaped) is added in
    the epilogue of the class launches."""
    _require_cuda(dy, add0)
    dy = ndhwc(dy)
    N, Cout = dy.shape[:2]
    d = make_conv_desc(N, tuple(in_size), C0, 0, Cout, 3, 2, padding)
    assert (d.Do, d.Ho, d.Wo) == tuple(dy.shape[2:])
    dx = new_act(N, C0, *in_size, dy.device)
    PA = ctypes.c_void_p * 8
    wh = PA(*[_ptr(w.halfs) for w in class_weights])
    ws = PA(*[_ptr(w.scale) for w in class_weights])
    if add0 is not None:
        add0 = ndhwc(add0)
        assert add0.shape == dx.shape
        call = lambda: _lib.lib().adell_conv3d_bwd_data_s2_f16x3_add(
            ctypes.byref(d), _ptr(dy), wh, ws, _ptr(add0), _ptr(dx), _ptr(amax), _stream())
    else:
        call = lambda: _lib.lib().adell_conv3d_bwd_data_s2_f16x3(
            ctypes.byref(d), _ptr(dy), wh, ws, _ptr(dx), _ptr(amax), _stream())
    check(_timed("adell_conv_igemm_f16_kernel", _conv_flops(d), call,
                 _conv_tag(d, "dgrad"), _conv_bytes(d), kernels=8))
    return dx


def conv3d_bwd_data_s2_fused_ok(in_size, C0, C1, Cout, kernel, stride, padding):
    """The one-launch backward-data of the 32 -> 32 stride-2 k = 3 padding-1 layer applies."""
    if FLAGS["no_s2fused"] or C1 != 0:
        return False
    d = make_conv_desc(1, tuple(in_size), C0, 0, Cout, kernel, stride, padding)
    return bool(_lib.lib().adell_conv3d_bwd_data_s2_fused_applicable(ctypes.byref(d)))


def conv3d_bwd_data_s2_fused(dy, w, in_size, amax=None, add0=None):
    """dX of that layer (csrc/conv_dgrad_s2.hip); ``w``: SplitWeight of the full weight, mode 1."""
    _require_cuda(dy, add0)
    dy = ndhwc(dy)
    N, Cout = dy.shape[:2]
    d = make_conv_desc(N, tuple(in_size), 32, 0, Cout, 3, 2, 1)
    assert (d.Do, d.Ho, d.Wo) == tuple(dy.shape[2:])
    dx = new_act(N, 32, *in_size, dy.device)
    if add0 is not None:
        add0 = ndhwc(add0)
        assert add0.shape == dx.shape
    check(_timed("adell_dgrad_s2_fused_kernel", _conv_flops(d),
                 lambda: _lib.lib().adell_conv3d_bwd_data_s2_fused(
                     ctypes.byref(d), _ptr(dy), _ptr(w.halfs), _ptr(w.scale), _ptr(add0), _ptr(dx),
                     _ptr(amax), _stream()),
                 _conv_tag(d, "dgrad"), _conv_bytes(d)))
    return dx


def _workspace(nbytes, device):
    return torch.empty((max(int(nbytes), 4) + 3) // 4, device=device, dtype=torch.float32)


def conv3d_bwd_weight_rows_ok(N, in_size, C0, C1, Cout, kernel, stride, padding):
    """The weight gradient of this conv reads split-row sources (z-ring kernel)."""
    d = make_conv_desc(N, tuple(in_size), C0, C1, Cout, kernel, stride, padding)
    return bool(_lib.lib().adell_conv3d_bwd_weight_f16x3_rows_ok(ctypes.byref(d)))


# launch plan of an f16x3 weight gradient (adell_conv3d_bwd_weight_f16x3_plan). route: one of
# WGRAD_ROUTES; R: partial slabs; instance: (MAXJ, PFX, PFY) of the per-plane kernel, else None;
# lTY .. grid: that kernel's geometry (else zeros); zring: the eight ints of adell_wgrad_zring_plan on
# the z-ring routes, else None; fp32_maxj: the instance conv3d_bwd_weight(f16x3=False) runs (0: none)
WGRAD_ROUTES = ("small", "zring32", "zring16", "s2", "plane")
WgradPlan = collections.namedtuple(
    "WgradPlan", "route R workspace rows_ok instance lTY TCI TCO ksplit lds grid zring fp32_maxj")


def conv3d_bwd_weight_plan(N, in_size, C0, C1, Cout, kernel, stride, padding):
    """What conv3d_bwd_weight(f16x3=True) would run under the current tuning switches; None when no
    kernel takes the problem. Host only: no GPU needed."""
    d = make_conv_desc(N, tuple(in_size), C0, C1, Cout, kernel, stride, padding)
    out = (ctypes.c_int * 25)()
    rc = _lib.lib().adell_conv3d_bwd_weight_f16x3_plan(ctypes.byref(d), out)
    if rc == _lib.E_UNSUPPORTED:
        return None
    check(rc)
    o = list(out)
    route = WGRAD_ROUTES[o[0]]
    return WgradPlan(route, o[1], o[2] + (o[3] << 31), bool(o[4]),
                     tuple(o[5:8]) if route == "plane" else None, o[8], o[9], o[10], o[11], o[12],
                     tuple(o[13:16]), tuple(o[16:24]) if route.startswith("zring") else None, o[24])


# what the z-ring weight gradient does with a share hint (adell_wgrad_zring_share_plan): zring: the
# eight ints of adell_wgrad_zring_plan; blocks_per_cu: resident blocks the launch is sized for (1: the
# hint was accepted); lds: dynamic LDS bytes it requests; room: LDS bytes of a CU left to another
# kernel's blocks beside them
WgradSharePlan = collections.namedtuple("WgradSharePlan", "zring blocks_per_cu lds room")


def conv3d_bwd_weight_share_plan(N, in_size, C0, C1, Cout, kernel, stride, padding, share):
    """The z-ring launch of conv3d_bwd_weight(f16x3=True, share=share); None when another kernel
    serves the problem. Host only: no GPU needed."""
    d = make_conv_desc(N, tuple(in_size), C0, C1, Cout, kernel, stride, padding)
    out = (ctypes.c_int * 11)()
    if not _lib.lib().adell_wgrad_zring_share_plan(ctypes.byref(d), int(share), out):
        return None
    o = list(out)
    return WgradSharePlan(tuple(o[:8]), o[8], o[9], o[10])


def conv3d_bwd_weight(x0, dy, kernel, stride, padding, x1=None, want_db=False, f16x3=False,
                      x_amax=None, dy_amax=None, rows0=None, rows1=None, share=False):
    """dW in torch's canonical [Cout, Cin, kD, kH, kW] layout (and db when want_db).
    f16x3: error-compensated f16 MFMA instead of the fp32 MFMA. ``rows0`` / ``rows1``
    (SplitRows): that source holds split rows (converted back when the kernel that serves the
    problem cannot read them: ROWS_FALLBACKS). ``share`` (f16x3 only): the launch runs beside
    another stream's kernels -- the z-ring kernel then leaves half of every CU to them
    (ADELL_WGRAD_SHARE_* of include/adell_hip.h; ``conv3d_bwd_weight_share_plan`` says what a hint
    does to a problem); the same bits either way. True: where the library expects it to pay (_AUTO);
    2: wherever the kernel form allows it (_ALWAYS)."""
    _require_cuda(x0, x1, dy)
    if rows0 is not None or rows1 is not None:
        ok = f16x3 and conv3d_bwd_weight_rows_ok(
            x0.shape[0], tuple(x0.shape[2:]), x0.shape[1], 0 if x1 is None else x1.shape[1],
            dy.shape[1], kernel, stride, padding)
        if not ok:
            ROWS_FALLBACKS[0] += 1
            if rows0 is not None:
                x0, rows0 = rows_to_f32(x0, rows0), None
            if rows1 is not None:
                x1, rows1 = rows_to_f32(x1, rows1), None
    x0, dy = ndhwc(x0), ndhwc(dy)
    N, C0, D, H, W = x0.shape
    C1 = 0
    if x1 is not None:
        x1 = ndhwc(x1)
        C1 = x1.shape[1]
    Cout = dy.shape[1]
    k = _triple(kernel)
    d = make_conv_desc(N, (D, H, W), C0, C1, Cout, kernel, stride, padding)
    assert (d.Do, d.Ho, d.Wo) == tuple(dy.shape[2:])
    L = _lib.lib()
    wsfn, fn, name = ((L.adell_conv3d_bwd_weight_f16x3_workspace, L.adell_conv3d_bwd_weight_f16x3,
                       "adell_conv_wgrad_f16_kernel") if f16x3 else
                      (L.adell_conv3d_bwd_weight_workspace, L.adell_conv3d_bwd_weight,
                       "adell_conv_wgrad_kernel"))
    nbytes = wsfn(ctypes.byref(d))
    if nbytes < 0:
        check(int(nbytes))
    ws = _workspace(nbytes, x0.device)
    dw = torch.empty((Cout, C0 + C1, *k), device=x0.device, dtype=torch.float32)
    db = torch.empty((Cout,), device=x0.device, dtype=torch.float32) if want_db else None
    # (no hint: the plain entry points, launch for launch what they always ran)
    hint = (int(share),) if share and f16x3 else ()
    if rows0 is not None or rows1 is not None:
        # (x_amax: the forward's by-product covers the fp32 source only, as this call needs it)
        rows_fn = (L.adell_conv3d_bwd_weight_f16x3_rows_share if hint
                   else L.adell_conv3d_bwd_weight_f16x3_rows)
        check(_timed(name, _conv_flops(d), lambda: rows_fn(
            ctypes.byref(d), _ptr(x0), None if rows0 is None else _ptr(rows0.xk), _ptr(x1),
            None if rows1 is None else _ptr(rows1.xk), _ptr(dy), _ptr(dw), _ptr(db), _ptr(x_amax),
            _ptr(dy_amax), _ptr(ws), ws.numel() * 4, _stream(), *hint), _conv_tag(d, "wgrad"),
                     _conv_bytes(d)))
    elif f16x3:
        if hint:
            fn = L.adell_conv3d_bwd_weight_f16x3_share
        check(_timed(name, _conv_flops(d), lambda: fn(
            ctypes.byref(d), _ptr(x0), _ptr(x1), _ptr(dy), _ptr(dw), _ptr(db), _ptr(x_amax),
            _ptr(dy_amax), _ptr(ws), ws.numel() * 4, _stream(), *hint), _conv_tag(d, "wgrad"),
                     _conv_bytes(d)))
    else:
        check(_timed(name, _conv_flops(d), lambda: fn(
            ctypes.byref(d), _ptr(x0), _ptr(x1), _ptr(dy), _ptr(dw), _ptr(db), _ptr(ws),
            ws.numel() * 4, _stream()), _conv_tag(d, "wgrad"), _conv_bytes(d)))
    return (dw, db) if want_db else dw


def bias_grad(dy):
    _require_cuda(dy)
    dy = ndhwc(dy)
    C = dy.shape[1]
    rows = dy.numel() // C
    nbytes = _lib.lib().adell_bias_grad_workspace(rows, C)
    ws = _workspace(nbytes, dy.device)
    db = torch.empty((C,), device=dy.device, dtype=torch.float32)
    check(_lib.lib().adell_bias_grad(_ptr(dy), rows, C, _ptr(db), _ptr(ws), ws.numel() * 4,
                                     _stream()))
    return db


def convtranspose3d_bwd_weight(x, dy, factors=(2, 2, 2)):
    """dW in torch's canonical [Cin, Cout, FD, FH, FW] layout (kernel = stride = factors)."""
    _require_cuda(x, dy)
    x, dy = ndhwc(x), ndhwc(dy)
    N, Cin, D, H, W = x.shape
    Cout = dy.shape[1]
    fd, fh, fw = factors
    nbytes = _lib.lib().adell_convtranspose3d_bwd_weight_workspace(N, D, H, W, Cin, Cout, fd, fh, fw)
    if nbytes < 0:
        check(int(nbytes))
    ws = _workspace(nbytes, x.device)
    dw = torch.empty((Cin, Cout, fd, fh, fw), device=x.device, dtype=torch.float32)
    flops = 2.0 * N * D * H * W * Cin * Cout * fd * fh * fw
    check(_timed("adell_conv_wgrad_kernel", flops, lambda: _lib.lib().adell_convtranspose3d_bwd_weight(
        N, D, H, W, Cin, Cout, fd, fh, fw, _ptr(x), _ptr(dy), _ptr(dw), _ptr(ws), ws.numel() * 4,
        _stream())))
    return dw


# ---- factor-2 transposed conv with 32 / 64 channels: streaming GEMMs, canonical weights ----------
def _convt_k2_fns(factors):
    L = _lib.lib()
    if tuple(factors) == (2, 2, 2):
        return (L.adell_convt_k2_applicable, L.adell_convt_k2_fwd, L.adell_convt_k2_bwd_data,
                L.adell_convt_k2_wgrad_workspace, L.adell_convt_k2_bwd_weight)
    if tuple(factors) == (2, 2, 1):
        return (L.adell_convt_k221_applicable, L.adell_convt_k221_fwd, L.adell_convt_k221_bwd_data,
                L.adell_convt_k221_wgrad_workspace, L.adell_convt_k221_bwd_weight)
    return None


def convt_k2_ok(x_shape, weight):
    """True when csrc/convt_k2.hip takes ConvTranspose3d(x) with this weight [Cin, Cout, 2, 2, 2]
    (or [Cin, Cout, 2, 2, 1]: depth and height doubled, width kept)."""
    if FLAGS.get("no_convt_k2") or weight.dim() != 5:
        return False
    fns = _convt_k2_fns(weight.shape[2:])
    if fns is None:
        return False
    N, _, D, H, W = x_shape
    return bool(fns[0](N, D, H, W, weight.shape[0], weight.shape[1]))


def convt_k2_fwd(x, weight, bias):
    _require_cuda(x, weight, bias)
    x = ndhwc(x)
    N, Cin, D, H, W = x.shape
    Cout = weight.shape[1]
    f = tuple(weight.shape[2:])
    y = new_act(N, Cout, f[0] * D, f[1] * H, f[2] * W, x.device)
    wc = weight.contiguous()   # bound to a local: must outlive the launch
    fn = _convt_k2_fns(f)[1]
    nf = f[0] * f[1] * f[2]
    check(_timed("adell_convt_k2_kernel", 2.0 * nf * N * D * H * W * Cin * Cout,
                 lambda: fn(N, D, H, W, Cin, Cout, _ptr(x), _ptr(wc), _ptr(bias), _ptr(y), _stream()),
                 f"convT fwd {Cin}->{Cout} in {D}x{H}x{W} f{f[0]}{f[1]}{f[2]}",
                 4.0 * (x.numel() + y.numel())))
    return y


def convt_k2_bwd_data(dy, weight):
    _require_cuda(dy, weight)
    dy = ndhwc(dy)
    N, Cout, D2, H2, W2 = dy.shape
    Cin = weight.shape[0]
    f = tuple(weight.shape[2:])
    D, H, W = D2 // f[0], H2 // f[1], W2 // f[2]
    dx = new_act(N, Cin, D, H, W, dy.device)
    wc = weight.contiguous()
    fn = _convt_k2_fns(f)[2]
    nf = f[0] * f[1] * f[2]
    check(_timed("adell_convt_k2_kernel", 2.0 * nf * N * D * H * W * Cin * Cout,
                 lambda: fn(N, D, H, W, Cin, Cout, _ptr(dy), _ptr(wc), _ptr(dx), _stream()),
                 f"convT dgrad {Cin}->{Cout} in {D}x{H}x{W} f{f[0]}{f[1]}{f[2]}",
                 4.0 * (dy.numel() + dx.numel())))
    return dx


def convt_k2_bwd_weight(x, dy, want_db=False, factors=(2, 2, 2)):
    """dW (and, with want_db, the bias gradient from the same pass over dy: returns (dw, db))."""
    _require_cuda(x, dy)
    x, dy = ndhwc(x), ndhwc(dy)
    N, Cin, D, H, W = x.shape
    Cout = dy.shape[1]
    f = tuple(factors)
    fns = _convt_k2_fns(f)
    nbytes = fns[3](N, D, H, W, Cin, Cout)
    check(min(nbytes, 0))
    ws = _workspace(nbytes, x.device)
    dw = torch.empty((Cin, Cout, *f), device=x.device, dtype=torch.float32)
    db = torch.empty(Cout, device=x.device, dtype=torch.float32) if want_db else None
    nf = f[0] * f[1] * f[2]
    check(_timed("adell_convt_k2_kernel", 2.0 * nf * N * D * H * W * Cin * Cout,
                 lambda: fns[4](N, D, H, W, Cin, Cout, _ptr(x), _ptr(dy), _ptr(dw), _ptr(db), _ptr(ws),
                                ws.numel() * 4, _stream()),
                 f"convT wgrad {Cin}->{Cout} in {D}x{H}x{W} f{f[0]}{f[1]}{f[2]}",
                 4.0 * (x.numel() + dy.numel())))
    return (dw, db) if want_db else dw


def convtranspose3d_k2s2_bwd_weight(x, dy):
    return convtranspose3d_bwd_weight(x, dy, (2, 2, 2))


def convtranspose3d_fwd(x, w_packed, bias, Cout, factors=(2, 2, 2)):
    """ConvTranspose3d with kernel = stride = factors (each 1 or 2), padding 0. ``w_packed``:
    fp32 pack (mode 2) or the SplitWeight of the virtual 1x1x1 weight (f16x3)."""
    _require_cuda(x, bias)
    x = ndhwc(x)
    N, Cin, D, H, W = x.shape
    fd, fh, fw = factors
    y = new_act(N, Cout, fd * D, fh * H, fw * W, x.device)
    flops = 2.0 * N * D * H * W * Cin * Cout * fd * fh * fw
    if isinstance(w_packed, SplitWeight):
        check(_timed("adell_conv_igemm_f16_kernel", flops,
                     lambda: _lib.lib().adell_convtranspose3d_fwd_f16x3(
                         N, D, H, W, Cin, Cout, fd, fh, fw, _ptr(x), _ptr(w_packed.halfs),
                         _ptr(w_packed.scale), _ptr(bias), _ptr(y), None, _stream()),
                     f"convT fwd {Cin}->{Cout} in {D}x{H}x{W} f{fd}{fh}{fw}",
                     4.0 * (x.numel() + y.numel())))
        return y
    _require_cuda(w_packed)
    check(_timed("adell_conv_igemm_kernel", flops, lambda: _lib.lib().adell_convtranspose3d_fwd(
        N, D, H, W, Cin, Cout, fd, fh, fw, _ptr(x), _ptr(w_packed), _ptr(bias), _ptr(y),
        _stream())))
    return y


def convtranspose3d_bwd_data(dy, w_packed_bwd, Cin, factors=(2, 2, 2)):
    _require_cuda(dy)
    dy = ndhwc(dy)
    N, Cout, D2, H2, W2 = dy.shape
    fd, fh, fw = factors
    D, H, W = D2 // fd, H2 // fh, W2 // fw
    dx = new_act(N, Cin, D, H, W, dy.device)
    flops = 2.0 * N * D * H * W * Cin * Cout * fd * fh * fw
    if isinstance(w_packed_bwd, SplitWeight):
        check(_timed("adell_conv_igemm_f16_kernel", flops,
                     lambda: _lib.lib().adell_convtranspose3d_bwd_data_f16x3(
                         N, D, H, W, Cin, Cout, fd, fh, fw, _ptr(dy), _ptr(w_packed_bwd.halfs),
                         _ptr(w_packed_bwd.scale), _ptr(dx), None, _stream()),
                     f"convT dgrad {Cin}->{Cout} in {D}x{H}x{W} f{fd}{fh}{fw}",
                     4.0 * (dy.numel() + dx.numel())))
        return dx
    _require_cuda(w_packed_bwd)
    check(_timed("adell_conv_igemm_kernel", flops, lambda: _lib.lib().adell_convtranspose3d_bwd_data(
        N, D, H, W, Cin, Cout, fd, fh, fw, _ptr(dy), _ptr(w_packed_bwd), _ptr(dx), _stream())))
    return dx


def convtranspose3d_k2s2_fwd(x, w_packed, bias, Cout):
    return convtranspose3d_fwd(x, w_packed, bias, Cout, (2, 2, 2))


def convtranspose3d_k2s2_bwd_data(dy, w_packed_bwd, Cin):
    return convtranspose3d_bwd_data(dy, w_packed_bwd, Cin, (2, 2, 2))


def stats_finalize(partials, count, eps, per_item=True):
    """(mean, rstd): [N, C] per item (instance norm) or [C] over the batch (batch norm)."""
    N, nt, C, _ = partials.shape
    mean = torch.empty((N, C) if per_item else (C,), device=partials.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    nbytes = _lib.lib().adell_stats_finalize_workspace(N, nt, C)
    ws = _workspace(nbytes, partials.device) if nbytes > 0 else None
    check(_lib.lib().adell_stats_finalize(_ptr(partials), N, nt, C, int(count), float(eps),
                                          1 if per_item else 0, _ptr(mean), _ptr(rstd), _ptr(ws),
                                          0 if ws is None else ws.numel() * 4, _stream()))
    return mean, rstd


# ---- synchronised batch norm: a site's reductions split around one all-reduce per direction ----
def _record(C, device):
    """The 2C + 1 fp64 record a synchronised batch-norm site all-reduces (csrc/norm_act.hip)."""
    return torch.empty((2 * C + 1,), device=device, dtype=torch.float64)


def _record_check(rec, C):
    if not rec.is_cuda or rec.dtype != torch.float64 or rec.numel() != 2 * C + 1 or not rec.is_contiguous():
        raise _lib.AdellHipError(f"a batch-norm record is a dense fp64 device tensor of 2C + 1 = "
                                 f"{2 * C + 1} values; got {rec.dtype} {tuple(rec.shape)}")


def bn_stats_sums(partials, count):
    """The forward record [sum x (C) | sum x^2 (C) | count] of a batch-norm site from partials
    [N, ntiles, C, 2] (channel_partials or a conv epilogue's), ``count`` elements per item: what
    the ranks of a synchronised batch norm sum. Same fold as stats_finalize(per_item=False)."""
    _require_cuda(partials)
    N, nt, C, _ = partials.shape
    rec = _record(C, partials.device)
    nbytes = _lib.lib().adell_stats_finalize_workspace(N, nt, C)
    ws = _workspace(nbytes, partials.device) if nbytes > 0 else None
    check(_lib.lib().adell_bn_stats_sums(_ptr(partials), N, nt, C, int(count), _ptr(rec), _ptr(ws),
                                         0 if ws is None else ws.numel() * 4, _stream()))
    return rec


def bn_stats_from_sums(rec, eps, running=None, momentum=0.1):
    """(mean, rstd) [C] of a (reduced) forward record, stats_finalize's formula; with ``running`` =
    (running_mean, running_var, num_batches_tracked) also bn_running_update with the record's
    count, in the same launch."""
    C = (rec.numel() - 1) // 2
    _record_check(rec, C)
    mean = torch.empty((C,), device=rec.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    rm = rv = nbt = None
    if running is not None and running[0] is not None:
        rm, rv, nbt = running
        _require_cuda(rm, rv)
        if nbt is not None and (not nbt.is_cuda or nbt.dtype != torch.int64):
            raise _lib.AdellHipError("num_batches_tracked must be an int64 device tensor")
        if nbt is None and momentum is None:
            raise ValueError("BatchNorm with momentum=None needs num_batches_tracked")
    check(_lib.lib().adell_bn_stats_from_sums(
        _ptr(rec), C, float(eps), _ptr(mean), _ptr(rstd), _ptr(rm), _ptr(rv),
        None if nbt is None else ctypes.c_void_p(nbt.data_ptr()),
        -1.0 if momentum is None else float(momentum), _stream()))
    return mean, rstd


def norm_act_bwd_sums(x, dout, mean, rstd, act, gamma=None, beta=None, act_w=None, act_p=0.0,
                      drop_p=0.0, seed=0, rng_offset=0, want_affine_grads=False):
    """First half of norm_act_bwd at a batch-norm site: the record [sum dt (C) | sum dt * xhat (C) |
    count] the ranks sum, and the local (dgamma, dbeta) when want_affine_grads."""
    _require_cuda(x, dout, mean, rstd, gamma, beta, act_w)
    x, dout = ndhwc(x), ndhwc(dout)
    C = x.shape[1]
    d = make_na_desc(x, act, 0, act_p, 0 if act_w is None else act_w.numel(), drop_p, seed,
                     rng_offset)
    rec = _record(C, x.device)
    dgamma = dbeta = None
    if want_affine_grads:
        dgamma = torch.empty((C,), device=x.device, dtype=torch.float32)
        dbeta = torch.empty_like(dgamma)
    ws = _workspace(_lib.lib().adell_norm_act_bwd_workspace(ctypes.byref(d)), x.device)
    # algorithmic bytes: read x and dout once
    check(_timed(NORM_ACT_FAMILY, 0.0, lambda: _lib.lib().adell_norm_act_bwd_sums(
        ctypes.byref(d), _ptr(x), _ptr(dout), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta),
        _ptr(act_w), _ptr(rec), _ptr(dgamma), _ptr(dbeta), _ptr(ws), ws.numel() * 4, _stream()),
        "bwd_sums", 8.0 * x.numel()))
    return rec, dgamma, dbeta


def norm_act_bwd_apply_sums(x, dout, mean, rstd, rec, act, gamma=None, beta=None, act_w=None,
                            act_p=0.0, drop_p=0.0, seed=0, rng_offset=0):
    """Second half: dx of a batch-norm site from a (reduced) backward record."""
    _require_cuda(x, dout, mean, rstd, gamma, beta, act_w)
    x, dout = ndhwc(x), ndhwc(dout)
    C = x.shape[1]
    _record_check(rec, C)
    d = make_na_desc(x, act, 0, act_p, 0 if act_w is None else act_w.numel(), drop_p, seed,
                     rng_offset)
    dx = new_act(*x.shape, x.device)
    ws = _workspace(8 * C, x.device)
    # algorithmic bytes: read x and dout once, write dx once
    check(_timed(NORM_ACT_FAMILY, 0.0, lambda: _lib.lib().adell_norm_act_bwd_apply_sums(
        ctypes.byref(d), _ptr(x), _ptr(dout), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta),
        _ptr(act_w), _ptr(rec), _ptr(dx), _ptr(ws), ws.numel() * 4, _stream()),
        "bwd_apply", 12.0 * x.numel()))
    return dx


def channel_partials(x):
    _require_cuda(x)
    x = ndhwc(x)
    N, C = x.shape[:2]
    V = x.shape[2] * x.shape[3] * x.shape[4]
    nt = _lib.lib().adell_channel_partials_ntiles(V)
    part = torch.empty((N, nt, C, 2), device=x.device, dtype=torch.float32)
    check(_lib.lib().adell_channel_partials(_ptr(x), N, V, C, _ptr(part), _stream()))
    return part


def instance_stats(x, eps=1e-5, partials=None):
    """(mean, rstd) of shape [N, C] over the spatial dims of x."""
    if partials is None:
        partials = channel_partials(x)
    V = x.shape[2] * x.shape[3] * x.shape[4]
    return stats_finalize(partials, V, eps)


def make_na_desc(x, act, stats_per_item=1, act_p=0.0, act_w_n=0, drop_p=0.0, seed=0,
                 rng_offset=0):
    N, C = x.shape[:2]
    V = x.shape[2] * x.shape[3] * x.shape[4]
    act_id = ACT_IDS[act] if isinstance(act, str) else int(act)
    return NormActDesc(N, V, C, stats_per_item, act_id, act_w_n, float(act_p), float(drop_p),
                       int(seed) & 0xFFFFFFFFFFFFFFFF, int(rng_offset) & 0xFFFFFFFF)


def norm_act_mask_ok(x):
    """The forward can store its dropout keep bits (the bandwidth-tuned kernel runs: power-of-two
    channel count from 4 to 1024, 16-byte aligned NDHWC tensor; norm_act_plan's "fast" route). All
    four words of every 256-element group are then written -- also of an item's last group when it
    holds fewer than four float4 (C = 4 or 8 with few voxels left) -- and the bits past the end of
    an item are 0."""
    C = x.shape[1]
    return x.dim() == 5 and C % 4 == 0 and C <= 1024 and (C & (C - 1)) == 0


# launch plan of a norm / dropout / activation site (adell_norm_act_plan). fwd, bwd: one of NA_ROUTES;
# fwd_grid, apply_grid: (x, y) of the forward / dx launch; rows: partial rows per item the backward's
# reduction pass writes (0: none); finalize: one of NA_FINALIZE; workspace: bytes norm_act_bwd
# requires; mask_bytes: keep bits the forward stores
NormActPlan = collections.namedtuple(
    "NormActPlan", "fwd fwd_grid bwd rows apply_grid finalize workspace mask_bytes")
NA_ROUTES = ("scalar", "float4", "fast", "narrow", "refused")
NA_FINALIZE = ("none", "per_item", "all_items")
_NA_ALIGNED = {"x": 1, "out": 2, "dout": 4, "dx": 8}
# reduction of a chain of partial rows (adell_norm_act_stats_plan). levels: 1 or 2; Z: rows per item
# after the first level; workspace: bytes of the folded rows; unroll8_from / unroll2_from: rows from
# which the all-items (and record) / per-item backward finalize kernels enter their unrolled loops
NormActStatsPlan = collections.namedtuple("NormActStatsPlan",
                                          "levels Z workspace unroll8_from unroll2_from")


def norm_act_plan(N, V, C, stats_per_item=1, drop_p=0.0, unaligned=(), want_mask=False, split=False,
                  lowrank=0, norm=True, affine_grads=False):
    """What norm_act_fwd / norm_act_bwd (and their _mask, _split, _lowrank, _sums, _from_dt forms)
    launch for a site of N items of V voxels and C channels. ``unaligned``: names among "x", "out",
    "dout", "dx" of the tensors that are NOT 16-byte aligned (none, from torch, unless a view starts
    inside a storage). Host only: no GPU needed."""
    d = NormActDesc(int(N), int(V), int(C), int(stats_per_item), 0, 0, 0.0, float(drop_p), 0, 0)
    al = sum(bit for name, bit in _NA_ALIGNED.items() if name not in unaligned)
    assert set(unaligned) <= set(_NA_ALIGNED), unaligned
    out = (ctypes.c_long * 10)()
    check(_lib.lib().adell_norm_act_plan(ctypes.byref(d), al, int(bool(want_mask)), int(bool(split)),
                                         int(lowrank), int(bool(norm)), int(bool(affine_grads)), out))
    o = list(out)
    return NormActPlan(NA_ROUTES[o[0]], (o[1], o[2]), NA_ROUTES[o[3]], o[4], (o[5], o[6]),
                       NA_FINALIZE[o[7]], o[8], o[9])


def norm_act_stats_plan(N, ntiles, C):
    """How stats_finalize, bn_stats_sums and norm_act_bwd_from_dt reduce ``ntiles`` partial rows per
    item (host only)."""
    out = (ctypes.c_long * 5)()
    check(_lib.lib().adell_norm_act_stats_plan(int(N), int(ntiles), int(C), out))
    return NormActStatsPlan(*list(out))


# ---- split rows: activations stored as the f16x3 kernels' LDS row image ------------------------------
class SplitRows:
    """Marks a tensor whose MEMORY holds, per voxel and 16-channel chunk, the 64-byte row
    [hi c0-7 | hi c8-15 | lo c0-7 | lo c8-15] of fp16 values of x * 2^exp (conv_igemm_f16.h) instead
    of fp32 values -- same logical shape [N, C, D, H, W], dtype and byte count. ``xk``: int32 device
    tensor [N, C / 16] of exponents (one value per tensor for the producers built so far: ``exp``)."""

    __slots__ = ("exp", "xk")

    def __init__(self, exp, xk):
        self.exp, self.xk = int(exp), xk


_XK_CACHE = {}


def split_exponents(N, C, exp, device):
    """Constant exponent table [N, C / 16] (cached: a handful of distinct (N, C, exp) per model)."""
    key = (device, int(N) * (int(C) // 16), int(exp))
    t = _XK_CACHE.get(key)
    if t is None:
        t = _XK_CACHE[key] = torch.full((key[1],), int(exp), device=device, dtype=torch.int32)
    return t


def rows_from_f32(x, exp):
    """fp32 NDHWC activation -> (tensor of split rows, SplitRows); |x| * 2^exp must stay below 2^15."""
    _require_cuda(x)
    x = ndhwc(x)
    N, C = x.shape[:2]
    V = x.numel() // (N * C)
    xk = split_exponents(N, C, exp, x.device)
    out = new_act(*x.shape, x.device)
    check(_lib.lib().adell_split_rows_from_f32(_ptr(x), N, V, C, _ptr(xk), _ptr(out), _stream()))
    return out, SplitRows(exp, xk)


def rows_to_f32(rows, sr):
    """The fp32 tensor a split-row tensor stands for ((hi + lo) * 2^-exp: 22 mantissa bits)."""
    _require_cuda(rows)
    rows = ndhwc(rows)
    N, C = rows.shape[:2]
    V = rows.numel() // (N * C)
    out = new_act(*rows.shape, rows.device)
    check(_lib.lib().adell_split_rows_to_f32(_ptr(rows), N, V, C, _ptr(sr.xk), _ptr(out), _stream()))
    return out


def conv3d_rows_ok(N, in_size, C0, C1, Cout, kernel, stride, padding):
    """The forward of this conv stages split-row sources (specialised f16x3 instances)."""
    k, st = _triple(kernel), _triple(stride)
    if k != (3, 3, 3) or st != (1, 1, 1) or C0 % 16 or C1 % 16:
        return False
    d = make_conv_desc(N, tuple(in_size), C0, C1, Cout, kernel, stride, padding)
    return bool(_lib.lib().adell_conv3d_f16x3_rows_ok(ctypes.byref(d)))


def norm_act_fwd(x, mean, rstd, act, gamma=None, beta=None, act_w=None, act_p=0.0,
                 stats_per_item=1, drop_p=0.0, seed=0, rng_offset=0, want_mask=False,
                 split_exp=None):
    """``want_mask`` (drop_p > 0): also returns the keep bits as an int64 tensor (1 bit per
    element) for the fused backward (conv3d_bwd_data_adn). ``split_exp``: the output is written as
    SPLIT ROWS scaled by 2^split_exp (SplitRows below) instead of fp32 values -- same shape, dtype
    and bytes, readable only by consumers that take rows (conv3d_fwd / conv3d_bwd_weight)."""
    _require_cuda(x, mean, rstd, gamma, beta, act_w)
    x = ndhwc(x)
    d = make_na_desc(x, act, stats_per_item, act_p, 0 if act_w is None else act_w.numel(),
                     drop_p, seed, rng_offset)
    out = new_act(*x.shape, x.device)
    mask = None
    if want_mask and drop_p > 0.0:
        nbytes = _lib.lib().adell_norm_act_mask_bytes(ctypes.byref(d))
        if nbytes < 0:
            check(int(nbytes))
        mask = torch.empty((nbytes // 8,), device=x.device, dtype=torch.int64)
    # HBM-bound family of the roofline report: algorithmic bytes = read x + write out
    if split_exp is not None:
        check(_timed(NORM_ACT_FAMILY, 0.0, lambda: _lib.lib().adell_norm_act_fwd_split(
            ctypes.byref(d), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(act_w),
            _ptr(out), int(split_exp), _ptr(mask), _stream()), "fwd", 8.0 * x.numel()))
    elif mask is not None:
        check(_timed(NORM_ACT_FAMILY, 0.0, lambda: _lib.lib().adell_norm_act_fwd_mask(
            ctypes.byref(d), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(act_w),
            _ptr(out), _ptr(mask), _stream()), "fwd", 8.0 * x.numel()))
    else:
        check(_timed(NORM_ACT_FAMILY, 0.0, lambda: _lib.lib().adell_norm_act_fwd(
            ctypes.byref(d), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(act_w),
            _ptr(out), _stream()), "fwd", 8.0 * x.numel()))
    return (out, mask) if want_mask else out


def norm_act_bwd_from_dt(x, dt, mean, rstd, partials, poff=0):
    """dx of an instance-norm site from dt = dout * act'(u) * keep / (1 - p) and the per-brick
    sums the fused backward-data epilogue left in ``partials`` [N, ntiles, pstride, 2] (the site's
    channels at columns [poff, poff + C)). Written in place over ``dt``."""
    _require_cuda(x, dt, mean, rstd, partials)
    x, dt = ndhwc(x), ndhwc(dt)
    d = make_na_desc(x, "identity", 1)
    N, C = x.shape[:2]
    ws = _workspace(4 * (2 + 2 * ((int(partials.shape[1]) + 255) // 256)) * N * C, x.device)
    check(_timed(NORM_ACT_FAMILY, 0.0, lambda: _lib.lib().adell_norm_act_bwd_from_dt(
        ctypes.byref(d), _ptr(x), _ptr(dt), _ptr(mean), _ptr(rstd), _ptr(partials),
        int(partials.shape[1]), int(partials.shape[2]), int(poff), _ptr(dt), _ptr(ws),
        ws.numel() * 4, _stream()), "bwd", 12.0 * x.numel()))
    return dt


def prelu_wgrad(x, dout, mean, rstd, act_w, gamma=None, beta=None, stats_per_item=1, drop_p=0.0,
                seed=0, rng_offset=0):
    """Gradient of the PReLU weight(s) of norm -> dropout -> PReLU (same operands as
    norm_act_bwd)."""
    _require_cuda(x, dout, mean, rstd, gamma, beta, act_w)
    x, dout = ndhwc(x), ndhwc(dout)
    d = make_na_desc(x, "prelu", stats_per_item, 0.0, act_w.numel(), drop_p, seed, rng_offset)
    ws = _workspace(_lib.lib().adell_prelu_wgrad_workspace(ctypes.byref(d)), x.device)
    dw = torch.empty_like(act_w)
    check(_lib.lib().adell_prelu_wgrad(ctypes.byref(d), _ptr(x), _ptr(dout), _ptr(mean), _ptr(rstd),
                                       _ptr(gamma), _ptr(beta), _ptr(dw), _ptr(ws),
                                       ws.numel() * 4, _stream()))
    return dw


def norm_act_bwd(x, dout, mean, rstd, act, gamma=None, beta=None, act_w=None, act_p=0.0,
                 stats_per_item=1, drop_p=0.0, seed=0, rng_offset=0, want_affine_grads=False):
    """dx (and dgamma, dbeta when want_affine_grads) of norm_act_fwd."""
    _require_cuda(x, dout, mean, rstd, gamma, beta, act_w)
    x, dout = ndhwc(x), ndhwc(dout)
    d = make_na_desc(x, act, stats_per_item, act_p, 0 if act_w is None else act_w.numel(),
                     drop_p, seed, rng_offset)
    dx = new_act(*x.shape, x.device)
    dgamma = dbeta = None
    if want_affine_grads:
        dgamma = torch.empty((x.shape[1],), device=x.device, dtype=torch.float32)
        dbeta = torch.empty_like(dgamma)
    ws = None
    if mean is not None or want_affine_grads:
        ws = _workspace(_lib.lib().adell_norm_act_bwd_workspace(ctypes.byref(d)), x.device)
    # algorithmic bytes: read x and dout once, write dx once
    check(_timed(NORM_ACT_FAMILY, 0.0, lambda: _lib.lib().adell_norm_act_bwd(
        ctypes.byref(d), _ptr(x), _ptr(dout), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta),
        _ptr(act_w), _ptr(dx), _ptr(dgamma), _ptr(dbeta), _ptr(ws),
        0 if ws is None else ws.numel() * 4, _stream()), "bwd", 12.0 * x.numel()))
    return dx, dgamma, dbeta


def norm_act_lowrank_ok(x, co):
    """Whether norm_act_bwd_lowrank takes this site: power-of-two channels, <= 4 factors."""
    C = x.shape[1]
    return 1 <= co <= 4 and 4 <= C <= 1024 and (C & (C - 1)) == 0


def norm_act_bwd_lowrank(x, g, w, mean, rstd, act, act_p=0.0, drop_p=0.0, seed=0, rng_offset=0):
    """dx of norm_act_fwd when the upstream gradient is g (x) w: g [N, co, ...] the gradient of a
    1x1x1 conv's output, w [co, C] its weight -- that conv's backward-data result is never formed
    (adell_norm_act_bwd_lowrank)."""
    _require_cuda(x, g, w, mean, rstd)
    x, g = ndhwc(x), ndhwc(g)
    co = g.shape[1]
    w = w.reshape(co, x.shape[1]).contiguous()
    assert g.shape[0] == x.shape[0] and g.shape[2:] == x.shape[2:]
    d = make_na_desc(x, act, 1, act_p, 0, drop_p, seed, rng_offset)
    dx = new_act(*x.shape, x.device)
    ws = _workspace(_lib.lib().adell_norm_act_bwd_workspace(ctypes.byref(d)), x.device)
    # algorithmic bytes: read x and g once, write dx once
    nb = 8.0 * x.numel() + 4.0 * g.numel()
    check(_timed(NORM_ACT_FAMILY, 0.0, lambda: _lib.lib().adell_norm_act_bwd_lowrank(
        ctypes.byref(d), _ptr(x), _ptr(g), _ptr(w), co, _ptr(mean), _ptr(rstd), _ptr(dx), _ptr(ws),
        ws.numel() * 4, _stream()), "bwd", nb))
    return dx


def dice_focal_fwd(prob, target, smooth, dice_eps, gamma, focal_eps, focal_alpha=1.0):
    """Per-item (dice[B], focal[B]) and the sums the backward needs. prob/target: [B, ...]."""
    _require_cuda(prob, target)
    prob, target = prob.contiguous(), target.contiguous()
    B = prob.shape[0]
    S = prob.numel() // B
    assert target.numel() == prob.numel()
    ws = _workspace(_lib.lib().adell_dice_focal_workspace(B, S), prob.device)
    dice = torch.empty((B,), device=prob.device, dtype=torch.float32)
    focal = torch.empty_like(dice)
    sums = torch.empty((B, 3), device=prob.device, dtype=torch.float32)
    check(_lib.lib().adell_dice_focal_fwd(_ptr(prob), _ptr(target), B, S, smooth, dice_eps, gamma,
                                          float(focal_alpha), focal_eps, _ptr(dice), _ptr(focal),
                                          _ptr(sums),
                                          _ptr(ws), ws.numel() * 4, _stream()))
    return dice, focal, sums


def dice_focal_bwd(prob, target, sums, smooth, dice_eps, gamma, focal_eps, gdice, gfocal,
                   focal_alpha=1.0):
    prob, target = prob.contiguous(), target.contiguous()
    B = prob.shape[0]
    S = prob.numel() // B
    dprob = torch.empty_like(prob)
    check(_lib.lib().adell_dice_focal_bwd(_ptr(prob), _ptr(target), B, S, smooth, dice_eps, gamma,
                                          float(focal_alpha), focal_eps, _ptr(sums), float(gdice),
                                          float(gfocal),
                                          _ptr(dprob), _stream()))
    return dprob


def dice_focal_bwd_dev(prob, target, sums, smooth, dice_eps, gamma, focal_eps, gdice, gfocal,
                       focal_alpha=1.0):
    """gdice / gfocal: per-item upstream gradients as CUDA tensors [B] (or None)."""
    prob, target = prob.contiguous(), target.contiguous()
    B = prob.shape[0]
    S = prob.numel() // B
    dprob = torch.empty_like(prob)
    gd = None if gdice is None else gdice.contiguous().float()
    gf = None if gfocal is None else gfocal.contiguous().float()
    check(_lib.lib().adell_dice_focal_bwd_dev(_ptr(prob), _ptr(target), B, S, smooth, dice_eps,
                                              gamma, float(focal_alpha), focal_eps, _ptr(sums),
                                              _ptr(gd), _ptr(gf), _ptr(dprob), _stream()))
    return dprob


def class_sums_fwd(p, t):
    """p, t: [B, V, C] contiguous -> sums [B, C, 3] = (sum p t, sum p, sum t) over the voxels."""
    _require_cuda(p, t)
    B, V, C = p.shape
    nbytes = _lib.lib().adell_class_sums_workspace(B, V, C)
    ws = _workspace(nbytes, p.device)
    sums = torch.empty((B, C, 3), device=p.device, dtype=torch.float32)
    check(_lib.lib().adell_class_sums_fwd(_ptr(p), _ptr(t), B, V, C, _ptr(sums), _ptr(ws),
                                          ws.numel() * 4, _stream()))
    return sums


def class_sums_bwd(t, gsums):
    """dp [B, V, C] = gsums[..., 0] * t + gsums[..., 1]."""
    _require_cuda(t, gsums)
    B, V, C = t.shape
    dp = torch.empty_like(t)
    g = gsums.contiguous()
    check(_lib.lib().adell_class_sums_bwd(_ptr(t), _ptr(g), B, V, C, _ptr(dp), _stream()))
    return dp


# Bumped whenever a HIP kernel rewrites parameters in place (torch's version
# counters do not see those writes); functional._packed keys its cache on it.
WEIGHT_EPOCH = 0


def _weights_changed():
    global WEIGHT_EPOCH
    WEIGHT_EPOCH += 1


def sgd_step(param, grad, buf, lr, momentum, weight_decay, nesterov, first, grad_scale=1.0):
    _require_cuda(param, grad, buf)
    check(_lib.lib().adell_sgd_step(_ptr(param), _ptr(grad), _ptr(buf), param.numel(), lr,
                                    momentum, weight_decay, int(nesterov), int(first),
                                    grad_scale, _stream()))
    _weights_changed()


def adamw_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step,
               grad_scale=1.0, decoupled=True):
    """torch.optim.AdamW (decoupled decay) or torch.optim.Adam (decay added to the gradient)."""
    _require_cuda(param, grad, exp_avg, exp_avg_sq)
    fn = _lib.lib().adell_adamw_step if decoupled else _lib.lib().adell_adam_step
    check(fn(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(), lr, beta1,
             beta2, eps, weight_decay, int(step), grad_scale, _stream()))
    _weights_changed()


def ema_update(shadow, param, decay):
    _require_cuda(shadow, param)
    check(_lib.lib().adell_ema_update(_ptr(shadow), _ptr(param), shadow.numel(), decay, _stream()))
    _weights_changed()


# ---- token-sequence ops (ViT encoder of UNETR) ------------------------------------------
def layernorm_fwd(x, gamma, beta, eps):
    """LayerNorm over the last dim of a contiguous tensor; returns (y, mean, rstd)."""
    _require_cuda(x, gamma, beta)
    x = x.contiguous()
    C = x.shape[-1]
    rows = x.numel() // C
    y = torch.empty_like(x)
    mean = torch.empty((rows,), device=x.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    check(_lib.lib().adell_layernorm_fwd(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(mean),
                                         _ptr(rstd), rows, C, float(eps), _stream()))
    return y, mean, rstd


def layernorm_bwd(x, dy, gamma, mean, rstd, want_affine):
    x, dy = x.contiguous(), dy.contiguous()
    C = x.shape[-1]
    rows = x.numel() // C
    dx = torch.empty_like(x)
    dg = db = ws = None
    if want_affine:
        dg = torch.empty((C,), device=x.device, dtype=torch.float32)
        db = torch.empty_like(dg)
        ws = _workspace(_lib.lib().adell_layernorm_bwd_workspace(rows, C), x.device)
    check(_lib.lib().adell_layernorm_bwd(_ptr(x), _ptr(dy), _ptr(gamma), _ptr(mean), _ptr(rstd),
                                         _ptr(dx), _ptr(dg), _ptr(db), rows, C, _ptr(ws),
                                         0 if ws is None else ws.numel() * 4, _stream()))
    return dx, dg, db


def add_bcast(a, b):
    """a + b where b is broadcast over a's leading dims (b.numel() divides a.numel())."""
    _require_cuda(a, b)
    a, b = a.contiguous(), b.contiguous()
    out = torch.empty_like(a)
    check(_lib.lib().adell_add_bcast(_ptr(a), _ptr(b), _ptr(out), a.numel(), b.numel(), _stream()))
    return out


def sum_bcast(g, period_shape):
    _require_cuda(g)
    g = g.contiguous()
    db = torch.empty(period_shape, device=g.device, dtype=torch.float32)
    period = db.numel()
    rows = g.numel() // period
    if rows >= 64 and period < 2 ** 31:
        # column sums of the [rows][period] view: chunked partials + fixed-order fold
        nbytes = _lib.lib().adell_bias_grad_workspace(rows, period)
        ws = _workspace(nbytes, g.device)
        check(_lib.lib().adell_bias_grad(_ptr(g), rows, period, _ptr(db), _ptr(ws),
                                         ws.numel() * 4, _stream()))
        return db
    check(_lib.lib().adell_sum_bcast(_ptr(g), _ptr(db), g.numel(), period, _stream()))
    return db


def _att_desc(BH, H, T, A, Dv, scale, drop_p, seed, offset, bias, labels, strides=None):
    """adell_attention_desc of one call. bias: [nbias,T,T] or None; labels: int32 [nlab,T] or None;
    strides: (item, head, row) element strides of the operands in the order q, k, v, out, dout, dq,
    dk, dv (as many triples as the entry reads), None for contiguous operands."""
    d = _lib.AttentionDesc(BH=int(BH), H=int(H), T=int(T), A=int(A), Dv=int(Dv), scale=float(scale),
                           drop_p=float(drop_p), rng_offset=int(offset) & 0xFFFFFFFF,
                           seed=int(seed) & 0xFFFFFFFFFFFFFFFF)
    if bias is not None:
        bias = bias.contiguous()
        d.bias, d.nbias = _ptr(bias), bias.numel() // (T * T)
    if labels is not None:
        if not labels.is_cuda:
            raise AdellHipError("adell_mri_amd kernels run on MI355X only: got CPU labels")
        if labels.dtype != torch.int32 or labels.dim() != 2 or labels.shape[1] != T:
            raise AdellHipError(f"attention: labels must be int32 [nlab, {T}], got "
                                f"{labels.dtype} {tuple(labels.shape)}")
        labels = labels.contiguous()
        d.labels, d.nlab = _ptr(labels), int(labels.shape[0])
    if strides is not None:
        d.strided = 1
        flat = (ctypes.c_int64 * len(strides)).from_buffer(d, _lib.AttentionDesc.stride.offset)
        flat[:] = [int(s) for s in strides]
    d.keep = (bias, labels)     # the descriptor holds their addresses
    return d


def attention_fwd(q, k, v, bias, scale, drop_p=0.0, seed=0, offset=0, labels=None, heads=1):
    """q,k: [BH,T,A]; v: [BH,T,Dv]; bias: [nbias,T,T] or None; labels: int32 [nlab,T] or None --
    item b = bh // heads reads row b % nlab, and scores between tokens whose labels differ gain
    -100. Returns (out, lse)."""
    _require_cuda(q, k, v, bias)
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    BH, T, A = q.shape
    Dv = v.shape[-1]
    out = torch.empty((BH, T, Dv), device=q.device, dtype=torch.float32)
    lse = torch.empty((BH, T), device=q.device, dtype=torch.float32)
    d = _att_desc(BH, heads, T, A, Dv, scale, drop_p, seed, offset, bias, labels)
    check(_lib.lib().adell_attention_fwd(ctypes.byref(d), _ptr(q), _ptr(k), _ptr(v), _ptr(out),
                                         _ptr(lse), _stream()))
    return out, lse


def attention_bwd(q, k, v, bias, out, dout, lse, scale, drop_p=0.0, seed=0, offset=0, labels=None,
                  heads=1):
    BH, T, A = q.shape
    Dv = v.shape[-1]
    dout = dout.contiguous()
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    d = _att_desc(BH, heads, T, A, Dv, scale, drop_p, seed, offset, bias, labels)
    check(_lib.lib().adell_attention_bwd(ctypes.byref(d), _ptr(q), _ptr(k), _ptr(v), _ptr(out),
                                         _ptr(dout), _ptr(lse), _ptr(dq), _ptr(dk), _ptr(dv),
                                         _stream()))
    return dq, dk, dv


def attention_bias_grad(q, k, v, bias, out, dout, lse, scale, nbias, drop_p=0.0, seed=0, offset=0,
                        labels=None, heads=1, strides=None, dims=None):
    """Gradient of the additive bias of attention_fwd / attention_fwd_strided, summed over the
    sequences that share a slice: [nbias, T, T] with dbias[j] = sum of dS[bh] over bh % nbias == j
    (``nbias`` = heads: a per-head bias; = BH: dS itself). ``bias`` may be None. Contiguous
    [BH,T,*] operands by default; with ``strides`` (15 element strides: (item, head, row) of q, k, v,
    out, dout) and ``dims`` = (B, H, T, A, Dv) the operands are addressed as in
    attention_bwd_strided. Device memory: the result and a workspace whose size depends on
    (nbias, T) alone."""
    _require_cuda(q, k, v, bias, out, dout, lse)
    if strides is None:
        q, k, v, out, dout = (t.contiguous() for t in (q, k, v, out, dout))
        BH, T, A = q.shape
        Dv = v.shape[-1]
        H = int(heads)
        if BH % H:
            raise AdellHipError(f"attention_bias_grad: {BH} sequences are not items of {H} heads")
    else:
        B, H, T, A, Dv = (int(x) for x in dims)
        BH = B * H
    nbias = int(nbias)
    if bias is not None and bias.numel() != nbias * T * T:
        raise AdellHipError("attention_bias_grad: bias is not [nbias, T, T]")
    d = _att_desc(BH, H, T, A, Dv, scale, drop_p, seed, offset, bias, labels, strides)
    d.nbias = nbias     # the number of result slices, with or without a bias
    dbias = torch.empty((nbias, T, T), device=q.device, dtype=torch.float32)
    nws = _lib.lib().adell_attention_bias_grad_workspace_floats(nbias, T)
    ws = _workspace(nws * 4, q.device) if nws else None
    check(_lib.lib().adell_attention_bias_grad(ctypes.byref(d), _ptr(q), _ptr(k), _ptr(v), _ptr(out),
                                               _ptr(dout), _ptr(lse), _ptr(dbias), _ptr(ws), nws,
                                               _stream()))
    return dbias


# launch plan of one attention pass (adell_attention_plan). path: one of ATT_PATHS; lds: dynamic LDS
# bytes; blocks: grid x (blocks per sequence); rows: query (dK/dV: key) rows per block
AttPlan = collections.namedtuple("AttPlan", "path lds blocks rows")
ATT_PATHS = ("valu", "mfma_resident", "mfma_streamed", "refused")
_ATT_PASSES = {"fwd": 0, "dq": 1, "dkv": 2}


def attention_plan(T, A, Dv, which="fwd", aligned=True):
    """What attention_fwd (``which`` "fwd") or the dQ / dK-dV kernel of attention_bwd ("dq", "dkv")
    would launch for T tokens and head dims (A, Dv) under the current tuning switches. ``aligned``:
    every tensor of the call is 16-byte aligned (always, from torch, unless a view starts inside a
    storage). Host only: no GPU needed."""
    out = (ctypes.c_int * 4)()
    check(_lib.lib().adell_attention_plan(_ATT_PASSES[which], int(T), int(A), int(Dv),
                                          int(bool(aligned)), out))
    return AttPlan(ATT_PATHS[out[0]], *list(out)[1:])


# ---- data movement (U-Net++ dense links) ----------------------------------------------------
def cat_channels(tensors):
    """Channel concat of NDHWC tensors [N,Ci,D,H,W] -> [N,sum Ci,D,H,W]."""
    _require_cuda(*tensors)
    tensors = [ndhwc(t) for t in tensors]
    N, _, D, H, W = tensors[0].shape
    Ct = sum(t.shape[1] for t in tensors)
    out = new_act(N, Ct, D, H, W, tensors[0].device)
    off = 0
    for t in tensors:
        assert tuple(t.shape[2:]) == (D, H, W) and t.shape[0] == N
        check(_lib.lib().adell_copy_channels(_ptr(out), _ptr(t), N * D * H * W, Ct, t.shape[1], off,
                                             0, _stream()))
        off += t.shape[1]
    return out


def split_channels(full, sizes):
    full = ndhwc(full)
    N, Ct, D, H, W = full.shape
    outs, off = [], 0
    for c in sizes:
        t = new_act(N, c, D, H, W, full.device)
        check(_lib.lib().adell_copy_channels(_ptr(full), _ptr(t), N * D * H * W, Ct, c, off, 1,
                                             _stream()))
        outs.append(t)
        off += c
    return outs


def interp_nearest(x, size, backward_from=None):
    """Forward: x [N,C,Di,Hi,Wi] -> [N,C,*size]. With backward_from=(Di,Hi,Wi): x is the
    output gradient and the result the input gradient."""
    _require_cuda(x)
    x = ndhwc(x)
    N, C = x.shape[:2]
    if backward_from is None:
        Di, Hi, Wi = x.shape[2:]
        Do, Ho, Wo = size
        y = new_act(N, C, Do, Ho, Wo, x.device)
        check(_lib.lib().adell_interp_nearest_fwd(_ptr(x), _ptr(y), N, C, Di, Hi, Wi, Do, Ho, Wo,
                                                  _stream()))
        return y
    Di, Hi, Wi = backward_from
    Do, Ho, Wo = x.shape[2:]
    dx = new_act(N, C, Di, Hi, Wi, x.device)
    check(_lib.lib().adell_interp_nearest_bwd(_ptr(x), _ptr(dx), N, C, Di, Hi, Wi, Do, Ho, Wo,
                                              _stream()))
    return dx


def interp_linear(x, scales, backward_from=None, size=None):
    """torch.nn.Upsample(scale_factor=scales, mode="trilinear", align_corners=False) on
    [N,C,Di,Hi,Wi]; with size=(Do,Ho,Wo): F.interpolate(size=..., align_corners=True) instead;
    with backward_from=(Di,Hi,Wi): x is the output gradient, result = dX."""
    _require_cuda(x)
    x = ndhwc(x)
    N, C = x.shape[:2]
    align = int(size is not None)
    sd, sh, sw = (1.0, 1.0, 1.0) if align else (float(s) for s in scales)
    if backward_from is None:
        Di, Hi, Wi = x.shape[2:]
        Do, Ho, Wo = size if align else (int(math.floor(n * s))
                                         for n, s in zip((Di, Hi, Wi), (sd, sh, sw)))
        y = new_act(N, C, Do, Ho, Wo, x.device)
        check(_lib.lib().adell_interp_linear_fwd(_ptr(x), _ptr(y), N, C, Di, Hi, Wi, Do, Ho, Wo,
                                                 sd, sh, sw, align, _stream()))
        return y
    Di, Hi, Wi = backward_from
    Do, Ho, Wo = x.shape[2:]
    dx = new_act(N, C, Di, Hi, Wi, x.device)
    check(_lib.lib().adell_interp_linear_bwd(_ptr(x), _ptr(dx), N, C, Di, Hi, Wi, Do, Ho, Wo,
                                             sd, sh, sw, align, _stream()))
    return dx


def fold_x_taps(x, K, P, Cp=16):
    """[N,Cin,D,H,W] -> [N,Cp,D,H,W+2P-K+1] with channel kx*Cin+ci = x[..., ox-P+kx] (zero fill)."""
    _require_cuda(x)
    x = ndhwc(x)
    N, Cin, D, H, W = x.shape
    Wo = W + 2 * P - K + 1
    out = new_act(N, Cp, D, H, Wo, x.device)
    check(_lib.lib().adell_fold_x_taps(_ptr(x), _ptr(out), N, D, H, W, Cin, K, P, Cp, _stream()))
    return out


def scale_bc(x, s):
    """x [N,C,D,H,W] (NDHWC memory) times s [N,C]."""
    _require_cuda(x, s)
    x = ndhwc(x)
    N, C = x.shape[:2]
    V = x.numel() // (N * C)
    y = new_act(N, C, *x.shape[2:], x.device)
    sc = s.contiguous()
    check(_lib.lib().adell_scale_bc(_ptr(x), _ptr(sc), _ptr(y), N, V, C, _stream()))
    return y


def scale_bc_dscale(x, dy):
    """ds[n,c] = sum over voxels of dy * x."""
    x, dy = ndhwc(x), ndhwc(dy)
    N, C = x.shape[:2]
    V = x.numel() // (N * C)
    ws = _workspace(4 * _lib.lib().adell_scale_bc_dscale_workspace_floats(N, V, C), x.device)
    ds = torch.empty((N, C), device=x.device, dtype=torch.float32)
    check(_lib.lib().adell_scale_bc_dscale(_ptr(x), _ptr(dy), _ptr(ds), N, V, C, _ptr(ws),
                                           _stream()))
    return ds


def cse_apply(x, s, c, inv=None, acc=None):
    """y = acc + x * (s[n, v] + c[n, ch]) * inv[n]; x/acc [N,C,D,H,W] (NDHWC memory), s [N,1,D,H,W],
    c [N,C], inv [N] or None, acc or None."""
    _require_cuda(x, s, c, inv, acc)
    x = ndhwc(x)
    N, C = x.shape[:2]
    V = x.numel() // (N * C)
    s, c = s.contiguous(), c.contiguous()
    if s.numel() != N * V or c.numel() != N * C:
        raise AdellHipError(f"cse_apply: gates {tuple(s.shape)}, {tuple(c.shape)} do not fit "
                            f"x {tuple(x.shape)}")
    acc = None if acc is None else ndhwc(acc)
    inv = None if inv is None else inv.contiguous()
    y = new_act(N, C, *x.shape[2:], x.device)
    check(_lib.lib().adell_cse_apply(_ptr(x), _ptr(s), _ptr(c), _ptr(inv), _ptr(acc), _ptr(y), N, V,
                                     C, _stream()))
    return y


def cse_apply_bwd(x, dy, s, c, inv=None):
    """(dx, ds [N,1,D,H,W], dc [N,C]) of cse_apply."""
    _require_cuda(x, dy, s, c, inv)
    x, dy = ndhwc(x), ndhwc(dy)
    N, C = x.shape[:2]
    V = x.numel() // (N * C)
    s, c = s.contiguous(), c.contiguous()
    inv = None if inv is None else inv.contiguous()
    ws = _workspace(4 * _lib.lib().adell_cse_apply_bwd_workspace_floats(N, V, C), x.device)
    dx = new_act(N, C, *x.shape[2:], x.device)
    ds = torch.empty((N, 1, *x.shape[2:]), device=x.device, dtype=torch.float32)
    dc = torch.empty((N, C), device=x.device, dtype=torch.float32)
    check(_lib.lib().adell_cse_apply_bwd(_ptr(x), _ptr(dy), _ptr(s), _ptr(c), _ptr(inv), _ptr(dx),
                                         _ptr(ds), _ptr(dc), N, V, C, _ptr(ws), _stream()))
    return dx, ds, dc


def bcast_nc(g, shape, scale=1.0):
    """out[n, c, ...] = g[n, c] * scale, out of logical shape [N, C, D, H, W] (NDHWC memory)."""
    _require_cuda(g)
    N, C = shape[:2]
    V = int(math.prod(shape[2:]))
    out = new_act(N, C, *shape[2:], g.device)
    gc = g.contiguous()
    check(_lib.lib().adell_bcast_nc(_ptr(gc), _ptr(out), N, V, C, float(scale), _stream()))
    return out


def maxpool3d_fwd(x, kernel, stride, padding):
    _require_cuda(x)
    x = ndhwc(x)
    N, C, D, H, W = x.shape
    d = make_conv_desc(N, (D, H, W), C, 0, C, kernel, stride, padding)
    y = new_act(N, C, d.Do, d.Ho, d.Wo, x.device)
    idx = torch.empty((N, d.Do, d.Ho, d.Wo, C), device=x.device, dtype=torch.int32)
    check(_lib.lib().adell_maxpool3d_fwd(ctypes.byref(d), _ptr(x), _ptr(y), _ptr(idx), _stream()))
    return y, idx


def maxpool3d_bwd(dy, idx, in_shape, kernel, stride, padding):
    dy = ndhwc(dy)
    N, C, D, H, W = in_shape
    d = make_conv_desc(N, (D, H, W), C, 0, C, kernel, stride, padding)
    dx = new_act(N, C, D, H, W, dy.device)
    check(_lib.lib().adell_maxpool3d_bwd(ctypes.byref(d), _ptr(dy), _ptr(idx), _ptr(dx), _stream()))
    return dx


# ---- ConvNeXt / VICReg -------------------------------------------------------------------------
def dwconv3d_fwd(x, w, bias):
    _require_cuda(x, w, bias)
    x = ndhwc(x)
    N, C, D, H, W = x.shape
    kd, kh, kw = w.shape[2:]
    y = new_act(N, C, D, H, W, x.device)
    wc = w.contiguous()
    check(_lib.lib().adell_dwconv3d_fwd(N, C, D, H, W, kd, kh, kw, _ptr(x), _ptr(wc),
                                        _ptr(bias), _ptr(y), _stream()))
    return y


def dwconv3d_bwd_data(dy, w):
    dy = ndhwc(dy)
    N, C, D, H, W = dy.shape
    kd, kh, kw = w.shape[2:]
    dx = new_act(N, C, D, H, W, dy.device)
    wc = w.contiguous()
    check(_lib.lib().adell_dwconv3d_bwd_data(N, C, D, H, W, kd, kh, kw, _ptr(dy),
                                             _ptr(wc), _ptr(dx), _stream()))
    return dx


def dwconv3d_bwd_weight(x, dy, kshape, want_db):
    x, dy = ndhwc(x), ndhwc(dy)
    N, C, D, H, W = x.shape
    kd, kh, kw = kshape
    dw = torch.empty((C, 1, kd, kh, kw), device=x.device, dtype=torch.float32)
    db = torch.empty((C,), device=x.device, dtype=torch.float32) if want_db else None
    nws = _lib.lib().adell_dwconv3d_bwd_weight_workspace_floats(N, C, D, H, W, kd, kh, kw)
    ws = torch.empty((nws,), device=x.device, dtype=torch.float32) if nws else None
    check(_lib.lib().adell_dwconv3d_bwd_weight(N, C, D, H, W, kd, kh, kw, _ptr(x), _ptr(dy),
                                               _ptr(dw), _ptr(db), _ptr(ws), _stream()))
    return dw, db


# launch plan of a depthwise conv (adell_dwconv3d_plan). form: one of DW_FORMS; K, WT: the tile
# instantiation (ring: 7, 16); nseg / seg: x segments of a tile row and outputs per segment, or z
# segments of the ring and planes per segment; vec: 16-byte channel loads; blocks of the main kernel;
# loop: the most work items one block loops over (rounds of the resident MFMA kernel, items per chunk,
# tiles per split, grid-stride rounds ...); parts: chunks / splits; workspace floats
DwPlan = collections.namedtuple("DwPlan", "form K WT nseg seg vec blocks loop parts workspace")
DW_FORMS = ("generic", "dense", "mfma", "mfma_stream", "zring", "tile", "wgrad_mfma")


def dwconv3d_plan(N, C, size, kernel, backward_weight=False, aligned=(True, True)):
    """What dwconv3d_fwd / dwconv3d_bwd_data (one dispatch) or, with ``backward_weight``,
    dwconv3d_bwd_weight would launch for these extents under the current tuning switches and conv
    precision. ``aligned``: the launch's two tensors are 16-byte aligned (always, from torch). Host
    only: no GPU needed."""
    kernel = (kernel,) * 3 if isinstance(kernel, int) else tuple(kernel)
    out = (ctypes.c_long * 10)()
    check(_lib.lib().adell_dwconv3d_plan(int(bool(backward_weight)), N, C, *size, *kernel,
                                         int(bool(aligned[0])), int(bool(aligned[1])), out))
    return DwPlan(DW_FORMS[out[0]], *list(out)[1:])


def multi_copy(table, rows, dst):
    """table: int64 device tensor [rows, 3] of (src pointer, dst offset, numel <= 16384)."""
    _require_cuda(dst)
    if not table.is_cuda or table.dtype != torch.int64:
        raise _lib.AdellHipError("multi_copy: the table must be an int64 CUDA tensor")
    check(_lib.lib().adell_multi_copy(_ptr(table), int(rows), _ptr(dst), _stream()))


def multi_accumulate(table, rows, dst):
    """``multi_copy`` with ``dst += src`` (the accumulate_grad_batches fold)."""
    _require_cuda(dst)
    if not table.is_cuda or table.dtype != torch.int64:
        raise _lib.AdellHipError("multi_accumulate: the table must be an int64 CUDA tensor")
    check(_lib.lib().adell_multi_accumulate(_ptr(table), int(rows), _ptr(dst), _stream()))


# ---- gradient-norm clipping (csrc/grad_clip.hip) ------------------------------------------------
def grad_norm_workspace_bytes(runs):
    return int(_lib.lib().adell_grad_norm_workspace(int(runs)))


def grad_norm_workspace(runs, device):
    """The fp64 partials of ``runs`` runs: allocate once, outside any graph capture."""
    return torch.empty(grad_norm_workspace_bytes(runs) // 8, dtype=torch.float64, device=device)


def grad_norm_partials(g, norm_inf, workspace, run):
    """Partial norm of the 1-D fp32 slice ``g`` (16-byte aligned) into slot ``run`` of ``workspace``."""
    _require_cuda(g)
    if workspace.dtype != torch.float64 or (run + 1) * grad_norm_workspace_bytes(1) > 8 * workspace.numel():
        raise _lib.AdellHipError("grad_norm_partials: the workspace has no slot for this run")
    check(_lib.lib().adell_grad_norm_partials(_ptr(g), g.numel(), int(bool(norm_inf)), _ptr(workspace),
                                              int(run), _stream()))


def grad_norm_finalize(workspace, runs, norm_inf, scale, max_norm, out):
    """out[0] = ||scale * g|| over the ``runs`` partials, out[1] = min(max_norm / (out[0] + 1e-6), 1)."""
    _require_cuda(out)
    if workspace.dtype != torch.float64 or grad_norm_workspace_bytes(runs) > 8 * workspace.numel():
        raise _lib.AdellHipError("grad_norm_finalize: the workspace holds fewer runs")
    if out.numel() < 2:
        raise _lib.AdellHipError("grad_norm_finalize: out needs two elements (norm, coefficient)")
    check(_lib.lib().adell_grad_norm_finalize(_ptr(workspace), int(runs), int(bool(norm_inf)),
                                              float(scale), float(max_norm), _ptr(out), _stream()))


def grad_scale_by(g, coef):
    """g *= coef[0] in place (``coef``: a device scalar; nothing happens when it is 1)."""
    _require_cuda(g, coef)
    if coef.numel() < 1:
        raise _lib.AdellHipError("grad_scale_by: empty coefficient")
    check(_lib.lib().adell_grad_scale_by(_ptr(g), g.numel(), _ptr(coef), _stream()))


# ---- elastic-weight-consolidation penalty (csrc/ewc.hip) ----------------------------------------
EWC_COLS = 5     # longs per chunk row: parameter, anchor, count, tensor index, destination offset


def ewc_chunk():
    """Elements per chunk row of the penalty's tables (the library's compile-time constant)."""
    return int(_lib.lib().adell_ewc_chunk())


def ewc_workspace(chunks, tensors, device):
    """The fp64 workspace of ``ewc_partials`` / ``ewc_finalize``: allocate once per table."""
    n = int(_lib.lib().adell_ewc_workspace_doubles(int(chunks), int(tensors)))
    if n <= 0:
        raise _lib.AdellHipError(f"ewc_workspace: bad table extents ({chunks} chunks, {tensors} tensors)")
    return torch.empty(n, dtype=torch.float64, device=device)


def _ewc_table(table, chunks, what):
    if not table.is_cuda or table.dtype != torch.int64 or table.numel() < int(chunks) * EWC_COLS:
        raise _lib.AdellHipError(f"{what}: the table must be an int64 CUDA tensor of {EWC_COLS} "
                                 "columns per chunk")


def ewc_partials(table, chunks, p, workspace):
    """workspace[r] = sum |param - anchor|^p over chunk row ``r`` of ``table``."""
    _ewc_table(table, chunks, "ewc_partials")
    if workspace.dtype != torch.float64 or not workspace.is_cuda or workspace.numel() < chunks:
        raise _lib.AdellHipError("ewc_partials: the workspace is too small (ewc_workspace)")
    check(_lib.lib().adell_ewc_partials(_ptr(table), int(chunks), float(p), _ptr(workspace), _stream()))


def ewc_finalize(tensor_first, tensors, chunks, p, workspace, norms, total):
    """norms[k] = ||param_k - anchor_k||_p (fp32), total[0] = their sum."""
    _require_cuda(norms, total)
    if not tensor_first.is_cuda or tensor_first.dtype != torch.int64 or tensor_first.numel() < tensors + 1:
        raise _lib.AdellHipError("ewc_finalize: tensor_first must be an int64 CUDA tensor of tensors + 1")
    if workspace.dtype != torch.float64 or not workspace.is_cuda or workspace.numel() < chunks + tensors:
        raise _lib.AdellHipError("ewc_finalize: the workspace is too small (ewc_workspace)")
    if norms.numel() < tensors or total.numel() < 1:
        raise _lib.AdellHipError("ewc_finalize: norms needs one element per tensor, total one")
    check(_lib.lib().adell_ewc_finalize(_ptr(tensor_first), int(tensors), int(chunks), float(p),
                                        _ptr(workspace), _ptr(norms), _ptr(total), _stream()))


def ewc_grad(table, chunks, p, norms, c, c_dev, add, base):
    """The penalty's gradient times ``c * c_dev[0]`` (``c_dev``: a device scalar or None), written to
    (``add`` false) or added into ``base`` at every chunk's destination offset. The table lives on
    the device: its pointers, counts and offsets are the caller's word (whoever builds a table keeps
    ``offset + count <= base.numel()``), they cannot be checked here without a host read."""
    _ewc_table(table, chunks, "ewc_grad")
    _require_cuda(norms, c_dev, base)
    if c_dev is not None and c_dev.numel() < 1:
        raise _lib.AdellHipError("ewc_grad: empty device scalar")
    check(_lib.lib().adell_ewc_grad(_ptr(table), int(chunks), float(p), _ptr(norms), float(c),
                                    _ptr(c_dev), int(bool(add)), _ptr(base), _stream()))


# ---- segmentation metrics (csrc/seg_metrics.hip) ------------------------------------------------
SEG_METRIC_KINDS = {"iou": 0, "precision": 1, "fbeta": 2, "dice": 3}
SEG_MAX_CLASSES = 32
_SEG_TARGET_TYPES = {torch.float32: 0, torch.uint8: 1, torch.bool: 1, torch.int64: 2}


def seg_confusion_update(pred, target, states):
    """Add the confusion counts of one update into every state of ``states`` (at most 8 int64 CUDA
    tensors of 3 C + 1 elements). ``pred``: fp32 [B, C, *spatial] (C = 1: binary), NCDHW or
    channels-last memory; ``target``: [B, *spatial] or [B, 1, *spatial] of fp32, uint8, bool or int64
    (other dtypes are converted). Two launches, no host synchronisation."""
    if pred.dim() < 3:
        raise AdellHipError(f"seg_confusion_update: pred must be [B, C, *spatial], got {tuple(pred.shape)}")
    B, C = int(pred.shape[0]), int(pred.shape[1])
    spatial = tuple(pred.shape[2:])
    if C > SEG_MAX_CLASSES:
        raise AdellHipError(f"seg_confusion_update: {C} classes; at most {SEG_MAX_CLASSES} are supported")
    if tuple(target.shape) not in ((B,) + spatial, (B, 1) + spatial):
        raise AdellHipError(f"seg_confusion_update: target of shape {tuple(target.shape)} does not match "
                            f"pred {tuple(pred.shape)} (expected {(B,) + spatial} or {(B, 1) + spatial})")
    if not 1 <= len(states) <= 8:
        raise AdellHipError(f"seg_confusion_update: {len(states)} states (1..8 per update)")
    for s in states:
        if s.dtype != torch.int64 or s.numel() != 3 * C + 1 or not s.is_contiguous():
            raise AdellHipError(f"seg_confusion_update: a state must be a contiguous int64 tensor of "
                                f"{3 * C + 1} elements for {C} classes")
        if s.device != pred.device:
            raise AdellHipError(f"seg_confusion_update: state on {s.device}, pred on {pred.device}")
    _require_cuda(pred)
    if not target.is_cuda or target.device != pred.device:
        raise AdellHipError("seg_confusion_update: the target must be on the device of pred")
    S = 1
    for d in spatial:
        S *= int(d)
    channels_last = 0
    if C > 1 and not pred.is_contiguous():
        cl = {5: torch.channels_last_3d, 4: torch.channels_last}.get(pred.dim())
        channels_last = int(cl is not None and pred.is_contiguous(memory_format=cl))
    if not (pred.is_contiguous() or channels_last):
        pred = pred.contiguous()
    if target.dtype not in _SEG_TARGET_TYPES:
        target = target.to(torch.float32 if target.is_floating_point() else torch.int64)
    if not target.is_contiguous():
        target = target.contiguous()      # a cropped ground truth (crop_if_necessary)
    n = B * S
    ws_bytes = int(_lib.lib().adell_seg_confusion_workspace(n, C))
    ws = _workspace(ws_bytes, pred.device)
    ptrs = (ctypes.c_void_p * len(states))(*[s.data_ptr() for s in states])
    check(_lib.lib().adell_seg_confusion_update(
        _ptr(pred), _ptr(target), _SEG_TARGET_TYPES[target.dtype], B, C, S, channels_last, _ptr(ws),
        ws_bytes, ptrs, len(states), _stream()))


def seg_metric_compute(state, kind, beta=1.0, num_classes=None):
    """The metric ``kind`` ('iou', 'precision', 'fbeta', 'dice') of an int64 state as a 0-dim fp32
    device tensor (fp64 arithmetic on the counts; macro mean over the classes that occur)."""
    if kind not in SEG_METRIC_KINDS:
        raise AdellHipError(f"seg_metric_compute: unknown metric {kind!r} (one of {sorted(SEG_METRIC_KINDS)})")
    C = (state.numel() - 1) // 3 if num_classes is None else int(num_classes)
    if state.dtype != torch.int64 or state.numel() != 3 * C + 1 or not 1 <= C <= SEG_MAX_CLASSES:
        raise AdellHipError("seg_metric_compute: the state must be int64 [3 C + 1], 1 <= C <= 32")
    if not state.is_cuda:
        raise AdellHipError("adell_mri_amd kernels run on MI355X only: got a CPU tensor (no CPU fallback)")
    out = torch.empty((), dtype=torch.float32, device=state.device)
    check(_lib.lib().adell_seg_metric_compute(_ptr(state), C, SEG_METRIC_KINDS[kind], float(beta),
                                              _ptr(out), _stream()))
    return out


# ---- connected components and PI-CAI lesion tables (csrc/components.hip) -----------------------
def _volumes(x, name):
    """``x`` as a contiguous fp32 [NV, D, H, W] device tensor: a 3-D volume, or a batch of them with
    any number of leading dimensions. Masks of other dtypes are converted (non-zero is foreground)."""
    if x.dim() < 3:
        raise AdellHipError(f"{name}: expected a 3-D volume or a batch of them, got shape {tuple(x.shape)} "
                            f"(the reference's 3x3x3 structure needs 3-D input)")
    if not x.is_cuda:
        raise AdellHipError("adell_mri_amd kernels run on MI355X only: got a CPU tensor (no CPU fallback)")
    if x.dtype != torch.float32:
        x = x.to(torch.float32)
    D, H, W = (int(v) for v in x.shape[-3:])
    return x.contiguous().view(-1, D, H, W)


def label_components(x, threshold=None):
    """``scipy.ndimage.label(x, structure=np.ones((3, 3, 3)))`` on the device: 26-connected components
    of a 3-D volume [D, H, W] or of every volume of a batch [..., D, H, W], numbered 1..N in the raster
    order of their first voxel, bit-identical to scipy. Foreground is ``x > threshold`` when a
    threshold is given, else ``x != 0``. Returns (labels int32 of x's shape, counts int32 of x's
    leading shape, 0-dim for one volume), both on the device; no host synchronisation."""
    lead = tuple(x.shape[:-3])
    if x.dtype != torch.float32 and x.is_cuda:
        # foreground decided in x's own dtype (an fp32 copy could round 0.1000000001 down to the
        # threshold or a tiny float64 value to 0); the kernel then labels the exact 0 / 1 mask
        x = ((x > threshold) if threshold is not None else (x != 0)).to(torch.float32)
        threshold = None
    v = _volumes(x, "label_components")
    NV, D, H, W = (int(s) for s in v.shape)
    labels = torch.empty(v.shape, dtype=torch.int32, device=v.device)
    counts = torch.empty(NV, dtype=torch.int32, device=v.device)
    if NV == 0:
        return labels.view(x.shape), counts.view(lead)
    ws_bytes = int(_lib.lib().adell_cc_workspace(NV, D, H, W))
    if ws_bytes <= 0:
        raise AdellHipError(f"label_components: unsupported shape {tuple(x.shape)}")
    ws = _workspace(ws_bytes, v.device)
    check(_lib.lib().adell_cc_label(_ptr(v), NV, D, H, W, int(threshold is not None),
                                    float(threshold if threshold is not None else 0.0), _ptr(labels),
                                    _ptr(counts), _ptr(ws), ws_bytes, _stream()))
    return labels.view(x.shape), counts.view(lead)


def picai_tables(pred, target, threshold=0.1):
    """The lesion tables of B cases (csrc/components.hip, adell_picai_tables): ``pred`` and ``target``
    are [B, D, H, W] (any dtype; converted to fp32). Candidates are the 26-connected components of
    ``pred > threshold`` (confidence 1, the reference's ``get_lesions``) or, with ``threshold=None``,
    of ``pred != 0`` (confidence = the maximum of pred over the component); GT lesions those of
    ``target.astype(int32) != 0``. The prediction is taken in fp32, as the reference's
    ``y_det.astype("float32")`` does (eval.py:128); a target of another dtype is truncated in its own
    dtype first (a float64 0.9999999999 is a 0, as astype(int32) makes it). Returns (hdr, out)
    device int32 tensors without synchronising: ``hdr`` [B, 3] = (N_cand, N_gt, n_pairs), ``out``
    the packed records (include/adell_hip.h)."""
    if target.dtype != torch.float32 and target.is_cuda:
        target = (torch.trunc(target) if target.is_floating_point() else target) != 0
    p = _volumes(pred, "picai_tables")
    t = _volumes(target, "picai_tables")
    if p.shape != t.shape or p.device != t.device:
        raise AdellHipError(f"picai_tables: prediction {tuple(pred.shape)} and target {tuple(target.shape)} "
                            "must have the same shape and device")
    B, D, H, W = (int(s) for s in p.shape)
    lib = _lib.lib()
    ws_bytes = int(lib.adell_picai_tables_workspace(B, D, H, W))
    cap = int(lib.adell_picai_tables_capacity(B, D, H, W))
    if ws_bytes <= 0 or cap <= 0:
        raise AdellHipError(f"picai_tables: unsupported shape {tuple(pred.shape)}")
    ws = _workspace(ws_bytes, p.device)
    hdr = torch.empty((B, 3), dtype=torch.int32, device=p.device)
    out = torch.empty(cap, dtype=torch.int32, device=p.device)
    check(lib.adell_picai_tables(_ptr(p), _ptr(t), B, D, H, W, int(threshold is not None),
                                 float(threshold if threshold is not None else 0.0), _ptr(hdr), _ptr(out),
                                 cap, _ptr(ws), ws_bytes, _stream()))
    return hdr, out


_LC_MODES = {"dynamic-fast": 1, "dynamic": 2}


def _lesion_candidates(x, threshold, min_voxels_detection, num_lesions_to_extract,
                       dynamic_threshold_factor, max_prob_round_decimals,
                       remove_adjacent_lesion_candidates):
    """``lesion_candidates`` plus the unrounded peak of every kept component and the number of
    rounds the dynamic mode ran (None for the static modes)."""
    import math

    if not torch.is_tensor(x):
        raise TypeError(f"lesion_candidates: expected a device tensor, got {type(x).__name__}")
    if x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(
            f"lesion_candidates: {x.dtype} input: the device path is fp32 (float16 / bfloat16 are "
            "converted, as the reference converts float16); float64 maxima cannot be kept, and integer "
            "or complex maps are not probabilities")
    if isinstance(threshold, str):
        if threshold not in _LC_MODES:
            raise ValueError(f"lesion_candidates: threshold {threshold!r}: 'dynamic', 'dynamic-fast' "
                             "or a number")
        mode, thr = _LC_MODES[threshold], 0.0
    else:
        mode, thr = 0, float(threshold)
    lead = tuple(x.shape[:-3])
    v = _volumes(x, "lesion_candidates")
    NV, D, H, W = (int(s) for s in v.shape)
    minvox = max(-1, min(int(math.floor(min_voxels_detection)), 2 ** 31 - 1))
    num = max(0, min(int(num_lesions_to_extract), 2 ** 31 - 1))
    use_round = max_prob_round_decimals is not None
    lib = _lib.lib()
    cap = int(lib.adell_lesion_candidates_capacity(D, H, W, mode, minvox, num))
    ws_bytes = int(lib.adell_lesion_candidates_workspace(max(NV, 1), D, H, W, mode))
    if cap <= 0 or ws_bytes <= 0:
        raise AdellHipError(f"lesion_candidates: unsupported shape {tuple(x.shape)}")
    dev = v.device
    hard = torch.empty(v.shape, dtype=torch.float32, device=dev)
    indexed = torch.empty(v.shape, dtype=torch.int32, device=dev)
    n = torch.zeros(NV, dtype=torch.int32, device=dev)
    ids = torch.zeros((NV, cap), dtype=torch.int32, device=dev)
    conf = torch.zeros((NV, cap), dtype=torch.float32, device=dev)
    peak = torch.zeros((NV, cap), dtype=torch.float32, device=dev)
    rounds = ctypes.c_int(0)
    if NV:
        ws = _workspace(ws_bytes, dev)
        check(lib.adell_lesion_candidates(
            _ptr(v), NV, D, H, W, mode, thr, float(dynamic_threshold_factor), minvox, num,
            int(max_prob_round_decimals) if use_round else 0, int(use_round),
            int(bool(remove_adjacent_lesion_candidates)), _ptr(hard), _ptr(indexed), _ptr(n), _ptr(ids),
            _ptr(conf), _ptr(peak), cap, ctypes.byref(rounds), _ptr(ws), ws_bytes, _stream()))
    return (hard.view(x.shape), indexed.view(x.shape), n.view(lead), ids.view(lead + (cap,)),
            conf.view(lead + (cap,)), peak.view(lead + (cap,)), rounds.value if mode == 2 else None)


def lesion_candidates(x, threshold="dynamic-fast", min_voxels_detection=10, num_lesions_to_extract=5,
                      dynamic_threshold_factor=2.5, max_prob_round_decimals=None,
                      remove_adjacent_lesion_candidates=True):
    """The reference's ``extract_lesion_candidates`` (adell_mri/modules/extract_lesion_candidates.py,
    Report-Guided-Annotation) on the device (csrc/components.hip, adell_lesion_candidates): a
    probability map [D, H, W], or every volume of a batch [..., D, H, W], becomes a detection map whose
    26-connected components carry their peak probability. ``threshold``: a number (static, :19-55:
    foreground ``x >= threshold``, components of ``<= min_voxels_detection`` voxels dropped),
    ``"dynamic-fast"`` (:198-211: static at ``max(x) / dynamic_threshold_factor`` per volume) or
    ``"dynamic"`` (:58-134: up to ``num_lesions_to_extract`` rounds per volume, each at the remaining
    maximum over the factor, taking the component of the largest confidence and rejecting it when it
    touches a stored one and ``remove_adjacent_lesion_candidates``). Bit-identical to the reference
    run on every volume, its whole-volume candidate of confidence 0 included (the dynamic mode on a
    map whose components are all too small).

    Input: float32; float16 and bfloat16 are converted to float32; anything else raises TypeError.
    Values are assumed finite and non-negative (probabilities).

    Returns device tensors ``(hard_blobs, indexed, n, ids, confidences)``: ``hard_blobs`` float32 and
    ``indexed`` int32 of x's shape; ``n`` int32 of x's leading shape, the number of candidates;
    ``ids`` int32 and ``confidences`` float32 [..., K], of which the first ``n`` entries per volume
    are the candidates in ascending index (the scipy label in the static modes, 1..n in the dynamic
    one) with the value they are painted with (rounded to ``max_prob_round_decimals`` as
    ``float32(np.round(float64(peak), d))``), the rest 0.

    Host synchronisations: none in the static and dynamic-fast modes. The dynamic mode synchronises
    once per round plus once (rounds + 1; the rounds of a batch are those of its slowest volume, at
    most ``num_lesions_to_extract`` plus the rejected candidates), each time reading back one int32
    per volume."""
    return _lesion_candidates(x, threshold, min_voxels_detection, num_lesions_to_extract,
                              dynamic_threshold_factor, max_prob_round_decimals,
                              remove_adjacent_lesion_candidates)[:5]


# ---- shifted-window (SWIN) token path -----------------------------------------------------
def gather_nd(x, dims, axes, out=None):
    """Flat contiguous gather of ``x`` (csrc/window.hip). ``dims``: [(size, axis, mult)] of the
    output, outermost first; ``axes``: [(extent, stride, shift)] of the input, in elements.
    ``out``: optional contiguous destination of exactly prod(sizes) elements."""
    import ctypes

    _require_cuda(x)
    nd, na = len(dims), len(axes)
    total = 1
    for d in dims:
        total *= int(d[0])
    if out is None:
        out = torch.empty((total,), device=x.device, dtype=torch.float32)
    else:
        _require_cuda(out)
        if out.numel() != total or not out.is_contiguous():
            raise AdellHipError("gather_nd: out must be contiguous with prod(sizes) elements")
    IntA, LongD, LongA = ctypes.c_int * nd, ctypes.c_long * nd, ctypes.c_long * na
    check(_lib.lib().adell_gather_nd(
        _ptr(x), _ptr(out), nd, IntA(*[int(d[0]) for d in dims]), IntA(*[int(d[1]) for d in dims]),
        LongD(*[int(d[2]) for d in dims]), na, LongA(*[int(a[0]) for a in axes]),
        LongA(*[int(a[1]) for a in axes]), LongA(*[int(a[2]) for a in axes]), _stream()))
    return out


def attention_strided_ok(T, A, Dv):
    """Whether the strided forms run (T, A, Dv): the forward plan of aligned operands is an MFMA path."""
    return attention_plan(T, A, Dv, "fwd", aligned=True).path in ("mfma_resident", "mfma_streamed")


def attention_fwd_strided(q, k, v, out, strides, bias, B, H, T, A, Dv, scale, drop_p=0.0, seed=0,
                          offset=0, labels=None):
    """q, k, v, out: tensors whose data pointers are the first rows of sequence 0 (flat views
    into packed buffers are fine); strides: 12 element strides, (item, head, row) for each of
    q, k, v, out. Writes ``out``; returns lse [B*H, T]."""
    _require_cuda(q, k, v, out, bias)
    lse = torch.empty((B * H, T), device=q.device, dtype=torch.float32)
    d = _att_desc(B * H, H, T, A, Dv, scale, drop_p, seed, offset, bias, labels, strides)
    check(_lib.lib().adell_attention_fwd(ctypes.byref(d), _ptr(q), _ptr(k), _ptr(v), _ptr(out),
                                         _ptr(lse), _stream()))
    return lse


def attention_bwd_strided(q, k, v, out, dout, lse, dq, dk, dv, strides, bias, B, H, T, A, Dv, scale,
                          drop_p=0.0, seed=0, offset=0, labels=None):
    """strides: 24 element strides, (item, head, row) for q, k, v, out, dout, dq, dk, dv."""
    _require_cuda(q, k, v, out, dout, lse, dq, dk, dv, bias)
    d = _att_desc(B * H, H, T, A, Dv, scale, drop_p, seed, offset, bias, labels, strides)
    check(_lib.lib().adell_attention_bwd(ctypes.byref(d), _ptr(q), _ptr(k), _ptr(v), _ptr(out),
                                         _ptr(dout), _ptr(lse), _ptr(dq), _ptr(dk), _ptr(dv),
                                         _stream()))


def layernorm_rows_fwd(x, rows, C, inner, so, si, gamma, beta, eps):
    """LayerNorm of ``rows`` rows of C <= 512 values read at (r//inner)*so + (r%inner)*si."""
    _require_cuda(x, gamma, beta)
    y = torch.empty((rows, C), device=x.device, dtype=torch.float32)
    mean = torch.empty((rows,), device=x.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    check(_lib.lib().adell_layernorm_rows_fwd(_ptr(x), rows, C, inner, so, si, _ptr(gamma),
                                              _ptr(beta), float(eps), _ptr(y), _ptr(mean),
                                              _ptr(rstd), _stream()))
    return y, mean, rstd


def layernorm_rows_bwd(x, dy, gamma, mean, rstd, rows, C, inner, so, si, dx, dso, dsi,
                       want_affine):
    """dx is written INTO ``dx`` at the strided row positions (dso, dsi)."""
    _require_cuda(x, dy, dx)
    dg = db = ws = None
    nbytes = 0
    if want_affine:
        dg = torch.empty((C,), device=x.device, dtype=torch.float32)
        db = torch.empty_like(dg)
        nbytes = _lib.lib().adell_layernorm_rows_bwd_workspace(rows, C)
        ws = _workspace(nbytes, x.device)
    check(_lib.lib().adell_layernorm_rows_bwd(_ptr(x), _ptr(dy), _ptr(gamma), _ptr(mean),
                                              _ptr(rstd), rows, C, inner, so, si, _ptr(dx), dso,
                                              dsi, _ptr(dg), _ptr(db), _ptr(ws),
                                              0 if ws is None else ws.numel() * 4, _stream()))
    return dg, db


def winattn_fwd(q, k, v, v_ts, v_hs, rel, mask, W, H, T, A, Dv, scale, drop_p, seed, offset):
    _require_cuda(q, k, v, rel, mask)
    out = torch.empty((W * T, H, Dv), device=q.device, dtype=torch.float32)
    lse = torch.empty((W * H * T,), device=q.device, dtype=torch.float32)
    n_mask = 0 if mask is None else mask.shape[0]
    check(_lib.lib().adell_winattn_fwd(_ptr(q), _ptr(k), _ptr(v), v_ts, v_hs, _ptr(rel),
                                       _ptr(mask), n_mask, W, H, T, A, Dv, float(scale),
                                       float(drop_p), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                       int(offset) & 0xFFFFFFFF, _ptr(out), _ptr(lse), _stream()))
    return out, lse


def winattn_bwd(q, k, v, v_ts, v_hs, rel, mask, o, dout, lse, W, H, T, A, Dv, scale, drop_p,
                seed, offset, dq, dk, dv, want_ds):
    _require_cuda(q, k, v, o, dout, lse, dq, dk, dv)
    n_mask = 0 if mask is None else mask.shape[0]
    ds = torch.empty((W, H * T * T), device=q.device, dtype=torch.float32) if want_ds else None
    check(_lib.lib().adell_winattn_bwd(_ptr(q), _ptr(k), _ptr(v), v_ts, v_hs, _ptr(rel),
                                       _ptr(mask), n_mask, _ptr(o), _ptr(dout), _ptr(lse), W, H, T,
                                       A, Dv, float(scale), float(drop_p),
                                       int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFF,
                                       _ptr(dq), _ptr(dk), _ptr(dv), _ptr(ds), _stream()))
    return ds


def _gemm_launch(kernel, ws_query, call, M, N, K, a_kc, b_kc, device, mn_tensors, tag=""):
    """Workspace by the family's shape-only query, then ``call(workspace)`` under the kernel timer
    (algorithmic bytes: each operand once and ``mn_tensors`` tensors of [M, N])."""
    nws = ws_query(M, N, K)
    ws = _workspace(nws * 4, device) if nws else None
    _timed(kernel, 2.0 * M * N * K, lambda: check(call(_ptr(ws))),
           lambda: f"{M}x{N}x{K} {'kc' if a_kc else 'outer'}/{'kc' if b_kc else 'outer'}{tag}",
           4.0 * (M * K + K * N + M * N * mn_tensors))


def gemm(M, N, K, A, lda, a_kc, B, ldb, b_kc, out=None, bias=None, residual=None):
    """out[M, N] = A x B (+ bias) (+ residual) on the fp32 MFMA GEMM (csrc/gemm.hip).
    a_kc: A(m,k) = A[m*lda + k] else A[k*lda + m]; b_kc: B(k,n) = B[n*ldb + k] else B[k*ldb + n]."""
    _require_cuda(A, B, bias, residual)
    if out is None:
        out = torch.empty((M, N), device=A.device, dtype=torch.float32)
    h, ldr = _lib.lib(), 0 if residual is None else N
    _gemm_launch("adell_gemm_f32_kernel", h.adell_gemm_f32_workspace_floats, lambda ws: h.adell_gemm_f32(
        M, N, K, _ptr(A), lda, int(a_kc), _ptr(B), ldb, int(b_kc), _ptr(out), N, _ptr(bias), _ptr(residual),
        ldr, ws, _stream()), M, N, K, a_kc, b_kc, A.device, 1 + (residual is not None))
    return out


def absmax_word(x):
    """Device word (int32 tensor holding float bits) with the absmax of a dense fp32 tensor: the
    operand scale of ``gemm_f16x3``."""
    _require_cuda(x)
    x = x.contiguous()
    word = torch.zeros(1, device=x.device, dtype=torch.int32)
    check(_lib.lib().adell_absmax_f32(_ptr(x), x.numel(), _ptr(word), _stream()))
    return word


# launch plans of the two GEMM families (adell_gemm_plan, include/adell_hip.h: routes and fields)
GemmF32Plan = collections.namedtuple(
    "GemmF32Plan", "route splits ksteps_per_split reduce chunk_rows per_thread blocks workspace")
GemmF16x3Plan = collections.namedtuple(
    "GemmF16x3Plan", "route epilogue slices pack_rows blocks tiles_per_block wide splits stages_per_split "
    "fold_v fold_s workspace many_rows cu")
GEMM_ROUTES = {"f32": ("rows_small", "tall_lds", "tall_small", "tile_skinny", "tile_square"),
               "f16x3": ("refused", "rows", "tile")}
GEMM_REDUCES, GEMM_EPILOGUES = ("none", "flat", "tree"), ("none", "act_gelu", "act", "dact")
GEMM_OPERANDS = ("a", "b", "c", "bias", "residual", "workspace")


def gemm_plan(family, M, N, K, a_kc=True, b_kc=True, lda=None, ldb=None, unaligned=(), epilogue="none"):
    """What ``gemm`` (``family`` "f32") or ``gemm_f16x3`` / ``gemm_f16x3_act`` ("f16x3") would launch
    under the current tuning switches. ``lda`` / ``ldb``: dense by default; ``unaligned``: the
    GEMM_OPERANDS that are not 16-byte aligned (c / residual: or whose row stride is not a multiple of
    4); ``epilogue``: one of GEMM_EPILOGUES. Host only: no GPU needed."""
    out = (ctypes.c_long * 16)()
    aligned = sum(1 << i for i, name in enumerate(GEMM_OPERANDS) if name not in unaligned)
    check(_lib.lib().adell_gemm_plan(
        family == "f16x3", M, N, K, bool(a_kc), bool(b_kc), (K if a_kc else M) if lda is None else lda,
        (K if b_kc else N) if ldb is None else ldb, aligned, GEMM_EPILOGUES.index(epilogue), out))
    if family == "f16x3":
        return GemmF16x3Plan(GEMM_ROUTES[family][out[0]], GEMM_EPILOGUES[out[1]], *out[2:14])
    return GemmF32Plan(GEMM_ROUTES[family][out[0]], out[1], out[2], GEMM_REDUCES[out[3]], *out[4:8])


@functools.lru_cache(maxsize=None)
def _gemm_f16x3_facts(M, N, K, a_kc, b_kc, lda, ldb, unaligned):
    """(the streaming regime, the f16x3 family refuses it, the fp32 family streams it) off the two plans.
    None of the three depends on a tuning switch, so a shape is asked once (Linear layers ask per call)."""
    h = gemm_plan("f16x3", M, N, K, a_kc, b_kc, lda, ldb, unaligned)
    return (bool(h.many_rows), h.route == "refused",
            gemm_plan("f32", M, N, K, a_kc, b_kc, lda, ldb).route == "rows_small")


def gemm_f16x3_ok(M, N, K, A, lda, a_kc, B, ldb, b_kc):
    """Policy only (the three FLAGS entries) on top of what the plans say: not where the fp32 family
    streams the problem (rows_small), not what the f16x3 family refuses."""
    if not FLAGS["gemm_f16x3"] or K < FLAGS["gemm_f16x3_min_k"]:
        return False
    many_rows, refused, rows_small = _gemm_f16x3_facts(
        M, N, K, bool(a_kc), bool(b_kc), lda, ldb,
        tuple(name for name, t in (("a", A), ("b", B)) if t.data_ptr() % 16))
    # below the default size rule only the streaming regime
    if min(M, N) < FLAGS["gemm_f16x3_min_mn"] and (FLAGS["gemm_f16x3_min_mn"] != 64 or not many_rows):
        return False
    return not rows_small and not refused


def gemm_f16x3(M, N, K, A, lda, a_kc, B, ldb, b_kc, a_amax=None, b_amax=None, out=None, bias=None,
               residual=None):
    """``gemm`` on the f16 MFMA with the error-compensated split (csrc/gemm_f16x3.hip);
    ``a_amax`` / ``b_amax``: None (scales chosen inside the kernel) or the ``absmax_word`` of the
    two operand tensors."""
    _require_cuda(A, B, bias, residual)
    if (a_amax is None) != (b_amax is None) or (a_amax is not None
                                                and not (a_amax.is_cuda and b_amax.is_cuda)):
        raise _lib.AdellHipError("gemm_f16x3: both absmax words (device tensors) or neither")
    if out is None:
        out = torch.empty((M, N), device=A.device, dtype=torch.float32)
    h, ldr = _lib.lib(), 0 if residual is None else N
    _gemm_launch("adell_gemm_f16x3_kernel", h.adell_gemm_f16x3_workspace_floats, lambda ws: h.adell_gemm_f16x3(
        M, N, K, _ptr(A), lda, int(a_kc), _ptr(B), ldb, int(b_kc), _ptr(out), N, _ptr(bias), _ptr(residual),
        ldr, _ptr(a_amax), _ptr(b_amax), ws, _stream()), M, N, K, a_kc, b_kc, A.device,
        1 + (residual is not None))
    return out


def gemm_f16x3_act(M, N, K, A, lda, a_kc, B, ldb, b_kc, act, act_p=0.0, bias=None, residual=None,
                   want_act=False, dact_in=None):
    """``gemm_f16x3`` with an activation in the epilogue (csrc/gemm_f16x3.hip,
    adell_gemm_f16x3_act): ``want_act`` -> returns (C, act(C)); ``dact_in`` [M, N] (a saved
    pre-activation) -> returns (C * act'(dact_in), None)."""
    _require_cuda(A, B, bias, residual, dact_in)
    out = torch.empty((M, N), device=A.device, dtype=torch.float32)
    act_out = torch.empty_like(out) if want_act else None
    h, ldr = _lib.lib(), 0 if residual is None else N
    _gemm_launch("adell_gemm_f16x3_kernel", h.adell_gemm_f16x3_workspace_floats, lambda ws: h.adell_gemm_f16x3_act(
        M, N, K, _ptr(A), lda, int(a_kc), _ptr(B), ldb, int(b_kc), _ptr(out), N, _ptr(bias), _ptr(residual),
        ldr, None, None, ws, _lib.ACT_IDS[act], float(act_p), _ptr(act_out), _ptr(dact_in), _stream()),
        M, N, K, a_kc, b_kc, A.device, 1 + (residual is not None) + want_act + (dact_in is not None), " act")
    return out, act_out


def vicreg_fwd(x1, x2, min_var, eps):
    _require_cuda(x1, x2)
    x1, x2 = x1.contiguous(), x2.contiguous()
    B, D = x1.shape
    scratch = torch.empty(_lib.lib().adell_vicreg_scratch_floats(B, D), device=x1.device,
                          dtype=torch.float32)
    out = torch.empty(3, device=x1.device, dtype=torch.float32)
    check(_lib.lib().adell_vicreg_fwd(_ptr(x1), _ptr(x2), B, D, float(min_var), float(eps),
                                      _ptr(scratch), _ptr(out), _stream()))
    return out, scratch


def vicreg_bwd(x1, x2, scratch, min_var, eps, g, need1, need2):
    B, D = x1.shape
    if not (need1 or need2):
        return None, None
    g = g.contiguous().float()
    dx1 = torch.empty_like(x1) if need1 else None
    dx2 = torch.empty_like(x2) if need2 else None
    check(_lib.lib().adell_vicreg_bwd(_ptr(x1), _ptr(x2), B, D, float(min_var), float(eps),
                                      _ptr(scratch), _ptr(g), _ptr(dx1), _ptr(dx2), _stream()))
    return dx1, dx2


def _top_pairs_check(rc):
    """ADELL_E_UNSUPPORTED of the top-pairs entries (gamma beyond 64 or beyond T^2) is the caller's
    value error, not a library failure."""
    if rc == _lib.E_UNSUPPORTED:
        raise ValueError(_lib.lib().adell_last_error().decode("utf-8", "replace"))
    check(rc)


def top_pairs(a, b, gamma, return_dist2=False):
    """int32 [B, gamma, 2]: per item the (i, j) of the gamma LARGEST Euclidean distances between the
    rows of ``a`` and ``b`` ([B, T, C], dense), ordered by (distance descending, i * T + j
    ascending); with ``return_dist2`` also the squared distances [B, gamma] (csrc/vicregl.hip)."""
    _require_cuda(a, b)
    if a.shape != b.shape or a.dim() != 3:
        raise ValueError(f"top_pairs: two [B, T, C] tensors of one shape, got {tuple(a.shape)} "
                         f"and {tuple(b.shape)}")
    a, b = a.contiguous(), b.contiguous()
    B, T, C = a.shape
    gamma = int(gamma)
    words = _lib.lib().adell_top_pairs_workspace_words(B, T, gamma)
    ws = torch.empty(max(words, 1), device=a.device, dtype=torch.int64)
    pairs = torch.empty((B, gamma, 2), device=a.device, dtype=torch.int32)
    d2 = torch.empty((B, gamma), device=a.device, dtype=torch.float32) if return_dist2 else None
    _top_pairs_check(_lib.lib().adell_top_pairs(
        _ptr(a), _ptr(b), B, T, C, gamma, ctypes.c_void_p(ws.data_ptr()), words,
        ctypes.c_void_p(pairs.data_ptr()), _ptr(d2), _stream()))
    return (pairs, d2) if return_dist2 else pairs


def top_pairs_boxes(box1, box2, spatial, gamma, return_dist2=False):
    """``top_pairs`` of the distances between the token grid of shape ``spatial`` (2 or 3 sizes)
    mapped into the boxes of the two views, ``grid * (hi - lo) + lo`` with ``box = (lo..., hi...)``
    as [B, 2 * ndim]; the coordinates exist in registers only."""
    box1 = box1.float().contiguous()
    box2 = box2.float().contiguous()
    _require_cuda(box1, box2)
    spatial = [int(s) for s in spatial]
    ndim = len(spatial)
    if ndim not in (2, 3):
        raise ValueError(f"top_pairs_boxes: 2 or 3 spatial dimensions, got {ndim}")
    if box1.shape != box2.shape or box1.dim() != 2 or box1.shape[1] != 2 * ndim:
        raise ValueError(f"top_pairs_boxes: boxes of shape [B, {2 * ndim}] expected, got "
                         f"{tuple(box1.shape)} and {tuple(box2.shape)}")
    B, T, gamma = box1.shape[0], int(math.prod(spatial)), int(gamma)
    words = _lib.lib().adell_top_pairs_workspace_words(B, min(T, 65536), gamma)
    ws = torch.empty(max(words, 1), device=box1.device, dtype=torch.int64)
    pairs = torch.empty((B, gamma, 2), device=box1.device, dtype=torch.int32)
    d2 = torch.empty((B, gamma), device=box1.device, dtype=torch.float32) if return_dist2 else None
    dims = (ctypes.c_int * 3)(*(spatial + [1] * (3 - ndim)))
    _top_pairs_check(_lib.lib().adell_top_pairs_boxes(
        _ptr(box1), _ptr(box2), B, ndim, dims, gamma, ctypes.c_void_p(ws.data_ptr()), words,
        ctypes.c_void_p(pairs.data_ptr()), _ptr(d2), _stream()))
    return (pairs, d2) if return_dist2 else pairs


def _pairs_arg(pairs, B):
    if (not pairs.is_cuda or pairs.dtype != torch.int32 or pairs.dim() != 3
            or pairs.shape[0] != B or pairs.shape[2] != 2 or not pairs.is_contiguous()):
        raise _lib.AdellHipError("gather_rows: pairs must be a dense int32 [B, gamma, 2] device tensor")
    return ctypes.c_void_p(pairs.data_ptr())


def gather_rows_fwd(x, pairs, col):
    """out[b * gamma + k] = x[b, pairs[b, k, col]] for x [B, T, C]: [B * gamma, C]."""
    _require_cuda(x)
    x = x.contiguous()
    B, T, C = x.shape
    gamma = pairs.shape[1]
    out = torch.empty((B * gamma, C), device=x.device, dtype=torch.float32)
    check(_lib.lib().adell_gather_rows_fwd(_ptr(x), _pairs_arg(pairs, B), int(col), B, T, C, gamma,
                                           _ptr(out), _stream()))
    return out


def gather_rows_bwd(dout, pairs, col, shape):
    """dx [B, T, C] of ``gather_rows_fwd``: the rows of dout added back in the order of k."""
    _require_cuda(dout)
    dout = dout.contiguous()
    B, T, C = shape
    gamma = pairs.shape[1]
    dx = torch.empty((B, T, C), device=dout.device, dtype=torch.float32)
    check(_lib.lib().adell_gather_rows_bwd(_ptr(dout), _pairs_arg(pairs, B), int(col), B, T, C,
                                           gamma, _ptr(dx), _stream()))
    return dx


# ---- DINO (csrc/dino.hip) ---------------------------------------------------------------------
def dino_loss_plan(R, K):
    """(chunks per row, chunk length): how dino_loss_fwd / dino_loss_bwd split each of the R rows of
    K columns over workgroups. Host only: no GPU needed; the launches call the same function."""
    out = (ctypes.c_int * 2)()
    check(_lib.lib().adell_dino_loss_plan(int(R), int(K), out))
    return int(out[0]), int(out[1])


def _dino_rows(x):
    """[..., K] -> dense [R, K]."""
    return x.reshape(-1, x.shape[-1]).contiguous()


def _dino_centers(centers, K):
    if centers is None:
        return None
    centers = centers.reshape(-1).contiguous()
    if centers.numel() != K:
        raise ValueError(f"dino: {centers.numel()} centres for {K} columns")
    return centers


def dino_loss_fwd(a, b, centers, t1, t2, teacher_is_scores=False, want_mean=False):
    """(loss_rows [R], stats [R, 4]) with loss_r = -sum_k p_t[r, k] log_softmax(a / t1)[r, k] and
    p_t = softmax((b - centers) / t2), or ``b`` itself with ``teacher_is_scores``. stats = (lse of
    a / t1, lse of (b - centers) / t2 | sum_k b, loss_r, sum_k p_t a | 0): all the backward needs. Inputs of more
    than two dimensions are rows of their last one. One pass over a and b, rows split over
    workgroups as ``dino_loss_plan`` says. ``want_mean``: also the mean of the rows (a 0-d tensor,
    from the merge launch itself)."""
    _require_cuda(a, b, centers)
    if a.shape != b.shape:
        raise ValueError(f"dino_loss: shapes {tuple(a.shape)} and {tuple(b.shape)} differ")
    a, b = _dino_rows(a), _dino_rows(b)
    R, K = a.shape
    centers = None if teacher_is_scores else _dino_centers(centers, K)
    floats = _lib.lib().adell_dino_loss_workspace_floats(R, K)
    # one allocation: statistics, row losses, the mean, then the partials of the plan
    buf = torch.empty((5 * R + 4 + floats,), device=a.device, dtype=torch.float32)
    stats, loss_rows, mean = buf[:4 * R].view(R, 4), buf[4 * R:5 * R], buf[5 * R]
    base = buf.data_ptr()
    check(_lib.lib().adell_dino_loss_fwd(_ptr(a), _ptr(b), _ptr(centers), R, K, float(t1), float(t2),
                                         int(bool(teacher_is_scores)),
                                         ctypes.c_void_p(base + 4 * (5 * R + 4)), floats,
                                         ctypes.c_void_p(base + 16 * R), ctypes.c_void_p(base),
                                         ctypes.c_void_p(base + 20 * R) if want_mean else None,
                                         _stream()))
    return (loss_rows, stats, mean) if want_mean else (loss_rows, stats)


def dino_loss_bwd(a, b, centers, stats, t1, t2, g_rows, need_a=True, need_b=False,
                  teacher_is_scores=False, g_mean=None):
    """(da, db) of ``dino_loss_fwd`` for the row gradients ``g_rows`` [R] -- or, with ``g_rows``
    None, for the gradient ``g_mean`` (one element) of the mean of the rows; everything is
    recomputed from ``stats``. db exists in centre mode only and is allocated only with ``need_b``."""
    _require_cuda(a, b, centers, stats, g_rows, g_mean)
    if g_rows is None and g_mean is None:
        raise ValueError("dino_loss_bwd: g_rows or g_mean")
    if need_b and teacher_is_scores:
        raise ValueError("dino_loss_bwd: scores given as they are take no gradient")
    shape = a.shape
    a, b = _dino_rows(a), _dino_rows(b)
    R, K = a.shape
    centers = None if teacher_is_scores else _dino_centers(centers, K)
    da = torch.empty_like(a) if need_a else None
    db = torch.empty_like(b) if need_b else None
    check(_lib.lib().adell_dino_loss_bwd(_ptr(a), _ptr(b), _ptr(centers), _ptr(stats.contiguous()),
                                         None if g_rows is None else _ptr(g_rows.contiguous()),
                                         None if g_rows is not None else _ptr(g_mean.contiguous()),
                                         1.0 / R, R, K, float(t1), float(t2),
                                         int(bool(teacher_is_scores)), _ptr(da), _ptr(db), _stream()))
    return (None if da is None else da.view(shape)), (None if db is None else db.view(shape))


def dino_log_softmax(x, t):
    """log_softmax(x / t) over the last dimension (any width)."""
    x2 = _dino_rows(x)
    _, stats = dino_loss_fwd(x2, x2, None, t, t)
    out = torch.empty_like(x2)
    check(_lib.lib().adell_dino_scores(_ptr(x2), None, _ptr(stats), 0, 0, x2.shape[0], x2.shape[1],
                                       float(t), _ptr(out), _stream()))
    return out.view(x.shape)


def dino_softmax(x, centers, t):
    """softmax((x - centers) / t) over the last dimension (any width)."""
    x2 = _dino_rows(x)
    centers = _dino_centers(centers, x2.shape[1])
    _, stats = dino_loss_fwd(x2, x2, centers, t, t)
    out = torch.empty_like(x2)
    check(_lib.lib().adell_dino_scores(_ptr(x2), _ptr(centers), _ptr(stats), 1, 1, x2.shape[0],
                                       x2.shape[1], float(t), _ptr(out), _stream()))
    return out.view(x.shape)


def dino_center_sum(x):
    """[1, K]: the sum of the rows of x [R, K], rows added in order."""
    _require_cuda(x)
    x = _dino_rows(x)
    out = torch.empty((1, x.shape[1]), device=x.device, dtype=torch.float32)
    check(_lib.lib().adell_dino_center_sum(_ptr(x), x.shape[0], x.shape[1], _ptr(out), _stream()))
    return out


def dino_center_apply(centers, batch_sum, m, denom):
    """In place: centers = centers * m + (batch_sum / denom) * (1 - m)."""
    _require_cuda(centers, batch_sum)
    if not centers.is_contiguous() or batch_sum.numel() != centers.numel():
        raise ValueError("dino_center_apply: dense centres and a sum of the same length expected")
    check(_lib.lib().adell_dino_center_apply(_ptr(centers), _ptr(batch_sum.contiguous()),
                                             centers.numel(), float(m), 1 - float(m), float(denom),
                                             _stream()))
    return centers


def dino_sk_scores(x, t2, iterations, world_size=1, reduce=None):
    """Sinkhorn-Knopp assignment of exp(x / t2) for x [R, K] (DinoLoss.sinkhorn_knopp_teacher): [R, K]
    scores whose rows sum to 1. Factored form Q[k, r] = u_k exp(x[r, k] / t2) v_r: each iteration
    updates the prototype weights u [K] (a column reduction; ``reduce(tensor)`` is called on the
    prototype sums between launches -- torch.distributed.all_reduce where the reference all-reduces
    ``sum_of_rows``) and the sample weights v [R]; exp is recomputed per pass and only the final
    scores are written. The reference's first division by the (all-reduced) total cancels in the
    first prototype normalisation and is not computed."""
    _require_cuda(x)
    if int(iterations) < 1:
        raise ValueError("dino_sk_scores: at least one iteration")
    shape = x.shape
    x = _dino_rows(x)
    R, K = x.shape
    samples = float(R * int(world_size))
    v = torch.ones((R,), device=x.device, dtype=torch.float32)
    t = torch.empty((K,), device=x.device, dtype=torch.float32)
    lib = _lib.lib()
    for _ in range(int(iterations)):
        check(lib.adell_dino_sk_proto_sums(_ptr(x), _ptr(v), R, K, float(t2), _ptr(t), _stream()))
        if reduce is not None:
            reduce(t)
        check(lib.adell_dino_sk_sample_weights(_ptr(x), _ptr(t), R, K, float(t2), samples, _ptr(v),
                                               _stream()))
    out = torch.empty_like(x)
    check(lib.adell_dino_sk_final(_ptr(x), _ptr(t), _ptr(v), R, K, float(t2), samples, _ptr(out),
                                  _stream()))
    return out.view(shape)


L2_NORMALIZE_EPS = 1e-12   # torch.nn.functional.normalize


def l2_normalize_rows_fwd(x):
    """(y, inv): y = x / max(||x||, 1e-12) over the last dimension, inv [rows] the factor."""
    _require_cuda(x)
    x = x.contiguous()
    C = x.shape[-1]
    rows = x.numel() // C
    y = torch.empty_like(x)
    inv = torch.empty((rows,), device=x.device, dtype=torch.float32)
    check(_lib.lib().adell_l2_normalize_rows_fwd(_ptr(x), rows, C, L2_NORMALIZE_EPS, _ptr(y),
                                                 _ptr(inv), _stream()))
    return y, inv


def l2_normalize_rows_bwd(y, dy, inv):
    _require_cuda(y, dy, inv)
    dy = dy.contiguous()
    C = y.shape[-1]
    dx = torch.empty_like(y)
    check(_lib.lib().adell_l2_normalize_rows_bwd(_ptr(y), _ptr(dy), _ptr(inv), y.numel() // C, C,
                                                 L2_NORMALIZE_EPS, _ptr(dx), _stream()))
    return dx


def row_inv_norm_fwd(v, g):
    """s [out] = g / ||v_row|| for v [out, in] and g [out] or [out, 1] (weight norm over dim 0)."""
    _require_cuda(v, g)
    v = v.contiguous()
    rows, C = v.shape
    s = torch.empty((rows,), device=v.device, dtype=torch.float32)
    check(_lib.lib().adell_row_inv_norm_fwd(_ptr(v), _ptr(g.reshape(-1).contiguous()), rows, C,
                                            _ptr(s), _stream()))
    return s


def row_inv_norm_bwd(v, g, ds):
    """dv of ``row_inv_norm_fwd`` (g is frozen: no gradient to it)."""
    _require_cuda(v, g, ds)
    v = v.contiguous()
    rows, C = v.shape
    dv = torch.empty_like(v)
    check(_lib.lib().adell_row_inv_norm_bwd(_ptr(v), _ptr(g.reshape(-1).contiguous()),
                                            _ptr(ds.contiguous()), rows, C, _ptr(dv), _stream()))
    return dv


def row_mean_fwd(x):
    """[..., C] -> [...]: the mean over the last dimension."""
    _require_cuda(x)
    x = x.contiguous()
    C = x.shape[-1]
    out = torch.empty(x.shape[:-1], device=x.device, dtype=torch.float32)
    check(_lib.lib().adell_row_mean_fwd(_ptr(x), x.numel() // C, C, _ptr(out), _stream()))
    return out


def row_mean_bwd(dout, shape):
    _require_cuda(dout)
    dout = dout.contiguous()
    dx = torch.empty(shape, device=dout.device, dtype=torch.float32)
    check(_lib.lib().adell_row_mean_bwd(_ptr(dout), dout.numel(), shape[-1], _ptr(dx), _stream()))
    return dx


def col_scale(x, s):
    """x [R, K] * s [K]."""
    _require_cuda(x, s)
    x = x.contiguous()
    y = torch.empty_like(x)
    check(_lib.lib().adell_col_scale(_ptr(x), _ptr(s.contiguous()), x.shape[0], x.shape[1], _ptr(y),
                                     _stream()))
    return y


def col_scale_dscale(dy, y0):
    """ds [K] = sum_r dy[r, k] * y0[r, k], rows added in order."""
    _require_cuda(dy, y0)
    dy, y0 = dy.contiguous(), y0.contiguous()
    ds = torch.empty((dy.shape[1],), device=dy.device, dtype=torch.float32)
    check(_lib.lib().adell_col_scale_dscale(_ptr(dy), _ptr(y0), dy.shape[0], dy.shape[1], _ptr(ds),
                                            _stream()))
    return ds


# ---- iBOT (csrc/ibot.hip) ---------------------------------------------------------------------
class TokenRows:
    """A set of token rows of a sequence of ``n`` tokens, checked on the host -- the kernels read the
    tables unchecked: ``host`` (int64 numpy, sorted, unique, every entry in [0, n)), ``dev`` the same
    as int32 [M] on ``device`` and ``inv`` int32 [n], token -> its position in ``host`` or -1. Both
    tables travel to the device in one copy."""

    def __init__(self, idx, n, device):
        if isinstance(idx, torch.Tensor):
            idx = idx.detach().cpu().numpy()
        host = np.asarray(idx).reshape(-1)
        if host.size < 1:
            raise ValueError("token rows: at least one row (M >= 1)")
        if not np.issubdtype(host.dtype, np.integer):
            raise TypeError(f"token rows: integer indices expected, got {host.dtype}")
        host = host.astype(np.int64)
        if int(host.min()) < 0 or int(host.max()) >= int(n):
            bad = int(host.max()) if int(host.max()) >= int(n) else int(host.min())
            raise IndexError(f"index {bad} is out of bounds for a sequence of {int(n)} tokens")
        if host.size > 1 and bool((np.diff(host) <= 0).any()):
            raise ValueError("token rows: indices must be sorted and unique")
        self.host, self.n, self.device = host, int(n), torch.device(device)
        both = np.full((host.size + self.n,), -1, dtype=np.int32)
        both[:host.size] = host
        both[host.size + host] = np.arange(host.size, dtype=np.int32)
        self._both = torch.from_numpy(both).to(self.device)
        self.dev, self.inv = self._both[:host.size], self._both[host.size:]

    def __len__(self):
        return int(self.host.size)


_TOKEN_ROWS = collections.OrderedDict()    # (indices, n, device) -> TokenRows, the last few
_TOKEN_ROWS_KEPT = 16


def token_rows(idx, n, device):
    """``TokenRows`` of host indices ``idx`` (numpy / list / tensor; a ``TokenRows`` of the same
    length and device passes through). Raises IndexError for an index outside [0, n) -- before
    anything touches the device. The last few tables per (indices, n, device) are kept: a fixed
    mask costs one upload."""
    device = torch.device(device)
    if isinstance(idx, TokenRows):
        if idx.n != int(n) or idx.device != device:
            return token_rows(idx.host, n, device)
        return idx
    if isinstance(idx, torch.Tensor):
        idx = idx.detach().cpu().numpy()
    arr = np.asarray(idx).reshape(-1)
    key = (arr.astype(np.int64).tobytes() if np.issubdtype(arr.dtype, np.integer) else None,
           int(n), str(device))
    hit = _TOKEN_ROWS.get(key) if key[0] is not None else None
    if hit is not None:
        _TOKEN_ROWS.move_to_end(key)
        return hit
    rows = TokenRows(arr, n, device)
    _TOKEN_ROWS[key] = rows
    while len(_TOKEN_ROWS) > _TOKEN_ROWS_KEPT:
        _TOKEN_ROWS.popitem(last=False)
    return rows


def _ibot_3d(what, *ts):
    for t in ts:
        if t.dim() != 3 or not t.is_contiguous():
            raise ValueError(f"{what}: dense [B, tokens, features] tensors expected, got shape "
                             f"{tuple(t.shape)}, strides {t.stride()}")


def ibot_mask_tokens_fwd(x, idx, token):
    """y = x [B, N, E] with the rows ``idx`` of every item replaced by ``token`` [E] (out of place)."""
    if x.dim() != 3:
        raise ValueError(f"ibot_mask_tokens: [B, N, E] expected, got {tuple(x.shape)}")
    B, N, E = x.shape
    rows = token_rows(idx, N, x.device)
    _require_cuda(x, token)
    _ibot_3d("ibot_mask_tokens", x)
    token = token.reshape(-1).contiguous()
    if token.numel() != E:
        raise ValueError(f"ibot_mask_tokens: a token of {token.numel()} features for {E}")
    y = torch.empty_like(x)
    check(_lib.lib().adell_ibot_mask_tokens_fwd(_ptr(x), _ptr(rows.dev), _ptr(token), B, N, E,
                                                len(rows), _ptr(y), _stream()))
    return y


def ibot_mask_tokens_bwd(dy, idx, need_x=True, need_token=True):
    """(dx, dtoken): dy with the rows ``idx`` zeroed, and their sum over items and rows [E]."""
    if dy.dim() != 3:
        raise ValueError(f"ibot_mask_tokens: [B, N, E] expected, got {tuple(dy.shape)}")
    B, N, E = dy.shape
    rows = token_rows(idx, N, dy.device)
    _require_cuda(dy)
    _ibot_3d("ibot_mask_tokens", dy)
    dx = torch.empty_like(dy) if need_x else None
    dtoken = torch.empty((E,), device=dy.device, dtype=torch.float32) if need_token else None
    check(_lib.lib().adell_ibot_mask_tokens_bwd(_ptr(dy), _ptr(rows.dev), B, N, E, len(rows),
                                                _ptr(dx), _ptr(dtoken), _stream()))
    return dx, dtoken


def ibot_token_sums_plan(B, T, K):
    """(splits of the token axis, tokens per split) of ``ibot_token_sums`` over T tokens. Host only."""
    out = (ctypes.c_int * 2)()
    check(_lib.lib().adell_ibot_token_sums_plan(int(B), int(T), int(K), out))
    return int(out[0]), int(out[1])


def ibot_token_sums(x, first=0, scale=1.0, want_raw=False, raw_out=None):
    """out [B, K] = scale * sum_{t >= first} x[b, t, :] for x [B, Tt, K], accumulated in fp64; with
    ``want_raw`` also the unscaled sums kept in fp64 ([B, K] float64: what ``ibot_center_sum`` adds
    up), written into ``raw_out`` when given (B dense rows of a caller's buffer: no ``cat`` of the
    views). One read of x; tokens added in a fixed order."""
    _require_cuda(x)
    _ibot_3d("ibot_token_sums", x)
    B, Tt, K = x.shape
    if not 0 <= int(first) < Tt:
        raise IndexError(f"ibot_token_sums: first token {first} of {Tt}")
    raw = None
    if want_raw or raw_out is not None:
        raw = torch.empty((B, K), device=x.device, dtype=torch.float64) if raw_out is None else raw_out
        if (raw.dtype != torch.float64 or tuple(raw.shape) != (B, K) or not raw.is_contiguous()
                or raw.device != x.device):
            raise ValueError(f"ibot_token_sums: raw_out must be a dense float64 [{B}, {K}] on "
                             f"{x.device}, got {raw.dtype} {tuple(raw.shape)}")
    doubles = _lib.lib().adell_ibot_token_sums_workspace_doubles(B, Tt - int(first), K)
    out = torch.empty((B, K), device=x.device, dtype=torch.float32)
    work = torch.empty((doubles,), device=x.device, dtype=torch.float64) if doubles else None
    check(_lib.lib().adell_ibot_token_sums(_ptr(x), B, Tt, K, int(first), float(scale), _ptr(work),
                                           doubles, _ptr(out), _ptr(raw), _stream()))
    return (out, raw) if raw is not None else out


def ibot_center_sum(sums):
    """[1, K] float32: the sum over the rows of fp64 token sums [R, K] (``ibot_token_sums``'s raw
    output for the items of every view), rounded once -- ``dino_center_sum`` of all the teacher's
    patch tokens without reading them again."""
    if (not sums.is_cuda or sums.dtype != torch.float64 or sums.dim() != 2
            or not sums.is_contiguous()):
        raise _lib.AdellHipError("ibot_center_sum: dense float64 [R, K] sums on the GPU expected "
                                 "(adell_mri_amd kernels run on MI355X only)")
    out = torch.empty((1, sums.shape[1]), device=sums.device, dtype=torch.float32)
    check(_lib.lib().adell_ibot_center_sum(_ptr(sums), sums.shape[0], sums.shape[1], _ptr(out),
                                           _stream()))
    return out


def ibot_loss_fwd(s, y, rows, centers, t1, t2, teacher_is_scores=False, want_mean=False):
    """``dino_loss_fwd`` over the rows ``(b, rows[j])`` of s [B, Tt, K], read in place: (loss_rows
    [B * M], stats [B * M, 4]) and with ``want_mean`` their mean. The teacher is y [B, Tt, K], read
    at the same rows, or with ``teacher_is_scores`` the dense scores [B * M, K] of those rows."""
    if s.dim() != 3:
        raise ValueError(f"ibot_loss: [B, tokens, K] expected, got {tuple(s.shape)}")
    B, Tt, K = s.shape
    rows = token_rows(rows, Tt, s.device)
    M = len(rows)
    _require_cuda(s, y, centers)
    _ibot_3d("ibot_loss", s)
    if teacher_is_scores:
        if tuple(y.shape) != (B * M, K) or not y.is_contiguous():
            raise ValueError(f"ibot_loss: dense scores [{B * M}, {K}] expected, got {tuple(y.shape)}")
        centers = None
    else:
        _ibot_3d("ibot_loss", y)
        if y.shape != s.shape:
            raise ValueError(f"ibot_loss: shapes {tuple(s.shape)} and {tuple(y.shape)} differ")
        centers = _dino_centers(centers, K)
    R = B * M
    floats = _lib.lib().adell_dino_loss_workspace_floats(R, K)
    buf = torch.empty((5 * R + 4 + floats,), device=s.device, dtype=torch.float32)
    stats, loss_rows, mean = buf[:4 * R].view(R, 4), buf[4 * R:5 * R], buf[5 * R]
    base = buf.data_ptr()
    check(_lib.lib().adell_ibot_loss_fwd(_ptr(s), _ptr(y), _ptr(centers), _ptr(rows.dev), B, Tt, K, M,
                                         float(t1), float(t2), int(bool(teacher_is_scores)),
                                         ctypes.c_void_p(base + 4 * (5 * R + 4)), floats,
                                         ctypes.c_void_p(base + 16 * R), ctypes.c_void_p(base),
                                         ctypes.c_void_p(base + 20 * R) if want_mean else None,
                                         _stream()))
    return (loss_rows, stats, mean) if want_mean else (loss_rows, stats)


def ibot_bwd(s, y, rows, centers, stats, d_red, g_loss, class_token, reduce, t1, t2,
             teacher_is_scores=False, shape=None):
    """ds [B, Tt, K], every element written once by one launch: the gradient ``d_red`` [B, K] of the
    reduced output (``reduce`` "cls": to the class row; "mean": to every patch row, / T) plus, on the
    rows ``rows``, the gradient of the mean masked-row loss for its incoming gradient ``g_loss`` (one
    element), recomputed from ``stats``. Either gradient may be None; without ``g_loss`` only
    ``shape`` (or ``s``) and ``d_red`` are read."""
    if reduce not in ("cls", "mean"):
        raise ValueError(f"ibot_bwd: reduce {reduce!r}")
    B, Tt, K = tuple(s.shape) if shape is None else tuple(shape)
    c = int(bool(class_token))
    M, inv = 0, None
    if g_loss is not None:
        rows = token_rows(rows, Tt, s.device)
        M, inv = len(rows), rows.inv
        _require_cuda(s, y, centers, stats, g_loss)
        _ibot_3d("ibot_bwd", s)
        centers = None if teacher_is_scores else _dino_centers(centers, K)
        stats, g_loss = stats.contiguous(), g_loss.contiguous()
    else:
        s = y = centers = stats = None
    if d_red is None and g_loss is None:
        raise ValueError("ibot_bwd: d_red or g_loss")
    _require_cuda(d_red)
    if d_red is not None:
        d_red = d_red.contiguous()
        if tuple(d_red.shape) != (B, K):
            raise ValueError(f"ibot_bwd: d_red {tuple(d_red.shape)} for [{B}, {K}]")
    dev = d_red.device if d_red is not None else g_loss.device
    ds = torch.empty((B, Tt, K), device=dev, dtype=torch.float32)
    check(_lib.lib().adell_ibot_bwd(_ptr(s), _ptr(y), _ptr(centers), _ptr(stats), _ptr(inv),
                                    _ptr(d_red), _ptr(g_loss), B, Tt, K, M, c,
                                    int(reduce == "cls"), float(t1), float(t2),
                                    int(bool(teacher_is_scores)), _ptr(ds), _stream()))
    return ds


# ---- I-JEPA (csrc/ijepa.hip) ------------------------------------------------------------------
def ijepa_gather_fwd(x, rows):
    """y [B, M, E] = x[:, rows] for x [B, N, E] and sorted unique ``rows`` (host indices or a
    ``TokenRows``). IndexError, on the host, for a row outside [0, N)."""
    if x.dim() != 3:
        raise ValueError(f"ijepa_gather: [B, N, E] expected, got {tuple(x.shape)}")
    B, N, E = x.shape
    rows = token_rows(rows, N, x.device)
    _require_cuda(x)
    _ibot_3d("ijepa_gather", x)
    y = torch.empty((B, len(rows), E), device=x.device, dtype=torch.float32)
    check(_lib.lib().adell_ijepa_gather_fwd(_ptr(x), _ptr(rows.dev), B, N, E, len(rows), _ptr(y),
                                            _stream()))
    return y


def ijepa_gather_bwd(dy, rows, N):
    """dx [B, N, E], written whole by one launch: row n is dy[:, inv[n]] or zeros."""
    if dy.dim() != 3:
        raise ValueError(f"ijepa_gather: [B, M, E] expected, got {tuple(dy.shape)}")
    rows = token_rows(rows, N, dy.device)
    B, M, E = dy.shape
    if M != len(rows):
        raise ValueError(f"ijepa_gather: a gradient of {M} rows for a table of {len(rows)}")
    _require_cuda(dy)
    _ibot_3d("ijepa_gather", dy)
    dx = torch.empty((B, int(N), E), device=dy.device, dtype=torch.float32)
    check(_lib.lib().adell_ijepa_gather_bwd(_ptr(dy), _ptr(rows.inv), B, int(N), E, M, _ptr(dx),
                                            _stream()))
    return dx


def _ijepa_predictor_tables(ctx_rows, tgt_rows, T, device):
    ctx, tgt = token_rows(ctx_rows, T, device), token_rows(tgt_rows, T, device)
    if np.intersect1d(ctx.host, tgt.host).size:
        raise ValueError("ijepa_predictor: context and target rows must be disjoint")
    return ctx, tgt


def ijepa_predictor_fwd(e, pos, mask, ctx_rows, tgt_rows):
    """out [B, nc + nt, P]: ``e + pos[:, ctx]`` followed by ``mask + pos[:, tgt]`` for e [B, nc, P],
    pos [1, T, P] and mask [1, 1, P]; the two row sets are disjoint."""
    if e.dim() != 3 or pos.dim() != 3 or pos.shape[0] != 1 or pos.shape[2] != e.shape[2]:
        raise ValueError(f"ijepa_predictor: e [B, nc, P] and pos [1, T, P] expected, got "
                         f"{tuple(e.shape)} and {tuple(pos.shape)}")
    B, nc, P = e.shape
    T = pos.shape[1]
    ctx, tgt = _ijepa_predictor_tables(ctx_rows, tgt_rows, T, e.device)
    if len(ctx) != nc:
        raise ValueError(f"ijepa_predictor: {nc} context tokens for a table of {len(ctx)}")
    if mask.numel() != P:
        raise ValueError(f"ijepa_predictor: a mask token of {mask.numel()} features for {P}")
    _require_cuda(e, pos, mask)
    _ibot_3d("ijepa_predictor", e, pos)
    mask = mask.reshape(-1).contiguous()
    out = torch.empty((B, nc + len(tgt), P), device=e.device, dtype=torch.float32)
    check(_lib.lib().adell_ijepa_predictor_fwd(_ptr(e), _ptr(pos), _ptr(mask), _ptr(ctx.dev),
                                               _ptr(tgt.dev), B, nc, len(tgt), T, P, _ptr(out),
                                               _stream()))
    return out


def ijepa_predictor_bwd(dout, ctx_rows, tgt_rows, T, need_e=True, need_pos=True, need_mask=True):
    """(de [B, nc, P], dpos [1, T, P], dmask [1, 1, P]) of ``ijepa_predictor_fwd``; dpos is written
    whole (zeros outside both tables), every sum in a fixed order. A gradient that is not needed
    is None (dmask is summed from dpos, which is then computed too)."""
    if dout.dim() != 3:
        raise ValueError(f"ijepa_predictor: [B, nc + nt, P] expected, got {tuple(dout.shape)}")
    ctx, tgt = _ijepa_predictor_tables(ctx_rows, tgt_rows, T, dout.device)
    B, n, P = dout.shape
    nc, nt = len(ctx), len(tgt)
    if n != nc + nt:
        raise ValueError(f"ijepa_predictor: a gradient of {n} rows for {nc} + {nt}")
    _require_cuda(dout)
    _ibot_3d("ijepa_predictor", dout)
    dev = dout.device
    de = torch.empty((B, nc, P), device=dev, dtype=torch.float32) if need_e else None
    dpos = torch.empty((1, int(T), P), device=dev, dtype=torch.float32) \
        if (need_pos or need_mask) else None
    dmask = torch.empty((1, 1, P), device=dev, dtype=torch.float32) if need_mask else None
    check(_lib.lib().adell_ijepa_predictor_bwd(_ptr(dout), _ptr(tgt.dev), _ptr(ctx.inv), _ptr(tgt.inv),
                                               B, nc, nt, int(T), P, _ptr(de), _ptr(dpos),
                                               _ptr(dmask), _stream()))
    return de, (dpos if need_pos else None), dmask


def ijepa_loss_fwd(pred, h, rows):
    """(loss, stats [B * nt, 2]): ``SmoothL1Loss()(pred, layer_norm(h, (E,))[:, rows])`` for pred
    [B, nt, E] and the teacher's raw output h [B, N, E]; the normalised h is never written. stats
    holds (mean, rstd) of every target row for the backward."""
    if pred.dim() != 3 or h.dim() != 3 or h.shape[0] != pred.shape[0] or h.shape[2] != pred.shape[2]:
        raise ValueError(f"ijepa_loss: pred [B, nt, E] and h [B, N, E] expected, got "
                         f"{tuple(pred.shape)} and {tuple(h.shape)}")
    B, nt, E = pred.shape
    N = h.shape[1]
    rows = token_rows(rows, N, pred.device)
    if len(rows) != nt:
        raise ValueError(f"ijepa_loss: {nt} predicted rows for a table of {len(rows)}")
    _require_cuda(pred, h)
    _ibot_3d("ijepa_loss", pred, h)
    R = B * nt
    buf = torch.empty((3 * R + 1,), device=pred.device, dtype=torch.float32)
    stats, part, loss = buf[:2 * R].view(R, 2), buf[2 * R:3 * R], buf[3 * R]
    base = buf.data_ptr()
    check(_lib.lib().adell_ijepa_loss_fwd(_ptr(pred), _ptr(h), _ptr(rows.dev), B, nt, N, E,
                                          ctypes.c_void_p(base), ctypes.c_void_p(base + 8 * R),
                                          ctypes.c_void_p(base + 12 * R), _stream()))
    return loss, stats


def ijepa_loss_bwd(pred, h, rows, stats, g):
    """dpred = g * clamp(pred - target, -1, 1) / (B * nt * E) from the saved statistics; g is the
    incoming gradient (one element, on the device)."""
    B, nt, E = pred.shape
    N = h.shape[1]
    rows = token_rows(rows, N, pred.device)
    _require_cuda(pred, h, stats, g)
    _ibot_3d("ijepa_loss", pred, h)
    if len(rows) != nt or tuple(stats.shape) != (B * nt, 2) or not stats.is_contiguous():
        raise ValueError(f"ijepa_loss: rows / statistics do not match pred {tuple(pred.shape)}")
    g = g.reshape(-1).contiguous()
    dpred = torch.empty_like(pred)
    check(_lib.lib().adell_ijepa_loss_bwd(_ptr(pred), _ptr(h), _ptr(rows.dev), _ptr(stats), _ptr(g),
                                          B, nt, N, E, _ptr(dpred), _stream()))
    return dpred


# ---- masked autoencoder (csrc/mae.hip) --------------------------------------------------------
class MaeShuffle:
    """The per-item token shuffle of ``random_masking``, checked on the host -- the kernels read the
    tables unchecked. ``ids_shuffle`` [B, L] integers, every row a permutation of 0..L-1, and
    ``1 <= len_keep <= L`` (ValueError / IndexError otherwise, before anything touches the device).
    On ``device``, int32: ``keep`` [B, K] = ids_shuffle[:, :K] (kept tokens, in shuffled order),
    ``restore`` [B, L] = the inverse permutation (ids_restore), ``inv`` [B, L] = restore where it is
    < K, else -1 (token -> its kept position); ``mask`` [B, L] float32, 0 keep / 1 remove. The four
    travel to the device in one copy. ``host`` / ``restore_host`` are the int64 numpy originals."""

    def __init__(self, ids_shuffle, len_keep, device):
        if isinstance(ids_shuffle, torch.Tensor):
            ids_shuffle = ids_shuffle.detach().cpu().numpy()
        host = np.asarray(ids_shuffle)
        if host.ndim != 2 or host.size < 1:
            raise ValueError(f"mae shuffle: ids_shuffle [B, L] expected, got shape {host.shape}")
        if not np.issubdtype(host.dtype, np.integer):
            raise TypeError(f"mae shuffle: integer indices expected, got {host.dtype}")
        host = host.astype(np.int64)
        B, L = host.shape
        if int(host.min()) < 0 or int(host.max()) >= L:
            bad = int(host.max()) if int(host.max()) >= L else int(host.min())
            raise IndexError(f"index {bad} is out of bounds for a sequence of {L} tokens")
        if not np.array_equal(np.sort(host, axis=1), np.broadcast_to(np.arange(L), (B, L))):
            raise ValueError("mae shuffle: every row of ids_shuffle must be a permutation of 0..L-1")
        if int(len_keep) != len_keep or not 1 <= int(len_keep) <= L:
            raise ValueError(f"mae shuffle: len_keep must be an integer in [1, {L}], got {len_keep}")
        K = int(len_keep)
        restore = np.argsort(host, axis=1, kind="stable")
        self.host, self.restore_host = host, restore
        self.B, self.L, self.K, self.device = B, L, K, torch.device(device)
        mask = (restore >= K).astype(np.float32)
        packed = np.concatenate([host[:, :K].reshape(-1), restore.reshape(-1),
                                 np.where(restore < K, restore, -1).reshape(-1)]).astype(np.int32)
        packed = np.concatenate([packed, mask.reshape(-1).view(np.int32)])
        self._packed = torch.from_numpy(packed).to(self.device)
        n = B * L
        self.keep = self._packed[:B * K].view(B, K)
        self.restore = self._packed[B * K:B * K + n].view(B, L)
        self.inv = self._packed[B * K + n:B * K + 2 * n].view(B, L)
        self.mask = self._packed[B * K + 2 * n:].view(torch.float32).view(B, L)

    def check(self, what, B, device):
        if B != self.B or torch.device(device) != self.device:
            raise ValueError(f"{what}: a shuffle of {self.B} items on {self.device} for a batch of "
                             f"{B} on {device}")


def _mae_shuffle(what, shuffle, x):
    if not isinstance(shuffle, MaeShuffle):
        raise TypeError(f"{what}: an ops.MaeShuffle expected, got {type(shuffle).__name__}")
    if x.dim() != 3:
        raise ValueError(f"{what}: [B, tokens, E] expected, got {tuple(x.shape)}")
    shuffle.check(what, x.shape[0], x.device)


def mae_gather_rows(x, tab):
    """out [B, No, E]: out[b, o] = x[b, tab[b, o]], zeros where tab[b, o] < 0, for x [B, Ni, E] and a
    device int32 table [B, No] of a ``MaeShuffle`` (checked there; read unchecked here)."""
    _require_cuda(x)
    _ibot_3d("mae_gather_rows", x)
    B, Ni, E = x.shape
    if tab.dtype != torch.int32 or tab.dim() != 2 or tab.shape[0] != B or not tab.is_contiguous():
        raise ValueError(f"mae_gather_rows: a dense int32 table [{B}, No] expected, got "
                         f"{tab.dtype} {tuple(tab.shape)}")
    No = tab.shape[1]
    out = torch.empty((B, No, E), device=x.device, dtype=torch.float32)
    check(_lib.lib().adell_mae_gather_rows(_ptr(x), _ptr(tab), B, No, Ni, E, _ptr(out), _stream()))
    return out


def mae_keep_fwd(x, shuffle):
    """x_masked [B, K, E] = torch.gather(x, 1, ids_keep) for x [B, L, E]."""
    _mae_shuffle("mae_keep", shuffle, x)
    if x.shape[1] != shuffle.L:
        raise ValueError(f"mae_keep: {x.shape[1]} tokens for a shuffle of {shuffle.L}")
    return mae_gather_rows(x, shuffle.keep)


def mae_keep_bwd(dy, shuffle):
    """dx [B, L, E], written whole by one launch: the gradient row of a kept token, zeros elsewhere."""
    _mae_shuffle("mae_keep", shuffle, dy)
    if dy.shape[1] != shuffle.K:
        raise ValueError(f"mae_keep: a gradient of {dy.shape[1]} rows for {shuffle.K} kept tokens")
    return mae_gather_rows(dy, shuffle.inv)


def _mae_restore_shapes(what, rows, mask_token, scale, pos, shuffle, n_rows):
    _mae_shuffle(what, shuffle, rows)
    B, n, E = rows.shape
    if n != n_rows:
        raise ValueError(f"{what}: {n} rows for a shuffle with {n_rows}")
    if mask_token.numel() != E or scale.numel() != 1:
        raise ValueError(f"{what}: a mask token of {E} features and one scale expected, got "
                         f"{tuple(mask_token.shape)} and {tuple(scale.shape)}")
    if pos is not None and (pos.dim() != 3 or tuple(pos.shape) != (1, shuffle.L, E)):
        raise ValueError(f"{what}: pos [1, {shuffle.L}, {E}] expected, got {tuple(pos.shape)}")
    return B, E


def mae_restore_fwd(enc, mask_token, scale, pos, shuffle):
    """out [B, L, E]: the encoded kept tokens enc [B, K, E] back at their places, ``scale *
    mask_token`` at the masked ones, plus pos [1, L, E]; scale [1] is read on the device."""
    B, E = _mae_restore_shapes("mae_restore", enc, mask_token, scale, pos, shuffle, shuffle.K)
    _require_cuda(enc, mask_token, scale, pos)
    _ibot_3d("mae_restore", enc, pos)
    mask_token, scale = mask_token.reshape(-1).contiguous(), scale.reshape(-1).contiguous()
    out = torch.empty((B, shuffle.L, E), device=enc.device, dtype=torch.float32)
    check(_lib.lib().adell_mae_restore_fwd(_ptr(enc), _ptr(mask_token), _ptr(scale), _ptr(pos),
                                           _ptr(shuffle.restore), B, shuffle.L, shuffle.K, E,
                                           _ptr(out), _stream()))
    return out


def mae_restore_bwd(dout, mask_token, scale, shuffle, need_enc=True, need_mask=True,
                    need_scale=True, need_pos=True):
    """(denc [B, K, E], dmask_token [1, 1, E], dscale [1], dpos [1, L, E]) of ``mae_restore_fwd`` in
    at most three launches, every sum in a fixed order; a gradient that is not needed is None."""
    B, E = _mae_restore_shapes("mae_restore", dout, mask_token, scale, None, shuffle, shuffle.L)
    _require_cuda(dout, mask_token, scale)
    _ibot_3d("mae_restore", dout)
    dev, L, K = dout.device, shuffle.L, shuffle.K
    mask_token, scale = mask_token.reshape(-1).contiguous(), scale.reshape(-1).contiguous()
    denc = torch.empty((B, K, E), device=dev, dtype=torch.float32) if need_enc else None
    dpos = torch.empty((1, L, E), device=dev, dtype=torch.float32) if need_pos else None
    dmask = torch.empty((1, 1, E), device=dev, dtype=torch.float32) if need_mask else None
    dscale = torch.empty((1,), device=dev, dtype=torch.float32) if need_scale else None
    part, chunks = None, 0
    if need_mask or need_scale:
        chunks = _lib.lib().adell_mae_restore_bwd_chunks(B, L)
        part = torch.empty((chunks, E), device=dev, dtype=torch.float64)
    check(_lib.lib().adell_mae_restore_bwd(
        _ptr(dout), _ptr(mask_token), _ptr(scale), _ptr(shuffle.keep), _ptr(shuffle.restore), B, L, K,
        E, _ptr(denc), _ptr(dpos), _ptr(dmask), _ptr(dscale),
        None if part is None else ctypes.c_void_p(part.data_ptr()), chunks, _stream()))
    return denc, dmask, dscale, dpos


def _mae_image_shapes(what, pred, image_shape, patch_elems):
    """(B, C, L, P) of token rows pred [B, L, P * C] against an image [B, C, H, W]."""
    if pred.dim() != 3 or len(image_shape) != 4:
        raise ValueError(f"{what}: pred [B, L, P * C] and an image [B, C, H, W] expected, got "
                         f"{tuple(pred.shape)} and {tuple(image_shape)}")
    B, C, H, W = (int(v) for v in image_shape)
    P = int(patch_elems)
    if P < 1 or (H * W) % P:
        raise ValueError(f"{what}: {P} elements per patch do not divide an image of {H} x {W}")
    L = H * W // P
    if tuple(pred.shape) != (B, L, P * C):
        raise ValueError(f"{what}: pred [{B}, {L}, {P * C}] expected for an image {tuple(image_shape)} "
                         f"and {P} elements per patch, got {tuple(pred.shape)}")
    return B, C, L, P


def mae_loss_fwd(pred, x, patch_elems):
    """loss (0-d) = ``MSELoss()(image(pred), x)`` for pred [B, L, P * C] and x [B, C, H, W], where
    image(pred)[b, c].flatten()[l * P + p] = pred[b, l, p * C + c]; the image of pred is not written."""
    B, C, L, P = _mae_image_shapes("mae_loss", pred, x.shape, patch_elems)
    _require_cuda(pred, x)
    if not pred.is_contiguous() or not x.is_contiguous():
        raise ValueError("mae_loss: dense pred and x expected")
    buf = torch.empty((B * L + 1,), device=pred.device, dtype=torch.float32)
    base = buf.data_ptr()
    check(_lib.lib().adell_mae_loss_fwd(_ptr(pred), _ptr(x), B, C, L, P, ctypes.c_void_p(base),
                                        ctypes.c_void_p(base + 4 * B * L), _stream()))
    return buf[B * L]


def mae_loss_bwd(pred, x, patch_elems, g):
    """dpred = g * 2 * (pred - x_at) / (B * C * H * W); g is the incoming gradient (one element, on
    the device)."""
    B, C, L, P = _mae_image_shapes("mae_loss", pred, x.shape, patch_elems)
    _require_cuda(pred, x, g)
    g = g.reshape(-1).contiguous()
    dpred = torch.empty_like(pred)
    check(_lib.lib().adell_mae_loss_bwd(_ptr(pred), _ptr(x), _ptr(g), B, C, L, P, _ptr(dpred),
                                        _stream()))
    return dpred


def mae_to_image(pred, image_shape, patch_elems):
    """[B, C, H, W] with image[b, c].flatten()[l * P + p] = pred[b, l, p * C + c] (C > 1: a copy)."""
    B, C, L, P = _mae_image_shapes("mae_to_image", pred, image_shape, patch_elems)
    _require_cuda(pred)
    _ibot_3d("mae_to_image", pred)
    out = torch.empty(tuple(int(v) for v in image_shape), device=pred.device, dtype=torch.float32)
    check(_lib.lib().adell_mae_to_image(_ptr(pred), B, C, L, P, _ptr(out), _stream()))
    return out


def mae_from_image(image, patch_elems):
    """The inverse copy of ``mae_to_image`` (its gradient): [B, L, P * C] from [B, C, H, W]."""
    if image.dim() != 4:
        raise ValueError(f"mae_from_image: [B, C, H, W] expected, got {tuple(image.shape)}")
    B, C, H, W = image.shape
    P = int(patch_elems)
    if P < 1 or (H * W) % P:
        raise ValueError(f"mae_from_image: {P} elements per patch do not divide {H} x {W}")
    _require_cuda(image)
    if not image.is_contiguous():
        raise ValueError("mae_from_image: a dense image expected")
    L = H * W // P
    out = torch.empty((B, L, P * C), device=image.device, dtype=torch.float32)
    check(_lib.lib().adell_mae_from_image(_ptr(image), B, C, L, P, _ptr(out), _stream()))
    return out


# ---- classification (csrc/classify.hip) -------------------------------------------------------
CLS_LOSS_KINDS = {"bce": 0, "ce": 1, "ordinal": 2}


def _cls_on_device(*ts):
    """Labels and counts are int64 here: only the device is checked (dtypes by each wrapper)."""
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.AdellHipError(
                "adell_mri_amd kernels run on MI355X only: got a CPU tensor (no CPU fallback)")


def _cls_loss_args(kind, logits, target, weight, n_classes):
    """(kind id, logits [B, W], float target or None, int64 target or None, weight or None, nw, B, K)
    checked on the host; K is the number of classes (1 for "bce")."""
    kid = CLS_LOSS_KINDS[kind]
    _cls_on_device(logits, target)
    if logits.dtype != torch.float32:
        raise TypeError(f"cls_loss: fp32 logits expected, got {logits.dtype}")
    B = int(target.shape[0]) if target.dim() else 1
    if kid == 0:
        if logits.numel() != B or target.numel() != B:
            raise ValueError(f"cls_loss (bce): one logit per target expected, got logits "
                             f"{tuple(logits.shape)} and target {tuple(target.shape)}")
        K, W = 1, 1
        tf, ti = target.detach().reshape(B).to(torch.float32).contiguous(), None
    else:
        K = int(n_classes)
        W = K if kid == 1 else K - 1
        if logits.dim() != 2 or tuple(logits.shape) != (B, W) or target.dim() != 1:
            raise ValueError(f"cls_loss ({kind}): logits [{B}, {W}] and labels [{B}] expected for "
                             f"{K} classes, got {tuple(logits.shape)} and {tuple(target.shape)}")
        if target.dtype != torch.int64:
            raise TypeError(f"cls_loss ({kind}): int64 labels expected, got {target.dtype}")
        tf, ti = None, target.detach().contiguous()
    nw = 0
    if weight is not None:
        weight = weight.detach().to(device=logits.device, dtype=torch.float32).reshape(-1).contiguous()
        nw = weight.numel()
        if not (nw in (1, B) if kid == 0 else nw == K):
            raise ValueError(f"cls_loss ({kind}): {nw} weights ("
                             + ("1 or one per item" if kid == 0 else f"one per class, {K}") + " expected)")
    return kid, logits.contiguous().reshape(B, W), tf, ti, weight, nw, B, K


def cls_loss_fwd(kind, logits, target, weight=None, n_classes=None):
    """(item [B], reduced 0-d, aux) of the loss ``kind`` in CLS_LOSS_KINDS on logits; one launch.
    "bce": ``BCEWithLogitsLoss(weight)`` (item weights, 1 or B), reduced = mean; "ce":
    ``CrossEntropyLoss(weight)`` (class weights), reduced = sum(item) / sum(w[y]); "ordinal":
    ``ordinal_sigmoidal_loss`` on [B, K - 1] logits, reduced = mean. A label outside [0, K) gives a
    NaN item (and gradient); it is never used as an index. ``aux`` (the denominator, a double on the
    device) goes to ``cls_loss_bwd``."""
    kid, x, tf, ti, w, nw, B, K = _cls_loss_args(kind, logits, target, weight, n_classes)
    buf = torch.empty((B + 1,), device=x.device, dtype=torch.float32)
    aux = torch.empty((1,), device=x.device, dtype=torch.float64)
    base = buf.data_ptr()
    check(_lib.lib().adell_cls_loss_fwd(kid, _ptr(x), _ptr(tf), _ptr(ti), _ptr(w), nw, B, K,
                                        ctypes.c_void_p(base), ctypes.c_void_p(base + 4 * B), _ptr(aux),
                                        _stream()))
    return buf[:B], buf[B], aux


def cls_loss_bwd(kind, logits, target, weight, n_classes, g, per_item, aux):
    """dlogits from the gradient of the reduced value (``g`` one element) or of the items (``g``
    [B], ``per_item``); one launch."""
    kid, x, tf, ti, w, nw, B, K = _cls_loss_args(kind, logits, target, weight, n_classes)
    _cls_on_device(g)
    g = g.detach().to(torch.float32).reshape(-1).contiguous()
    if g.numel() != (B if per_item else 1):
        raise ValueError(f"cls_loss_bwd: a gradient of {g.numel()} elements for {B} items")
    dx = torch.empty_like(x)
    check(_lib.lib().adell_cls_loss_bwd(kid, _ptr(x), _ptr(tf), _ptr(ti), _ptr(w), nw, _ptr(g),
                                        int(bool(per_item)), _ptr(aux), B, K, _ptr(dx), _stream()))
    return dx.view(logits.shape)


def _cls_roc_args(pre_bias, target):
    _cls_on_device(pre_bias, target)
    B = int(target.shape[0])
    if pre_bias.numel() != B or target.dim() != 1 or target.dtype != torch.int64:
        raise ValueError(f"cls_roc: pre_bias of {B} elements and int64 labels [{B}] expected, got "
                         f"{tuple(pre_bias.shape)} and {target.dtype} {tuple(target.shape)}")
    if pre_bias.dtype != torch.float32:
        raise TypeError(f"cls_roc: fp32 pre_bias expected, got {pre_bias.dtype}")
    return pre_bias.contiguous().reshape(B), target.detach().contiguous(), B


def cls_roc_fwd(pre_bias, target):
    """(loss 0-d, aux): ``relative_order_consistency``; aux[0] = the number of ordered pairs M (a
    double on the device). M = 0 gives NaN."""
    p, y, B = _cls_roc_args(pre_bias, target)
    rows = torch.empty((B + 1,), device=p.device, dtype=torch.float64)
    loss = torch.empty((1,), device=p.device, dtype=torch.float32)
    base = rows.data_ptr()
    check(_lib.lib().adell_cls_roc_fwd(_ptr(p), _ptr(y), B, ctypes.c_void_p(base), _ptr(loss),
                                       ctypes.c_void_p(base + 8 * B), _stream()))
    return loss[0], rows[B:]


def cls_roc_bwd(pre_bias, target, g, aux):
    p, y, B = _cls_roc_args(pre_bias, target)
    _cls_on_device(g)
    g = g.detach().to(torch.float32).reshape(-1).contiguous()
    dp = torch.empty_like(p)
    check(_lib.lib().adell_cls_roc_bwd(_ptr(p), _ptr(y), _ptr(g), _ptr(aux), B, _ptr(dp), _stream()))
    return dp.view(pre_bias.shape)


def cls_mixup(x, factor, partner):
    """out[b] = factor[b] * x[b] + (1 - factor[b]) * x[partner[b]] for x [B, ...] (fp32, dense; any
    element offset), the three operations rounded one by one as torch's expression; a row with
    ``partner[b] == b`` is copied. ``partner``: host integers in [0, B) (checked here)."""
    _cls_on_device(x)
    if x.dtype != torch.float32 or x.dim() < 1 or not x.is_contiguous():
        raise ValueError(f"cls_mixup: a dense fp32 batch expected, got {x.dtype} {tuple(x.shape)} "
                         f"strides {x.stride()}")
    B = int(x.shape[0])
    V = x.numel() // max(B, 1)
    host = np.asarray(partner).reshape(-1)
    if host.shape[0] != B or not np.issubdtype(host.dtype, np.integer):
        raise ValueError(f"cls_mixup: {B} integer partners expected, got {host.dtype} {host.shape}")
    if B and (host.min() < 0 or host.max() >= B):
        raise IndexError(f"cls_mixup: a partner outside [0, {B})")
    factor = torch.as_tensor(factor, dtype=torch.float32, device=x.device).reshape(-1).contiguous()
    if factor.numel() != B:
        raise ValueError(f"cls_mixup: {B} factors expected, got {factor.numel()}")
    out = torch.empty_like(x)
    if B == 0 or V == 0:
        return out
    tab = torch.from_numpy(host.astype(np.int32)).to(x.device)
    check(_lib.lib().adell_cls_mixup(_ptr(x), _ptr(factor), _ptr(tab), B, V, _ptr(out), _stream()))
    return out


def cls_confusion_update(preds, target, counts):
    """counts (int64 [C * C + 1], on the device; row = label, column = prediction, last = samples
    with a label or an integer prediction outside [0, C)) += the samples of one update. ``preds``:
    fp32 [N, C] (argmax: first maximal index, a NaN wins), fp32 [N] probabilities (``p > 0.5``,
    C = 2) or int64 [N] classes; ``target`` int64 [N]. No host synchronisation."""
    _cls_on_device(preds, target, counts)
    if counts.dtype != torch.int64 or counts.dim() != 1 or not counts.is_contiguous():
        raise ValueError("cls_confusion_update: counts must be a dense int64 vector")
    C = int(round(math.sqrt(counts.numel() - 1)))
    if C < 2 or C * C + 1 != counts.numel():
        raise ValueError(f"cls_confusion_update: counts of {counts.numel()} elements are no C * C + 1")
    N = int(target.shape[0])
    if target.dtype != torch.int64 or target.dim() != 1:
        raise ValueError(f"cls_confusion_update: int64 labels [N] expected, got {target.dtype} "
                         f"{tuple(target.shape)}")
    target = target.contiguous()
    pf = pi = None
    if preds.dtype == torch.int64:
        mode, pi = 2, preds.contiguous()
        ok = tuple(preds.shape) == (N,)
    elif preds.dtype == torch.float32 and preds.dim() == 2:
        mode, pf = 0, preds.contiguous()
        ok = tuple(preds.shape) == (N, C)
    elif preds.dtype == torch.float32:
        mode, pf = 1, preds.contiguous()
        ok = tuple(preds.shape) == (N,) and C == 2
    else:
        raise TypeError(f"cls_confusion_update: fp32 or int64 predictions expected, got {preds.dtype}")
    if not ok:
        raise ValueError(f"cls_confusion_update: predictions {tuple(preds.shape)} do not match {N} "
                         f"labels and {C} classes")
    if N == 0:
        return
    check(_lib.lib().adell_cls_confusion_update(mode, _ptr(pf), _ptr(pi), _ptr(target), N, C,
                                                _ptr(counts), _stream()))


def cls_auroc_pairs(scores, target):
    """int64 [3] on the device: (2 #{pos > neg} + #{pos == neg}, positives, negatives) over the
    pairs of a positive (label 1) and a negative (label 0) sample; exact."""
    _cls_on_device(scores, target)
    N = int(target.shape[0])
    if scores.dtype != torch.float32 or target.dtype != torch.int64 or tuple(scores.shape) != (N,) \
            or target.dim() != 1:
        raise ValueError(f"cls_auroc_pairs: fp32 scores [N] and int64 labels [N] expected, got "
                         f"{scores.dtype} {tuple(scores.shape)} and {target.dtype} {tuple(target.shape)}")
    out = torch.zeros((3,), device=scores.device, dtype=torch.int64)
    if N:
        check(_lib.lib().adell_cls_auroc_pairs(_ptr(scores.contiguous()), _ptr(target.contiguous()), N,
                                               _ptr(out), _stream()))
    return out


# ---- multiple-instance classification (csrc/mil.hip) -------------------------------------------
MIL_MODES = {"mean": 0, "max": 1, "vocabulary": 2}


def _mil_dense(what, *ts):
    """fp32 device tensors, dense row-major (a view with gaps or a permuted one is refused here,
    whatever ADELL_CHECK_DENSE says: these kernels index from the shape alone)."""
    _require_cuda(*ts)
    for t in ts:
        if t is not None and not t.is_contiguous():
            raise _lib.AdellHipError(f"{what}: non-dense tensor handed to a kernel: shape "
                                     f"{tuple(t.shape)}, strides {t.stride()}")


def mil_volume_to_slices(x):
    """[B, C, H, W, S] -> [B * S, C, H, W], item b * S + s holding slice s of item b
    (``"b c h w s -> (b s) c h w"``); a copy, one launch."""
    if x.dim() != 5:
        raise ValueError(f"mil_volume_to_slices: a volume [B, C, H, W, S] expected, got "
                         f"{tuple(x.shape)}")
    _mil_dense("mil_volume_to_slices", x)
    B, C, H, W, S = (int(v) for v in x.shape)
    out = torch.empty((B * S, C, H, W), device=x.device, dtype=torch.float32)
    if out.numel():
        check(_lib.lib().adell_mil_volume_to_slices(_ptr(x), B, C, H * W, S, _ptr(out), _stream()))
    return out


def mil_slices_to_volume(y, n_slices):
    """The inverse copy: [B * S, C, H, W] -> [B, C, H, W, S]."""
    S = int(n_slices)
    if y.dim() != 4 or S < 1 or y.shape[0] % S:
        raise ValueError(f"mil_slices_to_volume: slices [B * {S}, C, H, W] expected, got "
                         f"{tuple(y.shape)}")
    _mil_dense("mil_slices_to_volume", y)
    BS, C, H, W = (int(v) for v in y.shape)
    out = torch.empty((BS // S, C, H, W, S), device=y.device, dtype=torch.float32)
    if out.numel():
        check(_lib.lib().adell_mil_slices_to_volume(_ptr(y), BS // S, C, H * W, S, _ptr(out),
                                                    _stream()))
    return out


def _mil_pool_args(what, mode, feat, hv, hu, w, b, with_bias=True):
    """(mode id, B, S, N, F) checked on the host; ``feat`` or the gate inputs may be None (the
    backward has no use for the bias: ``with_bias=False``)."""
    if mode not in MIL_MODES:
        raise ValueError(f"{what}: mode must be one of {sorted(MIL_MODES)}, got {mode!r}")
    gate = (hv, hu, w, b) if with_bias else (hv, hu, w)
    if any(t is None for t in gate) and not all(t is None for t in gate):
        raise ValueError(f"{what}: hv, hu, w and b go together (all or none)")
    if hv is None and feat is None:
        raise ValueError(f"{what}: neither gate inputs nor features")
    lead = feat if feat is not None else hv
    if lead.dim() != 3:
        raise ValueError(f"{what}: [B, S, features] expected, got {tuple(lead.shape)}")
    B, S = int(lead.shape[0]), int(lead.shape[1])
    F = int(feat.shape[2]) if feat is not None else 0
    N = 0
    if hv is not None:
        N = int(hv.shape[-1])
        if tuple(hv.shape) != (B, S, N) or tuple(hu.shape) != (B, S, N) or w.numel() != N \
                or (with_bias and b.numel() != 1):
            raise ValueError(f"{what}: hv and hu [{B}, {S}, N], w [N] and b [1] expected, got "
                             f"{tuple(hv.shape)}, {tuple(hu.shape)}, {tuple(w.shape)}"
                             + (f", {tuple(b.shape)}" if with_bias else ""))
    if B < 1 or S < 1 or (feat is not None and F < 1) or (hv is not None and N < 1):
        raise ValueError(f"{what}: empty input {tuple(lead.shape)}")
    _mil_dense(what, feat, hv, hu, w, b)
    return MIL_MODES[mode], B, S, N, F


def mil_pool_fwd(mode, feat, hv=None, hu=None, w=None, b=None):
    """(pooled [B, F] or None, A [B, S, 1], saved) in one launch: A the gated-attention softmax over
    the slices of hv, hu [B, S, N] with the row w [N] and bias b [1] (1 / S without them), pooled
    by ``mode`` in MIL_MODES from feat [B, S, F] (None: only A). ``saved``: the int32 arg-max
    [B, F] ("max"), the row (max, log-sum) [B, S, 2] ("vocabulary"), else None."""
    mid, B, S, N, F = _mil_pool_args("mil_pool_fwd", mode, feat, hv, hu, w, b)
    dev = (feat if feat is not None else hv).device
    A = torch.empty((B, S, 1), device=dev, dtype=torch.float32)
    pooled = torch.empty((B, F), device=dev, dtype=torch.float32) if F else None
    arg = rowstat = None
    if F and mid == 1:
        arg = torch.empty((B, F), device=dev, dtype=torch.int32)
    if F and mid == 2:
        rowstat = torch.empty((B, S, 2), device=dev, dtype=torch.float32)
    check(_lib.lib().adell_mil_pool_fwd(
        mid, _ptr(hv), _ptr(hu), _ptr(w), _ptr(b), _ptr(feat), B, S, N, F, _ptr(A), _ptr(pooled),
        None if arg is None else ctypes.c_void_p(arg.data_ptr()), _ptr(rowstat), _stream()))
    return pooled, A, (arg if mid == 1 else rowstat)


def mil_pool_bwd(mode, feat, hv, hu, w, A, saved, g, gA):
    """(dfeat, dhv, dhu, dw, db) of ``mil_pool_fwd`` from the gradient g [B, F] of pooled and gA
    [B, S, 1] (or None) of A; two launches, one without the gate. A gradient whose input was None
    is None."""
    mid, B, S, N, F = _mil_pool_args("mil_pool_bwd", mode, feat, hv, hu, w, None, with_bias=False)
    dev = A.device
    if F:
        g = (torch.zeros((B, F), device=dev, dtype=torch.float32) if g is None
             else g.to(torch.float32).contiguous())
        if tuple(g.shape) != (B, F):
            raise ValueError(f"mil_pool_bwd: a gradient [{B}, {F}] expected, got {tuple(g.shape)}")
    else:
        g = None
    if gA is not None:
        gA = gA.to(torch.float32).contiguous()
        if gA.numel() != B * S:
            raise ValueError(f"mil_pool_bwd: a gradient of A with {B * S} elements expected, got "
                             f"{tuple(gA.shape)}")
    if tuple(A.shape) != (B, S, 1):
        raise ValueError(f"mil_pool_bwd: A [{B}, {S}, 1] expected, got {tuple(A.shape)}")
    _mil_dense("mil_pool_bwd", A, g, gA)
    arg = saved if mid == 1 else None
    rowstat = saved if mid == 2 else None
    if F and mid == 1 and (arg is None or arg.dtype != torch.int32 or tuple(arg.shape) != (B, F)
                           or not arg.is_cuda or not arg.is_contiguous()):
        raise ValueError(f"mil_pool_bwd: the int32 arg-max [{B}, {F}] of the forward expected")
    if F and mid == 2 and (rowstat is None or tuple(rowstat.shape) != (B, S, 2)):
        raise ValueError(f"mil_pool_bwd: the row statistics [{B}, {S}, 2] of the forward expected")
    _mil_dense("mil_pool_bwd", rowstat)
    dfeat = torch.empty_like(feat) if F else None
    dhv = dhu = dw = db = part = None
    if hv is not None:
        dhv, dhu = torch.empty_like(hv), torch.empty_like(hu)
        dwb = torch.empty((N + 1,), device=dev, dtype=torch.float32)
        dw, db = dwb[:N], dwb[N:]
        part = torch.empty((B, N + 1), device=dev, dtype=torch.float64)
    check(_lib.lib().adell_mil_pool_bwd(
        mid, _ptr(hv), _ptr(hu), _ptr(w), _ptr(feat), _ptr(A),
        None if arg is None else ctypes.c_void_p(arg.data_ptr()), _ptr(rowstat), _ptr(g), _ptr(gA),
        B, S, N, F, _ptr(dfeat), _ptr(dhv), _ptr(dhu),
        None if dw is None else ctypes.c_void_p(dw.data_ptr()),
        None if db is None else ctypes.c_void_p(db.data_ptr()),
        None if part is None else ctypes.c_void_p(part.data_ptr()), _stream()))
    return dfeat, dhv, dhu, dw, db


def _mil_token_args(what, x, pos, class_token):
    if x.dim() != 3:
        raise ValueError(f"{what}: x [B, S, E] expected, got {tuple(x.shape)}")
    B, S, E = (int(v) for v in x.shape)
    if pos is not None and tuple(pos.shape) != (1, S, 1):
        raise ValueError(f"{what}: pos [1, {S}, 1] (one scalar per slice) expected, got "
                         f"{tuple(pos.shape)}")
    if class_token is not None and tuple(class_token.shape) != (1, 1, E):
        raise ValueError(f"{what}: class_token [1, 1, {E}] expected, got {tuple(class_token.shape)}")
    if B < 1 or S < 1 or E < 1:
        raise ValueError(f"{what}: empty input {tuple(x.shape)}")
    return B, S, E


def mil_slice_tokens_fwd(x, pos=None, class_token=None):
    """out [B, S (+ 1), E]: row 0 the class token (when given), row (1 +) s = x[b, s] + pos[s];
    one launch."""
    B, S, E = _mil_token_args("mil_slice_tokens", x, pos, class_token)
    _mil_dense("mil_slice_tokens", x, pos, class_token)
    ct = 0 if class_token is None else 1
    out = torch.empty((B, S + ct, E), device=x.device, dtype=torch.float32)
    check(_lib.lib().adell_mil_slice_tokens_fwd(_ptr(x), _ptr(pos), _ptr(class_token), B, S, E,
                                                _ptr(out), _stream()))
    return out


def mil_slice_tokens_bwd(dout, n_slices, has_class_token, need_x=True, need_pos=True,
                         need_class_token=True):
    """(dx [B, S, E], dpos [1, S, 1], dclass_token [1, 1, E]) in one launch, the two sums over the
    batch in order in fp64; a gradient that is not needed is None."""
    ct, S = int(bool(has_class_token)), int(n_slices)
    if dout.dim() != 3 or dout.shape[1] != S + ct:
        raise ValueError(f"mil_slice_tokens_bwd: a gradient [B, {S + ct}, E] expected, got "
                         f"{tuple(dout.shape)}")
    _mil_dense("mil_slice_tokens_bwd", dout)
    B, _, E = (int(v) for v in dout.shape)
    dev = dout.device
    dx = torch.empty((B, S, E), device=dev, dtype=torch.float32) if need_x else None
    dpos = torch.empty((1, S, 1), device=dev, dtype=torch.float32) if need_pos else None
    dcls = (torch.empty((1, 1, E), device=dev, dtype=torch.float32)
            if need_class_token and ct else None)
    check(_lib.lib().adell_mil_slice_tokens_bwd(_ptr(dout), B, S, E, ct, _ptr(dx), _ptr(dpos),
                                                _ptr(dcls), _stream()))
    return dx, dpos, dcls


PAIR_LOSS_KINDS = {"simsiam": 0, "byol": 1, "ntxent": 2}


def pair_loss_fwd(x1, x2, kind, temperature=1.0, apply_relu=False):
    """(loss [1], scratch) of a cosine-similarity loss between two [B, D] embedding batches."""
    _require_cuda(x1, x2)
    x1, x2 = x1.contiguous(), x2.contiguous()
    if x1.dim() != 2 or x1.shape != x2.shape:
        raise AdellHipError(f"pair_loss: two [B, D] tensors of one shape expected, got "
                            f"{tuple(x1.shape)} and {tuple(x2.shape)}")
    B, D = x1.shape
    scratch = torch.empty(max(_lib.lib().adell_pair_loss_scratch_floats(B, D), 1),
                          device=x1.device, dtype=torch.float32)
    loss = torch.empty(1, device=x1.device, dtype=torch.float32)
    check(_lib.lib().adell_pair_loss_fwd(_ptr(x1), _ptr(x2), B, D, PAIR_LOSS_KINDS[kind],
                                         float(temperature), int(bool(apply_relu)),
                                         _ptr(scratch), _ptr(loss), _stream()))
    return loss, scratch


def pair_loss_bwd(x1, x2, kind, temperature, apply_relu, scratch, g, need1, need2):
    if not (need1 or need2):
        return None, None
    B, D = x1.shape
    g = g.reshape(1).contiguous().float()
    dx1 = torch.empty_like(x1) if need1 else None
    dx2 = torch.empty_like(x2) if need2 else None
    check(_lib.lib().adell_pair_loss_bwd(_ptr(x1), _ptr(x2), B, D, PAIR_LOSS_KINDS[kind],
                                         float(temperature), int(bool(apply_relu)),
                                         _ptr(scratch), _ptr(g), _ptr(dx1), _ptr(dx2), _stream()))
    return dx1, dx2


def loco_loss_fwd(f1, f2, temperature, eps):
    """Per-item local contrastive loss [B] of two NDHWC feature maps [B, C, *spatial]
    (semi_supervised_segmentation/losses.py:498-526)."""
    _require_cuda(f1, f2)
    f1, f2 = ndhwc(f1), ndhwc(f2)
    if f1.shape != f2.shape:
        raise AdellHipError(f"loco_loss: feature shapes differ ({tuple(f1.shape)} vs "
                            f"{tuple(f2.shape)})")
    B, C = f1.shape[0], f1.shape[1]
    S = f1.numel() // (B * C)
    nbytes = _lib.lib().adell_loco_loss_workspace(B, S, C)
    check(min(nbytes, 0))
    ws = _workspace(nbytes, f1.device)
    loss = torch.empty(B, device=f1.device, dtype=torch.float32)
    check(_lib.lib().adell_loco_loss_fwd(_ptr(f1), _ptr(f2), B, S, C, float(temperature),
                                         float(eps), _ptr(loss), _ptr(ws), ws.numel() * 4,
                                         _stream()))
    return loss


def loco_loss_bwd(f1, f2, gloss, temperature, eps, need1, need2):
    if not (need1 or need2):
        return None, None
    f1, f2 = ndhwc(f1), ndhwc(f2)
    B, C = f1.shape[0], f1.shape[1]
    S = f1.numel() // (B * C)
    gloss = gloss.contiguous().float()
    df1 = new_act(*f1.shape, f1.device) if need1 else None
    df2 = new_act(*f2.shape, f2.device) if need2 else None
    check(_lib.lib().adell_loco_loss_bwd(_ptr(f1), _ptr(f2), _ptr(gloss), B, S, C,
                                         float(temperature), float(eps), _ptr(df1), _ptr(df2),
                                         _stream()))
    return df1, df2


# ---- class-axis softmax head, channel max pooling -------------------------------------------------
def channel_softmax_fwd(x):
    """softmax over dim 1 of a logical [N, C, *spatial] tensor (NDHWC memory), C <= 32."""
    _require_cuda(x)
    x = ndhwc(x)
    C = x.shape[1]
    y = new_act(*x.shape, x.device)
    check(_lib.lib().adell_channel_softmax_fwd(_ptr(x), _ptr(y), x.numel() // C, C, _stream()))
    return y


def channel_softmax_bwd(y, dy):
    _require_cuda(y, dy)
    y, dy = ndhwc(y), ndhwc(dy)
    C = y.shape[1]
    dx = new_act(*y.shape, y.device)
    check(_lib.lib().adell_channel_softmax_bwd(_ptr(y), _ptr(dy), _ptr(dx), y.numel() // C, C,
                                               _stream()))
    return dx


def channel_max_fwd(x):
    """[N, C, D, H, W] -> ([N, C] maxima over the voxels, [N, C] int32 voxel indices)."""
    _require_cuda(x)
    x = ndhwc(x)
    N, C = x.shape[:2]
    V = x.numel() // (N * C)
    out = torch.empty((N, C), device=x.device, dtype=torch.float32)
    arg = torch.empty((N, C), device=x.device, dtype=torch.int32)
    check(_lib.lib().adell_channel_max_fwd(_ptr(x), _ptr(out), _ptr(arg), N, V, C, _stream()))
    return out, arg


def channel_max_bwd(dout, arg, shape):
    _require_cuda(dout)
    if not arg.is_cuda or arg.dtype != torch.int32:
        raise _lib.AdellHipError("channel_max_bwd: arg must be the int32 CUDA tensor of the forward")
    N, C = shape[:2]
    V = int(math.prod(shape[2:]))
    dx = new_act(N, C, *shape[2:], dout.device)
    dc = dout.contiguous()
    check(_lib.lib().adell_channel_max_bwd(_ptr(dc), _ptr(arg), _ptr(dx), N, V, C, _stream()))
    return dx


# ---- element-wise segmentation losses (loss_factory members beyond dice + focal) ---------------
SEG_LOSS_KINDS = {"binary_cross_entropy": 0, "cat_cross_entropy": 1, "mc_focal": 2, "mc_dice": 3}


def seg_loss_fwd(kind, p, t, cw, eps, scale, ls, gamma, smooth, w_pos):
    """p, t: [B, V, C] contiguous (NDHWC order). Returns (loss [B], sums [B, C, 2])."""
    _require_cuda(p, t, cw)
    B, V, C = p.shape
    ws = _workspace(_lib.lib().adell_seg_loss_workspace(B, V, C), p.device)
    loss = torch.empty((B,), device=p.device, dtype=torch.float32)
    sums = torch.empty((B, C, 2), device=p.device, dtype=torch.float32)
    check(_lib.lib().adell_seg_loss_fwd(kind, _ptr(p), _ptr(t), _ptr(cw), B, V, C, eps, scale, ls,
                                        gamma, smooth, w_pos, _ptr(loss), _ptr(sums), _ptr(ws),
                                        ws.numel() * 4, _stream()))
    return loss, sums


def seg_loss_bwd(kind, p, t, cw, eps, scale, ls, gamma, smooth, w_pos, sums, gout):
    _require_cuda(p, t, cw, sums, gout)
    B, V, C = p.shape
    dp = torch.empty_like(p)
    gc = gout.contiguous()
    check(_lib.lib().adell_seg_loss_bwd(kind, _ptr(p), _ptr(t), _ptr(cw), B, V, C, eps, scale, ls,
                                        gamma, smooth, w_pos, _ptr(sums), _ptr(gc), _ptr(dp),
                                        _stream()))
    return dp


OPTIM_KINDS = {"adamax": 0, "adagrad": 1, "nadam": 2, "radam": 3, "rmsprop": 4}


def optim_step(kind, param, grad, s1, s2, weight_decay, eps, grad_scale, c5):
    """One fused step of adamax / adagrad / nadam / radam / rmsprop on flat fp32 buffers."""
    _require_cuda(param, grad, s1, s2)
    # doubles: the kernel's 1 - beta comes from the betas as given, not from their fp32 roundings
    arr = (ctypes.c_double * 5)(*[float(v) for v in (list(c5) + [0.0] * 5)[:5]])
    check(_lib.lib().adell_optim_step(OPTIM_KINDS[kind], _ptr(param), _ptr(grad), _ptr(s1),
                                      _ptr(s2), param.numel(), weight_decay, eps, grad_scale, arr,
                                      _stream()))
    _weights_changed()


# ---- device-side batch augmentation (csrc/augment.hip) -------------------------------------------
def item_stats(x):
    """[N, 4] = (min, max, mean, population std) of every batch item of ``x`` (any layout: the
    statistics are over all elements of the item)."""
    _require_cuda(x)
    N = x.shape[0]
    per = x.numel() // N
    assert x.is_contiguous() or ndhwc(x).data_ptr() == x.data_ptr()
    out = torch.empty((N, 4), device=x.device, dtype=torch.float32)
    ws = _workspace(_lib.lib().adell_item_stats_workspace(N, per), x.device)
    check(_lib.lib().adell_item_stats(_ptr(x), N, per, _ptr(out), _ptr(ws), ws.numel() * 4, _stream()))
    return out


def aug_intensity(x, params, seed=0, rng_offset=0):
    """Gamma contrast -> std shift -> Rician noise of every item in one pass; ``params`` [N, 8]
    device rows {min, range, gamma, shift, noise std, 0, 0, 0} (adell_aug_intensity)."""
    _require_cuda(x, params)
    N = x.shape[0]
    out = torch.empty_like(x)
    check(_lib.lib().adell_aug_intensity(_ptr(x), _ptr(out), N, x.numel() // N, _ptr(params),
                                         int(seed) & 0xFFFFFFFFFFFFFFFF, int(rng_offset) & 0xFFFFFFFF,
                                         _stream()))
    return out


def affine_sample(x, theta, linear=True, pad_mode="reflection"):
    """Affine resampling of [N, C, D, H, W] (NDHWC memory) volumes about their centres; ``theta``
    [N, 12] device rows of the 3 x 4 voxel-space matrices (adell_affine_sample)."""
    _require_cuda(x, theta)
    x = ndhwc(x)
    N, C, D, H, W = x.shape
    out = new_act(N, C, D, H, W, x.device)
    check(_lib.lib().adell_affine_sample(_ptr(x), _ptr(out), N, D, H, W, C, _ptr(theta),
                                         1 if linear else 0,
                                         {"zeros": 0, "border": 1, "reflection": 2}[pad_mode],
                                         _stream()))
    return out


def axis_filter(x, taps, axis):
    """1-D filter along spatial axis 0 / 1 / 2 (zero padding); ``taps`` [N, 2 R + 1] device rows."""
    _require_cuda(x, taps)
    x = ndhwc(x)
    N, C, D, H, W = x.shape
    out = new_act(N, C, D, H, W, x.device)
    check(_lib.lib().adell_axis_filter(_ptr(x), _ptr(out), N, D, H, W, C, int(axis), _ptr(taps),
                                       (taps.shape[1] - 1) // 2, _stream()))
    return out


def bias_field(x, coef):
    """x * exp(Legendre polynomial field); ``coef`` [N, 64] device rows (dense 4 x 4 x 4 cube)."""
    _require_cuda(x, coef)
    x = ndhwc(x)
    N, C, D, H, W = x.shape
    out = new_act(N, C, D, H, W, x.device)
    check(_lib.lib().adell_bias_field(_ptr(x), _ptr(out), N, D, H, W, C, _ptr(coef), _stream()))
    return out


def axis_lut_sample(x, lut, linear=True):
    """Resampling through per-axis coordinate tables ``lut`` [N, D + H + W] (border padding)."""
    _require_cuda(x, lut)
    x = ndhwc(x)
    N, C, D, H, W = x.shape
    out = new_act(N, C, D, H, W, x.device)
    check(_lib.lib().adell_axis_lut_sample(_ptr(x), _ptr(out), N, D, H, W, C, _ptr(lut),
                                           1 if linear else 0, _stream()))
    return out


def gibbs_lowpass(x, radius):
    """k-space low-pass per item: spectrum zeroed outside ``radius`` [N] (device) about the centre of
    the shifted spectrum."""
    _require_cuda(x, radius)
    x = ndhwc(x)
    N, C, D, H, W = x.shape
    out = new_act(N, C, D, H, W, x.device)
    nbytes = _lib.lib().adell_gibbs_workspace(N, D, H, W, C)
    if nbytes < 0:
        check(int(nbytes))
    ws = _workspace(nbytes, x.device)
    check(_lib.lib().adell_gibbs_lowpass(_ptr(x), _ptr(out), N, D, H, W, C, _ptr(radius), _ptr(ws),
                                         ws.numel() * 4, _stream()))
    return out


def resize_linear(x, size):
    """F.interpolate(x, size=size, mode="trilinear", align_corners=False) on [N, C, D, H, W]."""
    _require_cuda(x)
    x = ndhwc(x)
    N, C, Di, Hi, Wi = x.shape
    Do, Ho, Wo = (int(v) for v in size)
    y = new_act(N, C, Do, Ho, Wo, x.device)
    check(_lib.lib().adell_interp_linear_fwd(_ptr(x), _ptr(y), N, C, Di, Hi, Wi, Do, Ho, Wo,
                                             Do / Di, Ho / Hi, Wo / Wi, 0, _stream()))
    return y


# ---- 3-D object detection (csrc/detect.hip) -----------------------------------------------------
def _det_layout(what, *ts):
    """0 when every tensor is dense row-major, 1 when every one is dense channels-last (the layout
    the conv kernels produce: [B, C, H, W, D] logical, [B, H, W, D, C] in memory); anything else --
    a view with gaps, a mix -- is refused, whatever ADELL_CHECK_DENSE says."""
    ts = [t for t in ts if t is not None]
    if all(t.is_contiguous() for t in ts):
        return 0
    if all(t.dim() == 5 and t.is_contiguous(memory_format=torch.channels_last_3d) for t in ts):
        return 1
    raise _lib.AdellHipError(f"{what}: non-dense tensor (or a mix of layouts) handed to a kernel: "
                             + ", ".join(f"shape {tuple(t.shape)} strides {t.stride()}" for t in ts))


def _det_dense(what, *ts, dtype=torch.float32, layouts=False):
    """Device tensors of ``dtype``, dense row-major (``layouts``: or dense channels-last, checked by
    ``_det_layout``): these kernels index from the shape alone."""
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.AdellHipError(f"{what}: adell_mri_amd kernels run on MI355X only: got a CPU "
                                     "tensor (no CPU fallback)")
        if t.dtype != dtype:
            raise _lib.AdellHipError(f"{what}: {dtype} expected, got {t.dtype}")
        if not t.is_contiguous() and not (
                layouts and t.dim() == 5 and t.is_contiguous(memory_format=torch.channels_last_3d)):
            raise _lib.AdellHipError(f"{what}: non-dense tensor handed to a kernel: shape "
                                     f"{tuple(t.shape)}, strides {t.stride()}")


def _det_grid(what, obj_like, n_anchors, per_anchor):
    if obj_like.dim() != 5:
        raise ValueError(f"{what}: a [B, C, H, W, D] map expected, got {tuple(obj_like.shape)}")
    B, C, H, W, D = (int(v) for v in obj_like.shape)
    A = int(n_anchors)
    if A < 1 or B < 1 or H * W * D < 1:
        raise ValueError(f"{what}: empty grid {tuple(obj_like.shape)} with {A} anchors")
    return B, C, H, W, D, A


def det_positive_table(target, n_anchors, threshold, first_channel=1, per_anchor=7):
    """(table int32 [B A H W D, 5], count int32 [1]): the rows (b, h, w, d, a) of the cells of
    ``target`` [B, first_channel + per_anchor * A, H, W, D] whose objectness channel
    (``first_channel + per_anchor * a``) is > ``threshold``, in ``torch.where``'s order on the stacked
    [B, H, W, D, A] view; rows beyond ``count`` are not written. Three launches, no host read."""
    what = "det_positive_table"
    _det_dense(what, target, layouts=True)
    B, C, H, W, D, A = _det_grid(what, target, n_anchors, per_anchor)
    if per_anchor not in (1, 7) or first_channel < 0 or first_channel + per_anchor * A > C:
        raise ValueError(f"{what}: {C} channels cannot hold {A} anchors of {per_anchor} from channel "
                         f"{first_channel}")
    cells = B * A * H * W * D
    table = torch.empty((cells, 5), device=target.device, dtype=torch.int32)
    count = torch.empty((1,), device=target.device, dtype=torch.int32)
    scratch = torch.empty((int(_lib.lib().adell_det_table_blocks(cells)),), device=target.device,
                          dtype=torch.int32)
    check(_lib.lib().adell_det_positive_table(_ptr(target), B, A, H, W, D, C, int(first_channel),
                                              int(per_anchor), _det_layout(what, target),
                                              float(threshold), _ptr(scratch),
                                              _ptr(table), _ptr(count), _stream()))
    return table, count


def _det_heads(what, centre, size, obj, target, anchors, table, count, first_channel):
    _det_dense(what, centre, size, obj, target, layouts=True)
    _det_dense(what, anchors)
    _det_dense(what, table, count, dtype=torch.int32)
    B, A, H, W, D = (int(v) for v in obj.shape) if obj.dim() == 5 else (0,) * 5
    if obj.dim() != 5 or tuple(centre.shape) != (B, 3 * A, H, W, D) or tuple(size.shape) != tuple(centre.shape):
        raise ValueError(f"{what}: centre and size [B, 3 A, H, W, D] and objectness [B, A, H, W, D] "
                         f"expected, got {tuple(centre.shape)}, {tuple(size.shape)}, {tuple(obj.shape)}")
    if anchors.numel() != 3 * A:
        raise ValueError(f"{what}: {A} anchors of 3 sizes expected, got {tuple(anchors.shape)}")
    if tuple(table.shape) != (B * A * H * W * D, 5) or count.numel() != 1:
        raise ValueError(f"{what}: the table of det_positive_table for this grid expected, got "
                         f"{tuple(table.shape)}")
    Ct = 0
    if target is not None:
        Ct = int(target.shape[1])
        if target.dim() != 5 or tuple(target.shape) != (B, Ct, H, W, D) or first_channel < 0 \
                or first_channel + 7 * A > Ct:
            raise ValueError(f"{what}: target [B, {first_channel} + 7 A, H, W, D] expected, got "
                             f"{tuple(target.shape)}")
    return B, A, H, W, D, Ct, _det_layout(what, target), _det_layout(what, centre, size, obj)


def det_loss_fwd(centre, size, obj, target, anchors, table, count, corr, first_channel=1):
    """(out [5] = loss, bce mean, mean(1 - iou), mean(cpd), mean(ar); rows [4, cells] = iou, cpd, ar
    and the cross-entropy correction of every positive, valid up to ``count``). Two launches."""
    what = "det_loss_fwd"
    B, A, H, W, D, Ct, cl_t, cl_h = _det_heads(what, centre, size, obj, target, anchors, table, count,
                                               first_channel)
    cells = B * A * H * W * D
    dev = obj.device
    partial = torch.empty((int(_lib.lib().adell_det_loss_partials(cells)),), device=dev, dtype=torch.float64)
    rows = torch.empty((4, cells), device=dev, dtype=torch.float32)
    out = torch.empty((5,), device=dev, dtype=torch.float32)
    check(_lib.lib().adell_det_loss_fwd(_ptr(centre), _ptr(size), _ptr(obj), _ptr(target), _ptr(anchors),
                                        _ptr(table), _ptr(count), float(corr[0]), float(corr[1]),
                                        float(corr[2]), B, A, H, W, D, Ct, int(first_channel),
                                        cl_t, cl_h, _ptr(partial), _ptr(rows), _ptr(out), _stream()))
    return out, rows


def det_loss_bwd(centre, size, obj, target, anchors, table, count, corr, grad_out, first_channel=1):
    """(dcentre, dsize, dobj) of ``det_loss_fwd``'s loss times ``grad_out`` [1] (device); written
    whole, two launches."""
    what = "det_loss_bwd"
    B, A, H, W, D, Ct, cl_t, cl_h = _det_heads(what, centre, size, obj, target, anchors, table, count,
                                               first_channel)
    _det_dense(what, grad_out)
    if grad_out.numel() != 1:
        raise ValueError(f"{what}: a scalar gradient expected, got {tuple(grad_out.shape)}")
    # the gradients take the heads' layout: the dense pass walks memory, not indices
    fmt = torch.channels_last_3d if cl_h else torch.contiguous_format
    dcentre, dsize, dobj = (torch.empty(t.shape, device=t.device, dtype=t.dtype, memory_format=fmt)
                            for t in (centre, size, obj))
    check(_lib.lib().adell_det_loss_bwd(_ptr(centre), _ptr(size), _ptr(obj), _ptr(target), _ptr(anchors),
                                        _ptr(table), _ptr(count), float(corr[0]), float(corr[1]),
                                        float(corr[2]), B, A, H, W, D, Ct, int(first_channel),
                                        cl_t, cl_h, _ptr(grad_out), _ptr(dcentre),
                                        _ptr(dsize), _ptr(dobj), _stream()))
    return dcentre, dsize, dobj


def det_nms_max():
    return int(_lib.lib().adell_det_nms_max())


def det_nms_keep(boxes, iou_threshold):
    """keep int32 [n] (1: survives) of the greedy sweep over ``boxes`` [n, 6], which are sorted by
    descending score: candidate j > i goes when i is kept, ``check_overlap(i, j)`` and
    ``calculate_iou(i, j) > iou_threshold``. Two launches."""
    what = "det_nms_keep"
    _det_dense(what, boxes)
    if boxes.dim() != 2 or boxes.shape[1] != 6:
        raise ValueError(f"{what}: boxes [n, 6] expected, got {tuple(boxes.shape)}")
    n = int(boxes.shape[0])
    if n > det_nms_max():
        raise ValueError(f"{what}: {n} candidates, at most {det_nms_max()}")
    keep = torch.empty((n,), device=boxes.device, dtype=torch.int32)
    if n:
        mask = torch.empty((n * ((n + 63) // 64),), device=boxes.device, dtype=torch.int64)
        check(_lib.lib().adell_det_nms(_ptr(boxes), n, float(iou_threshold), _ptr(mask), _ptr(keep),
                                       _stream()))
    return keep


def det_decode(centre, size, obj, cls, anchors, table, count, corr):
    """(boxes [cells, 6], scores [cells], classes [cells, NC] or [cells], starts int32 [B + 1]) of the
    cells in ``table`` (objectness > 0.5, ``det_positive_table(obj, A, 0.5, 0, 1)``); rows beyond
    ``starts[B]`` are not written. ``cls`` None: the classes are the objectness. One launch."""
    what = "det_decode"
    B, A, H, W, D, _, _, cl_h = _det_heads(what, centre, size, obj, None, anchors, table, count, 0)
    NC = 0
    if cls is not None:
        _det_dense(what, cls, layouts=True)
        cl_h = _det_layout(what, centre, size, obj, cls)
        NC = int(cls.shape[1])
        if tuple(cls.shape) != (B, NC, H, W, D) or NC < 1:
            raise ValueError(f"{what}: class head [B, C, H, W, D] expected, got {tuple(cls.shape)}")
    cells, dev = B * A * H * W * D, obj.device
    boxes = torch.empty((cells, 6), device=dev, dtype=torch.float32)
    scores = torch.empty((cells,), device=dev, dtype=torch.float32)
    classes = torch.empty((cells, NC) if NC else (cells,), device=dev, dtype=torch.float32)
    starts = torch.empty((B + 1,), device=dev, dtype=torch.int32)
    check(_lib.lib().adell_det_decode(_ptr(centre), _ptr(size), _ptr(obj), _ptr(cls), NC, _ptr(anchors),
                                      _ptr(table), _ptr(count), float(corr[0]), float(corr[1]),
                                      float(corr[2]), B, A, H, W, D, cl_h, _ptr(boxes), _ptr(scores),
                                      _ptr(classes), _ptr(starts), _stream()))
    return boxes, scores, classes, starts


def det_match(targets, target_image, preds, pred_start):
    """(best int32 [T], iou [T]): for target box t of image ``target_image[t]`` the prediction among
    ``preds[pred_start[img]:pred_start[img + 1]]`` with the highest IoU of the overlapping ones, its
    index within the image (lowest on a tie; 0 with IoU 0 when none overlaps; -1 without predictions)."""
    what = "det_match"
    _det_dense(what, targets, preds)
    _det_dense(what, target_image, pred_start, dtype=torch.int32)
    T = int(targets.shape[0])
    if targets.dim() != 2 or targets.shape[1] != 6 or preds.dim() != 2 or preds.shape[1] != 6 \
            or target_image.numel() != T:
        raise ValueError(f"{what}: targets [T, 6], their images [T] and predictions [P, 6] expected")
    best = torch.empty((T,), device=targets.device, dtype=torch.int32)
    iou = torch.empty((T,), device=targets.device, dtype=torch.float32)
    if T:
        check(_lib.lib().adell_det_match(_ptr(targets), _ptr(target_image), T, _ptr(preds),
                                         _ptr(pred_start), _ptr(best), _ptr(iou), _stream()))
    return best, iou


def det_encode(boxes, classes, counts, half, rel, thresh, output_sh):
    """The anchor maps [B, 1 + 7 A, *output_sh] (fp64) of padded boxes [B, N, 6], classes [B, N] and
    counts [B] (int32): ``BBToAdjustedAnchors.__call__`` per item. ``half`` [A, 3] fp64 = anchor /
    rel_sh / 2, ``rel`` the three input / output ratios the boxes are divided by. One launch."""
    what = "det_encode"
    _det_dense(what, boxes, classes, half, dtype=torch.float64)
    _det_dense(what, counts, dtype=torch.int32)
    if boxes.dim() != 3 or boxes.shape[2] != 6 or tuple(classes.shape) != tuple(boxes.shape[:2]) \
            or counts.numel() != boxes.shape[0] or half.dim() != 2 or half.shape[1] != 3:
        raise ValueError(f"{what}: boxes [B, N, 6], classes [B, N], counts [B], half [A, 3] expected, got "
                         f"{tuple(boxes.shape)}, {tuple(classes.shape)}, {tuple(counts.shape)}, "
                         f"{tuple(half.shape)}")
    B, N, A = int(boxes.shape[0]), int(boxes.shape[1]), int(half.shape[0])
    H, W, D = (int(v) for v in output_sh)
    out = torch.empty((B, 1 + 7 * A, H, W, D), device=counts.device, dtype=torch.float64)
    check(_lib.lib().adell_det_encode(_ptr(boxes) if N else None, _ptr(classes) if N else None,
                                      _ptr(counts), _ptr(half), float(rel[0]), float(rel[1]),
                                      float(rel[2]), float(thresh), B, N, A, H, W, D, _ptr(out),
                                      _stream()))
    return out


def adamw_amsgrad_step(param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, lr, beta1, beta2, eps,
                       weight_decay, step, grad_scale=1.0):
    """torch.optim.AdamW(amsgrad=True) over one flat run; one launch."""
    _require_cuda(param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq)
    check(_lib.lib().adell_adamw_amsgrad_step(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq),
                                              _ptr(max_exp_avg_sq), param.numel(), lr, beta1, beta2,
                                              eps, weight_decay, int(step), grad_scale, _stream()))
    _weights_changed()


# ---- DDPM diffusion (csrc/diffusion.hip) ---------------------------------------------------------
ECA_MAX_SITES = 32        # gate blocks per grouped launch
ECA_MAX_DIM = 1024        # widest site / embedding of the grouped gate kernels
DIFFUSION_X0, DIFFUSION_CLIP = 1, 2
_ECA_PARAMS = 8           # class_to_channels.{weight,bias}, op.1.*, op.2.*, op.4.*


def _dif_layout(what, *ts):
    """0 when every tensor is dense row-major, 1 when every one is dense channels-last (4-D or 5-D, the
    layout the conv kernels leave); a view with gaps or a mix of layouts is refused whatever
    ADELL_CHECK_DENSE says, and so are CPU tensors and other dtypes."""
    ts = [t for t in ts if t is not None]
    for t in ts:
        if not t.is_cuda:
            raise _lib.AdellHipError(f"{what}: adell_mri_amd kernels run on MI355X only: got a CPU "
                                     "tensor (no CPU fallback)")
        if t.dtype != torch.float32:
            raise _lib.AdellHipError(f"{what}: adell_mri_amd kernels are fp32; got {t.dtype}")
    if all(t.is_contiguous() for t in ts):
        return 0
    if all((t.dim() == 5 and t.is_contiguous(memory_format=torch.channels_last_3d))
           or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last)) for t in ts):
        return 1
    raise _lib.AdellHipError(f"{what}: non-dense tensor (or a mix of layouts) handed to a kernel: "
                             + ", ".join(f"shape {tuple(t.shape)} strides {t.stride()}" for t in ts))


def _dif_channels_last(what, x):
    """(N, V, C) of an activation [N, C, *spatial] whose memory is dense [N, *spatial, C]."""
    if not x.is_cuda:
        raise _lib.AdellHipError(f"{what}: adell_mri_amd kernels run on MI355X only: got a CPU tensor "
                                 "(no CPU fallback)")
    if x.dtype != torch.float32:
        raise _lib.AdellHipError(f"{what}: adell_mri_amd kernels are fp32; got {x.dtype}")
    if x.dim() not in (4, 5):
        raise ValueError(f"{what}: [N, C, H, W] or [N, C, D, H, W] expected, got {tuple(x.shape)}")
    fmt = torch.channels_last_3d if x.dim() == 5 else torch.channels_last
    if not x.is_contiguous(memory_format=fmt):
        raise _lib.AdellHipError(f"{what}: the activation must be dense channels-last memory (the "
                                 f"layout the conv kernels leave): shape {tuple(x.shape)}, strides "
                                 f"{x.stride()}")
    N, C = int(x.shape[0]), int(x.shape[1])
    if N < 1 or C < 1 or x.numel() == 0:
        raise ValueError(f"{what}: empty activation {tuple(x.shape)}")
    return N, x.numel() // (N * C), C


def _eca_gate_rows(what, x_shape_n, z, C):
    if z.dim() != 2 or z.shape[1] != C or z.shape[0] not in (1, x_shape_n):
        raise ValueError(f"{what}: gate logits [1 or {x_shape_n}, {C}] expected, got {tuple(z.shape)}")
    _dif_layout(what, z)
    return int(z.shape[0])


def eca_gates_fwd(t, cls, params, eps):
    """Gate logits of every site in one launch. ``t`` [Gt] fp32 (None: no sinusoidal part), ``cls`` [Ng, T] or None, ``params``
    one tuple of the eight parameter tensors per site, ``eps`` LayerNorm's. Returns (z per site
    [Ng, C], saved) with saved = (emb [Ng, T], the sites' records)."""
    what = "eca_gates_fwd"
    n_sites = len(params)
    if not 1 <= n_sites <= ECA_MAX_SITES:
        raise ValueError(f"{what}: 1..{ECA_MAX_SITES} sites per call, got {n_sites}")
    _dif_layout(what, t, cls, *[p for site in params for p in site])
    T = int(params[0][0].shape[1])
    if t is None and cls is None:
        raise ValueError(f"{what}: neither timesteps nor class rows")
    Gt = int(t.numel()) if t is not None else 0
    Ng = int(cls.shape[0]) if cls is not None else Gt
    if cls is not None and (cls.dim() != 2 or cls.shape[1] != T):
        raise ValueError(f"{what}: class embedding [{Ng}, {T}] expected, got {tuple(cls.shape)}")
    if t is not None and Gt not in (1, Ng):
        raise ValueError(f"{what}: {Gt} timesteps for {Ng} class rows (1 or {Ng})")
    dev = params[0][0].device
    emb = torch.empty((Ng, T), device=dev, dtype=torch.float32)
    zs, recs, words = [], [], []
    for site in params:
        w0, b0, w1, b1, lg, lb, w2, b2 = site
        C = int(w0.shape[0])
        shapes = [(C, T), (C,), (C, C), (C,), (C,), (C,), (C, C), (C,)]
        if len(site) != _ECA_PARAMS or [tuple(p.shape) for p in site] != shapes:
            raise ValueError(f"{what}: a site's parameters must have shapes {shapes}, got "
                             f"{[tuple(p.shape) for p in site]}")
        z = torch.empty((Ng, C), device=dev, dtype=torch.float32)
        rec = torch.empty((Ng, 8 * C + 4), device=dev, dtype=torch.float32)
        zs.append(z)
        recs.append(rec)
        words += [C] + [p.data_ptr() for p in site] + [z.data_ptr(), rec.data_ptr()]
    table = (ctypes.c_longlong * len(words))(*words)
    check(_lib.lib().adell_eca_gates_fwd(table, n_sites, _ptr(t), Gt, _ptr(cls), Ng, T, float(eps),
                                         _ptr(emb), _stream()))
    return zs, (emb, recs)


def eca_gates_bwd(params, saved, gzs, need_cls):
    """Gradients of ``eca_gates_fwd`` in two launches: (one tuple of eight parameter gradients per
    site, the gradient [Ng, T] of the class embedding or None). ``gzs``: per site the gradient of its
    logits, or None where none arrived."""
    what = "eca_gates_bwd"
    emb, recs = saved
    Ng, T = int(emb.shape[0]), int(emb.shape[1])
    _dif_layout(what, emb, *recs, *[g for g in gzs if g is not None])
    words, grads = [], []
    for site, rec, gz in zip(params, recs, gzs):
        C = int(site[0].shape[0])
        if gz is not None and tuple(gz.shape) != (Ng, C):
            raise ValueError(f"{what}: a gradient [{Ng}, {C}] expected, got {tuple(gz.shape)}")
        d = tuple(torch.empty_like(p) for p in site)
        grads.append(d)
        words += ([C] + [p.data_ptr() for p in site] + [gz.data_ptr() if gz is not None else 0,
                                                          rec.data_ptr()] + [g.data_ptr() for g in d])
    de = torch.empty_like(emb) if need_cls else None
    table = (ctypes.c_longlong * len(words))(*words)
    check(_lib.lib().adell_eca_gates_bwd(table, len(params), _ptr(emb), _ptr(de), Ng, T, _stream()))
    return grads, de


def eca_apply_fwd(x, z):
    """x [N, C, *spatial] (channels-last memory) times sigmoid(z) with z [1 or N, C]; one launch."""
    N, V, C = _dif_channels_last("eca_apply", x)
    Ng = _eca_gate_rows("eca_apply", N, z, C)
    y = torch.empty_like(x)
    check(_lib.lib().adell_eca_apply_fwd(_ptr(x), _ptr(z), Ng, _ptr(y), N, V, C, _stream()))
    return y


def eca_apply_bwd(x, z, dy, need_x=True, need_z=True):
    """(dx, dz) of ``eca_apply_fwd``: one pass over x and dy, then the fold of its partial sums."""
    what = "eca_apply_bwd"
    N, V, C = _dif_channels_last(what, x)
    Ng = _eca_gate_rows(what, N, z, C)
    if dy.shape != x.shape:
        raise ValueError(f"{what}: gradient {tuple(dy.shape)} for an activation {tuple(x.shape)}")
    _dif_channels_last(what, dy)
    dx = torch.empty_like(x) if need_x else None
    dz = part = None
    if need_z:
        dz = torch.empty_like(z)
        n = _lib.lib().adell_eca_apply_bwd_workspace_doubles(N, V, C)
        part = torch.empty(n, device=x.device, dtype=torch.float64)
    if dx is None and dz is None:
        return None, None
    check(_lib.lib().adell_eca_apply_bwd(_ptr(x), _ptr(dy), _ptr(z), Ng, _ptr(dx), _ptr(dz),
                                         _ptr(part), N, V, C, _stream()))
    return dx, dz


def diffusion_noise(x, epsilon, alpha_bar, t):
    """sqrt(alpha_bar[t_n]) x + sqrt(1 - alpha_bar[t_n]) epsilon per item; ``alpha_bar`` [S] fp32 and
    ``t`` [N] int64 on the device; one launch."""
    what = "diffusion_noise"
    _dif_layout(what, x, epsilon)
    _dif_layout(what, alpha_bar)
    if x.shape != epsilon.shape or x.dim() < 1 or x.numel() == 0:
        raise ValueError(f"{what}: x {tuple(x.shape)} and epsilon {tuple(epsilon.shape)} differ")
    N = int(x.shape[0])
    if not t.is_cuda:
        raise _lib.AdellHipError(f"{what}: adell_mri_amd kernels run on MI355X only: got CPU timesteps")
    if t.dtype != torch.int64 or t.numel() != N or not t.is_contiguous():
        raise _lib.AdellHipError(f"{what}: t must be a dense int64 tensor of {N} timesteps, got "
                                 f"{t.dtype} {tuple(t.shape)}")
    y = torch.empty_like(x)
    check(_lib.lib().adell_diffusion_noise(_ptr(x), _ptr(epsilon), _ptr(alpha_bar),
                                           int(alpha_bar.numel()), _ptr(t), _ptr(y), N,
                                           x.numel() // N, _stream()))
    return y


def diffusion_reverse_step(x, eps, eps_uncond, noise, coef, scale, flags):
    """out = c_x x + c_e e + c_x0 x0 + c_n noise (adell_diffusion_reverse_step); ``coef`` = (sb, sa,
    c_x0, c_x, c_e, c_n); one launch."""
    what = "diffusion_reverse_step"
    _dif_layout(what, x, eps, eps_uncond, noise)
    for other in (eps, eps_uncond, noise):
        if other is not None and other.shape != x.shape:
            raise ValueError(f"{what}: shapes differ: {tuple(x.shape)} and {tuple(other.shape)}")
    out = torch.empty_like(eps)
    sb, sa, c_x0, c_x, c_e, c_n = (float(v) for v in coef)
    check(_lib.lib().adell_diffusion_reverse_step(_ptr(x), _ptr(eps), _ptr(eps_uncond), _ptr(noise),
                                                  _ptr(out), x.numel(), sb, sa, c_x0, c_x, c_e, c_n,
                                                  float(scale), int(flags), _stream()))
    return out


def mse_fwd(pred, target):
    """mean((pred - target)^2) as a one-element device tensor; one launch (and its counter's memset)."""
    what = "mse_loss"
    _dif_layout(what, pred, target)
    if pred.shape != target.shape or pred.numel() == 0:
        raise ValueError(f"{what}: prediction {tuple(pred.shape)} and target {tuple(target.shape)}")
    ws = torch.empty(_lib.lib().adell_mse_workspace_bytes() // 8, device=pred.device, dtype=torch.float64)
    loss = torch.empty(1, device=pred.device, dtype=torch.float32)
    check(_lib.lib().adell_mse_fwd(_ptr(pred), _ptr(target), pred.numel(), _ptr(ws), _ptr(loss),
                                   _stream()))
    return loss


def mse_bwd(pred, target, g):
    """g 2 (pred - target) / n with g a one-element device tensor; one launch."""
    _dif_layout("mse_loss", pred, target)
    _dif_layout("mse_loss", g)
    dpred = torch.empty_like(pred)
    check(_lib.lib().adell_mse_bwd(_ptr(pred), _ptr(target), _ptr(g), pred.numel(), _ptr(dpred),
                                   _stream()))
    return dpred


# ---- ensemble classifiers and the Gaussian-process head (csrc/ensemble.hip) ---------------------------
GP_ROUTES = {0: "fused", 1: "composed"}
ENSEMBLE_MAX = 8        # ADELL_ENSEMBLE_MAX: members of one ensemble_pool / ensemble_average launch


def gp_route(n, i, r):
    """The route of a Gaussian-process layer over ``n`` rows of ``i`` inputs with ``r`` random
    features, by the library's own host function (no device needed): "fused" (gp_phi_fwd / _bwd) or
    "composed" (layer norm, GEMM and gp_cos)."""
    rc = _lib.lib().adell_gp_route(int(n), int(i), int(r))
    check(min(rc, 0))
    return GP_ROUTES[rc]


def _ens_rows(what, *ts):
    """Dense row-major fp32 device tensors, whatever ADELL_CHECK_DENSE says (as ``_mil_dense`` and
    ``_dif_layout`` refuse for their kernels); the addresses themselves are taken by ``_ptr``."""
    for t in ts:
        if t is None:
            continue
        _require_cuda(t)
        if not t.is_contiguous():
            raise _lib.AdellHipError(f"{what}: non-dense tensor handed to a kernel: shape "
                                     f"{tuple(t.shape)}, strides {t.stride()}")


def _gp_args(what, x, gamma, beta, W, b, weights):
    if x.dim() != 2:
        raise NotImplementedError(f"{what}: rows [N, in_channels] expected, got {tuple(x.shape)}: "
                                  "inputs of rank above 2 are not built")
    N, I = (int(v) for v in x.shape)
    R = int(W.shape[-2])
    if W.numel() != R * I or b.numel() != R or N < 1:
        raise ValueError(f"{what}: x [N, {I}], W [1, r, {I}] and b [1, r] expected, got "
                         f"{tuple(x.shape)}, {tuple(W.shape)}, {tuple(b.shape)}")
    if (gamma is None) != (beta is None) or (gamma is not None and (gamma.numel() != I
                                                                    or beta.numel() != I)):
        raise ValueError(f"{what}: the norm's weight and bias [{I}] go together")
    O = 0
    if weights is not None:
        O = int(weights.shape[0])
        if tuple(weights.shape) != (O, R):
            raise ValueError(f"{what}: weights [o, {R}] expected, got {tuple(weights.shape)}")
    _ens_rows(what, x, gamma, beta, W, b, weights)
    return N, I, R, O


def gp_phi_fwd(x, gamma, beta, W, b, weights, scale, eps=1e-5):
    """(phi [N, r], logits [N, o] or None, mean [N], rstd [N]) in one launch (the fused route)."""
    N, I, R, O = _gp_args("gp_phi_fwd", x, gamma, beta, W, b, weights)
    dev = x.device
    phi = torch.empty((N, R), device=dev, dtype=torch.float32)
    logits = torch.empty((N, O), device=dev, dtype=torch.float32) if O else None
    mean = rstd = None
    if gamma is not None:
        stats = torch.empty((2, N), device=dev, dtype=torch.float32)
        mean, rstd = stats[0], stats[1]
    check(_lib.lib().adell_gp_phi_fwd(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(W), _ptr(b),
                                      _ptr(weights), N, I, R, O, float(scale), float(eps), _ptr(phi),
                                      _ptr(logits), _ptr(mean), _ptr(rstd), _stream()))
    return phi, logits, mean, rstd


def gp_phi_bwd(x, gamma, beta, W, b, weights, phi, mean, rstd, dlogits, dphi, scale, eps=1e-5,
               need_x=True, need_norm=True, need_weights=True):
    """(dx, dgamma, dbeta, dweights) of ``gp_phi_fwd`` from dlogits [N, o] and / or dphi [N, r]; at
    most two launches. A gradient that is not needed (or has no input) is None."""
    what = "gp_phi_bwd"
    N, I, R, O = _gp_args(what, x, gamma, beta, W, b, weights)
    if dlogits is None and dphi is None:
        return None, None, None, None
    dev = x.device
    if dlogits is not None:
        dlogits = dlogits.to(torch.float32).contiguous()
        if tuple(dlogits.shape) != (N, O):
            raise ValueError(f"{what}: a gradient [{N}, {O}] expected, got {tuple(dlogits.shape)}")
    if dphi is not None:
        dphi = dphi.to(torch.float32).contiguous()
        if tuple(dphi.shape) != (N, R):
            raise ValueError(f"{what}: a gradient of phi [{N}, {R}] expected, got {tuple(dphi.shape)}")
    _ens_rows(what, phi, mean, rstd, dlogits, dphi)
    need_norm = need_norm and gamma is not None
    need_weights = need_weights and dlogits is not None
    dx = torch.empty((N, I), device=dev, dtype=torch.float32) if need_x else None
    dxhat = dgamma = dbeta = dweights = None
    if need_norm:
        dxhat = torch.empty((N, I), device=dev, dtype=torch.float32)
        dgb = torch.empty((2, I), device=dev, dtype=torch.float32)
        dgamma, dbeta = dgb[0], dgb[1]
    if need_weights:
        dweights = torch.empty((O, R), device=dev, dtype=torch.float32)
    if dx is None and dgamma is None and dweights is None:
        return None, None, None, None
    check(_lib.lib().adell_gp_phi_bwd(
        _ptr(x), _ptr(gamma), _ptr(beta), _ptr(W), _ptr(b), _ptr(weights), _ptr(phi), _ptr(mean),
        _ptr(rstd), _ptr(dlogits), _ptr(dphi), N, I, R, O, float(scale), float(eps), _ptr(dx),
        _ptr(dxhat), _ptr(dgamma), _ptr(dbeta), _ptr(dweights), _stream()))
    return dx, dgamma, dbeta, dweights


def gp_cos(t, b, scale, dphi=None):
    """The composed route's epilogue over t = x^ W^T [rows, r]: scale cos(b - t), or with ``dphi`` the
    gradient of t, scale sin(b - t) dphi; one launch."""
    what = "gp_cos"
    R = int(t.shape[-1])
    if b.numel() != R or t.numel() == 0 or (dphi is not None and dphi.shape != t.shape):
        raise ValueError(f"{what}: t [rows, r], b [1, r] (and dphi like t) expected, got "
                         f"{tuple(t.shape)}, {tuple(b.shape)}")
    _ens_rows(what, t, b, dphi)
    out = torch.empty_like(t)
    check(_lib.lib().adell_gp_cos(_ptr(t), _ptr(b), _ptr(dphi), t.numel() // R, R, float(scale),
                                  _ptr(out), _stream()))
    return out


def gp_precision_update(inv_cov, phi, probabilities, use_momentum=False, m=0.999):
    """In place on ``inv_cov`` [1, r, r] (or [r, r]): += sum_n c_n phi_n phi_n^T, or the momentum form,
    with c_n = sum over the row of p (1 - p) of ``probabilities`` [N] or [N, C]; one launch, no host
    read. The result is exactly symmetric."""
    what = "gp_precision_update"
    if phi.dim() != 2:
        raise NotImplementedError(f"{what}: phi [N, r] expected, got {tuple(phi.shape)}")
    N, R = (int(v) for v in phi.shape)
    p = probabilities.to(torch.float32)
    if p.dim() == 1:
        p = p[:, None]
    if p.dim() != 2 or p.shape[0] != N or p.shape[1] < 1:
        raise ValueError(f"{what}: probabilities [{N}] or [{N}, C] expected, got "
                         f"{tuple(probabilities.shape)}")
    if inv_cov.numel() != R * R or inv_cov.shape[-1] != R:
        raise ValueError(f"{what}: a precision matrix [1, {R}, {R}] expected, got "
                         f"{tuple(inv_cov.shape)}")
    _ens_rows(what, inv_cov, phi, p)
    check(_lib.lib().adell_gp_precision_update(_ptr(phi), _ptr(p), N, R, int(p.shape[1]),
                                               int(bool(use_momentum)), float(m), _ptr(inv_cov),
                                               _stream()))
    return inv_cov


def gp_variance(phi, cov):
    """var [N] = phi_n^T cov phi_n; one launch."""
    what = "gp_variance"
    if phi.dim() != 2:
        raise NotImplementedError(f"{what}: phi [N, r] expected, got {tuple(phi.shape)}")
    N, R = (int(v) for v in phi.shape)
    if cov.numel() != R * R or cov.shape[-1] != R:
        raise ValueError(f"{what}: a covariance [1, {R}, {R}] expected, got {tuple(cov.shape)}")
    _ens_rows(what, phi, cov)
    var = torch.empty((N,), device=phi.device, dtype=torch.float32)
    check(_lib.lib().adell_gp_variance(_ptr(phi), _ptr(cov), N, R, _ptr(var), _stream()))
    return var


def gp_sample(mean, var, eps):
    """(samples [S, N, o], their mean [N, o], their unbiased std [N, o]) from mean [N, o], var [N] and
    eps [S, N, o]: mean + sqrt(max(var, 0)) eps; one launch."""
    what = "gp_sample"
    if mean.dim() != 2 or eps.dim() != 3 or tuple(eps.shape[1:]) != tuple(mean.shape) \
            or var.numel() != mean.shape[0] or eps.shape[0] < 1:
        raise ValueError(f"{what}: mean [N, o], var [N] and eps [S, N, o] expected, got "
                         f"{tuple(mean.shape)}, {tuple(var.shape)}, {tuple(eps.shape)}")
    _ens_rows(what, mean, var, eps)
    S, N, O = (int(v) for v in eps.shape)
    samples = torch.empty_like(eps)
    stats = torch.empty((2, N, O), device=mean.device, dtype=torch.float32)
    check(_lib.lib().adell_gp_sample(_ptr(mean), _ptr(var), _ptr(eps), S, N, O, _ptr(samples),
                                     _ptr(stats[0]), _ptr(stats[1]), _stream()))
    return samples, stats[0], stats[1]


def _ens_member(what, x):
    """A member's output as the kernel reads it: ([B, V, C] channels-last memory, C, V)."""
    _require_cuda(x)
    if x.dim() == 2:
        if not x.is_contiguous():
            raise _lib.AdellHipError(f"{what}: non-dense tensor handed to a kernel: shape "
                                     f"{tuple(x.shape)}, strides {x.stride()}")
        return x, int(x.shape[1]), 1
    if x.dim() == 4:
        x = x.unsqueeze(2)
    if x.dim() != 5:
        raise ValueError(f"{what}: members [B, C], [B, C, H, W] or [B, C, D, H, W] expected, got "
                         f"{tuple(x.shape)}")
    if not x.is_contiguous(memory_format=torch.channels_last_3d):
        raise _lib.AdellHipError(f"{what}: non-dense tensor handed to a kernel (channels-last "
                                 f"memory expected): shape {tuple(x.shape)}, strides {x.stride()}")
    return x, int(x.shape[1]), int(x.shape[2] * x.shape[3] * x.shape[4])


def _ens_pointers(tensors):
    """Host array of the tensors' device addresses (``_ptr``: the dense-layout check of every other
    kernel argument); None stays a null pointer."""
    ptrs = [_ptr(t) for t in tensors]
    return (ctypes.c_void_p * len(ptrs))(*[None if p is None else p.value for p in ptrs])


def _ens_arrays(tensors, C, V):
    K = len(C)
    return _ens_pointers(tensors), (ctypes.c_int * K)(*C), (ctypes.c_long * K)(*V)


def ensemble_pool_fwd(members):
    """(out [B, sum C_k], arg int32 [B, sum C_k]) of up to ENSEMBLE_MAX members [B, C_k, *spatial]
    (channels-last memory; max over the voxels, lowest index on a tie) or [B, C_k] (copied); one
    launch, no per-member pooled tensor and no cat."""
    what = "ensemble_pool_fwd"
    if not 1 <= len(members) <= ENSEMBLE_MAX:
        raise ValueError(f"{what}: {len(members)} members, 1 to {ENSEMBLE_MAX} go in one launch")
    xs, C, V = zip(*[_ens_member(what, x) for x in members])
    B = int(xs[0].shape[0])
    if any(x.shape[0] != B for x in xs) or B < 1:
        raise ValueError(f"{what}: the members' batch sizes differ: {[tuple(x.shape) for x in xs]}")
    Ct = sum(C)
    out = torch.empty((B, Ct), device=xs[0].device, dtype=torch.float32)
    arg = torch.empty((B, Ct), device=xs[0].device, dtype=torch.int32)
    px, pc, pv = _ens_arrays(xs, C, V)
    check(_lib.lib().adell_ensemble_pool_fwd(px, pc, pv, len(xs), B, _ptr(out), _ptr(arg),
                                             _stream()))
    return out, arg


def ensemble_pool_bwd(g, arg, shapes, needs=None):
    """The members' dense gradients (channels-last memory, the forward's logical shapes) from g
    [B, sum C_k] and the forward's arg-max; one launch. ``needs[k]`` False: None."""
    what = "ensemble_pool_bwd"
    K = len(shapes)
    needs = [True] * K if needs is None else list(needs)
    B = int(shapes[0][0])
    C = [int(s[1]) for s in shapes]
    V = [int(math.prod(s[2:])) for s in shapes]
    g = g.to(torch.float32).contiguous()
    if tuple(g.shape) != (B, sum(C)) or tuple(arg.shape) != tuple(g.shape) \
            or arg.dtype != torch.int32 or not arg.is_cuda or not arg.is_contiguous():
        raise ValueError(f"{what}: g and the int32 arg-max [{B}, {sum(C)}] expected, got "
                         f"{tuple(g.shape)} and {arg.dtype} {tuple(arg.shape)}")
    _ens_rows(what, g)
    dxs = []
    for s, need in zip(shapes, needs):
        if not need:
            dxs.append(None)
        elif len(s) == 2:
            dxs.append(torch.empty(tuple(s), device=g.device, dtype=torch.float32))
        else:
            dxs.append(torch.empty((s[0], *s[2:], s[1]), device=g.device, dtype=torch.float32)
                       .permute(0, len(s) - 1, *range(1, len(s) - 1)))
    pd, pc, pv = _ens_arrays(dxs, C, V)
    check(_lib.lib().adell_ensemble_pool_bwd(_ptr(g), _ptr(arg), pc, pv, K, B,
                                             pd, _stream()))
    return dxs


def _ens_logits(what, logits):
    if not 1 <= len(logits) <= ENSEMBLE_MAX:
        raise ValueError(f"{what}: {len(logits)} members, 1 to {ENSEMBLE_MAX} go in one launch")
    shape = tuple(logits[0].shape)
    if len(shape) != 2 or any(tuple(x.shape) != shape for x in logits) or 0 in shape:
        raise ValueError(f"{what}: members [B, C] of one shape expected, got "
                         f"{[tuple(x.shape) for x in logits]}")
    _ens_rows(what, *logits)
    return int(shape[0]), int(shape[1])


def ensemble_average_fwd(logits):
    """sigmoid (C = 1) or softmax of the mean of up to ENSEMBLE_MAX logit tensors [B, C]; one launch."""
    B, C = _ens_logits("ensemble_average_fwd", logits)
    y = torch.empty((B, C), device=logits[0].device, dtype=torch.float32)
    px = _ens_pointers(logits)
    check(_lib.lib().adell_ensemble_average_fwd(px, len(logits), B, C, _ptr(y), _stream()))
    return y


def ensemble_average_bwd(y, dy, K, needs=None):
    """The K members' gradients (every one the gradient of the mean / K) from y and dy; one launch."""
    what = "ensemble_average_bwd"
    dy = dy.to(torch.float32).contiguous()
    if dy.shape != y.shape or y.dim() != 2:
        raise ValueError(f"{what}: y and dy [B, C] expected, got {tuple(y.shape)}, {tuple(dy.shape)}")
    _ens_rows(what, y, dy)
    needs = [True] * K if needs is None else list(needs)
    dxs = [torch.empty_like(y) if need else None for need in needs]
    pd = _ens_pointers(dxs)
    check(_lib.lib().adell_ensemble_average_bwd(_ptr(y), _ptr(dy), K, int(y.shape[0]),
                                                int(y.shape[1]), pd, _stream()))
    return dxs


# ---- batch-ensemble layers (csrc/batch_ensemble.hip) -----------------------------------------------------
def _be_activation(what, x):
    """(B, V, C) of rows [B, C] (V = 1, dense) or of an activation [B, C, *spatial] whose memory is
    dense channels-last; anything else is refused whatever ADELL_CHECK_DENSE says."""
    if x.dim() == 2:
        _ens_rows(what, x)
        if x.dtype != torch.float32:
            raise _lib.AdellHipError(f"{what}: adell_mri_amd kernels are fp32; got {x.dtype}")
        if x.numel() == 0:
            raise ValueError(f"{what}: empty rows {tuple(x.shape)}")
        return int(x.shape[0]), 1, int(x.shape[1])
    return _dif_channels_last(what, x)


def _be_table(what, table, C):
    if table.dim() != 2 or table.shape[1] != C or table.shape[0] < 1:
        raise ValueError(f"{what}: a table [n, {C}] expected, got {tuple(table.shape)}")
    _dif_layout(what, table)
    return int(table.shape[0])


def _be_idx(what, idx, B):
    if idx is None:
        return
    if (not idx.is_cuda or idx.dtype != torch.int32 or tuple(idx.shape) != (B,)
            or not idx.is_contiguous()):
        raise ValueError(f"{what}: item indices are a dense int32 [{B}] device tensor, got "
                         f"{idx.dtype} {tuple(idx.shape)} on {idx.device}")


def _be_members(what, m0, m1, n):
    if not 0 <= m0 < m1 <= n:
        raise ValueError(f"{what}: members [{m0}, {m1}) of {n}")
    return m1 - m0


def _be_like(x, rows):
    """An uninitialised tensor of ``rows`` items in ``x``'s layout."""
    shape = (rows,) + tuple(x.shape[1:])
    if x.dim() == 2:
        return torch.empty(shape, device=x.device, dtype=torch.float32)
    fmt = torch.channels_last_3d if x.dim() == 5 else torch.channels_last
    return torch.empty(shape, device=x.device, dtype=torch.float32, memory_format=fmt)


def be_expand(x, table, idx=None, m0=0, m1=1, scale=1.0):
    """out[(m - m0) B + b] = x[b] * table[m] * scale for m0 <= m < m1, or with ``idx`` (int32 [B] on
    the device, one copy) x[b] * table[idx[b]]; ``table`` None: the scale alone. One launch."""
    what = "be_expand"
    B, V, C = _be_activation(what, x)
    n = _be_table(what, table, C) if table is not None else 1
    _be_idx(what, idx, B)
    K = 1 if idx is not None else _be_members(what, m0, m1, n)
    out = _be_like(x, K * B)
    check(_lib.lib().adell_be_expand(_ptr(x), _ptr(table), _ptr(idx), int(m0), K, n, float(scale),
                                     _ptr(out), B, V, C, _stream()))
    return out


def be_members_sum(y, table, m0, m1, acc=None, scale=None):
    """out[b] = acc[b] + sum_m table[m] y[(m - m0) B + b] as one fma chain in member order, times
    ``scale`` when one is given. One launch."""
    what = "be_members_sum"
    rows, V, C = _be_activation(what, y)
    n = _be_table(what, table, C)
    K = _be_members(what, m0, m1, n)
    if rows % K:
        raise ValueError(f"{what}: {rows} rows for {K} members")
    B = rows // K
    out = _be_like(y, B)
    if acc is not None:
        if tuple(acc.shape) != tuple(out.shape):
            raise ValueError(f"{what}: the running sum must be {tuple(out.shape)}, got "
                             f"{tuple(acc.shape)}")
        _be_activation(what, acc)
    check(_lib.lib().adell_be_members_sum(_ptr(y), _ptr(table), _ptr(acc), int(m0), K, n,
                                          float(scale if scale is not None else 1.0),
                                          int(scale is not None), _ptr(out), B, V, C, _stream()))
    return out


def be_tgrad(p, q, n, m0=0, m1=0, scale=1.0, table=None, idx=None, need_x=False, need_t=True):
    """(dx, dtable [n, C]). ``m1 > m0``: p holds the members [m0, m1) side by side over the items of q,
    dtable[m] = scale sum_b sum_v p[(m - m0) B + b] q[b]. ``m1 == m0`` (the training scale's
    backward, p = dy, q = x): dx = p table[idx] in the same pass and dtable[m] the sum over the items
    that drew m, in item order. One pass and a fold."""
    what = "be_tgrad"
    B, V, C = _be_activation(what, q)
    K = m1 - m0
    rows, Vp, Cp = _be_activation(what, p)
    if (rows, Vp, Cp) != (max(K, 1) * B, V, C) or p.dim() != q.dim():
        raise ValueError(f"{what}: {tuple(p.shape)} against {tuple(q.shape)} for {max(K, 1)} members")
    if K > 0:
        _be_members(what, m0, m1, n)
    if table is not None and _be_table(what, table, C) != n:
        raise ValueError(f"{what}: a table of {n} rows expected")
    _be_idx(what, idx, B)
    dx = _be_like(q, B) if need_x else None
    dt = part = None
    if need_t:
        dt = torch.empty((n, C), device=q.device, dtype=torch.float32)
        words = _lib.lib().adell_be_tgrad_workspace_doubles(B, V, C, max(K, 1))
        check(min(words, 0))
        part = torch.empty(words, device=q.device, dtype=torch.float64)
    if dx is None and dt is None:
        return None, None
    check(_lib.lib().adell_be_tgrad(_ptr(p), _ptr(q), _ptr(table), _ptr(idx), int(m0), K, n,
                                    float(scale), _ptr(dx), _ptr(dt), _ptr(part), B, V, C, _stream()))
    return dx, dt


# ---- deconfounded classification (csrc/deconfound.hip) ---------------------------------------------------
DECONF_ROUTES = {0: "fused", 1: "composed"}
DECONF_MAX_HEADS = _lib.DECONF_MAX_HEADS   # ADELL_DECONF_MAX_HEADS
DECONF_MAX_CLASSES = 64                    # ADELL_DECONF_MAX_CLASSES
DECONF_MAX_CONT = 64                       # ADELL_DECONF_MAX_CONT
DECONF_MAX_CONF = 1024                     # ADELL_DECONF_MAX_CONF


def _deconf_features(what, features, n_conf):
    """(B, F) of the dense fp32 device rows [B, F] the kernels read in place, 0 < n_conf < F."""
    if features.dim() != 2:
        raise ValueError(f"{what}: features [B, F] expected, got {tuple(features.shape)}")
    B, F = (int(v) for v in features.shape)
    n_conf = int(n_conf)
    if not 0 < n_conf < F:
        raise ValueError(f"{what}: n_conf must lie in (0, {F}), got {n_conf}")
    if B < 1:
        raise ValueError(f"{what}: empty batch {tuple(features.shape)}")
    _ens_rows(what, features)
    return B, F


def deconf_route(n_conf, cat_classes=(), n_cont=0):
    """The route of the confounder heads over ``n_conf`` columns with categorical heads of
    ``cat_classes`` classes and ``n_cont`` regression outputs, by the library's own host function (no
    device needed): "fused" (deconf_heads_fwd / _bwd) or "composed"."""
    K = [int(k) for k in cat_classes]
    arr = (ctypes.c_int * max(1, len(K)))(*K)
    rc = _lib.lib().adell_deconf_route(int(n_conf), len(K), arr, int(n_cont or 0))
    check(min(rc, 0))
    return DECONF_ROUTES[rc]


def deconf_split_fwd(features, n_conf):
    """The dense halves [B, n_conf] and [B, F - n_conf] of the rows; one launch."""
    what = "split_columns"
    B, F = _deconf_features(what, features, n_conf)
    a = torch.empty((B, n_conf), device=features.device, dtype=torch.float32)
    b = torch.empty((B, F - n_conf), device=features.device, dtype=torch.float32)
    check(_lib.lib().adell_deconf_split_fwd(_ptr(features), _ptr(a), _ptr(b), B, F, int(n_conf),
                                            _stream()))
    return a, b


def deconf_split_bwd(da, db, B, F, n_conf, device):
    """The whole [B, F] gradient from the halves' (None: zeros); one launch."""
    what = "split_columns backward"
    for g, w in ((da, n_conf), (db, F - n_conf)):
        if g is not None and tuple(g.shape) != (B, w):
            raise ValueError(f"{what}: a gradient [{B}, {w}] expected, got {tuple(g.shape)}")
    _ens_rows(what, da, db)
    dx = torch.empty((B, F), device=device, dtype=torch.float32)
    check(_lib.lib().adell_deconf_split_bwd(_ptr(da), _ptr(db), _ptr(dx), B, F, int(n_conf),
                                            _stream()))
    return dx


def deconf_corr_fwd(features, n_conf):
    """(loss [1], saved): the mean squared clamped correlation of the pairs (confounded column,
    other column); ``saved`` holds the per-column means and centred norms and the ratio of every
    pair before the clamp, in fp64. One launch (and its counter's memset)."""
    what = "deconf_correlation_loss"
    B, F = _deconf_features(what, features, n_conf)
    h = _lib.lib()
    words = h.adell_deconf_corr_workspace_doubles(B, F, int(n_conf))
    keep = h.adell_deconf_corr_saved_doubles(B, F, int(n_conf))
    check(min(words, keep, 0))
    ws = torch.empty(words, device=features.device, dtype=torch.float64)
    saved = torch.empty(keep, device=features.device, dtype=torch.float64)
    loss = torch.empty(1, device=features.device, dtype=torch.float32)
    check(h.adell_deconf_corr_fwd(_ptr(features), B, F, int(n_conf), _ptr(ws), _ptr(saved), _ptr(loss),
                                  _stream()))
    return loss, saved


def deconf_corr_bwd(features, n_conf, saved, g):
    """g times the gradient of the loss, the whole [B, F]; one launch."""
    what = "deconf_correlation_loss backward"
    B, F = _deconf_features(what, features, n_conf)
    _ens_rows(what, g)
    if g.numel() != 1 or saved.dtype != torch.float64 or not saved.is_cuda \
            or saved.numel() != 2 * F + n_conf * (F - n_conf):
        raise ValueError(f"{what}: a one-element gradient and the forward's statistics expected")
    dx = torch.empty_like(features)
    check(_lib.lib().adell_deconf_corr_bwd(_ptr(features), _ptr(saved), _ptr(g), B, F, int(n_conf),
                                           _ptr(dx), _stream()))
    return dx


def _deconf_heads(what, features, n_conf, cat_heads, cat_targets, cont_head, cont_target):
    """(B, F, O, adell_deconf_heads) after the argument checks of the fused heads."""
    B, F = _deconf_features(what, features, n_conf)
    cat_heads = list(cat_heads or [])
    if not cat_heads and cont_head is None:
        raise ValueError(f"{what}: no head")
    if len(cat_heads) > DECONF_MAX_HEADS:
        raise NotImplementedError(f"{what}: {len(cat_heads)} heads, the fused route takes "
                                  f"{DECONF_MAX_HEADS}")
    hd = _lib.DeconfHeads()
    hd.n_heads, hd.n_cont = len(cat_heads), 0
    O = 0
    for h, (W, b) in enumerate(cat_heads):
        if W.dim() != 2 or W.shape[1] != n_conf or b is None or tuple(b.shape) != (W.shape[0],):
            raise ValueError(f"{what}: head {h}: W [K, {n_conf}] and b [K] expected, got "
                             f"{tuple(W.shape)} and {None if b is None else tuple(b.shape)}")
        _ens_rows(what, W, b)
        hd.K[h], hd.W[h], hd.b[h] = int(W.shape[0]), W.data_ptr(), b.data_ptr()
        O += int(W.shape[0])
    if cat_heads:
        if (cat_targets is None or not cat_targets.is_cuda or cat_targets.dtype != torch.int64
                or tuple(cat_targets.shape) != (len(cat_heads), B) or not cat_targets.is_contiguous()):
            raise ValueError(f"{what}: the labels are one dense int64 [{len(cat_heads)}, {B}] device "
                             f"table, got {None if cat_targets is None else (cat_targets.dtype, tuple(cat_targets.shape), cat_targets.device)}")
    if cont_head is not None:
        W, b = cont_head
        if W.dim() != 2 or W.shape[1] != n_conf or b is None or tuple(b.shape) != (W.shape[0],):
            raise ValueError(f"{what}: regression head: W [n_cont, {n_conf}] and b [n_cont] expected")
        if cont_target is None or tuple(cont_target.shape) != (B, W.shape[0]):
            raise ValueError(f"{what}: a regression target [{B}, {W.shape[0]}] expected, got "
                             f"{None if cont_target is None else tuple(cont_target.shape)}")
        _ens_rows(what, W, b, cont_target)
        hd.n_cont, hd.Wc, hd.bc = int(W.shape[0]), W.data_ptr(), b.data_ptr()
        O += int(W.shape[0])
    if deconf_route(n_conf, [int(W.shape[0]) for W, _ in cat_heads], hd.n_cont) != "fused":
        raise NotImplementedError(
            f"{what}: beyond the fused route (n_conf <= {DECONF_MAX_CONF}, heads of <= "
            f"{DECONF_MAX_CLASSES} classes, <= {DECONF_MAX_CONT} regression outputs)")
    return B, F, O, hd


def deconf_heads_fwd(features, n_conf, cat_heads, cat_targets, cont_head, cont_target, conf_mult=1.0):
    """out [2] = (cat_loss, cont_loss) of the linear heads on features[:, :n_conf] read in place; one
    launch (and its counter's memset)."""
    what = "deconf_heads_loss"
    B, F, _, hd = _deconf_heads(what, features, n_conf, cat_heads, cat_targets, cont_head, cont_target)
    h = _lib.lib()
    ws = torch.empty(h.adell_deconf_heads_workspace_doubles(B), device=features.device,
                     dtype=torch.float64)
    out = torch.empty(2, device=features.device, dtype=torch.float32)
    check(h.adell_deconf_heads_fwd(ctypes.byref(hd), _ptr(features), _ptr(cat_targets),
                                   _ptr(cont_target if cont_head is not None else None), B, F,
                                   int(n_conf), float(conf_mult), _ptr(ws), _ptr(out), _stream()))
    return out


def deconf_heads_bwd(features, n_conf, cat_heads, cat_targets, cont_head, cont_target, conf_mult,
                     g_cat, g_cont, need_x=True, need_w=True):
    """(dx [B, F] or None, [(dW, db) per categorical head], (dWc, dbc) or None); two launches, one
    without the heads' gradients. ``g_cat`` / ``g_cont``: one-element device gradients or None."""
    what = "deconf_heads_loss backward"
    B, F, O, hd = _deconf_heads(what, features, n_conf, cat_heads, cat_targets, cont_head, cont_target)
    _ens_rows(what, g_cat, g_cont)
    dev = features.device
    dz = torch.empty((B, O), device=dev, dtype=torch.float64)
    dx = torch.empty_like(features) if need_x else None
    gr, cat_grads, cont_grads = None, [], None
    if need_w:
        gr = _lib.DeconfHeadGrads()
        for h, (W, b) in enumerate(cat_heads or []):
            dW, db = torch.empty_like(W), torch.empty_like(b)
            gr.dW[h], gr.db[h] = dW.data_ptr(), db.data_ptr()
            cat_grads.append((dW, db))
        if cont_head is not None:
            cont_grads = (torch.empty_like(cont_head[0]), torch.empty_like(cont_head[1]))
            gr.dWc, gr.dbc = cont_grads[0].data_ptr(), cont_grads[1].data_ptr()
    check(_lib.lib().adell_deconf_heads_bwd(
        ctypes.byref(hd), ctypes.byref(gr) if gr is not None else None, _ptr(features),
        _ptr(cat_targets), _ptr(cont_target if cont_head is not None else None), _ptr(g_cat),
        _ptr(g_cont), B, F, int(n_conf), float(conf_mult), _ptr(dz), _ptr(dx), _stream()))
    return dx, cat_grads, cont_grads


# ---- evaluation with uncertainty (csrc/bootstrap.hip) ---------------------------------------------------
BOOT_ROUTES = {0: "bitmask", 1: "loop"}
BOOT_MAX_N = 196608          # ADELL_BOOT_MAX_N: 3 n / 8 bytes of LDS = 72 KiB, two blocks per CU of 160 KiB
APS_MAX_CLASSES = 64         # ADELL_APS_MAX_CLASSES


def boot_auroc_route(n):
    """The route of the bootstrap AUC over ``n`` stored samples, by the library's own host function (no
    device needed): "bitmask" (``boot_auroc_pairs``, n <= BOOT_MAX_N) or "loop" (one
    ``cls_auroc_pairs`` per resample)."""
    rc = _lib.lib().adell_boot_auroc_route(int(n))
    check(min(rc, 0))
    return BOOT_ROUTES[rc]


def boot_auroc_tables(scores, labels):
    """(pos, gstart, gend, lab), int32 [n] each, of fp32 scores [n] and 0 / 1 / -1 labels [n]: the
    once-per-class preparation of ``boot_auroc_pairs`` in torch, without a host synchronisation.
    A stable ascending sort; ``pos[i]`` the sorted position of sample i; ``[gstart[p], gend[p])`` the
    run of equal scores around sorted position p (a NaN score gets the empty run [0, 0): it counts 0
    against every negative, as in ``cls_auroc_pairs``); ``lab`` the labels in sorted order."""
    n = int(scores.shape[0])
    dev = scores.device
    vals, perm = torch.sort(scores, stable=True)
    ar = torch.arange(n, device=dev, dtype=torch.int64)
    pos = torch.empty(n, device=dev, dtype=torch.int64)
    pos[perm] = ar
    change = vals[1:] != vals[:-1]
    one = torch.ones(1, device=dev, dtype=torch.bool)
    first = torch.cat([one, change])          # p starts a run
    last = torch.cat([change, one])           # p ends a run
    gstart = torch.cummax(torch.where(first, ar, torch.zeros_like(ar)), 0).values
    gend = torch.cummin(torch.where(last, ar + 1, torch.full_like(ar, n)).flip(0), 0).values.flip(0)
    nan = torch.isnan(vals)
    gstart = torch.where(nan, torch.zeros_like(ar), gstart)
    gend = torch.where(nan, torch.zeros_like(ar), gend)
    i32 = torch.int32
    return (pos.to(i32), gstart.to(i32), gend.to(i32), labels[perm].to(i32).contiguous())


def boot_auroc_pairs(sample_idxs, pos, gstart, gend, lab):
    """int64 [R, 4] on the device: per row of ``sample_idxs`` (int32 [R, m], distinct values in
    [0, n)) the exact (2 #{pos > neg} + #{pos == neg}, positives, negatives, bad indices) over the
    selected samples, from ONE launch (a block per row) and the tables of ``boot_auroc_tables``.
    n <= BOOT_MAX_N (``boot_auroc_route``). Raises ``ValueError`` when a row holds an index twice or
    one outside [0, n) (one host read of the counts)."""
    what = "boot_auroc_pairs"
    ts = (sample_idxs, pos, gstart, gend, lab)
    _cls_on_device(*ts)
    if any(t.dtype != torch.int32 for t in ts):
        raise ValueError(f"{what}: int32 tensors expected, got {[str(t.dtype) for t in ts]}")
    n = int(pos.shape[0])
    if sample_idxs.dim() != 2 or any(tuple(t.shape) != (n,) for t in ts[1:]):
        raise ValueError(f"{what}: indices [R, m] and four tables [n] expected, got "
                         f"{[tuple(t.shape) for t in ts]}")
    if n < 1 or boot_auroc_route(n) != "bitmask":
        raise ValueError(f"{what}: n = {n} is outside [1, {BOOT_MAX_N}]")
    R, m = (int(v) for v in sample_idxs.shape)
    out = torch.zeros((R, 4), device=pos.device, dtype=torch.int64)
    if R == 0 or m == 0:
        return out
    check(_lib.lib().adell_boot_auroc_pairs(
        _ptr(sample_idxs.contiguous()), R, m, _ptr(pos.contiguous()), _ptr(gstart.contiguous()),
        _ptr(gend.contiguous()), _ptr(lab.contiguous()), n, _ptr(out), _stream()))
    bad = out[:, 3] != 0
    if bool(bad.any()):
        rows = torch.nonzero(bad).reshape(-1)[:8].tolist()
        raise ValueError(f"{what}: a resample holds an index twice or one outside [0, {n}): rows {rows}")
    return out


def aps_route(n_classes):
    """ "kernel" (``aps_cumulative``, at most APS_MAX_CLASSES classes) or "composite" (torch)."""
    return "kernel" if 1 <= int(n_classes) <= APS_MAX_CLASSES else "composite"


def aps_cumulative(pred, labels=None):
    """(cum [N, C], scores [N] or None) of fp32 probabilities [N, C], C <= APS_MAX_CLASSES, one
    launch: ``cum[i, c]`` is the cumulative probability of row i at the rank of class c in the
    stable descending order (of equal probabilities the lower index first), each prefix an fp64 sum
    in rank order rounded to fp32; ``scores[i] = cum[i, labels[i]]`` (int64 labels; NaN outside
    [0, C))."""
    what = "aps_cumulative"
    _cls_on_device(pred, labels)
    if pred.dtype != torch.float32 or pred.dim() != 2:
        raise ValueError(f"{what}: fp32 probabilities [N, C] expected, got {pred.dtype} "
                         f"{tuple(pred.shape)}")
    N, C = (int(v) for v in pred.shape)
    if aps_route(C) != "kernel":
        raise ValueError(f"{what}: {C} classes, the kernel takes 1 to {APS_MAX_CLASSES}")
    if labels is not None and (labels.dtype != torch.int64 or tuple(labels.shape) != (N,)):
        raise ValueError(f"{what}: int64 labels [{N}] expected, got {labels.dtype} "
                         f"{tuple(labels.shape)}")
    cum = torch.empty((N, C), device=pred.device, dtype=torch.float32)
    scores = None if labels is None else torch.empty((N,), device=pred.device, dtype=torch.float32)
    if N:
        check(_lib.lib().adell_aps_cumulative(
            _ptr(pred.contiguous()), _ptr(None if labels is None else labels.contiguous()), N, C,
            _ptr(cum), _ptr(scores), _stream()))
    return cum, scores


# ---- semi-supervised U-Net losses beyond the local contrastive one (csrc/semisl.hip) ---------------------
SEMISL_KINDS = {"anchor": 0, "nn": 1, "pseudo_label": 2}   # ADELL_SEMISL_ANCHOR / _NN / _PSEUDO_LABEL
SEMISL_ROUTES = {0: "fused", 1: "composed"}
SEMISL_ANCHOR_MAX_C = 1024    # ADELL_SEMISL_ANCHOR_MAX_C
SEMISL_NN_MAX_C = 64          # ADELL_SEMISL_NN_MAX_C
SEMISL_MAX_CLASSES = 64       # ADELL_SEMISL_MAX_CLASSES
SEMISL_PUT_CHUNK = 4096       # ADELL_SEMISL_PUT_CHUNK


def semisl_route(kind, C=1, K=1):
    """The route of one of the semi-supervised losses by the library's own host function (no device
    needed): "fused" or "composed". ``kind``: "anchor" (C channels), "nn" (C channels, K classes),
    "pseudo_label" (K classes)."""
    if kind not in SEMISL_KINDS:
        raise ValueError(f"semisl_route: kind {kind!r}, expected one of {sorted(SEMISL_KINDS)}")
    rc = _lib.lib().adell_semisl_route(SEMISL_KINDS[kind], int(C), int(K))
    check(min(rc, 0))
    return SEMISL_ROUTES[rc]


def _semisl_rows(what, *ts):
    """(B, V, C) of dense fp32 device rows [B, V, C] of one shape."""
    _ens_rows(what, *ts)
    shape = tuple(ts[0].shape)
    if len(shape) != 3 or any(tuple(t.shape) != shape for t in ts) or 0 in shape:
        raise ValueError(f"{what}: non-empty rows [B, V, C] of one shape expected, got "
                         f"{[tuple(t.shape) for t in ts]}")
    return shape


def loco_anchor_fwd(x, a1, a2, temperature):
    """(loss [B], sim1 [B, V], sim2 [B, V], stats [B, 6] fp64) of feature rows [B, V, C]; four launches."""
    what = "loco_anchor_loss"
    B, V, C = _semisl_rows(what, x, a1, a2)
    h = _lib.lib()
    words = h.adell_loco_anchor_workspace_doubles(B, V, C)
    check(min(words, 0))
    dev = x.device
    ws = torch.empty(words, device=dev, dtype=torch.float64)
    sim1 = torch.empty((B, V), device=dev, dtype=torch.float32)
    sim2 = torch.empty((B, V), device=dev, dtype=torch.float32)
    stats = torch.empty((B, 6), device=dev, dtype=torch.float64)
    loss = torch.empty(B, device=dev, dtype=torch.float32)
    check(h.adell_loco_anchor_fwd(_ptr(x), _ptr(a1), _ptr(a2), B, V, C, float(temperature), _ptr(sim1),
                                  _ptr(sim2), _ptr(stats), _ptr(loss), _ptr(ws), words, _stream()))
    return loss, sim1, sim2, stats


def loco_anchor_bwd(x, a1, a2, sim1, sim2, stats, gloss, temperature, need1, need2):
    """(dx, da1 or None, da2 or None) as rows [B, V, C]; one launch."""
    what = "loco_anchor_loss backward"
    B, V, C = _semisl_rows(what, x, a1, a2)
    gloss = gloss.contiguous().float()
    _ens_rows(what, sim1, sim2, gloss)
    if tuple(sim1.shape) != (B, V) or tuple(sim2.shape) != (B, V) or gloss.numel() != B \
            or stats.dtype != torch.float64 or tuple(stats.shape) != (B, 6) or not stats.is_cuda:
        raise ValueError(f"{what}: the forward's rows and statistics and a gradient [{B}] expected")
    dx = torch.empty_like(x)
    da1 = torch.empty_like(x) if need1 else None
    da2 = torch.empty_like(x) if need2 else None
    check(_lib.lib().adell_loco_anchor_bwd(_ptr(x), _ptr(a1), _ptr(a2), _ptr(sim1), _ptr(sim2),
                                           _ptr(stats), _ptr(gloss), B, V, C, float(temperature),
                                           _ptr(dx), _ptr(da1), _ptr(da2), _stream()))
    return dx, da1, da2


def _nn_queue_args(what, x, y, pastn, past_class):
    B, V, C = _semisl_rows(what, x)
    _ens_rows(what, y, pastn)
    if y.dim() != 3 or y.shape[0] != B or y.shape[2] != V:
        raise ValueError(f"{what}: labels [{B}, K, {V}] expected, got {tuple(y.shape)}")
    if pastn.dim() != 2 or pastn.shape[1] != C or pastn.shape[0] < 1:
        raise ValueError(f"{what}: past samples [Q, {C}] expected, got {tuple(pastn.shape)}")
    Q = int(pastn.shape[0])
    if not past_class.is_cuda or past_class.dtype != torch.int32 or tuple(past_class.shape) != (Q,) \
            or not past_class.is_contiguous():
        raise ValueError(f"{what}: int32 device classes [{Q}] expected")
    return B, V, C, int(y.shape[1]), Q


def nn_queue_normalize(past):
    """The rows of ``past`` [Q, C] divided by max(their norm, 1e-8); one launch."""
    what = "nn_queue_normalize"
    _ens_rows(what, past)
    if past.dim() != 2 or 0 in past.shape:
        raise ValueError(f"{what}: non-empty rows [Q, C] expected, got {tuple(past.shape)}")
    out = torch.empty_like(past)
    check(_lib.lib().adell_nn_queue_normalize(_ptr(past), int(past.shape[0]), int(past.shape[1]),
                                              _ptr(out), _stream()))
    return out


def nn_queue_loss_fwd(x, y, pastn, past_class, temperature):
    """(loss [1], S [B V], O [B V], stats [2] fp64) of rows x [B, V, C], labels y [B, K, V], the
    normalised past rows [Q, C] and their int32 classes [Q]; two launches."""
    what = "nn_queue_loss"
    B, V, C, K, Q = _nn_queue_args(what, x, y, pastn, past_class)
    h = _lib.lib()
    words = h.adell_nn_queue_workspace_doubles(B, V)
    check(min(words, 0))
    dev = x.device
    ws = torch.empty(words, device=dev, dtype=torch.float64)
    S = torch.empty(B * V, device=dev, dtype=torch.float32)
    O = torch.empty(B * V, device=dev, dtype=torch.float32)
    stats = torch.empty(2, device=dev, dtype=torch.float64)
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    check(h.adell_nn_queue_loss_fwd(_ptr(x), _ptr(y), _ptr(pastn), _ptr(past_class), B, V, C, K, Q,
                                    float(temperature), _ptr(S), _ptr(O), _ptr(stats), _ptr(loss),
                                    _ptr(ws), words, _stream()))
    return loss, S, O, stats


def nn_queue_loss_bwd(x, y, pastn, past_class, S, O, stats, g, temperature):
    """dx [B, V, C]; one launch."""
    what = "nn_queue_loss backward"
    B, V, C, K, Q = _nn_queue_args(what, x, y, pastn, past_class)
    g = g.reshape(1).contiguous().float()
    _ens_rows(what, S, O, g)
    if S.numel() != B * V or O.numel() != B * V or stats.dtype != torch.float64 or stats.numel() != 2 \
            or not stats.is_cuda:
        raise ValueError(f"{what}: the forward's sums and statistics expected")
    dx = torch.empty_like(x)
    check(_lib.lib().adell_nn_queue_loss_bwd(_ptr(x), _ptr(y), _ptr(pastn), _ptr(past_class), _ptr(S),
                                             _ptr(O), _ptr(stats), _ptr(g), B, V, C, K, Q,
                                             float(temperature), _ptr(dx), _stream()))
    return dx


def nn_queue_count(y):
    """int32 [B, K, chunks]: the positives (y > 0) of labels [B, K, V] per chunk of SEMISL_PUT_CHUNK
    voxels; one launch."""
    what = "nn_queue_count"
    _ens_rows(what, y)
    if y.dim() != 3 or 0 in y.shape:
        raise ValueError(f"{what}: non-empty labels [B, K, V] expected, got {tuple(y.shape)}")
    B, K, V = (int(v) for v in y.shape)
    chunks = (V + SEMISL_PUT_CHUNK - 1) // SEMISL_PUT_CHUNK
    cc = torch.empty((B, K, chunks), device=y.device, dtype=torch.int32)
    check(_lib.lib().adell_nn_queue_count(_ptr(y), B, K, V, _ptr(cc), _stream()))
    return cc


def nn_queue_put(x, y, select):
    """The gather behind ``NearestNeighbourLoss.put``. ``x`` [B, C, *spatial] (dense, channel-major or
    channels-last) and ``y`` [B, K, *spatial]; ``select(counts)`` receives the int64 numpy table [B, K]
    of positives (y > 0) -- the one host read -- and returns, per class, None or the int64 ranks to
    keep among the positives of that class in the order of ``torch.where(y > 0)`` (item-major, then
    voxel). Returns a list with, per class, None or the gathered rows [n, C]: bit-equal to
    ``x.flatten(2)[b[idx], :, v[idx]][ranks]``. Neither the index triples nor the rows of all
    positives are materialised: a count launch, a scan of the small table, one gather launch."""
    what = "nn_queue_put"
    _require_cuda(x, y)
    if x.dim() < 3 or y.dim() != x.dim() or x.shape[0] != y.shape[0] \
            or tuple(x.shape[2:]) != tuple(y.shape[2:]) or 0 in x.shape or 0 in y.shape:
        raise ValueError(f"{what}: x [B, C, *spatial] and y [B, K, *spatial] expected, got "
                         f"{tuple(x.shape)} and {tuple(y.shape)}")
    B, C, K = int(x.shape[0]), int(x.shape[1]), int(y.shape[1])
    V = x.numel() // (B * C)
    x = x.detach()
    rows = x.dim() == 5 and x.is_contiguous(memory_format=torch.channels_last_3d) \
        and not x.is_contiguous()
    if rows:
        strides = (V * C, 1, C)
    else:
        x = x.contiguous()
        strides = (C * V, V, 1)
    y3 = y.detach().reshape(B, K, V).contiguous()
    cc = nn_queue_count(y3)
    counts = cc.sum(-1, dtype=torch.int64).cpu().numpy()
    ranks = select(counts)
    picked = [(cl, np.asarray(r, dtype=np.int64).reshape(-1)) for cl, r in enumerate(ranks)
              if r is not None and len(r) > 0]
    out = [None] * K
    if not picked:
        return out
    for cl, r in picked:
        if r.min() < 0 or r.max() >= counts[:, cl].sum():
            raise ValueError(f"{what}: a rank outside the {int(counts[:, cl].sum())} positives of "
                             f"class {cl}")
    incl = cc.permute(1, 0, 2).reshape(K, -1).cumsum(-1, dtype=torch.int64).contiguous()
    sel = np.concatenate([r for _, r in picked])
    cls = np.concatenate([np.full(len(r), cl, dtype=np.int32) for cl, r in picked])
    n = int(sel.shape[0])
    sel_d = torch.from_numpy(sel).to(x.device)
    cls_d = torch.from_numpy(cls).to(x.device)
    rows_out = torch.empty((n, C), device=x.device, dtype=torch.float32)
    xp = ctypes.c_void_p(x.data_ptr())   # dense in one of the two layouts checked above
    check(_lib.lib().adell_nn_queue_gather(xp, _ptr(y3), _ptr(incl), _ptr(cls_d), _ptr(sel_d), n, B, K,
                                           V, C, *strides, _ptr(rows_out), _stream()))
    at = 0
    for cl, r in picked:
        out[cl] = rows_out[at:at + len(r)]
        at += len(r)
    return out


def _pl_ce_args(what, pred, proba, weight):
    _ens_rows(what, pred, proba, weight)
    if pred.dim() != 3 or tuple(proba.shape) != tuple(pred.shape) or 0 in pred.shape:
        raise ValueError(f"{what}: logits and probabilities [B, K, V] of one shape expected, got "
                         f"{tuple(pred.shape)} and {tuple(proba.shape)}")
    B, K, V = (int(v) for v in pred.shape)
    if weight is not None and tuple(weight.shape) != (K,):
        raise ValueError(f"{what}: a weight [{K}] expected, got {tuple(weight.shape)}")
    return B, K, V


def pseudo_label_ce_fwd(pred, proba, threshold, weight, label_smoothing, mean):
    """loss [1] of logits and probabilities [B, K, V]; one launch (and the clearing of its ticket)."""
    what = "pseudo_label_ce"
    B, K, V = _pl_ce_args(what, pred, proba, weight)
    h = _lib.lib()
    words = h.adell_pseudo_label_ce_workspace_doubles(B, V)
    check(min(words, 0))
    ws = torch.empty(words, device=pred.device, dtype=torch.float64)
    ws[:1].zero_()
    loss = torch.empty(1, device=pred.device, dtype=torch.float32)
    check(h.adell_pseudo_label_ce_fwd(_ptr(pred), _ptr(proba), _ptr(weight), B, K, V, float(threshold),
                                      float(label_smoothing), int(bool(mean)), _ptr(loss), _ptr(ws),
                                      words, _stream()))
    return loss


def pseudo_label_ce_bwd(pred, proba, threshold, weight, label_smoothing, mean, g):
    """d pred [B, K, V]; one launch."""
    what = "pseudo_label_ce backward"
    B, K, V = _pl_ce_args(what, pred, proba, weight)
    g = g.reshape(1).contiguous().float()
    _ens_rows(what, g)
    dpred = torch.empty_like(pred)
    check(_lib.lib().adell_pseudo_label_ce_bwd(_ptr(pred), _ptr(proba), _ptr(weight), _ptr(g), B, K, V,
                                               float(threshold), float(label_smoothing),
                                               int(bool(mean)), _ptr(dpred), _stream()))
    return dpred


# ---- spectral normalisation of a weight (csrc/spectral_norm.hip) -------------------------------------------
SN_ROUTES = {0: "block", 1: "grid", 2: "composed"}   # ADELL_SN_BLOCK / _GRID / _COMPOSED
SN_MAX_DIM = 32768                                    # ADELL_SN_MAX_DIM


def spectral_norm_route(h, w):
    """The route of the spectral normalisation of an ``h x w`` matrix by the library's own host
    function (no device needed): "block", "grid" or "composed"."""
    rc = _lib.lib().adell_spectral_norm_route(int(h), int(w))
    check(min(rc, 0))
    return SN_ROUTES[rc]


def spectral_norm_matrix(shape, dim):
    """(outer, h, inner) of a weight of this shape read as the matrix ``[h, outer * inner]`` with
    ``dim`` in front (torch's ``_reshape_weight_to_matrix`` without the permuted copy)."""
    shape = tuple(int(s) for s in shape)
    if len(shape) < 2 or not 0 <= dim < len(shape) or 0 in shape:
        raise ValueError(f"spectral_normalize: a non-empty weight of rank >= 2 and 0 <= dim < rank "
                         f"expected, got shape {shape}, dim {dim}")
    outer = inner = 1
    for s in shape[:dim]:
        outer *= s
    for s in shape[dim + 1:]:
        inner *= s
    return outer, shape[dim], inner


def _sn_workspace(h, w, device):
    words = _lib.lib().adell_spectral_norm_workspace_doubles(h, w)
    check(min(words, 0))
    return torch.empty(words, device=device, dtype=torch.float64), words


def spectral_norm_fwd(weight, u, v, n_iter, eps, dim):
    """(W_sn, sigma [1] fp64, u_used, v_used). ``n_iter`` power iterations update ``u`` [h] and ``v``
    [w] IN PLACE (0: eval mode, both only read); ``u_used`` / ``v_used`` are the copies sigma was
    taken with. Block route: one launch; grid route: 2 n_iter + 1 (2 in eval mode)."""
    what = "spectral_normalize"
    outer, h, inner = spectral_norm_matrix(weight.shape, dim)
    w = outer * inner
    _ens_rows(what, weight, u, v)
    if weight.dtype != torch.float32 or u.dtype != torch.float32 or v.dtype != torch.float32 \
            or u.numel() != h or v.numel() != w:
        raise ValueError(f"{what}: fp32 weight, u [{h}] and v [{w}] expected, got "
                         f"{tuple(u.shape)} {u.dtype} and {tuple(v.shape)} {v.dtype}")
    dev = weight.device
    ws, words = _sn_workspace(h, w, dev)
    out = torch.empty_like(weight)
    u_used, v_used = torch.empty_like(u), torch.empty_like(v)
    sigma = torch.empty(1, device=dev, dtype=torch.float64)
    check(_lib.lib().adell_spectral_norm_fwd(_ptr(weight), _ptr(u), _ptr(v), outer, h, inner,
                                             int(n_iter), float(eps), _ptr(ws), words, _ptr(u_used),
                                             _ptr(v_used), _ptr(sigma), _ptr(out), _stream()))
    return out, sigma, u_used, v_used


def spectral_norm_bwd(g, w_sn, u, v, sigma, dim):
    """dW = (g - <g, W_sn> u v^T) / sigma in the weight's layout; one launch (block) or two (grid)."""
    what = "spectral_normalize backward"
    outer, h, inner = spectral_norm_matrix(w_sn.shape, dim)
    _ens_rows(what, g, w_sn, u, v)
    if tuple(g.shape) != tuple(w_sn.shape) or sigma.dtype != torch.float64 or not sigma.is_cuda \
            or sigma.numel() != 1 or u.numel() != h or v.numel() != outer * inner:
        raise ValueError(f"{what}: an fp32 gradient of the weight's shape and the forward's u, v and "
                         f"sigma expected")
    ws, words = _sn_workspace(h, outer * inner, g.device)
    dw = torch.empty_like(w_sn)
    check(_lib.lib().adell_spectral_norm_bwd(_ptr(g), _ptr(w_sn), _ptr(u), _ptr(v), _ptr(sigma), outer, h,
                                             inner, _ptr(ws), words, _ptr(dw), _stream()))
    return dw
