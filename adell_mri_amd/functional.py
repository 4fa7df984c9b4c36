"""torch.autograd glue over the HIP kernels (``ops.py``).

Each Function is one fused site of the reference's hot path:

* ``conv3d``            Conv3d (+ virtual concat of two sources, + residual add,
                        + per-channel statistics for the norm that follows)
* ``conv_transpose3d_k2s2``  ConvTranspose3d(k=2, s=2)
* ``norm_drop_act``     Norm -> Dropout -> Activation of ActDropNorm ("NDA")

Statistics produced by the conv epilogue ride on the output tensor as
``y._adell_partials`` so that the following ``norm_drop_act`` does not re-read
``y``; they are dropped by any other consumer.
"""
import collections
import ctypes
import itertools
import math
import os
import weakref

import numpy as np
import torch
import torch.distributed as dist

from . import _lib, ops

_dropout_counter = itertools.count(1)

# How the MFMA convolutions multiply fp32 operands:
#   "f16x3": three f16 MFMAs on error-compensated hi/lo splits (fp32-class accuracy,
#            ~2^-22 per product; 5.3x the fp32 MFMA rate)            [default]
#   "fp32":  v_mfma_f32_32x32x2_f32, bit-exact k-ordered fp32 FMA chain
CONV_PRECISION = os.environ.get("ADELL_CONV_PRECISION", "f16x3")
# dispatch switches for A/B tests, read from the environment once at import (tests flip the
# dictionary entries): parity-class stride-2 backward-data at every size / never; no folding
# of the x taps of <= 4-channel inputs into the 16-channel MFMA chunk
FLAGS = {"s2class_always": bool(os.environ.get("ADELL_S2CLASS_ALWAYS")),
         "no_s2class": bool(os.environ.get("ADELL_NO_S2CLASS")),
         "no_fold": bool(os.environ.get("ADELL_NO_FOLD")),
         # norm / dropout / activation backward left to its own two passes (no fused epilogue)
         "no_adn_fuse": bool(os.environ.get("ADELL_NO_ADN_FUSE")),
         # the logits head's backward-data tensor is formed (no factored site backward)
         "no_lowrank": bool(os.environ.get("ADELL_NO_LOWRANK")),
         # weight gradients of the convolutions / linear layers on a second HIP stream (side_run);
         # ADELL_WGRAD_STREAM=0 keeps every launch on the caller's stream
         "wgrad_stream": os.environ.get("ADELL_WGRAD_STREAM", "1") != "0",
         # a conv weight gradient that runs on the side stream tells the library so (the share hint
         # of ops.conv3d_bwd_weight: one z-ring block per CU, the other half of the CU stays with the
         # main stream's kernels); ADELL_NO_WGRAD_SHARE=1: no hint, two blocks per CU (A/B)
         "no_wgrad_share": bool(os.environ.get("ADELL_NO_WGRAD_SHARE")),
         # an ADN output whose only reader is a 3x3x3 stride-1 conv is written as SPLIT ROWS (the
         # conv kernels' LDS row image: ops.SplitRows) instead of fp32; ADELL_NO_ROWS=1: always fp32
         "no_rows": bool(os.environ.get("ADELL_NO_ROWS")),
         # 1x1x1 stride-1 convolutions with >= 64 channels on one side (>= 8 on the other) stay on the implicit-GEMM
         # conv kernels instead of the Linear-layer GEMMs (conv3d)
         "no_pointwise_gemm": bool(os.environ.get("ADELL_NO_POINTWISE_GEMM")),
         # full-sequence attention by slices + copies around the kernels (the pre-round-4 form)
         "no_seq_attention": bool(os.environ.get("ADELL_NO_SEQ_ATTENTION")),
         # Linear -> activation -> Linear as separate layers with an element-wise pass between them.
         # The DEFAULT: with the wide epilogue on every GEMM the fused form (functional.mlp,
         # ADELL_MLP_FUSE=1) measured 20.03 against 19.71 ms on the VICReg ConvNeXt step -- the erf of
         # 100 M hidden elements costs more inside a GEMM epilogue than in two passes that run at the
         # HBM rate -- and 21.6 against 21.3 ms on UNETR.
         "no_mlp_fuse": not bool(os.environ.get("ADELL_MLP_FUSE")),
         # (fused form only from this many hidden elements on)
         "mlp_min_elems": int(os.environ.get("ADELL_MLP_MIN_ELEMS", str(1 << 20))),
         # weight gradient of the narrow-input convs on the exact fp32-MFMA kernel (A/B)
         "no_cinfold_wgrad_f16": bool(os.environ.get("ADELL_NO_CINFOLD_WGRAD_F16"))}


def set_conv_precision(mode):
    global CONV_PRECISION
    if mode not in ("f16x3", "fp32"):
        raise ValueError("conv precision must be 'f16x3' or 'fp32'")
    CONV_PRECISION = mode
    _sync_dw_precision()


def _sync_dw_precision():
    """The depthwise 7^3 kernels choose their arithmetic inside the library (csrc/dw_mfma.hip: the
    f16x3 Toeplitz form on the MFMA): "fp32" keeps them on the exact fp32-FMA kernels too."""
    if os.path.exists(_lib.LIB_PATH) and not os.environ.get("ADELL_DW_NOMFMA"):
        _lib.lib().adell_set_tuning(b"dw_nomfma", 1 if CONV_PRECISION == "fp32" else 0)


if CONV_PRECISION == "fp32":
    _sync_dw_precision()


class _Ref:
    """Opaque holder so a Parameter object can ride through autograd.Function.apply."""

    __slots__ = ("obj",)

    def __init__(self, obj):
        self.obj = obj


# Conv weights packed for the f16x3 kernels (modes 0 / 1) are registered here so that, after an
# optimiser step has rewritten the parameters, ALL of them are repacked by one launch
# (adell_pack_weight_f16x3_multi) instead of one ~6 us launch per weight and mode.
_PACK_REG = {}      # (id(weight), mode) -> [weakref(weight), mode, SplitWeight, tag, fence]
_PACK_BATCH = {"epoch": -1, "sig": None, "table": None, "blocks": 0}


class _PackFence:
    """Where a pack was launched: a consumer on ANOTHER stream waits for the event first (the
    packed copies and the absmax arena used to assume that one stream drives every forward /
    backward-data launch of the process; two micro-batches on two streams read half-written
    packs -- round 3's diverged A/B run)."""

    __slots__ = ("stream", "event")

    def __init__(self):
        self.stream = ops._stream().value
        self.event = torch.cuda.Event()
        self.event.record()

    def order(self):
        if ops._stream().value != self.stream:
            torch.cuda.current_stream().wait_event(self.event)


def _pack_tag(w):
    return (w._version, w.data_ptr(), ops.WEIGHT_EPOCH)


def _repack_registered():
    """Repack every live registered weight in one launch; returns False when nothing is
    registered."""
    live = []
    for key, ent in list(_PACK_REG.items()):
        w = ent[0]()
        if w is None or not w.is_contiguous() or not w.is_cuda:
            del _PACK_REG[key]
            continue
        live.append((w, ent))
    if not live:
        return False
    rows, first = [], 0
    for w, ent in live:
        d0, d1 = w.shape[0], w.shape[1]
        taps = w.shape[2] * w.shape[3] * w.shape[4]
        rows.append((w.data_ptr(), ent[2].halfs.data_ptr(), ent[2].scale.data_ptr(), ent[1], d0,
                     d1, taps, first))
        first += d0 if ent[1] == 0 else d1
    sig = tuple(rows)
    if _PACK_BATCH["sig"] != sig and torch.cuda.is_current_stream_capturing():
        # the set of live weights changed inside a graph capture (another module died since the
        # warm-up step): the table upload is a pageable host copy, which a capture cannot hold --
        # the caller packs weight by weight (captured launches of the single-weight kernel)
        return False
    if _PACK_BATCH["sig"] != sig:
        _PACK_BATCH["table"] = torch.tensor(rows, dtype=torch.int64, device=live[0][0].device)
        _PACK_BATCH["sig"] = sig
        _PACK_BATCH["blocks"] = first
    ops.pack_weight_f16x3_multi(_PACK_BATCH["table"], len(rows), _PACK_BATCH["blocks"])
    fence = _PackFence()
    for w, ent in live:
        ent[3] = _pack_tag(w)
        ent[4] = fence
    _PACK_BATCH["epoch"] = ops.WEIGHT_EPOCH
    return True


def _tensor_pack_cache(w, key, build):
    """``build()`` cached under ``key`` ON the tensor object (so the cache dies with it), valid only for the
    same storage address, version counter and weight epoch; a hit waits for its pack launch (_PackFence)."""
    cache = getattr(w, "_adell_packs", None)
    if cache is None:
        cache = w._adell_packs = {}
    tag = _pack_tag(w)
    hit = cache.get(key)
    if hit is not None and hit[0] == tag:
        if w.is_cuda:
            hit[2].order()
        return hit[1]
    p = build()
    cache[key] = (tag, p, _PackFence() if w.is_cuda else None)
    return p


def _packed(w, mode):
    """Repacked copy of a weight (see _tensor_pack_cache; the f16x3 conv operands of modes 0 / 1
    live in _PACK_REG instead, for the one-launch repack)."""
    split = CONV_PRECISION == "f16x3" and mode in (0, 1, 2, 3)
    # the value of a parametrised weight is a fresh tensor on every access: registered under its id it
    # would leave a dead entry, and the packs it holds, behind per step -- its packs live on the tensor
    # (a view of it, Conv2d's unsqueeze, under no_grad: its base carries the mark)
    transient = w.grad_fn is not None or getattr(w, "_adell_transient", False) \
        or (w._base is not None and getattr(w._base, "_adell_transient", False))
    if split and mode in (0, 1) and w.dim() == 5 and w.is_contiguous() and not transient:
        key = (id(w), mode)
        ent = _PACK_REG.get(key)
        if ent is not None and ent[0]() is not w:
            ent = None
        if ent is not None:
            if ent[3] == _pack_tag(w):
                ent[4].order()
                return ent[2]
            if _PACK_BATCH["epoch"] != ops.WEIGHT_EPOCH and _repack_registered() \
                    and ent[3] == _pack_tag(w):
                ent[4].order()
                return ent[2]
        p = ops.pack_weight_f16x3(w.detach(), mode)
        _PACK_REG[key] = [weakref.ref(w), mode, p, _pack_tag(w), _PackFence()]
        return p

    def build():
        wd = w.detach()
        if wd.dim() == 2:  # torch.nn.Linear weight == 1x1x1 convolution weight
            wd = wd.view(wd.shape[0], wd.shape[1], 1, 1, 1)
        if split and mode == 2:
            # transposed conv forward = 1x1x1 conv with F*Cout outputs: V[(f, co)][ci] = w[ci][co][f]
            v = wd.permute(2, 3, 4, 1, 0).reshape(-1, wd.shape[0], 1, 1, 1)
            return ops.pack_weight_f16x3(v, 0)
        if split and mode == 3:
            # its backward-data = kernel == stride conv with Cin outputs / Cout inputs: w as is
            return ops.pack_weight_f16x3(wd, 0)
        return ops.pack_weight_f16x3(wd, mode) if split else ops.pack_weight(wd, mode)
    return _tensor_pack_cache(w, (mode, split), build)


def _packed_s2_classes(w, padding):
    """The 8 parity-class sub-kernels of a stride-2 k = 3 conv weight, packed for the
    backward-data kernel (mode 1); cached on the tensor."""
    def build():
        wd = w.detach()
        packs = []
        for c in range(8):
            par = (c >> 2, (c >> 1) & 1, c & 1)
            t0 = [(par[a] + padding[a]) & 1 for a in range(3)]
            sub = wd[:, :, t0[0]::2, t0[1]::2, t0[2]::2].contiguous()
            packs.append(ops.pack_weight_f16x3(sub, 1))
        return packs
    return _tensor_pack_cache(w, ("s2", tuple(padding)), build)


def _packed_folded(w):
    """f16x3 pack of W'[co][kx * Cin + ci][kz][ky][0] = w[co][ci][kz][ky][kx], zero-padded to 16
    input channels (the weight of the folded conv, see ops.fold_x_taps); cached on the tensor."""
    def build():
        wd = w.detach()
        co, ci, kd, kh, kw = wd.shape
        wf = wd.permute(0, 4, 1, 2, 3).reshape(co, kw * ci, kd, kh, 1)
        if kw * ci < 16:
            wf = torch.cat([wf, wf.new_zeros(co, 16 - kw * ci, kd, kh, 1)], 1)
        return ops.pack_weight_f16x3(wf.contiguous(), 0)
    return _tensor_pack_cache(w, "fold", build)


# absmax by-product slots ([0]: input(s) of a conv, [1]: its dy), zeroed in bulk: every slot is
# handed out once and never reused, so a slot stays valid as long as the graph that holds it --
# one fill per 256 conv calls instead of one per call
# (one arena per launching stream: the bulk fill is ordered before the kernels that use its slots
# only on the stream it was issued on)
_AMAX_ARENAS = {}


def _amax_pair(device):
    key = (device, ops._stream().value)
    a = _AMAX_ARENAS.get(key)
    if a is None:
        a = _AMAX_ARENAS[key] = {"buf": None, "next": 0}
    if a["buf"] is None or a["next"] + 2 > a["buf"].numel():
        a["buf"] = torch.zeros(512, device=device, dtype=torch.int32)
        a["next"] = 0
    pair = a["buf"][a["next"]:a["next"] + 2]
    a["next"] += 2
    return pair


# ---- the weight-gradient branch on a second HIP stream --------------------------------------------
# dW of a conv depends on (x, dY) only and nothing in the backward pass waits for it: on its own
# stream the MFMA-bound weight-gradient kernels (and their small partial-slab folds) run beside the
# HBM-bound norm / dropout / activation passes and the launch tails of the backward-data chain.
# Ordering: the side stream waits for everything queued on the main stream so far (dY, the absmax
# slots); the main stream waits for the side stream when the backward pass ends (engine callback)
# and wherever a gradient is read before that (join_side_stream: GradSync buckets, the optimiser).
_SIDE = {"stream": None, "pending": False, "callback": False, "mains": [], "keep": [],
         "bytes": 0, "task": -1}
# the tensors the side stream reads are kept alive until the join: past this many bytes the main
# stream joins early (mid-backward) and lets them go -- bounds what the overlap adds to the
# step's peak memory (default: 1/8 of the device; ADELL_SIDE_KEEP_GB overrides)
_SIDE_KEEP_LIMIT = {"bytes": None}


def _side_keep_limit(device):
    if _SIDE_KEEP_LIMIT["bytes"] is None:
        env = os.environ.get("ADELL_SIDE_KEEP_GB")
        if env is not None:
            _SIDE_KEEP_LIMIT["bytes"] = int(float(env) * (1 << 30))
        else:
            _SIDE_KEEP_LIMIT["bytes"] = torch.cuda.get_device_properties(device).total_memory // 8
    return _SIDE_KEEP_LIMIT["bytes"]


def _side_join_callback():
    _SIDE["callback"] = False
    join_side_stream()


def join_side_stream():
    """Make the current stream -- and every stream a backward node handed work over from (the
    engine's final callbacks need not run under the stream of the forward pass) -- wait for the
    weight gradients still running on the side stream."""
    # (also re-arms the end-of-backward callback: a backward pass that raised never ran it)
    _SIDE["callback"] = False
    if _SIDE["pending"]:
        side = _SIDE["stream"]
        cur = torch.cuda.current_stream(side.device)
        cur.wait_stream(side)
        for m in _SIDE["mains"]:
            if m != cur:
                m.wait_stream(side)
        _SIDE["mains"] = []
        _SIDE["pending"] = False
        # the tensors the side stream read may go back to the allocator now: whatever stream
        # reuses their memory does so behind the wait just queued
        _SIDE["keep"].clear()
        _SIDE["bytes"] = 0


def side_stream_behind(main):
    """The weight-gradient stream, made to wait for ``main``, when it holds work of the running
    backward pass -- for consumers that would rather queue behind the gradients than stall the
    main stream for them (GradSync's bucket gathers); else None."""
    if not _SIDE["pending"] or _SIDE["stream"] is None or _SIDE["stream"].device != main.device:
        return None
    _SIDE["stream"].wait_stream(main)
    return _SIDE["stream"]


def side_keep(t):
    """Keep ``t`` alive until the side stream has been joined (for work a caller queued on it)."""
    _SIDE["keep"].append(t)


def side_run(fn, reads):
    """``fn()`` with its launches on the side stream; ``reads``: the tensors it reads. They are
    kept alive until the join (not ``record_stream``-ed: that defers the reuse of every such block
    behind an allocator event, and with the host a step ahead of the GPU the pools kept growing
    through fresh device allocations -- sporadic 0.3 s stalls in the first steps of a process)."""
    main = torch.cuda.current_stream()
    side = _SIDE["stream"]
    if side is None or side.device != main.device:
        # (a LOW-priority stream -- hipStreamCreateWithPriority, torch only hands out normal / high --
        # was measured: the main stream ends 0.3 ms earlier and waits that much longer at the join)
        side = _SIDE["stream"] = torch.cuda.Stream(device=main.device)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        out = fn()
    for t in reads:
        if t is not None:
            _SIDE["keep"].append(t)
            _SIDE["bytes"] += t.numel() * t.element_size()
    _SIDE["pending"] = True
    if main not in _SIDE["mains"]:
        _SIDE["mains"].append(main)
    # one end-of-backward join per GraphTask: a backward pass that raised after a side_run never
    # ran its callback, and the next pass must queue its own (the flag alone would suppress it)
    task = torch._C._current_graph_task_id()
    if not _SIDE["callback"] or _SIDE["task"] != task:
        _SIDE["callback"], _SIDE["task"] = True, task
        torch.autograd.Variable._execution_engine.queue_callback(_side_join_callback)
    if _SIDE["bytes"] > _side_keep_limit(main.device):
        join_side_stream()      # early join: the kept tensors go back to the allocator
    return out


def _note_use(weight):
    """Forward side of _side_ok: counts the graph nodes that hold this weight. Two nodes in one
    graph (the semi-supervised step runs the network twice) have their gradients added by the
    autograd engine on the main stream, which knows nothing of the side stream."""
    if torch.is_grad_enabled() and weight.requires_grad:
        n = getattr(weight, "_adell_uses", 0) + 1
        weight._adell_uses = n
        if n > 1 or _inside_torch_ddp():
            weight._adell_multi = True


def _inside_torch_ddp():
    """True while a torch DistributedDataParallel wrapper runs the forward pass: its Reducer reads
    every gradient from a C++ hook on the AccumulateGrad node, on the main stream, as soon as the
    node returns -- invisible to _side_ok's hook checks, so such weights stay on the main stream."""
    try:
        from torch.nn.parallel import DistributedDataParallel as _DDP
        return getattr(_DDP, "_active_ddp_module", None) is not None
    except Exception:       # torch built without distributed
        return False


def reset_uses(params):
    """A new step: forget graph nodes that never ran their backward (FlatParameters.zero_grad)."""
    if torch.cuda.is_available() and _SIDE["pending"]:
        join_side_stream()
    for p in params:
        if getattr(p, "_adell_uses", 0):
            p._adell_uses = 0
            p._adell_multi = False


def _side_ok(weight, *params):
    """Whether the gradients of these leaf parameters may be produced off the main stream: nothing
    on the main stream reads them before the join (one graph node per weight, no accumulation into
    an existing .grad, no tensor hooks, no further autograd nodes). Called once per backward node."""
    uses = getattr(weight, "_adell_uses", 0)
    multi = getattr(weight, "_adell_multi", False)
    if uses > 0:
        weight._adell_uses = uses - 1
        if uses == 1:
            weight._adell_multi = False
    if uses != 1 or multi:
        return False
    if not FLAGS["wgrad_stream"] or torch.is_grad_enabled():     # (create_graph: dW feeds a graph)
        return False
    dist_on = torch.distributed.is_available() and torch.distributed.is_initialized()
    for p in (weight,) + params:
        if p is None:
            continue
        if not p.is_leaf or p.grad is not None or p._backward_hooks:
            return False
        # OPT-IN: the gradient's consumer must be known to join the side stream before it reads.
        # That is optim.FlatParameters (collect / zero_grad join) on one process, and with a
        # process group up additionally parallel.GradSync (its hooks and its all_reduce() go
        # through collect). Anything else -- a torch optimiser, torch DDP's Reducer (a C++ hook on
        # the AccumulateGrad node that copies dW into its bucket on the main stream the moment the
        # node returns) -- gets its gradients on the main stream.
        if not getattr(p, "_adell_flat", False):
            return False
        if dist_on and not getattr(p, "_adell_gradsync", False):
            return False
        # post-accumulate hooks read the gradient on the main stream: only GradSync's own (which
        # join first, FlatParameters.collect) are known to be safe
        if getattr(p, "_post_accumulate_grad_hooks", None) and not getattr(p, "_adell_gradsync", False):
            return False
    return True


# ---- split rows between an ADN site and the conv that is its only reader -----------------------------
# Module code that knows "the output of THIS ActDropNorm is read by THAT Conv3d and by nothing else"
# says so before it runs the ADN (expect_rows); the ADN's forward takes the note (take_rows_reader)
# and, when the conv's kernels stage split rows for this shape, writes rows instead of fp32 values
# (same bytes). The note is keyed by the ADN module: no other norm_drop_act call can pick it up.
_ROWS_EXPECT = weakref.WeakKeyDictionary()   # keyed by the ADN module itself (an id() can be reused)
_ROWS_PLAN = {}


def _hooked(producers, readers):
    """Could anything but the announced conv see the tensor? Forward hooks on a module whose output
    it is (the ADN, the link / decoder block around it, anything inside), forward pre-hooks on a
    module whose input it is, or global module hooks (feature extraction, Grad-CAM, profilers):
    they would be handed fp32-typed memory holding fp16 row pairs."""
    gm = torch.nn.modules.module
    if gm._global_forward_hooks or gm._global_forward_pre_hooks:
        return True
    for top in producers:
        for m in top.modules():
            if m._forward_hooks:
                return True
    for top in readers:
        for m in top.modules():
            if m._forward_pre_hooks:
                return True
    return False


def expect_rows(adn_module, conv, as_x1=False, producers=(), readers=()):
    """``conv``: a modules.layers.conv.Conv3d; ``as_x1``: the tensor will be the conv's X_cat.
    ``producers`` / ``readers``: the enclosing modules that return / receive the same tensor (the
    link block and the decoder block of a skip hand-over); with the ADN and the conv themselves
    they are searched for hooks that would observe the tensor (``_hooked``): then it stays fp32."""
    spec = conv.rows_spec() if (not FLAGS["no_rows"] and hasattr(conv, "rows_spec")) else None
    if spec is not None and _hooked((adn_module,) + tuple(producers), (conv,) + tuple(readers)):
        spec = None
    if spec is None:
        _ROWS_EXPECT.pop(adn_module, None)
    else:
        _ROWS_EXPECT[adn_module] = spec + (bool(as_x1),)


def clear_row_expectations():
    """A new top-level forward: notes left by a pass that never reached its ADN are void."""
    if _ROWS_EXPECT:
        _ROWS_EXPECT.clear()


def take_rows_reader(adn_module):
    return _ROWS_EXPECT.pop(adn_module, None) if _ROWS_EXPECT else None


def _rows_exponent(x, reader, norm, gamma, beta, act, act_p, act_w, p):
    """Exponent for a split-row output of this site, or None when it must stay fp32: instance
    statistics without affine parameters bound the normalised value by sqrt(V), dropout scales by
    1 / (1 - p), and |act(u)| <= |u| for the activations listed -- so 2^exp is chosen on the host,
    without a pass over the data, with the largest possible value at 2^14 (fp16 tops out at 2^16;
    typical values sit ~2^10 below the bound, where hi + lo still carry 22 bits and the absolute
    error floor is 2^-25 of the scaled unit)."""
    if (reader is None or FLAGS["no_rows"] or CONV_PRECISION != "f16x3" or norm != "instance"
            or p >= 1.0
            or gamma is not None or beta is not None or act_w is not None or x.dim() != 5
            or act not in ("identity", "swish", "silu", "relu", "leaky_relu", "gelu")
            or (act == "leaky_relu" and abs(act_p) > 1.0)):
        return None
    weight, stride, padding, as_x1 = reader
    N, C = x.shape[:2]
    spatial = tuple(x.shape[2:])
    other = weight.shape[1] - C
    if weight.dim() != 5 or other < 0 or C < 16 or (C & (C - 1)) or C > 1024:
        return None
    C0, C1 = (other, C) if as_x1 else (C, other)
    if C0 == 0:
        C0, C1 = C1, 0
    grad = torch.is_grad_enabled() and weight.requires_grad
    key = (N, spatial, C0, C1, tuple(weight.shape), stride, padding, grad, ops.plan_epoch())
    ok = _ROWS_PLAN.get(key)
    if ok is None:
        k = tuple(weight.shape[2:])
        ok = ops.conv3d_rows_ok(N, spatial, C0, C1, weight.shape[0], k, stride, padding)
        if ok and grad:
            ok = ops.conv3d_bwd_weight_rows_ok(N, spatial, C0, C1, weight.shape[0], k, stride,
                                               padding)
        _ROWS_PLAN[key] = ok
    if not ok:
        return None
    V = spatial[0] * spatial[1] * spatial[2]
    bound = float(np.sqrt(V)) / (1.0 - p)
    return 14 - int(np.ceil(np.log2(max(bound, 1.0))))


def materialize(t):
    """``t`` as plain fp32 values (a split-row tensor converted back; anything else unchanged). For
    the rare reader that is not the conv the rows were written for. Not differentiable: use on
    tensors whose gradient does not matter or inside an autograd.Function."""
    rows = getattr(t, "_adell_rows", None)
    return t if rows is None else ops.rows_to_f32(t.detach(), rows)


class _Shape:
    """Stands in for a tensor in the ops.*_ok predicates, which read only ``.shape`` / ``.dim()``."""
    def __init__(self, shape):
        self.shape = tuple(shape)

    def dim(self):
        return len(self.shape)


def conv3d_route(x0_shape, weight_shape, stride, padding, C1=None, has_residual=False,
                 has_carry=False, has_rows=False):
    """The forward kernel of ``conv3d`` -- the one routing decision of the forward pass. Host only: shapes
    (or the tensors: only ``.shape`` is read), triples and flags (``C1``: channels of the second source,
    None without one; ``has_carry``: any GradCarry; ``has_rows``: x0 holds split rows); first match wins."""
    x0, w = x0_shape, weight_shape
    if isinstance(x0, tuple):       # (conv3d() passes its tensors: no stand-ins built per call)
        x0, w = _Shape(x0), _Shape(w)
    residual = has_residual or None       # (the predicates test ``is None`` only, as for x1 / C1)
    # A 1x1x1 stride-1 conv over channels-last memory IS a Linear layer over the voxels: the GEMM
    # kernels take it (fused bias). On the implicit-GEMM conv kernels a brick's voxels x one 16-channel
    # chunk per step is the wrong tiling for it: ConvNeXt's stage transitions (384 -> 768 at 64 x 2^3
    # voxels) ran 0.79 ms forward and 0.78 ms backward-data at 0.4 TF, UNETR's 512 -> 512 at 12^3
    # 0.19 / 0.21 / 0.32 ms. (No statistics partials then: a following instance norm computes its own.)
    if (w.dim() == 5 and w.shape[2:] == (1, 1, 1) and stride == (1, 1, 1)
            and padding == (0, 0, 0) and C1 is None and not has_residual and not has_carry
            and x0.dim() == 5 and not has_rows and max(w.shape[:2]) >= 64
            and min(w.shape[:2]) >= 8 and not FLAGS["no_pointwise_gemm"]):
        return "pointwise_gemm"
    # logits head: 1x1x1, Cout <= 4 -- one HBM-bound pass on canonical weights
    if ops.conv1_small_ok(w, x0.shape[1] + (C1 or 0), stride, padding, residual):
        return "conv1_small"
    # 2-channel input block: exact fp32 on the vector ALU, canonical weights
    if ops.conv_cin_small_ok(w, x0, C1, stride, padding, residual):
        return "cin_small"
    # K = 27 Cin im2col GEMM on the fp32 MFMA (forward, dW); dX: f16x3 igemm
    if ops.conv_cinfold_ok(w, x0, C1, stride, padding, residual):
        return "cinfold"
    # Cin <= 4, Kw * Cin <= 16: the x taps ride in the 16-channel MFMA chunk (forward only: the
    # gradients see the original tensors and weights)
    if (CONV_PRECISION == "f16x3" and C1 is None and w.dim() == 5 and x0.shape[1] <= 4
            and 3 <= w.shape[4] and w.shape[4] * x0.shape[1] <= 16
            and stride == (1, 1, 1) and not FLAGS["no_fold"]):
        return "fold"
    return "igemm"      # fp32 or f16x3 MFMA, by CONV_PRECISION


def conv3d_dgrad_route(fwd_route, x0_shape, weight_shape, stride, padding, C1=0, need0=True,
                       need1=False, has_x1=False, has_add0=False, sites=False, lowrank=False):
    """The backward-data kernel of a conv whose forward took ``fwd_route``; None when nothing needs a data
    gradient. Host only, first match wins, the library is asked only when the cheaper conditions before a
    query hold. ``need0`` / ``need1``: needs_input_grad of x0 / x1; ``has_add0``: a parked gradient joins
    dx0; ``sites``: single-use ADN sites with a fused-epilogue plan; ``lowrank``: the factored logits head."""
    f16x3 = CONV_PRECISION == "f16x3"      # (evaluated at backward time)
    N, C0, in_size = x0_shape[0], x0_shape[1], tuple(x0_shape[2:])
    Cout, k = weight_shape[0], tuple(weight_shape[2:]) or (1, 1, 1)
    need1 = has_x1 and need1
    if fwd_route == "conv1_small":
        if lowrank and need0:
            return "conv1_lowrank"      # dX = dy (x) weight stays factored
        return "conv1_small" if need0 or need1 else None
    if need0 and fwd_route == "cinfold" and _lib.lib().adell_conv_cinfold_dx_applicable(
            ctypes.byref(ops.make_conv_desc(N, in_size, C0, 0, Cout, 3, 1, padding))):
        return "cinfold"                # (refused: Cout > 64 or not a multiple of 4 -- falls through)
    if need0 and fwd_route == "cin_small":
        if Cout % 4 == 0:
            return "cin_small"
        # Cout <= 4 too (the 2 -> 2 conv of an input block whose input carries a gradient:
        # SWIN-UNet): dX is the same small conv of dY with the taps flipped and the channel
        # axes swapped (padding k - 1 - p) -- on the vector-ALU forward kernel instead of a
        # 32-column MFMA tile that is 94 % empty (1.37 ms -> 0.1 ms at 256 x 256 x 128)
        if (Cout <= 4 and stride == (1, 1, 1)
                and ops.conv_out_size(in_size, k, stride, padding) == in_size):
            return "cin_small_flipped"
    if need0 and not has_x1 and f16x3:
        # the U-Net downsampling layer at 32 channels: one persistent launch
        if ops.conv3d_bwd_data_s2_fused_ok(in_size, C0, C1, Cout, k, stride, padding):
            return "s2_fused"
        # stride-2 backward-data by parity classes (no zero-inserted MFMA work). Eight
        # launches: pays from ~1 M voxels (measured: 128^3 0.52 -> 0.33 ms, 32^3 0.06 -> 0.16)
        if (stride == (2, 2, 2) and k == (3, 3, 3) and all(p <= 1 for p in padding)
                and all(s % 2 == 0 for s in in_size) and not FLAGS["no_s2class"]
                and (FLAGS["s2class_always"] or N * in_size[0] * in_size[1] * in_size[2] >= 1 << 20)):
            return "s2_classes"
    # the input(s) are outputs of norm -> dropout -> activation sites read by this conv only: their
    # activation / dropout derivative and the two sums of the norm's backward come out of this
    # kernel's epilogue (AdnSite)
    if sites and need0 and (not has_x1 or need1) and (not has_add0 or C1 == 0) and f16x3:
        return "igemm_adn"
    return "igemm" if need0 or need1 else None


def conv3d_wgrad_route(fwd_route, need_w=True, want_db=False):
    """The weight-gradient kernel (which also yields the bias gradient when wanted); None when
    neither gradient is needed. Host only."""
    if fwd_route == "conv1_small":
        return "conv1_small" if need_w or want_db else None
    if need_w and fwd_route == "cinfold":
        # (0.297 vs 0.339 ms for 2 -> 32 at 2 x 128^3, 0.167 vs 0.207 ms for 1 -> 16 at
        # 4 x 96^3: tools/cinfold_wgrad_time.py)
        f16 = CONV_PRECISION == "f16x3" and not FLAGS["no_cinfold_wgrad_f16"]
        return "cinfold_f16x3" if f16 else "cinfold_fp32"
    if need_w:
        return "igemm_f16x3" if CONV_PRECISION == "f16x3" else "igemm_fp32"
    return "bias_only" if want_db else None


# One conv3d call as _Conv3dFn sees it. adn: (site0, site1, ntiles, plan epoch) of _adn_sites_of or None;
# lowrank_site: the AdnSite that takes (dy, weight) of the logits head or None; rows0 / rows1: ops.SplitRows
_ConvCall = collections.namedtuple("_ConvCall", "route stride padding want_stats wref carry_in "
                                   "carry_out carry_x0 carry_cat adn lowrank_site rows0 rows1")


class _Conv3dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x0, x1, weight, bias, residual, wp, call):
        """``wp``: the packed forward operand of the "fold" / "igemm" routes, else None."""
        route, stride, padding, want_stats = call[:4]
        rows0, rows1 = call.rows0, call.rows1
        f16x3 = route == "igemm" and isinstance(wp, ops.SplitWeight)
        if (rows0 is not None or rows1 is not None) and not f16x3:
            # a reader other than the f16x3 implicit-GEMM path: it gets fp32 values (and so does
            # its backward: the converted tensors are the ones saved)
            ops.ROWS_FALLBACKS[0] += 1
            if rows0 is not None:
                x0, rows0 = ops.rows_to_f32(x0, rows0), None
            if rows1 is not None:
                x1, rows1 = ops.rows_to_f32(x1, rows1), None
        k = tuple(weight.shape[2:]) or (1, 1, 1)     # (a 2-D Linear weight: 1x1x1)
        # the statistics partials are a non-differentiable by-product: without this autograd
        # materialises a zero gradient for them in every backward (a 2 MB fill per conv site)
        ctx.set_materialize_grads(False)
        part = amax = None
        if route == "conv1_small":
            y = ops.conv1_small_fwd(x0, x1, weight, bias)
        elif route == "cin_small":
            y, part = ops.conv_cin_small_fwd(x0, weight, bias, padding, want_stats)
        elif route == "cinfold":
            y, part = ops.conv_cinfold_fwd(x0, weight, bias, padding, want_stats,
                                           f16x3=CONV_PRECISION == "f16x3")
        elif route == "fold":
            xf = ops.fold_x_taps(x0, k[2], padding[2])
            y, part = ops.conv3d_fwd(xf, wp, bias, weight.shape[0], (k[0], k[1], 1), stride,
                                     (padding[0], padding[1], 0), residual=residual,
                                     want_stats=want_stats)
        elif route == "igemm":
            # [0]: absmax bits of the input(s), [1]: of dy -- by-products of the f16x3 forward /
            # backward-data kernels that the backward-weight kernel uses as operand scales
            if f16x3 and ctx.needs_input_grad[2]:
                amax = _amax_pair(x0.device)
            y, part = ops.conv3d_fwd(x0, wp, bias, weight.shape[0], k, stride, padding, x1=x1,
                                     residual=residual, want_stats=want_stats,
                                     amax=None if amax is None else amax[0:1], rows0=rows0,
                                     rows1=rows1)
        else:
            raise ValueError(f"conv3d: unknown forward route {route!r}")
        ctx.save_for_backward(x0, x1, weight)
        # (a residual reaches only the "fold" / "igemm" routes: the other predicates refuse one)
        ctx.rows, ctx.amax, ctx.bias_ref = (rows0, rows1), amax, _Ref(bias)
        ctx.conf = (call, k, bias is not None, residual is not None)
        part = y.new_empty(0) if part is None else part
        ctx.mark_non_differentiable(part)
        return y, part

    @staticmethod
    def backward(ctx, dy, _dpart):
        x0, x1, weight = ctx.saved_tensors
        call, k, has_bias, has_res = ctx.conf
        stride, padding, wref = call.stride, call.padding, call.wref
        need = ctx.needs_input_grad
        add0 = call.carry_in.take() if call.carry_in is not None else None
        if dy is None:   # the output took no part in the loss: only a parked gradient passes through
            _side_ok(wref.obj)      # (bookkeeping: this node is done)
            return (add0 if need[0] else None), None, None, None, None, None, None
        dy = ops.ndhwc(dy)
        dx0 = dx1 = dw = db = dres = None
        C0, in_size = x0.shape[1], tuple(x0.shape[2:])
        C1 = 0 if x1 is None else x1.shape[1]
        f16x3 = CONV_PRECISION == "f16x3"
        route = conv3d_dgrad_route(call.route, x0.shape, weight.shape, stride, padding, C1,
                                   need[0], need[1], x1 is not None, add0 is not None,
                                   call.adn is not None, call.lowrank_site is not None)
        # (only behind an f16x3 "igemm" forward; every backward-data launch from there writes the slot)
        amax = ctx.amax
        dy_amax = amax[1:2] if amax is not None and f16x3 and route is not None else None
        if route == "conv1_lowrank":
            call.lowrank_site.lowrank = (dy, weight.detach())
            dx0 = dy.new_zeros(()).expand(x0.shape)    # a stride-0 placeholder goes down the graph
        elif route == "conv1_small":
            dx0, dx1 = ops.conv1_small_bwd_data(dy, weight, in_size, C0, C1)
        elif route == "cinfold":
            dx0 = ops.conv_cinfold_bwd_data(dy, weight, in_size, padding, f16x3=f16x3)
        elif route == "cin_small":
            dx0 = ops.conv_cin_small_bwd_data(dy, weight, in_size, padding)
        elif route == "cin_small_flipped":
            wt = weight.detach().transpose(0, 1).flip(2, 3, 4).contiguous()
            pt = tuple(kk - 1 - pp for kk, pp in zip(k, padding))
            dx0, _ = ops.conv_cin_small_fwd(dy, wt, None, pt, False)
        elif route == "s2_fused":
            dx0 = ops.conv3d_bwd_data_s2_fused(dy, _packed(wref.obj, 1), in_size, amax=dy_amax,
                                               add0=add0)
            add0 = None
        elif route == "s2_classes":
            dx0 = ops.conv3d_bwd_data_s2(dy, _packed_s2_classes(wref.obj, padding), in_size, C0,
                                         padding, amax=dy_amax, add0=add0)
            add0 = None
        elif route in ("igemm_adn", "igemm"):
            wpb = _packed(wref.obj, 1)
            ntiles = 0
            if route == "igemm_adn":
                site0, site1, ntiles, epoch = call.adn
                if epoch != ops.plan_epoch():
                    # the launch plan changed since the forward (adell_set_tuning): the partial-sum rows are
                    # the CURRENT plan's, or the plain path if it has no fused epilogue (two-pass sites)
                    ntiles = ops.conv3d_bwd_data_adn_ntiles(in_size, x0.shape[0], C0, C1,
                                                            dy.shape[1], k, stride, padding)
            if ntiles > 0:
                dx0, dx1, part = ops.conv3d_bwd_data_adn(dy, wpb, in_size, C0, C1, k, stride,
                                                         padding, ntiles, site0=site0,
                                                         site1=site1, amax=dy_amax, add0=add0)
                add0 = None
                for site, poff in ((site0, 0), (site1, C0)):
                    if site is not None:
                        site.fused, site.part, site.poff = True, part, poff
            else:
                fused = add0 is not None and C1 == 0 and f16x3    # the add in the kernel epilogue
                dx0, dx1 = ops.conv3d_bwd_data(dy, wpb, in_size, C0, C1, k, stride, padding,
                                               amax=dy_amax, add0=add0 if fused else None)
                if fused:
                    add0 = None
        elif route is not None:
            raise ValueError(f"conv3d: unknown backward-data route {route!r}")
        dx0 = dx0 if need[0] else None
        dx1 = dx1 if x1 is not None and need[1] else None
        want_db = has_bias and need[3]
        wroute = conv3d_wgrad_route(call.route, need[2], want_db)

        def weight_grads(on_side=False):
            db = None
            if wroute == "conv1_small":
                dw, db = ops.conv1_small_bwd_weight(x0, x1, dy, want_db)
            elif wroute.startswith("cinfold"):
                dw, db = ops.conv_cinfold_bwd_weight(x0, dy, padding, want_db,
                                                     f16x3=wroute == "cinfold_f16x3")
            elif wroute.startswith("igemm"):
                dw = ops.conv3d_bwd_weight(x0, dy, k, stride, padding, x1=x1, want_db=want_db,
                                           f16x3=wroute == "igemm_f16x3",
                                           x_amax=None if amax is None else amax[0:1],
                                           dy_amax=dy_amax, rows0=ctx.rows[0], rows1=ctx.rows[1],
                                           share=on_side and not FLAGS["no_wgrad_share"])
                if want_db:
                    dw, db = dw
            elif wroute == "bias_only":
                return None, ops.bias_grad(dy)
            else:
                raise ValueError(f"conv3d: unknown weight-gradient route {wroute!r}")
            return (dw.view(weight.shape) if need[2] else None), db

        if wroute is not None:
            dw, db = (side_run(lambda: weight_grads(on_side=True), (x0, x1, dy))
                      if _side_ok(wref.obj, ctx.bias_ref.obj) else weight_grads())
        if add0 is not None and dx0 is not None:   # a route without the fused add
            dx0 = dx0 + add0
        # skip fork: leave dX of x0 / x1 with the consumer of the same tensor that runs later
        if dx0 is not None and call.carry_x0 is not None:
            call.carry_x0.grad, dx0 = dx0, None
        if dx1 is not None and call.carry_cat is not None:
            call.carry_cat.grad, dx1 = dx1, None
        if has_res and need[4]:
            if call.carry_out is not None:
                call.carry_out.grad = dy      # the head conv of the block adds it to its dX
            else:
                dres = dy
        return dx0, dx1, dw, db, dres, None, None


def grad_observed(t):
    """True when someone watches the gradient of ``t`` (tensor hooks, ``retain_grad()``): a
    GradCarry routes part of that gradient around autograd, so the watcher would see a partial
    value -- callers then leave the fork to autograd's own accumulation. ``ADELL_NO_GRAD_CARRY=1``
    switches the carries off altogether (gradient-inspection tools, partial
    ``torch.autograd.grad(inputs=...)`` calls that run the parking conv but not the taking one)."""
    return bool(getattr(t, "_backward_hooks", None)) or bool(getattr(t, "retains_grad", False))


class GradCarry:
    """Hands a gradient from one consumer of a tensor to another consumer of the SAME tensor whose
    backward runs later and whose backward-data kernel adds it in its epilogue -- one full-size
    add pass (autograd's accumulation) less per fork.
    * residual link (``op(X) + X``, res_blocks.py:192): the conv that adds the link parks its dy
      (``carry_out``), the conv at the head of the block takes it (``carry_in``);
    * U-Net skip fork (unet.py:768-822): the first conv of the link op parks its dX
      (``carry_x0``; with identity links it is the decoder conv that reads the level output as
      the second half of its channel concat, ``carry_cat``), the strided conv that downsamples the
      same level output takes it (``carry_in``). The downsampling conv's backward depends on the
      decoder's (through the bottleneck), so it always runs later."""

    __slots__ = ("grad",)

    def __init__(self):
        self.grad = None

    def take(self):
        g, self.grad = self.grad, None
        return g


class AdnSite:
    """A norm -> dropout -> activation site as the backward-data kernel of its consumer needs it
    (ops.conv3d_bwd_data_adn): the site's input ``x``, its instance statistics, the keep bits its
    forward stored and the activation. The consumer's backward sets ``fused`` / ``part`` / ``poff``
    when its epilogue produced dt and the partial sums; the site's own backward then runs ONE
    elementwise pass (ops.norm_act_bwd_from_dt) instead of two."""

    __slots__ = ("x", "mean", "rstd", "mask", "drop_p", "act", "act_p", "fused", "part", "poff",
                 "lowrank")

    def __init__(self, x, mean, rstd, mask, drop_p, act, act_p):
        self.x, self.mean, self.rstd, self.mask = x, mean, rstd, mask
        self.drop_p, self.act, self.act_p = drop_p, act, act_p
        self.fused, self.part, self.poff = False, None, 0
        # (dy, weight) of a 1x1x1 consumer with <= 4 output channels: its backward-data result is
        # never formed, the site's backward reads the two factors (ops.norm_act_bwd_lowrank)
        self.lowrank = None


def single_use(t):
    """Module code declares: the next ``conv3d`` that reads ``t`` (as x0 or x1) is the ONLY
    consumer of ``t``. Only then may that conv's backward-data kernel hand the site behind ``t``
    a pre-multiplied gradient (AdnSite): a second consumer would add a plain gradient to it."""
    if t is not None and getattr(t, "_adell_site", None) is not None:
        t._adell_single = True
    return t


_ADN_PLAN = {}


def _adn_sites_of(x0, x1, weight, stride, padding):
    """(site0, site1, ntiles) when x0 / x1 carry single-use ADN sites and the backward-data
    launch of this conv takes the fused epilogue, else None."""
    # (someone watching the gradient of the site's output -- a tensor hook, retain_grad() -- must see
    # the true gradient, not dt: such a site keeps its own two-pass backward)
    s0 = (getattr(x0, "_adell_site", None)
          if getattr(x0, "_adell_single", False) and not grad_observed(x0) else None)
    s1 = (getattr(x1, "_adell_site", None)
          if x1 is not None and getattr(x1, "_adell_single", False) and not grad_observed(x1)
          else None)
    if (s0 is None and s1 is None) or CONV_PRECISION != "f16x3" or FLAGS["no_adn_fuse"] \
            or weight.dim() != 5 or not torch.is_grad_enabled():
        return None
    C0 = x0.shape[1]
    C1 = 0 if x1 is None else x1.shape[1]
    # (the row count is a property of the library's launch plan, which process-wide switches --
    # adell_set_tuning -- change: one answer per plan epoch)
    key = (tuple(x0.shape), C1, tuple(weight.shape), stride, padding, ops.plan_epoch())
    nt = _ADN_PLAN.get(key)
    if nt is None:
        nt = ops.conv3d_bwd_data_adn_ntiles(tuple(x0.shape[2:]), x0.shape[0], C0, C1,
                                            weight.shape[0], tuple(weight.shape[2:]), stride,
                                            padding)
        _ADN_PLAN[key] = nt
    if nt <= 0:
        return None
    return (s0, s1, nt, key[-1])


def conv3d(x0, weight, bias=None, stride=1, padding=0, x1=None, residual=None, want_stats=True,
           carry_in=None, carry_out=None, carry_x0=None, carry_cat=None):
    """Conv3d over the virtual concatenation [x0, x1] (+ bias + residual). ``carry_in`` /
    ``carry_out`` / ``carry_x0`` / ``carry_cat``: see GradCarry."""
    stride, padding = ops._triple(stride), ops._triple(padding)
    rows0 = getattr(x0, "_adell_rows", None)
    rows1 = getattr(x1, "_adell_rows", None) if x1 is not None else None
    route = conv3d_route(x0, weight, stride, padding,
                         None if x1 is None else x1.shape[1], residual is not None,
                         not (carry_in is None and carry_out is None and carry_x0 is None
                              and carry_cat is None), rows0 is not None)
    if route == "pointwise_gemm":
        xr = ops.ndhwc(x0)
        N, C, D, H, W = xr.shape
        y2 = linear(xr.permute(0, 2, 3, 4, 1).reshape(-1, C), weight.view(weight.shape[0], C), bias)
        return y2.view(N, D, H, W, -1).permute(0, 4, 1, 2, 3)
    _note_use(weight)
    adn = _adn_sites_of(x0, x1, weight, stride, padding)
    # the logits head behind a single-use site: the site's backward takes (dy, weight)
    site = getattr(x0, "_adell_site", None) if getattr(x0, "_adell_single", False) else None
    lowrank_site = site if (route == "conv1_small" and site is not None and x1 is None
                            and carry_in is None and carry_x0 is None and not grad_observed(x0)
                            and not FLAGS["no_adn_fuse"] and not FLAGS["no_lowrank"]
                            and torch.is_grad_enabled()
                            and ops.norm_act_lowrank_ok(x0, weight.shape[0])) else None
    # (outside the Function: _packed orders this stream behind the launch that packed the weight)
    wp = (_packed_folded(weight) if route == "fold" else
          _packed(weight, 0) if route == "igemm" else None)
    call = _ConvCall(route, stride, padding, want_stats, _Ref(weight), carry_in, carry_out,
                     carry_x0, carry_cat, adn, lowrank_site, rows0, rows1)
    y, part = _Conv3dFn.apply(x0, x1, weight, bias, residual, wp, call)
    if want_stats and part.numel() > 0:
        y._adell_partials = part
    return y


def conv_transpose3d_route(x_shape, weight_shape):
    """"k2": the streaming factor-2 kernels on the canonical weight (csrc/convt_k2.hip);
    "igemm": the 1x1x1-conv form on the packed weight. Host only."""
    return "k2" if len(x_shape) == 5 and ops.convt_k2_ok(x_shape, _Shape(weight_shape)) else "igemm"


class _ConvT3dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, wp, wref, route):
        factors = tuple(weight.shape[2:])
        y = (ops.convt_k2_fwd(x, weight, bias) if route == "k2" else
             ops.convtranspose3d_fwd(x, wp, bias, weight.shape[1], factors))
        ctx.save_for_backward(x, weight)
        ctx.route, ctx.wref, ctx.factors = route, wref, factors
        ctx.has_bias, ctx.bias_ref = bias is not None, _Ref(bias)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        k2 = ctx.route == "k2"
        dy = ops.ndhwc(dy)
        dx = dw = db = None
        if need[0]:
            dx = (ops.convt_k2_bwd_data(dy, weight) if k2 else
                  ops.convtranspose3d_bwd_data(dy, _packed(ctx.wref.obj, 3), weight.shape[0],
                                               ctx.factors))
        want_db = ctx.has_bias and need[2]

        def weight_grads():
            dw = db = None
            if need[1] and k2 and want_db:
                dw, db = ops.convt_k2_bwd_weight(x, dy, want_db=True, factors=ctx.factors)   # db from the same pass over dy
            elif need[1]:
                dw = (ops.convt_k2_bwd_weight(x, dy, factors=ctx.factors) if k2 else
                      ops.convtranspose3d_bwd_weight(x, dy, ctx.factors))
            if want_db and db is None:
                db = ops.bias_grad(dy)
            return dw, db

        if (need[1] or want_db) and _side_ok(ctx.wref.obj, ctx.bias_ref.obj):
            dw, db = side_run(weight_grads, (x, dy))
        else:
            dw, db = weight_grads()
        return dx, dw, db, None, None, None


def conv_transpose3d(x, weight, bias=None):
    """ConvTranspose3d whose kernel equals its stride (each 1 or 2 per dim), padding 0."""
    route = conv_transpose3d_route(x.shape, weight.shape)
    wp = _packed(weight, 2) if route == "igemm" else None
    _note_use(weight)
    return _ConvT3dFn.apply(x, weight, bias, wp, _Ref(weight), route)


conv_transpose3d_k2s2 = conv_transpose3d


class _NormDropActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mean, rstd, gamma, beta, act_w, conf):
        act, act_p, per_item, drop_p, seed, offset, site, split_exp, _group = conf
        if site is not None:
            out, mask = ops.norm_act_fwd(x, mean, rstd, act, gamma=gamma, beta=beta, act_w=act_w,
                                         act_p=act_p, stats_per_item=per_item, drop_p=drop_p,
                                         seed=seed, rng_offset=offset, want_mask=True,
                                         split_exp=split_exp)
            site.x, site.mean, site.rstd, site.mask = x, mean, rstd, mask
        else:
            out = ops.norm_act_fwd(x, mean, rstd, act, gamma=gamma, beta=beta, act_w=act_w,
                                   act_p=act_p, stats_per_item=per_item, drop_p=drop_p, seed=seed,
                                   rng_offset=offset, split_exp=split_exp)
        ctx.save_for_backward(x, mean, rstd, gamma, beta, act_w)
        ctx.conf = conf
        return out

    @staticmethod
    def backward(ctx, dout):
        x, mean, rstd, gamma, beta, act_w = ctx.saved_tensors
        act, act_p, per_item, drop_p, seed, offset, site, _split_exp, group = ctx.conf
        if site is not None:
            fused, part, poff = site.fused, site.part, site.poff
            site.fused, site.part = False, None
            lowrank, site.lowrank = site.lowrank, None
            # the site is done: do not pin x / statistics / mask until the graph is freed
            site.x = site.mean = site.rstd = site.mask = None
            if lowrank is not None:
                dx = ops.norm_act_bwd_lowrank(x, lowrank[0], lowrank[1], mean, rstd, act,
                                              act_p=act_p, drop_p=drop_p, seed=seed,
                                              rng_offset=offset)
                return dx, None, None, None, None, None, None
            if fused:
                # dout is dt: the consumer's backward-data epilogue applied act' / dropout and
                # left the two sums of the normalisation's backward in `part`
                dx = ops.norm_act_bwd_from_dt(x, ops.ndhwc(dout), mean, rstd, part, poff)
                return dx, None, None, None, None, None, None
        dact_w = None
        if act_w is not None and ctx.needs_input_grad[5]:
            dact_w = ops.prelu_wgrad(x, dout, mean, rstd, act_w, gamma=gamma, beta=beta,
                                     stats_per_item=per_item, drop_p=drop_p, seed=seed,
                                     rng_offset=offset)
        want_affine = gamma is not None and (ctx.needs_input_grad[3] or ctx.needs_input_grad[4])
        if group is not None:
            # synchronised batch norm: sum dt and sum dt * xhat over the ranks before dx is formed;
            # dgamma / dbeta stay local (the gradient exchange averages them)
            rec, dgamma, dbeta = ops.norm_act_bwd_sums(
                x, dout, mean, rstd, act, gamma=gamma, beta=beta, act_w=act_w, act_p=act_p,
                drop_p=drop_p, seed=seed, rng_offset=offset, want_affine_grads=want_affine)
            dist.all_reduce(rec, op=dist.ReduceOp.SUM, group=group)
            dx = ops.norm_act_bwd_apply_sums(x, dout, mean, rstd, rec, act, gamma=gamma, beta=beta,
                                             act_w=act_w, act_p=act_p, drop_p=drop_p, seed=seed,
                                             rng_offset=offset)
            if beta is None:
                dbeta = None
            return dx, None, None, dgamma, dbeta, dact_w, None
        dx, dgamma, dbeta = ops.norm_act_bwd(
            x, dout, mean, rstd, act, gamma=gamma, beta=beta, act_w=act_w, act_p=act_p,
            stats_per_item=per_item, drop_p=drop_p, seed=seed, rng_offset=offset,
            want_affine_grads=want_affine)
        if beta is None:
            dbeta = None
        return dx, None, None, dgamma, dbeta, dact_w, None


def norm_drop_act(x, *, norm="none", eps=1e-5, gamma=None, beta=None, running=None,
                  momentum=0.1, act="identity", act_p=0.0, act_w=None, drop_p=0.0,
                  training=False, rows_reader=None, sync_group=None):
    """Fused Norm -> Dropout -> Activation.

    norm: "none" | "instance" | "batch". ``running`` = (running_mean, running_var,
    num_batches_tracked) buffers of a BatchNorm module (updated in training).
    ``sync_group``: a process group of more than one rank makes a batch norm in training
    synchronised (torch.nn.SyncBatchNorm): statistics over the items of every rank of the group,
    and the backward's two per-channel sums too -- one all-reduce of 2C + 1 doubles each way, ordered
    on the current stream. A group of one (or None) is the unsynchronised path.
    """
    part = getattr(x, "_adell_partials", None)
    x = ops.ndhwc(x)
    N, C = x.shape[:2]
    V = x.shape[2] * x.shape[3] * x.shape[4]
    mean = rstd = group = None
    per_item = 1
    if norm == "instance":
        if part is None:
            part = ops.channel_partials(x.detach())
        mean, rstd = ops.stats_finalize(part, V, eps, per_item=True)
    elif norm == "batch":
        per_item = 0
        if (training and sync_group is not None
                and dist.get_world_size(group=sync_group) > 1):
            if part is None:
                part = ops.channel_partials(x.detach())
            rec = ops.bn_stats_sums(part, V)
            dist.all_reduce(rec, op=dist.ReduceOp.SUM, group=sync_group)
            mean, rstd = ops.bn_stats_from_sums(rec, eps, running, momentum)
            group = sync_group
        elif training or running is None or running[0] is None:
            if part is None:
                part = ops.channel_partials(x.detach())
            mean, rstd = ops.stats_finalize(part, V, eps, per_item=False)
            if training and running is not None and running[0] is not None:
                rm, rv, nbt = running
                if nbt is None and momentum is None:
                    raise ValueError("BatchNorm with momentum=None needs num_batches_tracked")
                ops.bn_running_update(mean, rstd, rm, rv, nbt, N * V, eps, momentum)
        else:
            # running statistics are constants, not functions of x: fold them into the affine
            # pair (y = x * (rstd gamma) + (beta - mean rstd gamma)) so that the backward is the
            # plain elementwise one; [C]-sized parameter algebra, autograd carries dgamma / dbeta
            rstd_c = torch.rsqrt(running[1] + eps)
            gamma = rstd_c if gamma is None else rstd_c * gamma
            shift = -running[0] * gamma
            beta = shift if beta is None else beta + shift
    elif norm != "none":
        raise NotImplementedError(f"norm {norm!r} has no HIP kernel yet")
    p = float(drop_p) if training else 0.0
    seed, offset = 0, 0
    if p > 0.0:
        seed = torch.initial_seed()
        offset = next(_dropout_counter)
    # a site whose only consumer is a conv can leave half of its backward to that conv's
    # backward-data kernel (AdnSite): instance statistics, no affine parameters, an activation the
    # epilogue knows; the forward then also stores its keep bits
    site = None
    if (norm == "instance" and gamma is None and beta is None and act_w is None
            and act in ("identity", "swish", "silu", "relu", "leaky_relu") and x.requires_grad
            and torch.is_grad_enabled() and not FLAGS["no_adn_fuse"] and CONV_PRECISION == "f16x3"
            and ops.norm_act_mask_ok(x)):
        site = AdnSite(None, None, None, None, p, act, float(act_p))
    # (rows_reader: the conv that is the ONLY reader of the output, take_rows_reader)
    split_exp = _rows_exponent(x, rows_reader, norm, gamma, beta, act, float(act_p), act_w, p)
    conf = (act, float(act_p), per_item, p, seed, offset, site, split_exp, group)
    out = _NormDropActFn.apply(x, mean, rstd, gamma, beta, act_w, conf)
    if site is not None:
        out._adell_site = site
    if split_exp is not None:
        out._adell_rows = ops.SplitRows(split_exp, ops.split_exponents(N, C, split_exp, x.device))
    return out


# ---- token-sequence functions (ViT encoder of UNETR) -------------------------------------
def _rows_as_volume(x):
    """[..., C] contiguous -> logical [1, C, 1, 1, rows] tensor with NDHWC memory (a view)."""
    x = x.contiguous()
    C = x.shape[-1]
    return x.view(1, 1, 1, -1, C).permute(0, 4, 1, 2, 3)


def _volume_as_rows(y, lead_shape):
    """inverse of _rows_as_volume: [1, C, 1, 1, rows] (NDHWC memory) -> [*lead, C]."""
    C = y.shape[1]
    return y.permute(0, 2, 3, 4, 1).reshape(*lead_shape, C)


class _LinearFn(torch.autograd.Function):
    """x W^T (+ bias) (+ residual) on the fp32-MFMA GEMM (ops.gemm). Opt-in
    (``ops.FLAGS["gemm_f16x3"]`` / ADELL_GEMM_F16X3=1, with CONV_PRECISION "f16x3"): the three GEMMs
    on the f16 MFMA with the error-compensated split (ops.gemm_f16x3) whenever the operands
    qualify -- faster per launch, slower per step at the measured configurations."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual):
        N, K = weight.shape
        x2 = x.reshape(-1, K).contiguous()
        rows = x2.shape[0]
        w = weight.contiguous()
        res2 = None if residual is None else residual.reshape(rows, N).contiguous()
        split = CONV_PRECISION == "f16x3" and ops.gemm_f16x3_ok(rows, N, K, x2, K, True, w, K, True)
        if split:
            y = ops.gemm_f16x3(rows, N, K, x2, K, True, w, K, True, bias=bias, residual=res2)
        else:
            y = ops.gemm(rows, N, K, x2, K, True, w, K, True, bias=bias, residual=res2)
        ctx.save_for_backward(x2, w)
        ctx.split = split
        ctx.refs = (_Ref(weight), _Ref(bias))
        ctx.meta = (x.shape, bias is not None, residual is not None and residual.shape)
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x2, w = ctx.saved_tensors
        xshape, has_bias, res_shape = ctx.meta
        split = ctx.split
        N, K = w.shape
        rows = x2.shape[0]
        need = ctx.needs_input_grad
        dy2 = dy.reshape(rows, N).contiguous()
        dx = dw = db = dres = None
        if need[0]:
            if split and ops.gemm_f16x3_ok(rows, K, N, dy2, N, True, w, K, False):
                dx = ops.gemm_f16x3(rows, K, N, dy2, N, True, w, K, False)
            else:
                dx = ops.gemm(rows, K, N, dy2, N, True, w, K, False)
            dx = dx.view(xshape)
        def weight_grads():
            dw = db = None
            if need[1]:
                if split and ops.gemm_f16x3_ok(N, K, rows, dy2, N, False, x2, K, False):
                    dw = ops.gemm_f16x3(N, K, rows, dy2, N, False, x2, K, False)
                else:
                    dw = ops.gemm(N, K, rows, dy2, N, False, x2, K, False)
            if has_bias and need[2]:
                db = ops.bias_grad(_rows_as_volume(dy2))
            return dw, db

        if (need[1] or (has_bias and need[2])) and _side_ok(ctx.refs[0].obj, ctx.refs[1].obj):
            dw, db = side_run(weight_grads, (x2, dy2))
        else:
            dw, db = weight_grads()
        if res_shape and need[3]:
            dres = dy2.view(res_shape)
        return dx, dw, db, dres


class _MlpFn(torch.autograd.Function):
    """Linear -> activation -> Linear (+ residual) as three + four GEMMs and NO element-wise pass
    (ConvNeXt's pwconv1 -> GELU -> pwconv2 -> + input, res_blocks.py:559-566): the first GEMM's
    epilogue stores the pre-activation (for the backward) and the activation (for the second GEMM)
    in one pass, and the backward's dY W2 GEMM multiplies by act'(pre-activation) in its epilogue,
    so the gradient of the hidden layer is written once. f16x3 GEMMs only (the caller checks
    ``mlp_ok``)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, residual, act, act_p):
        H, K = w1.shape
        N = w2.shape[0]
        x2 = x.reshape(-1, K).contiguous()
        rows = x2.shape[0]
        w1c, w2c = w1.contiguous(), w2.contiguous()
        res2 = None if residual is None else residual.reshape(rows, N).contiguous()
        h, g = ops.gemm_f16x3_act(rows, H, K, x2, K, True, w1c, K, True, act, act_p, bias=b1,
                                  want_act=True)
        y = ops.gemm_f16x3(rows, N, H, g, H, True, w2c, H, True, bias=b2, residual=res2)
        ctx.save_for_backward(x2, w1c, w2c, h, g)
        ctx.act = (act, act_p)
        ctx.refs = (_Ref(w1), _Ref(b1), _Ref(w2), _Ref(b2))
        ctx.meta = (x.shape, b1 is not None, b2 is not None,
                    residual is not None and residual.shape)
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x2, w1, w2, h, g = ctx.saved_tensors
        xshape, has_b1, has_b2, res_shape = ctx.meta
        H, K = w1.shape
        N = w2.shape[0]
        rows = x2.shape[0]
        need = ctx.needs_input_grad
        dy2 = dy.reshape(rows, N).contiguous()
        # dh = (dy W2) * act'(h): the activation's backward rides the GEMM epilogue
        dh, _ = ops.gemm_f16x3_act(rows, H, N, dy2, N, True, w2, H, False, *ctx.act, dact_in=h)
        dx = None
        if need[0]:
            dx = ops.gemm_f16x3(rows, K, H, dh, H, True, w1, K, False).view(xshape)

        def grads2():
            dw2 = db2 = None
            if need[3]:
                dw2 = ops.gemm_f16x3(N, H, rows, dy2, N, False, g, H, False)
            if has_b2 and need[4]:
                db2 = ops.bias_grad(_rows_as_volume(dy2))
            return dw2, db2

        def grads1():
            dw1 = db1 = None
            if need[1]:
                dw1 = ops.gemm_f16x3(H, K, rows, dh, H, False, x2, K, False)
            if has_b1 and need[2]:
                db1 = ops.bias_grad(_rows_as_volume(dh))
            return dw1, db1

        r1, rb1, r2, rb2 = ctx.refs
        if (need[3] or (has_b2 and need[4])) and _side_ok(r2.obj, rb2.obj):
            dw2, db2 = side_run(grads2, (dy2, g))
        else:
            dw2, db2 = grads2()
        if (need[1] or (has_b1 and need[2])) and _side_ok(r1.obj, rb1.obj):
            dw1, db1 = side_run(grads1, (dh, x2))
        else:
            dw1, db1 = grads1()
        dres = dy2.view(res_shape) if (res_shape and need[5]) else None
        return dx, dw1, db1, dw2, db2, dres, None, None


def mlp_ok(x, w1, w2):
    """Whether ``mlp`` can take Linear(w1) -> act -> Linear(w2) on rows ``x``: all seven GEMMs on the
    f16x3 kernels."""
    if FLAGS["no_mlp_fuse"] or CONV_PRECISION != "f16x3" or not x.is_cuda:
        return False
    H, K = w1.shape
    N = w2.shape[0]
    rows = x.numel() // K
    if rows * H < FLAGS["mlp_min_elems"]:
        return False
    x2 = x.reshape(-1, K)
    ok = ops.gemm_f16x3_ok
    return (w2.shape[1] == H and x2.is_contiguous() and w1.is_contiguous() and w2.is_contiguous()
            and ok(rows, H, K, x2, K, True, w1, K, True) and ok(rows, N, H, x2, H, True, w2, H, True)
            and ok(rows, K, H, x2, H, True, w1, K, False) and ok(rows, H, N, x2, N, True, w2, H, False)
            and ok(N, H, rows, x2, N, False, x2, H, False) and ok(H, K, rows, x2, H, False, x2, K, False))


def mlp(x, w1, b1, w2, b2, act="gelu", act_p=0.0, residual=None):
    """act(x W1^T + b1) W2^T + b2 (+ residual) with the activation inside the GEMM epilogues
    (``act_p``: the slope / alpha of leaky_relu / elu)."""
    _note_use(w1)
    _note_use(w2)
    return _MlpFn.apply(x, w1, b1, w2, b2, residual, act, float(act_p))


def linear(x, weight, bias=None, residual=None):
    """torch.nn.functional.linear on the MFMA GEMMs (+ fused bias / residual add)."""
    _note_use(weight)
    return _LinearFn.apply(x, weight, bias, residual)


def elementwise(x, act="identity", act_p=0.0, drop_p=0.0, training=False):
    """Dropout -> activation on a tensor of any shape (channel axis irrelevant)."""
    shp = x.shape
    y = norm_drop_act(_rows_as_volume(x.reshape(-1, shp[-1])), act=act, act_p=act_p,
                      drop_p=drop_p, training=training)
    return _volume_as_rows(y, shp[:-1])


class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        y, mean, rstd = ops.layernorm_fwd(x, gamma, beta, eps)
        ctx.save_for_backward(x, gamma, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, rstd = ctx.saved_tensors
        want = gamma is not None and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        dx, dg, db = ops.layernorm_bwd(x, dy, gamma, mean, rstd, want)
        return dx, dg, db, None


def add(a, b):
    """a + b for same-shape tensors (HIP elementwise kernel)."""
    if a.shape != b.shape:
        raise ValueError("HF.add: shapes differ")
    return _AddBcastFn.apply(a.contiguous(), b.contiguous())


class _LayerNormRowsFn(torch.autograd.Function):
    """rows of C <= 512 values: several rows per wave (csrc/window.hip)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        C = x.shape[-1]
        rows = x.numel() // C
        y, mean, rstd = ops.layernorm_rows_fwd(x, rows, C, 1, C, 0, gamma, beta, eps)
        ctx.save_for_backward(x, gamma, mean, rstd)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, rstd = ctx.saved_tensors
        C = x.shape[-1]
        rows = x.numel() // C
        want = gamma is not None and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        dx = torch.empty_like(x)
        dg, db = ops.layernorm_rows_bwd(x, dy.contiguous(), gamma, mean, rstd, rows, C, 1, C, 0,
                                        dx, C, 0, want)
        return dx, dg, db, None


def layer_norm(x, gamma=None, beta=None, eps=1e-5):
    """torch.nn.LayerNorm over the last dimension."""
    if x.shape[-1] <= 512:
        return _LayerNormRowsFn.apply(x.contiguous(), gamma, beta, float(eps))
    return _LayerNormFn.apply(x.contiguous(), gamma, beta, float(eps))


# ---- gather-based rearranges (SWIN: window partition / merge, cyclic shift, rescale) -----
def _inverse_gather(dims, axes):
    """Spec of the inverse of a bijective gather whose input is dense over ``axes`` (listed
    outermost first): (inverse dims, inverse axes, roll spec or None)."""
    nd = len(dims)
    out_strides = [1] * nd
    for d in range(nd - 2, -1, -1):
        out_strides[d] = out_strides[d + 1] * dims[d + 1][0]
    inv_dims = []
    for a, (extent, _, _) in enumerate(axes):
        feed = sorted([d for d in range(nd) if dims[d][1] == a], key=lambda d: -dims[d][2])
        run = 1
        for d in reversed(feed):
            if dims[d][2] != run:
                raise ValueError("gather is not a mixed-radix bijection")
            run *= dims[d][0]
        if run != extent:
            raise ValueError("gather does not cover its input axis")
        inv_dims += [(dims[d][0], d, 1) for d in feed]
    inv_axes = [(dims[d][0], out_strides[d], 0) for d in range(nd)]
    roll = None
    if any(a[2] != 0 for a in axes):
        roll = ([(a[0], i, 1) for i, a in enumerate(axes)],
                [(a[0], a[1], -a[2]) for a in axes])
    return inv_dims, inv_axes, roll


class _GatherFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dims, axes, out_shape):
        ctx.spec = (dims, axes, x.shape)
        return ops.gather_nd(x, dims, axes).view(out_shape)

    @staticmethod
    def backward(ctx, g):
        dims, axes, in_shape = ctx.spec
        inv_dims, inv_axes, roll = _inverse_gather(dims, axes)
        gi = ops.gather_nd(g.contiguous(), inv_dims, inv_axes)
        if roll is not None:
            gi = ops.gather_nd(gi, *roll)
        return gi.view(in_shape), None, None, None


def _window_spec(shape, nwin, ppw, patch, shift):
    """shift: cyclic shift of the (X, Y, Z, c) axes of the [b, X, Y, Z, c] input."""
    b, X, Y, Z, c = shape
    (w1, w2, w3), (h, w, d), (px, py, pz) = nwin, ppw, patch
    assert (w1 * h * px, w2 * w * py, w3 * d * pz) == (X, Y, Z), "window grid does not tile the image"
    sx, sy, sz, sc = shift
    if sc % c == 0:
        # the innermost image axis and the channel axis are one dense axis of Z*c elements
        axes = [(b, X * Y * Z * c, 0), (X, Y * Z * c, sx), (Y, Z * c, sy), (Z * c, 1, sz * c)]
        dims = [(b, 0, 1), (w1, 1, h * px), (w2, 2, w * py), (w3, 3, d * pz * c), (h, 1, px),
                (w, 2, py), (d, 3, pz * c), (px, 1, 1), (py, 2, 1), (pz * c, 3, 1)]
    else:
        axes = [(b, X * Y * Z * c, 0), (X, Y * Z * c, sx), (Y, Z * c, sy), (Z, c, sz), (c, 1, sc)]
        dims = [(b, 0, 1), (w1, 1, h * px), (w2, 2, w * py), (w3, 3, d * pz), (h, 1, px),
                (w, 2, py), (d, 3, pz), (px, 1, 1), (py, 2, 1), (pz, 3, 1), (c, 4, 1)]
    return dims, axes


def window_partition(x, nwin, ppw, patch, shift=(0, 0, 0, 0)):
    """einops 'b (w1 h x) (w2 w y) (w3 d z) c -> b (w1 w2 w3) (h w d) (x y z c)' of
    torch.roll(x, [-s for s in shift], dims=(1, 2, 3, 4)) -- one gather (vit.py:650-676,
    1197-1203). ``shift`` covers the three image axes and the channel axis."""
    x = x.contiguous()
    shift = tuple(shift) + (0,) * (4 - len(shift))
    dims, axes = _window_spec(x.shape, nwin, ppw, patch, shift)
    b, c = x.shape[0], x.shape[-1]
    out_shape = (b, nwin[0] * nwin[1] * nwin[2], ppw[0] * ppw[1] * ppw[2],
                 patch[0] * patch[1] * patch[2] * c)
    return _GatherFn.apply(x, dims, axes, out_shape)


def window_merge(tokens, image_shape, nwin, ppw, patch):
    """inverse of window_partition without a shift: [b, nW, T, (x y z c)] -> [b, X, Y, Z, c]."""
    tokens = tokens.contiguous()
    dims, axes = _window_spec(image_shape, nwin, ppw, patch, (0, 0, 0, 0))
    inv_dims, inv_axes, _ = _inverse_gather(dims, axes)
    return _GatherFn.apply(tokens, inv_dims, inv_axes, tuple(image_shape))


def space_to_depth(x, scale):
    """einops_rescale (vit.py:33-45): 'b c (h p1) (w p2) (d p3) -> b (c p1 p2 p3) h w d' for an
    NDHWC activation; returns the logical [b, c*p1*p2*p3, h, w, d] tensor (NDHWC memory)."""
    x = ops.ndhwc(x)
    b, c, H, W, D = x.shape
    p1, p2, p3 = scale
    h, w, d = H // p1, W // p2, D // p3
    axes = [(b, H * W * D * c, 0), (H, W * D * c, 0), (W, D * c, 0), (D, c, 0), (c, 1, 0)]
    dims = [(b, 0, 1), (h, 1, p1), (w, 2, p2), (d, 3, p3), (c, 4, 1), (p1, 1, 1), (p2, 2, 1),
            (p3, 3, 1)]
    xr = x.permute(0, 2, 3, 4, 1)  # [b, H, W, D, c], contiguous
    out = _GatherFn.apply(xr, dims, axes, (b, h, w, d, c * p1 * p2 * p3))
    return out.permute(0, 4, 1, 2, 3)


def conv3d_dilated(x, weight, bias, rate):
    """``Conv3d(kernel_size=3, dilation=rate, padding="same")`` (stride 1) -- the dilated convs of the
    atrous pyramid (multi_resolution.py:392-403). A tap of a dilated kernel reads
    ``x[o + (t - 1) rate]``: output voxel ``o = rate q + p`` only ever meets the sub-lattice of voxels
    congruent to ``p`` (per axis), on which the operation is the PLAIN 3x3x3 convolution with
    padding 1. So: one gather (space-to-batch: the rate^3 sub-lattices become batch items), the
    ordinary conv kernels on a batch of N rate^3 volumes, one inverse gather. Extents that are not
    multiples of ``rate`` are zero-framed at the far end first (``adell_window_ndhwc``; the frame is
    what the conv's own zero padding would be) and the result is cropped back."""
    rate = tuple(int(r) for r in ops._triple(rate))
    x = ops.ndhwc(x)
    if rate == (1, 1, 1):
        return conv3d(x, weight, bias, 1, 1)
    if tuple(weight.shape[2:]) != (3, 3, 3):
        raise NotImplementedError("dilated convolutions: 3x3x3 kernels only")
    N, C, D, H, W = x.shape
    full = tuple(-(-n // r) * r for n, r in zip((D, H, W), rate))
    if full != (D, H, W):
        x = _CropFn.apply(x, full, (0, 0, 0))
    De, He, We = full
    sub = tuple(n // r for n, r in zip(full, rate))

    def spec(ch):
        axes = [(N, De * He * We * ch, 0), (De, He * We * ch, 0), (He, We * ch, 0), (We, ch, 0), (ch, 1, 0)]
        dims = [(N, 0, 1)]
        dims += [(r, a + 1, 1) for a, r in enumerate(rate) if r > 1]                       # the phases
        dims += [(n, a + 1, r) for a, (n, r) in enumerate(zip(sub, rate))] + [(ch, 4, 1)]  # the sub-lattice
        return dims, axes

    phases = rate[0] * rate[1] * rate[2]
    dims, axes = spec(C)
    xb = _GatherFn.apply(x.permute(0, 2, 3, 4, 1), dims, axes, (N * phases, *sub, C))
    yb = conv3d(xb.permute(0, 4, 1, 2, 3), weight, bias, 1, 1, want_stats=False)
    Cout = weight.shape[0]
    odims, oaxes = spec(Cout)
    inv_dims, inv_axes, _ = _inverse_gather(odims, oaxes)
    y = _GatherFn.apply(ops.ndhwc(yb).permute(0, 2, 3, 4, 1).contiguous(), inv_dims, inv_axes,
                        (N, De, He, We, Cout)).permute(0, 4, 1, 2, 3)
    if full != (D, H, W):
        y = _CropFn.apply(y, (D, H, W), (0, 0, 0))
    return y


class _WindowAttnFn(torch.autograd.Function):
    """q-norm, k-norm and windowed attention on a QKV buffer [tokens, H*(2a+hd)] whose heads
    are laid out q | k | v (linear_blocks.py:369-417). Nothing is sliced or permuted: the
    LayerNorm kernel reads the q / k slices in place, the attention kernel reads v in place,
    and the backward writes the three gradients straight into dQKV."""

    @staticmethod
    def forward(ctx, qkv, qg, qb, kg, kb, rel, mask, conf):
        W, H, T, a, hd, scale, drop_p, seed, offset, eps = conf
        per = 2 * a + hd
        ts = H * per
        flat = qkv.view(-1)
        rows = W * T * H
        qn, qm, qr = ops.layernorm_rows_fwd(flat, rows, a, H, ts, per, qg, qb, eps)
        kn, km, kr = ops.layernorm_rows_fwd(flat[a:], rows, a, H, ts, per, kg, kb, eps)
        o, lse = ops.winattn_fwd(qn, kn, flat[2 * a:], ts, per, rel, mask, W, H, T, a, hd, scale,
                                 drop_p, seed, offset)
        ctx.save_for_backward(qkv, qg, kg, qn, kn, qm, qr, km, kr, o, lse, rel, mask)
        ctx.conf = conf
        return o.view(W * T, H * hd)

    @staticmethod
    def backward(ctx, do):
        qkv, qg, kg, qn, kn, qm, qr, km, kr, o, lse, rel, mask = ctx.saved_tensors
        W, H, T, a, hd, scale, drop_p, seed, offset, eps = ctx.conf
        per = 2 * a + hd
        ts = H * per
        rows = W * T * H
        need = ctx.needs_input_grad
        flat = qkv.view(-1)
        dqkv = torch.empty_like(qkv)
        dflat = dqkv.view(-1)
        dqn, dkn = torch.empty_like(qn), torch.empty_like(kn)
        ds = ops.winattn_bwd(qn, kn, flat[2 * a:], ts, per, rel, mask, o, do.contiguous(), lse, W,
                             H, T, a, hd, scale, drop_p, seed, offset, dqn, dkn, dflat[2 * a:],
                             rel is not None and need[5])
        dqg, dqb = ops.layernorm_rows_bwd(flat, dqn, qg, qm, qr, rows, a, H, ts, per, dflat, ts,
                                          per, need[1] or need[2])
        dkg, dkb = ops.layernorm_rows_bwd(flat[a:], dkn, kg, km, kr, rows, a, H, ts, per,
                                          dflat[a:], ts, per, need[3] or need[4])
        drel = None
        if ds is not None:
            drel = ops.bias_grad(_rows_as_volume(ds)).view(rel.shape)
        return dqkv, dqg, dqb, dkg, dkb, drel, None, None


def window_attention(qkv, q_gamma, q_beta, k_gamma, k_beta, n_windows, n_heads, tokens, a, hd,
                     rel=None, mask=None, drop_p=0.0, training=False, eps=1e-5):
    """qkv: [n_windows * tokens, n_heads * (2a + hd)] -> [n_windows * tokens, n_heads * hd]."""
    p = float(drop_p) if training else 0.0
    seed, offset = 0, 0
    if p > 0.0:
        seed = torch.initial_seed()
        offset = next(_dropout_counter)
    conf = (int(n_windows), int(n_heads), int(tokens), int(a), int(hd), 1.0 / (a ** 0.5), p, seed,
            offset, float(eps))
    rel = None if rel is None else rel.contiguous()
    mask = None if mask is None else mask.contiguous()
    return _WindowAttnFn.apply(qkv.contiguous(), q_gamma, q_beta, k_gamma, k_beta, rel, mask, conf)


class _SeqAttnFn(torch.autograd.Function):
    """q-norm, k-norm and full-sequence attention on the projection output [B*T, H*(2a+hd)]
    whose heads are laid out q | k | v (linear_blocks.py:372-417), for the MFMA-shaped heads.
    As in the windowed form nothing is sliced or permuted: the LayerNorm kernel reads the q / k
    slices in place (token-major outputs), the attention kernels address every operand by
    (item, head, row) strides -- V inside the projection, O as [B, T, H*hd] token rows -- and the
    backward writes the three gradients straight into dQKV."""

    @staticmethod
    def _strides(T, H, a, hd):
        per = 2 * a + hd
        tok = (T * H * a, a, H * a)            # [B, T, H, a] token-major q / k (and dq / dk)
        pak = (T * H * per, per, H * per)      # rows inside the packed projection
        out = (T * H * hd, hd, H * hd)         # [B, T, H * hd]
        return tok, pak, out

    @staticmethod
    def forward(ctx, qkv, qg, qb, kg, kb, bias, labels, conf):
        B, H, T, a, hd, scale, drop_p, seed, offset, eps = conf
        per = 2 * a + hd
        flat = qkv.view(-1)
        rows = B * T * H
        qn, qm, qr = ops.layernorm_rows_fwd(flat, rows, a, 1, per, 0, qg, qb, eps)
        kn, km, kr = ops.layernorm_rows_fwd(flat[a:], rows, a, 1, per, 0, kg, kb, eps)
        tok, pak, out = _SeqAttnFn._strides(T, H, a, hd)
        o = torch.empty((B * T, H * hd), device=qkv.device, dtype=torch.float32)
        lse = ops.attention_fwd_strided(qn, kn, flat[2 * a:], o, tok + tok + pak + out, bias, B, H, T,
                                        a, hd, scale, drop_p, seed, offset, labels)
        ctx.save_for_backward(qkv, qg, kg, qn, kn, qm, qr, km, kr, o, lse, bias, labels)
        ctx.conf = conf
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, qg, kg, qn, kn, qm, qr, km, kr, o, lse, bias, labels = ctx.saved_tensors
        B, H, T, a, hd, scale, drop_p, seed, offset, eps = ctx.conf
        per = 2 * a + hd
        rows = B * T * H
        need = ctx.needs_input_grad
        flat = qkv.view(-1)
        dqkv = torch.empty_like(qkv)
        dflat = dqkv.view(-1)
        dqn, dkn = torch.empty_like(qn), torch.empty_like(kn)
        tok, pak, out = _SeqAttnFn._strides(T, H, a, hd)
        do = do.contiguous()
        ops.attention_bwd_strided(qn, kn, flat[2 * a:], o, do, lse, dqn, dkn,
                                  dflat[2 * a:], tok + tok + pak + out + out + tok + tok + pak, bias,
                                  B, H, T, a, hd, scale, drop_p, seed, offset, labels)
        dbias = None
        if bias is not None and need[5]:
            # summed over the sequences that share a slice, never materialised per sequence
            dbias = ops.attention_bias_grad(
                qn, kn, flat[2 * a:], bias, o, do, lse, scale, bias.numel() // (T * T), drop_p, seed,
                offset, labels, strides=tok + tok + pak + out + out,
                dims=(B, H, T, a, hd)).view(bias.shape)
        dqg, dqb = ops.layernorm_rows_bwd(flat, dqn, qg, qm, qr, rows, a, 1, per, 0, dflat, per, 0,
                                          need[1] or need[2])
        dkg, dkb = ops.layernorm_rows_bwd(flat[a:], dkn, kg, km, kr, rows, a, 1, per, 0, dflat[a:],
                                          per, 0, need[3] or need[4])
        return dqkv, dqg, dqb, dkg, dkb, dbias, None, None


def seq_attention_ok(tokens, a, hd):
    """Whether ``seq_attention`` covers these head sizes (otherwise: slices + ``attention``)."""
    return (not FLAGS["no_seq_attention"] and a % 4 == 0 and hd % 4 == 0
            and ops.attention_strided_ok(tokens, a, hd))


def seq_attention(qkv, q_gamma, q_beta, k_gamma, k_beta, batch, n_heads, tokens, a, hd, bias=None,
                  drop_p=0.0, training=False, eps=1e-5, labels=None):
    """qkv: [batch * tokens, n_heads * (2a + hd)] -> [batch * tokens, n_heads * hd]; bias
    [nbias, tokens, tokens] or None is added to the scores of sequence (b, h) as
    bias[(b * n_heads + h) % nbias] (a bias that requires grad gets its gradient, summed over the
    sequences that share a slice); labels int32 [nlab, tokens] or None: item b reads row
    b % nlab, and scores between tokens whose labels differ gain -100 (shifted windows)."""
    p = float(drop_p) if training else 0.0
    seed, offset = 0, 0
    if p > 0.0:
        seed = torch.initial_seed()
        offset = next(_dropout_counter)
    conf = (int(batch), int(n_heads), int(tokens), int(a), int(hd), 1.0 / (a ** 0.5), p, seed,
            offset, float(eps))
    bias = None if bias is None else bias.contiguous()
    return _SeqAttnFn.apply(qkv.contiguous(), q_gamma, q_beta, k_gamma, k_beta, bias, labels, conf)


class _AddBcastFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ctx.bshape = b.shape
        return ops.add_bcast(a, b)

    @staticmethod
    def backward(ctx, g):
        db = None
        if ctx.needs_input_grad[1]:
            same = int(np.prod(ctx.bshape)) == g.numel()
            db = g.reshape(ctx.bshape) if same else ops.sum_bcast(g, ctx.bshape)
        return g, db


def add_bcast(a, b):
    """a + b with b broadcast over a's leading dimensions (positional embedding)."""
    return _AddBcastFn.apply(a, b)


class _AttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, bias, scale, drop, labels, heads):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        ctx.bias_shape = None if bias is None else bias.shape
        if bias is not None:
            # an expanded mask ([1, 1, T, T] -> heads) reshapes to a stride-0 VIEW: the backward
            # must see the same materialised rows the forward used
            bias = bias.contiguous()
        out, lse = ops.attention_fwd(q, k, v, bias, scale, *drop, labels=labels, heads=heads)
        ctx.save_for_backward(q, k, v, bias, out, lse, labels)
        ctx.scale, ctx.drop, ctx.heads = scale, drop, heads
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, bias, out, lse, labels = ctx.saved_tensors
        dout = dout.contiguous()
        dq, dk, dv = ops.attention_bwd(q, k, v, bias, out, dout, lse, ctx.scale, *ctx.drop,
                                       labels=labels, heads=ctx.heads)
        dbias = None
        if bias is not None and ctx.needs_input_grad[3]:
            T = q.shape[1]
            dbias = ops.attention_bias_grad(q, k, v, bias, out, dout, lse, ctx.scale,
                                            bias.numel() // (T * T), *ctx.drop, labels=labels,
                                            heads=ctx.heads).view(ctx.bias_shape)
        return dq, dk, dv, dbias, None, None, None, None


def attention(q, k, v, bias=None, scale=None, drop_p=0.0, training=False, labels=None, heads=1):
    """dropout(softmax(q k^T * scale + bias + label term)) v for q,k [BH,T,A], v [BH,T,Dv]. bias
    [nbias,T,T] (sequence bh reads bias[bh % nbias]; its gradient is the sum over the sequences
    that share a slice); labels int32 [nlab,T] or None: item bh // heads reads row
    (bh // heads) % nlab, scores between tokens whose labels differ gain -100."""
    if scale is None:
        scale = 1.0 / (q.shape[-1] ** 0.5)
    drop = (0.0, 0, 0)
    if training and drop_p > 0:
        drop = (float(drop_p), torch.initial_seed(), next(_dropout_counter))
    return _AttentionFn.apply(q, k, v, bias, float(scale), drop, labels, int(heads))


# ---- data movement with autograd (U-Net++ dense links) ---------------------------------------
class _CatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *tensors):
        ctx.sizes = [t.shape[1] for t in tensors]
        return ops.cat_channels(list(tensors))

    @staticmethod
    def backward(ctx, g):
        return tuple(ops.split_channels(g, ctx.sizes))


def cat_channels(tensors):
    """torch.cat(tensors, 1) for [N,C,D,H,W] activations, staying NDHWC ([N,C,H,W]: depth-1
    volumes)."""
    tensors = list(tensors)
    if len(tensors) == 1:
        return tensors[0]
    if tensors[0].dim() == 4:
        return _CatFn.apply(*[t.unsqueeze(2) for t in tensors]).squeeze(2)
    return _CatFn.apply(*tensors)


def cat_tokens(a, b):
    """torch.cat([a, b], 1) for token tensors [B, T, E] (class token / registers in front of the
    patch tokens, vit.py:871-880): per item the rows are contiguous, so it is the channel concat of
    depth-1 volumes with T * E "channels"."""
    B, E = a.shape[0], a.shape[2]
    y = _CatFn.apply(a.reshape(B, -1, 1, 1, 1), b.reshape(B, -1, 1, 1, 1))
    return y.reshape(B, a.shape[1] + b.shape[1], E)


class _NearestFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, size):
        ctx.in_size = tuple(x.shape[2:])
        return ops.interp_nearest(x, size)

    @staticmethod
    def backward(ctx, g):
        return ops.interp_nearest(g, None, backward_from=ctx.in_size), None


def interpolate_nearest(x, size):
    """F.interpolate(x, size) (default mode='nearest') for 5-D activations."""
    size = tuple(int(s) for s in size)
    if tuple(x.shape[2:]) == size:
        return x
    if x.dim() == 4:
        return _NearestFn.apply(x.unsqueeze(2), (1, *size)).squeeze(2)
    return _NearestFn.apply(x, size)


class _LinearUpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scales):
        ctx.in_size, ctx.scales = tuple(x.shape[2:]), scales
        return ops.interp_linear(x, scales)

    @staticmethod
    def backward(ctx, g):
        return ops.interp_linear(g, ctx.scales, backward_from=ctx.in_size), None


def upsample_linear(x, scale_factor):
    """torch.nn.Upsample(scale_factor, mode="bilinear" (4-D) / "trilinear" (5-D),
    align_corners=False) as used by the "upsample" upscaling path (unet.py:419-443)."""
    nd = x.dim() - 2
    sc = (float(scale_factor),) * nd if not isinstance(scale_factor, (tuple, list)) else \
        tuple(float(s) for s in scale_factor)
    if nd == 2:
        return _LinearUpFn.apply(x.unsqueeze(2), (1.0,) + sc).squeeze(2)
    return _LinearUpFn.apply(x, sc)


def resize_linear_aligned(x, size):
    """F.interpolate(x, size, mode="linear"-family, align_corners=True) for [N, C, *spatial]
    tensors that need no gradient (the deep-supervision targets, pl.py:305-309)."""
    size = [int(v) for v in size]
    x = x.detach()
    nd = x.dim() - 2
    if nd == 3:
        return ops.interp_linear(x, None, size=tuple(size))
    if nd == 2:
        return ops.interp_linear(x.unsqueeze(2), None, size=(1, *size)).squeeze(2)
    return ops.interp_linear(x[:, :, None, None], None, size=(1, 1, *size))[:, :, 0, 0]


class _RowScaleFn(torch.autograd.Function):
    """(gamma[:, None] * W, gamma * b) with its backward, one launch each way (adell_rowscale_*)."""

    @staticmethod
    def forward(ctx, gamma, W, b):
        gamma, W = gamma.contiguous(), W.contiguous()
        C, K = W.shape
        W2 = torch.empty_like(W)
        b2 = None if b is None else torch.empty_like(b)
        ops.check(_lib.lib().adell_rowscale_fwd(ops._ptr(gamma), ops._ptr(W), ops._ptr(b), ops._ptr(W2),
                                                ops._ptr(b2), C, K, ops._stream()))
        ctx.save_for_backward(gamma, W, b)
        return W2, b2

    @staticmethod
    def backward(ctx, dW2, db2):
        gamma, W, b = ctx.saved_tensors
        C, K = W.shape
        dW2 = dW2.contiguous()
        if b is not None and db2 is None:
            db2 = torch.zeros_like(b)
        dgamma, dW = torch.empty_like(gamma), torch.empty_like(W)
        db = None if b is None else torch.empty_like(b)
        ops.check(_lib.lib().adell_rowscale_bwd(
            ops._ptr(gamma), ops._ptr(W), ops._ptr(b), ops._ptr(dW2),
            None if db2 is None else ops._ptr(db2.contiguous()), ops._ptr(dgamma), ops._ptr(dW),
            ops._ptr(db), C, K, ops._stream()))
        return dgamma, dW, db


class _CropFn(torch.autograd.Function):
    """Centre window of a volume as a dense tensor, and a zero frame around the gradient: one launch
    each way (adell_window_ndhwc) where slicing + ``contiguous`` + ``slice_backward`` ran a strided
    copy, three zero-fills and four more strided copies."""

    @staticmethod
    def forward(ctx, x, out_size, offset):
        x = ops.ndhwc(x)
        ctx.in_size, ctx.offset = tuple(x.shape[2:]), tuple(offset)
        return ops.window_ndhwc(x, out_size, offset)

    @staticmethod
    def backward(ctx, dy):
        dy = ops.ndhwc(dy)
        return ops.window_ndhwc(dy, ctx.in_size, tuple(-o for o in ctx.offset)), None, None


def crop3d(x, out_size):
    """crop_to_size of a [N, C, D, H, W] volume (layers/utils.py:30-52: offset ``diff // 2`` per axis)."""
    ops._require_cuda(x)
    offset = [(cur - out) // 2 for cur, out in zip(x.shape[2:], out_size)]
    return _CropFn.apply(x, tuple(int(v) for v in out_size), tuple(offset))


def rowscale(gamma, W, b=None):
    """Layer scale folded into a Linear layer: (gamma[:, None] * W, gamma * b) for W [C, K]."""
    ops._require_cuda(gamma, W, b)
    return _RowScaleFn.apply(gamma, W, b)


class _ScaleBcFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, s):
        ctx.save_for_backward(x, s)
        return ops.scale_bc(x, s)

    @staticmethod
    def backward(ctx, dy):
        x, s = ctx.saved_tensors
        dx = ops.scale_bc(dy, s) if ctx.needs_input_grad[0] else None
        ds = ops.scale_bc_dscale(x, dy) if ctx.needs_input_grad[1] else None
        return dx, ds


def scale_per_item_channel(x, s):
    """x [N, C, *spatial] times s [N, C] broadcast over the spatial axes (feature gates of the
    decoder, unet.py:803-810; U-out, regularization.py:48-55)."""
    nd = x.dim()
    if nd == 5:
        return _ScaleBcFn.apply(x, s)
    if nd == 4:
        return _ScaleBcFn.apply(x.unsqueeze(2), s).squeeze(2)
    if nd == 3:
        return _ScaleBcFn.apply(x.unsqueeze(2).unsqueeze(2), s).squeeze(2).squeeze(2)
    if nd == 2:
        return _ScaleBcFn.apply(x[:, :, None, None, None], s)[:, :, 0, 0, 0]
    raise ValueError(f"scale_per_item_channel: [N, C, ...] with <= 3 spatial dims, got {tuple(x.shape)}")


class _ChannelMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.shape = tuple(x.shape)
        mean, _ = ops.instance_stats(x)
        return mean

    @staticmethod
    def backward(ctx, g):
        V = int(np.prod(ctx.shape[2:]))
        return ops.bcast_nc(g, ctx.shape, 1.0 / V)


def channel_mean(x):
    """[N, C, D, H, W] -> [N, C]: mean over the voxels (torch.flatten(X, 2).mean(-1))."""
    return _ChannelMeanFn.apply(x)


class _CseApplyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, s, c, inv, acc):
        ctx.save_for_backward(x, s, c, inv)
        return ops.cse_apply(x, s, c, inv, acc)

    @staticmethod
    def backward(ctx, dy):
        x, s, c, inv = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx = ds = dc = None
        if need[0] or need[1] or need[2]:
            dx, ds, dc = ops.cse_apply_bwd(x, dy, s, c, inv)
        return (dx if need[0] else None, ds if need[1] else None, dc if need[2] else None, None,
                dy if need[4] else None)


def cse_apply(x, s, c, inv=None, acc=None):
    """acc + x * (s + c) * inv: the concurrent squeeze-and-excite gate (spatial gate s [N,1,D,H,W],
    channel gate c [N,C]) with the branch sum and the division by the summed branch weights of
    BrUNet.forward (unet.py:1186-1207) folded in. inv [N] carries no gradient."""
    return _CseApplyFn.apply(x, s, c, inv, acc)


class _MaxPool3dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel, stride, padding):
        y, idx = ops.maxpool3d_fwd(x, kernel, stride, padding)
        ctx.save_for_backward(idx)
        ctx.conf = (tuple(x.shape), kernel, stride, padding)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        shape, kernel, stride, padding = ctx.conf
        return ops.maxpool3d_bwd(dy, idx, shape, kernel, stride, padding), None, None, None


def max_pool3d(x, kernel, stride=None, padding=0):
    """torch.nn.functional.max_pool3d (ceil_mode=False, dilation=1)."""
    kernel = ops._triple(kernel)
    stride = kernel if stride is None else ops._triple(stride)
    return _MaxPool3dFn.apply(x, kernel, stride, ops._triple(padding))


# ---- ConvNeXt / VICReg ---------------------------------------------------------------------------
class _DwConv3dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        y = ops.dwconv3d_fwd(x, weight, bias)
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx = dw = db = None
        if need[0]:
            dx = ops.dwconv3d_bwd_data(dy, weight)
        if need[1] or (ctx.has_bias and need[2]):
            dw, db = ops.dwconv3d_bwd_weight(x, dy, tuple(weight.shape[2:]), ctx.has_bias)
        return dx, dw, db


def dwconv3d(x, weight, bias=None):
    """Depthwise Conv3d (groups = channels, stride 1, 'same' padding)."""
    return _DwConv3dFn.apply(x, weight, bias)


def channel_scale(x, gamma):
    """gamma[c] * x for a 5-D activation (layer scale of the ConvNeXt block)."""
    return norm_drop_act(x, norm="none", gamma=gamma)


class _VICRegFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x1, x2, min_var, eps):
        x1, x2 = x1.contiguous(), x2.contiguous()
        out, scratch = ops.vicreg_fwd(x1, x2, min_var, eps)
        ctx.save_for_backward(x1, x2, scratch)
        ctx.conf = (min_var, eps)
        return out

    @staticmethod
    def backward(ctx, g):
        x1, x2, scratch = ctx.saved_tensors
        dx1, dx2 = ops.vicreg_bwd(x1, x2, scratch, *ctx.conf, g,
                                  ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return dx1, dx2, None, None


def vicreg_terms(x1, x2, min_var=1.0, eps=1e-4):
    """(invariance, variance, covariance) terms of VICReg, unweighted, as a 3-vector."""
    return _VICRegFn.apply(x1, x2, float(min_var), float(eps))


class _TopPairsFn(torch.autograd.Function):
    """Ranking only: the pairs are a non-differentiable output, the tokens get no gradient."""

    @staticmethod
    def forward(ctx, a, b, gamma):
        pairs = ops.top_pairs(a, b, gamma)
        ctx.mark_non_differentiable(pairs)
        return pairs

    @staticmethod
    def backward(ctx, g):
        return None, None, None


class _TopPairsBoxesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, box1, box2, spatial, gamma):
        pairs = ops.top_pairs_boxes(box1, box2, spatial, gamma)
        ctx.mark_non_differentiable(pairs)
        return pairs

    @staticmethod
    def backward(ctx, g):
        return None, None, None, None


class _GatherRowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pairs, col):
        ctx.save_for_backward(pairs)
        ctx.conf = (col, tuple(x.shape))
        return ops.gather_rows_fwd(x, pairs, col)

    @staticmethod
    def backward(ctx, g):
        (pairs,) = ctx.saved_tensors
        col, shape = ctx.conf
        dx = ops.gather_rows_bwd(g, pairs, col, shape) if ctx.needs_input_grad[0] else None
        return dx, None, None


def top_pairs(a, b, gamma):
    """int32 [B, gamma, 2]: per item the token pairs (i of a, j of b) with the gamma LARGEST
    Euclidean distances between the rows of a and b ([B, T, C]); order (distance descending,
    i * T + j ascending). The T x T matrix is never formed. No gradient."""
    return _TopPairsFn.apply(a, b, int(gamma))


def top_pairs_boxes(box1, box2, spatial, gamma):
    """``top_pairs`` of the token-grid coordinates ``grid * (hi - lo) + lo`` of two boxes
    [B, 2 * ndim]; the boxes get no gradient."""
    return _TopPairsBoxesFn.apply(box1, box2, tuple(int(s) for s in spatial), int(gamma))


def gather_rows(x, pairs, col):
    """[B * gamma, C]: rows ``pairs[b, k, col]`` of x [B, T, C]; the backward adds the rows back in
    a fixed order (duplicates allowed, bit-reproducible)."""
    return _GatherRowsFn.apply(x, pairs, int(col))


# ---- DINO (csrc/dino.hip) -------------------------------------------------------------------------
class _DinoLossFn(torch.autograd.Function):
    """Mean over the rows of the fused DINO cross-entropy. Saved: the inputs and [R, 4] statistics;
    the backward recomputes both probabilities from them."""

    @staticmethod
    def forward(ctx, a, b, centers, t1, t2, teacher_is_scores):
        a, b = a.contiguous(), b.contiguous()
        _, stats, mean = ops.dino_loss_fwd(a, b, centers, t1, t2, teacher_is_scores, want_mean=True)
        ctx.save_for_backward(a, b, centers, stats)
        ctx.conf = (t1, t2, teacher_is_scores)
        return mean

    @staticmethod
    def backward(ctx, g):
        a, b, centers, stats = ctx.saved_tensors
        t1, t2, scores = ctx.conf
        need_a = ctx.needs_input_grad[0]
        need_b = ctx.needs_input_grad[1] and not scores
        if not (need_a or need_b):
            return None, None, None, None, None, None
        da, db = ops.dino_loss_bwd(a, b, centers, stats, t1, t2, None, need_a, need_b, scores,
                                   g_mean=g)
        return da, db, None, None, None, None


def dino_loss(a, b, centers, t1, t2, teacher_is_scores=False):
    """-mean_r sum_k p_t[r, k] log_softmax(a / t1)[r, k] with p_t = softmax((b - centers) / t2), or
    ``b`` as given (``teacher_is_scores``: Sinkhorn-Knopp scores, no gradient to them). The centres
    take no gradient. Inputs of more than two dimensions are rows of their last one."""
    if teacher_is_scores:
        b = b.detach()
    return _DinoLossFn.apply(a, b, None if centers is None else centers.detach(), float(t1),
                             float(t2), bool(teacher_is_scores))


class _L2NormalizeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y, inv = ops.l2_normalize_rows_fwd(x)
        ctx.save_for_backward(y, inv)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, inv = ctx.saved_tensors
        return ops.l2_normalize_rows_bwd(y, dy, inv)


def l2_normalize(x):
    """torch.nn.functional.normalize(x, dim=-1, p=2): x / max(||x||, 1e-12)."""
    return _L2NormalizeFn.apply(x)


class _RowInvNormFn(torch.autograd.Function):
    """s = g / ||v_row||; g is frozen (DINO.initialize_last_layer), so only v gets a gradient."""

    @staticmethod
    def forward(ctx, g, v):
        ctx.save_for_backward(g, v)
        return ops.row_inv_norm_fwd(v, g)

    @staticmethod
    def backward(ctx, ds):
        g, v = ctx.saved_tensors
        if ctx.needs_input_grad[0]:
            raise NotImplementedError("weight_norm_linear: the magnitude g is frozen as the reference "
                                      "freezes it; no kernel computes its gradient")
        return None, (ops.row_inv_norm_bwd(v, g, ds) if ctx.needs_input_grad[1] else None)


class _ColScaleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y0, s):
        ctx.save_for_backward(y0, s)
        return ops.col_scale(y0, s)

    @staticmethod
    def backward(ctx, dy):
        y0, s = ctx.saved_tensors
        dy = dy.contiguous()
        d0 = ops.col_scale(dy, s) if ctx.needs_input_grad[0] else None
        ds = ops.col_scale_dscale(dy, y0) if ctx.needs_input_grad[1] else None
        return d0, ds


def weight_norm_linear(x, g, v):
    """Bias-free Linear under torch's weight_norm (dim 0): x (g v / ||v_row||)^T computed as
    (x v^T) * (g / ||v_row||) -- the GEMM on the raw direction ``v``, then one scale per output
    column. The normalised [out, in] weight is never formed, forward or backward."""
    s = _RowInvNormFn.apply(g, v)
    y0 = linear(x, v)
    lead = y0.shape[:-1]
    return _ColScaleFn.apply(y0.reshape(-1, y0.shape[-1]), s).view(*lead, y0.shape[-1])


class _RowMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.shape = tuple(x.shape)
        return ops.row_mean_fwd(x)

    @staticmethod
    def backward(ctx, g):
        return ops.row_mean_bwd(g, ctx.shape)


def row_mean(x):
    """x.mean(-1)."""
    return _RowMeanFn.apply(x)


# ---- iBOT (csrc/ibot.hip) -------------------------------------------------------------------------
class _MaskTokensFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, token, rows):
        ctx.rows = rows
        return ops.ibot_mask_tokens_fwd(x.contiguous(), rows, token)

    @staticmethod
    def backward(ctx, dy):
        dx, dtoken = ops.ibot_mask_tokens_bwd(dy.contiguous(), ctx.rows, ctx.needs_input_grad[0],
                                              ctx.needs_input_grad[1])
        return dx, dtoken, None


def mask_tokens(x, idx, token):
    """x [B, N, E] with the rows ``idx`` (host indices, sorted and unique, or an ``ops.TokenRows``)
    of every item replaced by ``token`` [E], out of place. The replaced rows pass no gradient to
    ``x``; the token's gradient is their sum. IndexError for an index outside [0, N)."""
    if x.dim() != 3:
        raise ValueError(f"mask_tokens: [B, N, E] expected, got {tuple(x.shape)}")
    return _MaskTokensFn.apply(x, token, ops.token_rows(idx, x.shape[1], x.device))


class _TokenMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, first):
        ctx.conf = (tuple(x.shape), first)
        return ops.ibot_token_sums(x.contiguous(), first, 1.0 / (x.shape[1] - first))

    @staticmethod
    def backward(ctx, g):
        shape, first = ctx.conf
        return ops.ibot_bwd(None, None, None, None, None, g, None, first, "mean", 1.0, 1.0,
                            shape=shape), None


def token_mean(x, class_token=False):
    """x[:, c:].mean(1) for x [B, c + T, K], c = 1 with a class token (which gets a zero gradient)."""
    return _TokenMeanFn.apply(x, int(bool(class_token)))


class _IbotViewFn(torch.autograd.Function):
    """One view of iBOT on the token logits s [B, Tt, K]: the reduced output and the mean masked-row
    DINO loss. Saved: the inputs and [B * M, 4] statistics; the backward takes both incoming
    gradients and writes ds in one launch."""

    @staticmethod
    def forward(ctx, s, y, third, rows, t1, t2, class_token, reduce, scores):
        s, y = s.contiguous(), y.contiguous()
        if reduce == "cls":
            s_red = s[:, 0].contiguous()
        else:
            s_red = ops.ibot_token_sums(s, class_token, 1.0 / (s.shape[1] - class_token))
        teacher = third if scores else y
        _, stats, mean = ops.ibot_loss_fwd(s, teacher, rows, None if scores else third, t1, t2, scores,
                                           want_mean=True)
        ctx.save_for_backward(s, teacher, None if scores else third, stats)
        ctx.conf = (rows, t1, t2, class_token, reduce, scores)
        return s_red, mean

    @staticmethod
    def backward(ctx, d_red, g):
        s, teacher, centers, stats = ctx.saved_tensors
        rows, t1, t2, class_token, reduce, scores = ctx.conf
        if not ctx.needs_input_grad[0]:
            return (None,) * 9
        ds = ops.ibot_bwd(s, teacher, rows, centers, stats, d_red, g, class_token, reduce, t1, t2,
                          scores)
        return (ds,) + (None,) * 8


def ibot_view(s, y, rows, centers_or_scores, t1, t2, class_token, reduce, teacher_is_scores=False):
    """(s_red [B, K], loss_mask): the reduction of the student's token logits s [B, Tt, K] ("cls":
    the class row, "mean": the mean of the patch rows) and DinoLoss over the PATCH rows ``rows``
    (host indices into s[:, c:], c = 1 with a class token; or what ``patch_rows`` made of them) of s
    against the same rows of the teacher y [B, Tt, K], read in place. ``centers_or_scores``: the centres [K] or, with
    ``teacher_is_scores``, the dense [B * M, K] scores of the teacher's masked rows (Sinkhorn-Knopp).
    The teacher takes no gradient. IndexError for a row outside the T patch tokens."""
    if s.dim() != 3 or y.shape != s.shape:
        raise ValueError(f"ibot_view: [B, tokens, K] logits of one shape expected, got "
                         f"{tuple(s.shape)} and {tuple(y.shape)}")
    if reduce not in ("cls", "mean"):
        raise ValueError(f"ibot_view: reduce {reduce!r} (\"cls\" or \"mean\")")
    c = int(bool(class_token))
    if reduce == "cls" and not c:
        raise ValueError("ibot_view: the \"cls\" reduction needs a class token")
    table = patch_rows(rows, s.shape[1], c, s.device)
    third = centers_or_scores
    return _IbotViewFn.apply(s, y.detach(), None if third is None else third.detach(), table,
                             float(t1), float(t2), c, reduce, bool(teacher_is_scores))


def patch_rows(rows, tokens, class_token, device):
    """``ops.TokenRows`` of the rows ``c + rows`` of a [B, tokens, K] tensor for indices ``rows``
    into its ``tokens - c`` patch rows; IndexError, on the host, for an index beyond them (what
    ``a[:, 1:][:, rows]`` raises)."""
    c = int(bool(class_token))
    if isinstance(rows, ops.TokenRows):
        return ops.token_rows(rows, tokens, device)
    if isinstance(rows, torch.Tensor):
        rows = rows.detach().cpu().numpy()
    rows = np.asarray(rows).reshape(-1)
    T = int(tokens) - c
    if rows.size and (int(rows.max()) >= T or int(rows.min()) < 0):
        raise IndexError(f"index {int(rows.max())} is out of bounds for dimension 1 with size {T}")
    return ops.token_rows(rows + c, tokens, device)


# ---- I-JEPA (csrc/ijepa.hip) ----------------------------------------------------------------------
class _GatherTokensFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rows):
        ctx.conf = (rows, x.shape[1])
        return ops.ijepa_gather_fwd(x.contiguous(), rows)

    @staticmethod
    def backward(ctx, dy):
        rows, N = ctx.conf
        return ops.ijepa_gather_bwd(dy.contiguous(), rows, N), None


def gather_tokens(x, rows):
    """``x[:, rows]`` for x [B, N, E] and sorted unique host indices ``rows`` (or an
    ``ops.TokenRows``), the same rows of every item. The backward writes the whole gradient of x in
    one launch (zeros on the rows that were not taken). IndexError, on the host and before any
    launch, for a row outside [0, N)."""
    if x.dim() != 3:
        raise ValueError(f"gather_tokens: [B, N, E] expected, got {tuple(x.shape)}")
    return _GatherTokensFn.apply(x, ops.token_rows(rows, x.shape[1], x.device))


class _PredictorTokensFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e, pos, mask, ctx_rows, tgt_rows):
        ctx.conf = (ctx_rows, tgt_rows, pos.shape[1])
        return ops.ijepa_predictor_fwd(e.contiguous(), pos.contiguous(), mask, ctx_rows, tgt_rows)

    @staticmethod
    def backward(ctx, dout):
        ctx_rows, tgt_rows, T = ctx.conf
        de, dpos, dmask = ops.ijepa_predictor_bwd(dout.contiguous(), ctx_rows, tgt_rows, T,
                                                  *ctx.needs_input_grad[:3])
        return de, dpos, dmask, None, None


def predictor_tokens(e, pos, mask, ctx_rows, tgt_rows):
    """The I-JEPA predictor's input [B, nc + nt, P] in one launch: ``cat([e + pos[:, ctx_rows],
    (mask + pos[:, tgt_rows]).expand(B, -1, -1)], 1)`` for the embedded context e [B, nc, P], the
    positional embedding pos [1, T, P] and the mask token [1, 1, P]; the two (sorted, unique) row
    sets are disjoint. The backward writes the whole gradient of pos."""
    T = pos.shape[1]
    return _PredictorTokensFn.apply(e, pos, mask, ops.token_rows(ctx_rows, T, e.device),
                                    ops.token_rows(tgt_rows, T, e.device))


class _IjepaBlockLossFn(torch.autograd.Function):
    """Saved: pred, h and two floats per target row (mean, rstd)."""

    @staticmethod
    def forward(ctx, pred, h, rows):
        pred, h = pred.contiguous(), h.contiguous()
        loss, stats = ops.ijepa_loss_fwd(pred, h, rows)
        ctx.save_for_backward(pred, h, stats)
        ctx.rows = rows
        return loss

    @staticmethod
    def backward(ctx, g):
        pred, h, stats = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        return ops.ijepa_loss_bwd(pred, h, ctx.rows, stats, g), None, None


def ijepa_block_loss(pred, h, rows):
    """``SmoothL1Loss()(pred, layer_norm(h, (E,))[:, rows])`` for the predictions pred [B, nt, E] of
    one target block and the teacher's raw output h [B, N, E]: neither the normalised h nor the
    gathered target is written. h takes no gradient. IndexError on the host for a row outside
    [0, N)."""
    if pred.dim() != 3 or h.dim() != 3:
        raise ValueError(f"ijepa_block_loss: [B, nt, E] and [B, N, E] expected, got "
                         f"{tuple(pred.shape)} and {tuple(h.shape)}")
    return _IjepaBlockLossFn.apply(pred, h.detach(), ops.token_rows(rows, h.shape[1], h.device))


# ---- masked autoencoder (csrc/mae.hip) ------------------------------------------------------------
class _MaeKeepFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, shuffle):
        ctx.shuffle = shuffle
        return ops.mae_keep_fwd(x.contiguous(), shuffle)

    @staticmethod
    def backward(ctx, dy):
        return ops.mae_keep_bwd(dy.contiguous(), ctx.shuffle), None


def mae_keep_tokens(x, shuffle):
    """``torch.gather(x, 1, ids_keep)`` for x [B, L, E] and an ``ops.MaeShuffle``: the kept tokens
    of every item, in its own shuffled order. The backward writes the whole gradient of x in one
    launch (zeros on the masked tokens)."""
    if x.dim() != 3:
        raise ValueError(f"mae_keep_tokens: [B, L, E] expected, got {tuple(x.shape)}")
    return _MaeKeepFn.apply(x, shuffle)


class _MaeRestoreFn(torch.autograd.Function):
    """Saved: the mask token and its scale (E + 1 floats)."""

    @staticmethod
    def forward(ctx, enc, mask_token, scale, pos, shuffle):
        ctx.shuffle = shuffle
        ctx.save_for_backward(mask_token, scale)
        return ops.mae_restore_fwd(enc.contiguous(), mask_token, scale, pos.contiguous(), shuffle)

    @staticmethod
    def backward(ctx, dout):
        mask_token, scale = ctx.saved_tensors
        need_enc, need_mask, need_scale, need_pos = ctx.needs_input_grad[:4]
        denc, dmask, dscale, dpos = ops.mae_restore_bwd(dout.contiguous(), mask_token, scale,
                                                        ctx.shuffle, need_enc, need_mask,
                                                        need_scale, need_pos)
        if dmask is not None:
            dmask = dmask.view(mask_token.shape)
        if dscale is not None:
            dscale = dscale.view(scale.shape)
        return denc, dmask, dscale, dpos, None


def mae_restore_tokens(enc, mask_token, mask_token_scale, pos, shuffle):
    """The decoder's input [B, L, E] in one launch: ``torch.gather(cat([enc, mask_token_scale *
    mask_token.repeat(B, L - K, 1)], 1), 1, ids_restore) + pos`` for the encoded kept tokens enc
    [B, K, E], the mask token [1, 1, E], its scale [1] (read on the device) and the positional
    embedding pos [1, L, E]. The backward takes at most three launches, every sum in a fixed
    order."""
    if enc.dim() != 3 or pos.dim() != 3:
        raise ValueError(f"mae_restore_tokens: enc [B, K, E] and pos [1, L, E] expected, got "
                         f"{tuple(enc.shape)} and {tuple(pos.shape)}")
    return _MaeRestoreFn.apply(enc, mask_token, mask_token_scale, pos, shuffle)


class _MaeLossFn(torch.autograd.Function):
    """Saved: pred and x, nothing else."""

    @staticmethod
    def forward(ctx, pred, x, patch_elems):
        pred, x = pred.contiguous(), x.contiguous()
        ctx.save_for_backward(pred, x)
        ctx.patch_elems = patch_elems
        return ops.mae_loss_fwd(pred, x, patch_elems)

    @staticmethod
    def backward(ctx, g):
        pred, x = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        return ops.mae_loss_bwd(pred, x, ctx.patch_elems, g), None, None


def mae_reconstruction_loss(pred, x, patch_elems):
    """``MSELoss()(pred.view(B, L, ph, pw, C).permute(0, 4, 1, 2, 3).contiguous().view(B, C, H, W), x)``
    for the token predictions pred [B, L, P * C] (P = ``patch_elems`` = ph * pw) and the image x
    [B, C, H, W], without writing the permuted tensor: element (b, c, l P + p) of the reference's
    "image" is pred[b, l, p C + c]. x takes no gradient."""
    if x.dim() != 4:
        raise ValueError(f"mae_reconstruction_loss: an image [B, C, H, W] expected, got "
                         f"{tuple(x.shape)}")
    return _MaeLossFn.apply(pred, x.detach(), int(patch_elems))


class _MaeToImageFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, image_shape, patch_elems):
        ctx.patch_elems = patch_elems
        return ops.mae_to_image(pred.contiguous(), image_shape, patch_elems)

    @staticmethod
    def backward(ctx, dimage):
        return ops.mae_from_image(dimage.contiguous(), ctx.patch_elems), None, None


def mae_to_image(pred, image_shape):
    """The reference's ``pred.view(B, L, ph, pw, C).permute(0, 4, 1, 2, 3).contiguous().view(B, C, H,
    W)`` for pred [B, L, P * C] and ``image_shape`` (B, C, H, W): not a spatial un-patchify, element
    (b, c) of the result holds pred[b, l, p C + c] at flat offset l P + p. With one channel it is a
    view and nothing is launched."""
    image_shape = tuple(int(v) for v in image_shape)
    if pred.dim() != 3 or len(image_shape) != 4:
        raise ValueError(f"mae_to_image: pred [B, L, P * C] and (B, C, H, W) expected, got "
                         f"{tuple(pred.shape)} and {image_shape}")
    B, C, H, W = image_shape
    L = pred.shape[1]
    if L < 1 or (H * W) % L:
        raise ValueError(f"mae_to_image: {L} tokens do not divide an image of {H} x {W}")
    B, C, L, P = ops._mae_image_shapes("mae_to_image", pred, image_shape, H * W // L)
    if C == 1:
        return pred.reshape(image_shape)
    return _MaeToImageFn.apply(pred, image_shape, P)


class _PairLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x1, x2, kind, temperature, apply_relu):
        x1, x2 = x1.contiguous(), x2.contiguous()
        loss, scratch = ops.pair_loss_fwd(x1, x2, kind, temperature, apply_relu)
        ctx.save_for_backward(x1, x2, scratch)
        ctx.conf = (kind, temperature, apply_relu)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        x1, x2, scratch = ctx.saved_tensors
        dx1, dx2 = ops.pair_loss_bwd(x1, x2, *ctx.conf, scratch, g, ctx.needs_input_grad[0],
                                     ctx.needs_input_grad[1])
        return dx1, dx2, None, None, None


def pair_loss(x1, x2, kind, temperature=1.0, apply_relu=False):
    """Scalar cosine-similarity loss between two [B, D] embedding batches: ``kind`` = "simsiam",
    "byol" (self_supervised/losses/functional.py:138-164) or "ntxent" (losses/ntxent.py:11-46)."""
    return _PairLossFn.apply(x1, x2, kind, float(temperature), bool(apply_relu))


class _LocoLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f1, f2, temperature, eps):
        f1, f2 = ops.ndhwc(f1), ops.ndhwc(f2)
        loss = ops.loco_loss_fwd(f1, f2, temperature, eps)
        ctx.save_for_backward(f1, f2)
        ctx.conf = (temperature, eps)
        return loss

    @staticmethod
    def backward(ctx, g):
        f1, f2 = ctx.saved_tensors
        df1, df2 = ops.loco_loss_bwd(f1, f2, g, *ctx.conf, ctx.needs_input_grad[0],
                                     ctx.needs_input_grad[1])
        return df1, df2, None, None


def loco_loss(f1, f2, temperature=0.1, eps=1e-8):
    """Per-item local contrastive loss [B] between the features of two views [B, C, *spatial]
    (LocalContrastiveLoss.forward, semi_supervised_segmentation/losses.py:498-526)."""
    return _LocoLossFn.apply(f1, f2, float(temperature), float(eps))


class _ChannelSoftmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = ops.channel_softmax_fwd(x)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return ops.channel_softmax_bwd(y, dy)


def channel_softmax(x):
    """torch.nn.Softmax(dim=1) on a [N, C, *spatial] activation (the n_classes > 2 head,
    unet.py:641-655); 4-D inputs are depth-1 volumes."""
    if x.dim() == 4:
        return _ChannelSoftmaxFn.apply(x.unsqueeze(2)).squeeze(2)
    return _ChannelSoftmaxFn.apply(x)


class _ChannelMaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        out, arg = ops.channel_max_fwd(x)
        ctx.save_for_backward(arg)
        ctx.shape = tuple(x.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        (arg,) = ctx.saved_tensors
        return ops.channel_max_bwd(g, arg, ctx.shape)


def channel_max(x):
    """X.flatten(start_dim=2).max(-1).values for a [N, C, *spatial] activation (the pooling in
    front of the bottleneck classifier, unet.py:826-828)."""
    if x.dim() == 4:
        return _ChannelMaxFn.apply(x.unsqueeze(2))
    return _ChannelMaxFn.apply(x)


# ---- classification (csrc/classify.hip) -----------------------------------------------------------
class _ClsLossFn(torch.autograd.Function):
    """(item [B], reduced) of one of the losses on logits. Saved: the logits, the target, the
    weight and the denominator of the reduction."""

    @staticmethod
    def forward(ctx, logits, target, weight, kind, n_classes):
        item, red, aux = ops.cls_loss_fwd(kind, logits, target, weight, n_classes)
        ctx.save_for_backward(logits, target, aux)
        ctx.weight, ctx.kind, ctx.n_classes = weight, kind, n_classes
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(aux)
        return item, red, aux

    @staticmethod
    def backward(ctx, g_item, g_red, _):
        logits, target, aux = ctx.saved_tensors
        dx = None
        if ctx.needs_input_grad[0]:
            if g_red is not None:
                dx = ops.cls_loss_bwd(ctx.kind, logits, target, ctx.weight, ctx.n_classes, g_red,
                                      False, aux)
            if g_item is not None:
                di = ops.cls_loss_bwd(ctx.kind, logits, target, ctx.weight, ctx.n_classes, g_item,
                                      True, aux)
                dx = di if dx is None else dx + di
        return dx, None, None, None, None


def _cls_weight(weight, like):
    if weight is None:
        return None
    return torch.as_tensor(weight).detach().to(device=like.device, dtype=torch.float32)


def bce_with_logits(logits, target, weight=None, reduction="mean"):
    """``torch.nn.functional.binary_cross_entropy_with_logits(logits, target, weight)`` for one logit
    per item (logits [B] or [B, 1]); soft targets allowed; ``weight`` holds 1 or B elements and
    multiplies the item loss (torch's ``weight``, not ``pos_weight``). ``reduction``: "mean" or
    "none". The target takes no gradient."""
    if reduction not in ("mean", "none"):
        raise ValueError(f"bce_with_logits: reduction must be 'mean' or 'none', got {reduction!r}")
    item, red, _ = _ClsLossFn.apply(logits, target.detach(), _cls_weight(weight, logits), "bce", 1)
    return red if reduction == "mean" else item.view(target.shape)


def cross_entropy(logits, target, weight=None, reduction="mean"):
    """``torch.nn.functional.cross_entropy(logits [B, K], target int64 [B], weight [K])``: "mean" is
    sum(w[y] l) / sum(w[y]), "none" the weighted items. A label outside [0, K) is never used as an
    index: that row's loss and gradient are NaN (torch raises instead)."""
    if reduction not in ("mean", "none"):
        raise ValueError(f"cross_entropy: reduction must be 'mean' or 'none', got {reduction!r}")
    item, red, _ = _ClsLossFn.apply(logits, target.detach(), _cls_weight(weight, logits), "ce",
                                    int(logits.shape[-1]))
    return red if reduction == "mean" else item


def ordinal_sigmoidal_loss(pred, target, n_classes, weight=None):
    """The ordinal sigmoidal (CORAL) loss of classification/losses.py:9-62 on pred [B, K - 1] and int64
    labels [B]: the [B] vector -sum_j (logsig(p_j) t_j + (logsig(p_j) - p_j)(1 - t_j)), t_j = [y >= j],
    times ``weight[y]`` when class weights are given. A label outside [0, K) is never used as an
    index: that row's loss and gradient are NaN."""
    item, _, _ = _ClsLossFn.apply(pred, target.detach(), _cls_weight(weight, pred), "ordinal",
                                  int(n_classes))
    return item


class _ClsRocFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pre_bias, target):
        loss, aux = ops.cls_roc_fwd(pre_bias, target)
        ctx.save_for_backward(pre_bias, target, aux)
        return loss

    @staticmethod
    def backward(ctx, g):
        pre_bias, target, aux = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None
        return ops.cls_roc_bwd(pre_bias, target, g, aux), None


def relative_order_consistency(pred, target):
    """classification/losses.py:65-79: over every ordered pair i != j with y_i != y_j, the mean
    BCE-with-logits of p_i - p_j against clamp(y_i - y_j, 0, 1); ``pred`` [B] or [B, 1], int64 labels.
    NaN (value and gradient) when all labels are equal, as the reference's mean over no pairs."""
    return _ClsRocFn.apply(pred, target.detach())


def mixup_rows(x, factor, partner):
    """x[b] * factor[b] + x[partner[b]] * (1 - factor[b]) over a batch x [B, ...], bit for bit torch's
    three-operation expression; a row that is its own partner is returned as it is (a NaN or Inf in
    it stays what it was). Inputs carry no gradient."""
    return ops.cls_mixup(x.detach(), factor, partner)


# ---- multiple-instance classification (csrc/mil.hip) ----------------------------------------------
class _VolumeToSlicesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.n_slices = int(x.shape[-1])
        return ops.mil_volume_to_slices(x)

    @staticmethod
    def backward(ctx, dy):
        return ops.mil_slices_to_volume(dy.contiguous(), ctx.n_slices)


def volume_to_slices(x):
    """``einops.rearrange(x, "b c h w s -> (b s) c h w")`` for a dense volume [B, C, H, W, S]: item
    b * S + s of the result is slice s of item b. For fixed (b, c) a [H W, S] -> [S, H W] transpose,
    tiled through LDS so that both global sides are contiguous; the backward is the inverse copy.
    Both are bit-equal to torch's ``permute().contiguous()``. The slice axis is always the LAST
    one, as in the reference's live ``v_module`` (its ``dim`` argument is only read by the dead
    ``v_module_old``). A non-dense input is refused, not copied."""
    return _VolumeToSlicesFn.apply(x)


class _MilGatedPoolFn(torch.autograd.Function):
    """Saved: the inputs, A, and the arg-max ("max") or the row statistics ("vocabulary")."""

    @staticmethod
    def forward(ctx, feat, hv, hu, w, b, mode):
        pooled, A, saved = ops.mil_pool_fwd(mode, feat, hv, hu, w, b)
        ctx.mode = mode
        ctx.has = (feat is not None, hv is not None, saved is not None)
        keep = [t for t in (feat, hv, hu, w, saved) if t is not None]
        ctx.save_for_backward(A, *keep)
        ctx.set_materialize_grads(False)
        if pooled is None:
            pooled = A.new_empty((A.shape[0], 0))
            ctx.mark_non_differentiable(pooled)
        return pooled, A

    @staticmethod
    def backward(ctx, g, gA):
        A, *rest = ctx.saved_tensors
        rest = list(rest)
        has_feat, has_gate, has_saved = ctx.has
        feat = rest.pop(0) if has_feat else None
        hv, hu, w = (rest.pop(0), rest.pop(0), rest.pop(0)) if has_gate else (None, None, None)
        saved = rest.pop(0) if has_saved else None
        if not has_feat:
            g = None
        if not has_gate:
            gA = None       # A = 1 / S is a constant
        if g is None and gA is None:
            return None, None, None, None, None, None
        dfeat, dhv, dhu, dw, db = ops.mil_pool_bwd(ctx.mode, feat, hv, hu, w, A, saved, g, gA)
        if dw is not None:
            dw = dw.view(w.shape)
        return dfeat, dhv, dhu, dw, db, None


def mil_gated_pool(feat, hv=None, hu=None, w=None, b=None, mode="mean"):
    """(pooled [B, F], A [B, S, 1]) of ``MultipleInstanceClassifier.get_prediction`` in ONE launch:
    A = softmax over the slices of ``W(tanh(V x) * sigmoid(U x))`` from hv = V(x), hu = U(x)
    [B, S, N], the row w ([N] or [1, N]) and the bias b [1] of ``W`` (without them A = 1 / S and no
    gate input is read), and pooled = sum_s feat A ("mean"), max_s feat A ("max": lowest slice on
    a tie, a NaN propagates as in ``torch.max``) or sum_s softmax(feat, -1) A ("vocabulary") for
    feat [B, S, F]. Neither the gate product nor feat * A is written; "max" keeps its int32
    arg-max, "vocabulary" the row max and log-sum, not the softmax matrix. The backward (two
    launches, one without the gate) returns dfeat, dhv, dhu, dw and db and honours a gradient that
    arrives on A; db is whatever the fixed-order sum gives (zero up to rounding)."""
    if mode not in ops.MIL_MODES:
        raise ValueError(f"mil_gated_pool: mode must be one of {sorted(ops.MIL_MODES)}, got {mode!r}")
    if feat is None:
        raise ValueError("mil_gated_pool: feat [B, S, F] expected (mil_attention gives A alone)")
    cont = [None if t is None else t.contiguous() for t in (feat, hv, hu, w, b)]
    return _MilGatedPoolFn.apply(*cont, mode)


def mil_attention(hv, hu, w, b):
    """A [B, S, 1] alone (``MILAttention.calculate_attention`` behind its two Linear layers): the
    same kernel as ``mil_gated_pool`` without features."""
    cont = [t.contiguous() for t in (hv, hu, w, b)]
    return _MilGatedPoolFn.apply(None, *cont, "mean")[1]


class _SliceTokensFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pos, class_token):
        ctx.n_slices = int(x.shape[1])
        ctx.has_class_token = class_token is not None
        return ops.mil_slice_tokens_fwd(x, pos, class_token)

    @staticmethod
    def backward(ctx, dout):
        need = ctx.needs_input_grad
        return ops.mil_slice_tokens_bwd(dout.contiguous(), ctx.n_slices, ctx.has_class_token,
                                        need[0], need[1], need[2] and ctx.has_class_token)


def slice_tokens(x, pos=None, class_token=None):
    """The token rows of ``TransformableTransformer``: ``cat([class_token.expand(B, 1, E), x + pos],
    1)`` for x [B, S, E], pos [1, S, 1] (one scalar per slice, broadcast over the features; None:
    nothing added) and class_token [1, 1, E] (None: no row in front); one launch, bit-equal to
    torch's add and cat. The backward writes dx whole in one launch with dpos and dclass_token,
    their sums over the batch in order in fp64."""
    return _SliceTokensFn.apply(x.contiguous(), None if pos is None else pos.contiguous(),
                                None if class_token is None else class_token.contiguous())


# ---- 3-D object detection (csrc/detect.hip) --------------------------------------------------------
class _DetectionLossFn(torch.autograd.Function):
    """Saved: the three heads (the network's own outputs, no copy), the table and its count."""

    @staticmethod
    def forward(ctx, centre, size, obj, target, anchors, corr, iou_threshold, first_channel):
        table, count = ops.det_positive_table(target, obj.shape[1], iou_threshold, first_channel)
        out, rows = ops.det_loss_fwd(centre, size, obj, target, anchors, table, count, corr, first_channel)
        ctx.save_for_backward(centre, size, obj, target, anchors, table, count)
        ctx.corr, ctx.first_channel = corr, first_channel
        ctx.mark_non_differentiable(out, rows, table, count)
        return out[0], out, rows, table, count

    @staticmethod
    def backward(ctx, g, *_):
        centre, size, obj, target, anchors, table, count = ctx.saved_tensors
        dc, ds, do = ops.det_loss_bwd(centre, size, obj, target, anchors, table, count, ctx.corr,
                                      g.contiguous().view(1), ctx.first_channel)
        return dc, ds, do, None, None, None, None, None


def detection_loss(centre, size, objectness, target, anchors, correction_factor, iou_threshold=0.5,
                   first_channel=1, return_parts=False):
    """The loss of ``YOLONet3dPL.step`` with ``complete_iou_loss`` and ``F.binary_cross_entropy`` from
    the heads as the network returns them -- centre and size [B, 3 A, H, W, D] (anchor a: channels
    [3 a, 3 a + 3)), objectness [B, A, H, W, D] -- and the anchor map ``target`` [B, first_channel +
    7 A, H, W, D], all read in place: the positive cells (target objectness > ``iou_threshold``) are
    tabulated on the device in ``torch.where``'s order, their boxes decoded (cell index added,
    ``correction_factor`` (three host floats), ``exp(size) * anchor / 2``), complete IoU taken, and the
    objectness cross-entropy summed against a target of ``iou`` at the positives and 0 elsewhere:
    ``bce_mean + 0.1 * (mean(1 - iou) + mean(cpd) + mean(ar))``. Fixed-order fp64 sums: two runs are
    bit-equal. The positive count never leaves the device. With no positive cell the result is NaN,
    as the reference's means of empty tensors, and the objectness gradient is the cross-entropy's.
    The backward returns gradients for the three heads, including the cross-entropy's gradient
    through its TARGET (``iou`` is not detached in the reference). ``return_parts``: also (parts [5] = loss, bce, mean(1 - iou),
    mean(cpd), mean(ar); rows [4, cells] = iou, cpd, ar, bce correction per positive; table; count)."""
    corr = tuple(float(v) for v in correction_factor)
    if len(corr) != 3:
        raise ValueError(f"detection_loss: three correction factors expected, got {corr}")
    anchors = anchors.detach().reshape(-1).to(torch.float32).contiguous()
    loss, parts, rows, table, count = _DetectionLossFn.apply(
        centre, size, objectness, target, anchors, corr, float(iou_threshold), int(first_channel))
    if return_parts:
        return loss, parts, rows, table, count
    return loss


def detection_nms(boxes, scores, score_threshold, iou_threshold=0.5):
    """``nms_nd(..., suppress=True)`` on the device: the indices into ``boxes`` [n, 6] that survive,
    in descending score order. Scores are thresholded and sorted by torch on the device (a stable
    sort of the reference's flipped ascending order), the pairwise mask and the sweep are HIP;
    the candidate count is read once on the host."""
    idx = torch.nonzero(scores > score_threshold).flatten()
    # argsort(scores).flip(0) of the reference: ascending stable order reversed
    order = torch.argsort(scores[idx], stable=True).flip(0)
    idx = idx[order]
    if idx.numel() == 0:
        return idx
    if idx.numel() > ops.det_nms_max():
        raise ValueError(f"detection_nms: {idx.numel()} candidates above the score threshold, at most "
                         f"{ops.det_nms_max()}")
    keep = ops.det_nms_keep(boxes[idx].to(torch.float32).contiguous(), iou_threshold)
    return idx[keep.bool()]


def detection_decode(centre, size, objectness, class_pred, anchors, correction_factor=None):
    """``YOLONet3d.recover_boxes`` before its NMS / top-1000 tail for a whole batch, from the heads in
    place: per image the cells with objectness > 0.5 in ``torch.where``'s order -> a list of
    (boxes [n, 6], scores [n], classes [n, C] or [n]); ``class_pred`` None: the classes are the
    objectness values (the reference's ``n_classes == 2``). Four launches, one host read (the
    per-image row ranges)."""
    A = objectness.shape[1]
    corr = (1.0, 1.0, 1.0) if correction_factor is None else tuple(float(v) for v in correction_factor)
    anchors = anchors.detach().reshape(-1).to(torch.float32).contiguous()
    table, count = ops.det_positive_table(objectness, A, 0.5, 0, 1)
    boxes, scores, classes, starts = ops.det_decode(centre, size, objectness, class_pred, anchors, table,
                                                    count, corr)
    st = starts.tolist()
    return [(boxes[lo:hi], scores[lo:hi], classes[lo:hi]) for lo, hi in zip(st[:-1], st[1:])]


# ---- DDPM diffusion (csrc/diffusion.hip) ---------------------------------------------------------
def _eca_site_params(site):
    """The eight parameter tensors of an ``EfficientConditioningAttentionBlock(op_type="linear")`` in
    the kernels' order."""
    return (site.class_to_channels.weight, site.class_to_channels.bias, site.op[1].weight,
            site.op[1].bias, site.op[2].weight, site.op[2].bias, site.op[4].weight, site.op[4].bias)


class _EcaGatesFn(torch.autograd.Function):
    """Outputs: one [Ng, C] logits tensor per site. Inputs: t, the class-embedding rows (or None),
    LayerNorm's eps, the site count, then eight parameters per site."""

    @staticmethod
    def forward(ctx, t, cls, eps, n_sites, *flat):
        params = [tuple(flat[8 * i:8 * i + 8]) for i in range(n_sites)]
        zs, (emb, recs) = ops.eca_gates_fwd(t, cls, params, eps)
        ctx.save_for_backward(emb, *recs, *flat)
        ctx.n_sites = n_sites
        ctx.set_materialize_grads(False)
        return tuple(zs)

    @staticmethod
    def backward(ctx, *gzs):
        n = ctx.n_sites
        emb, recs, flat = ctx.saved_tensors[0], ctx.saved_tensors[1:1 + n], ctx.saved_tensors[1 + n:]
        params = [tuple(flat[8 * i:8 * i + 8]) for i in range(n)]
        gzs = [None if g is None else g.contiguous() for g in gzs]
        grads, de = ops.eca_gates_bwd(params, (emb, list(recs)), gzs, ctx.needs_input_grad[1])
        return (None, de, None, None) + tuple(g for site in grads for g in site)


def timestep_embedding(t, channels, max_period=10000):
    """``get_timestep_embedding`` (modules/diffusion/unet.py) in torch ops, its arithmetic in fp64 and
    the result rounded to fp32 once, as the gate kernel evaluates it: cos half, sin half, zero pad
    for an odd ``channels``; ``channels == 1`` gives zeros. ``t`` [G] or [G, 1] -> [G, channels]."""
    t = t.reshape(-1).to(torch.float32).double()
    half = channels // 2
    k = torch.arange(half, dtype=torch.float64, device=t.device)
    args = t[:, None] * torch.exp(-math.log(max_period) * k / max(half, 1))[None, :]
    emb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    if channels % 2 == 1:
        emb = torch.nn.functional.pad(emb, (0, 1, 0, 0))
    return emb.float()


def _eca_gates_composed(t, sites, cls_embedding):
    """The same logits from the package's Linear / LayerNorm / activation kernels, site by site."""
    T = sites[0].class_dimension
    emb = cls_embedding if t is None else timestep_embedding(t, T)
    if t is not None and cls_embedding is not None:
        emb = emb + cls_embedding
    out = []
    for site in sites:
        w0, b0, w1, b1, lg, lb, w2, b2 = _eca_site_params(site)
        h = elementwise(linear(emb, w0, b0), "silu")
        h = layer_norm(linear(h, w1, b1), lg, lb, site.op[2].eps)
        out.append(linear(elementwise(h, "silu"), w2, b2))
    return out


def eca_gates(t, sites, cls_embedding=None):
    """Pre-sigmoid gate logits ``z_site`` [G, C_site] of every ``EfficientConditioningAttentionBlock``
    (``op_type="linear"``) in ``sites`` for the timesteps ``t`` ([G] or [G, 1], a fraction or an
    integer step count; moved to the parameters' device): the sinusoidal embedding of
    ``get_timestep_embedding`` (evaluated in fp64, rounded to fp32 once), ``+ cls_embedding[g]``
    ([G, t_dim], the rows ``Embedding(cls)``; with one timestep and several class rows the timestep
    serves them all), then per site ``class_to_channels`` -> SiLU -> Linear -> LayerNorm -> SiLU ->
    Linear. ``t`` None: the embedding is ``cls_embedding`` alone (a stand-alone block's conditioning
    vector). One grouped launch forward, two backward, for all sites; the backward returns the
    gradients of every site's eight parameters and of ``cls_embedding``, summed over G in a fixed
    order. ``t`` gets no gradient.

    Up to 32 sites of at most 1024 channels and ``t_dim <= 1024`` take the grouped kernels. Anything
    beyond composes the same values from ``functional.linear`` / ``layer_norm`` / ``elementwise``,
    site by site (several launches per site; the embedding in torch ops)."""
    sites = list(sites)
    if not sites:
        return []
    params = [_eca_site_params(s) for s in sites]
    dev = params[0][0].device
    if t is not None:
        t = t.to(dev).reshape(-1).to(torch.float32)
    T = int(params[0][0].shape[1])
    if any(int(p[0].shape[1]) != T for p in params):
        raise ValueError("eca_gates: the sites read one embedding, their class_dimension must agree")
    eps = {float(s.op[2].eps) for s in sites}
    widest = max(int(p[0].shape[0]) for p in params)
    if (len(sites) > ops.ECA_MAX_SITES or widest > ops.ECA_MAX_DIM or T > ops.ECA_MAX_DIM
            or len(eps) > 1):
        ops._dif_layout("eca_gates", t, cls_embedding)
        return _eca_gates_composed(t, sites, cls_embedding)
    cls = None if cls_embedding is None else cls_embedding.contiguous()
    flat = [p for site in params for p in site]
    return list(_EcaGatesFn.apply(t, cls, eps.pop(), len(sites), *flat))


def _as_channels_last(what, x):
    """``x`` itself when its memory is dense channels-last; a dense row-major tensor is copied to
    that layout (the conv kernels never produce one); a view with gaps is refused."""
    if x.dim() not in (4, 5):
        raise ValueError(f"{what}: [N, C, H, W] or [N, C, D, H, W] expected, got {tuple(x.shape)}")
    fmt = torch.channels_last_3d if x.dim() == 5 else torch.channels_last
    if x.is_contiguous(memory_format=fmt):
        return x
    if x.is_cuda and not x.is_contiguous():
        raise ops.AdellHipError(f"{what}: non-dense tensor handed to a kernel: shape {tuple(x.shape)}, "
                                f"strides {x.stride()}")
    return x.contiguous(memory_format=fmt)


class _EcaApplyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, z):
        ctx.save_for_backward(x, z)
        return ops.eca_apply_fwd(x, z)

    @staticmethod
    def backward(ctx, dy):
        x, z = ctx.saved_tensors
        dy = _as_channels_last("eca_apply backward", dy)
        return ops.eca_apply_bwd(x, z, dy, ctx.needs_input_grad[0], ctx.needs_input_grad[1])


def eca_apply(x, z):
    """``x * sigmoid(z)`` for an activation ``x`` [N, C, *spatial] (2 or 3 spatial axes, channels-last
    memory as the conv kernels leave it) and gate logits ``z`` [Ng, C] with Ng in {1, N}: one gate
    row is broadcast over the batch inside the kernel. One launch forward. Backward: one pass over
    ``x`` and ``dy`` writes ``dx = dy * s`` and fp64 partial sums of ``dy * x``, a small second
    kernel folds them in a fixed order into ``dz = s (1 - s) sum`` (over the items too when Ng is
    1) -- three full-size tensor passes where ``scale_per_item_channel`` makes four."""
    x = _as_channels_last("eca_apply", x)
    return _EcaApplyFn.apply(x, z)


def diffusion_noise(x, epsilon, alpha_bar, t):
    """``sqrt(alpha_bar[t_n]) * x + sqrt(1 - alpha_bar[t_n]) * epsilon`` per item in one launch
    (``Diffusion.noise_images``). ``alpha_bar`` fp32 [noise_steps] and ``t`` int64 [N] live on the
    device and are read by the kernel; a ``t`` outside ``[0, noise_steps)`` is never used as an index
    and makes that item NaN. No autograd: ``x`` and ``epsilon`` are data."""
    return ops.diffusion_noise(x.detach(), epsilon.detach(), alpha_bar, t)


DIFFUSION_STEP_KINDS = ("ddpm", "ddim", "alpha_deblending")


def diffusion_step_coefficients(kind, t, tables, eta=1.0, clip=True):
    """Host fp64 scalars of one reverse step: ((sb, sa, c_x0, c_x, c_e, c_n), flags) such that
    ``out = c_x x + c_e e + c_x0 x0 + c_n noise`` with ``x0 = (x - sb e) / sa`` (clamped to [-1, 1]
    under the CLIP flag) restates ``ddpm_reverse_step`` / ``ddim_reverse_step`` /
    ``alpha_deblending_step`` of the reference. ``tables``: host sequences "beta", "alpha",
    "alpha_bar"."""
    if kind not in DIFFUSION_STEP_KINDS:
        raise ValueError(f"diffusion_reverse_step: kind must be one of {DIFFUSION_STEP_KINDS}, got {kind!r}")
    t = int(t)
    n = len(tables["alpha_bar"])
    if not 0 <= t < n:
        raise ValueError(f"diffusion_reverse_step: t = {t} outside [0, {n})")
    ab = float(tables["alpha_bar"][t])
    abp = float(tables["alpha_bar"][t - 1]) if t > 0 else 1.0        # alpha_bar_prev = 1 at t = 0
    beta, alpha = float(tables["beta"][t]), float(tables["alpha"][t])
    sb, sa = math.sqrt(1.0 - ab), math.sqrt(ab)
    if kind == "ddpm":
        bb = 1.0 - ab
        c_n = 0.0
        if t > 0 and eta > 0:
            c_n = math.sqrt((1.0 - abp) / (1.0 - ab) * beta) * eta
        flags = ops.DIFFUSION_X0 | (ops.DIFFUSION_CLIP if clip is True else 0)
        return (sb, sa, math.sqrt(abp) * beta / bb, math.sqrt(alpha) * (1.0 - abp) / bb, 0.0, c_n), flags
    if kind == "ddim":
        var = math.sqrt((1.0 - abp) / (1.0 - ab)) * math.sqrt(1.0 - ab / abp) * eta
        return (sb, sa, math.sqrt(abp), 0.0, math.sqrt(max(1.0 - abp - var ** 2, 0.0)), var), \
            ops.DIFFUSION_X0
    return (sb, sa, 0.0, 1.0, ab - abp, 0.0), 0


def diffusion_reverse_step(kind, x, eps, t, tables, noise=None, eps_uncond=None, scale=0.0, eta=1.0,
                           clip=True):
    """One reverse-diffusion step in one launch. ``kind``: "ddpm", "ddim" or "alpha_deblending",
    as ``Diffusion.ddpm_reverse_step`` / ``ddim_reverse_step`` / ``alpha_deblending_step`` write them
    (``alpha_bar_prev = 1`` at ``t = 0``; the [-1, 1] clamp of ``x_orig`` in DDPM only, under
    ``clip``; ``clamp(1 - alpha_bar_prev - var^2, min=0)`` in DDIM; DDPM adds no noise when ``t == 0``
    or ``eta <= 0``). With ``eps_uncond`` the guidance blend ``eps_uncond + scale * (eps -
    eps_uncond)`` is folded into the same launch. ``t`` is a Python int; the scalar coefficients are
    computed here in fp64 from ``tables``, host copies of "beta", "alpha" and "alpha_bar", so the
    step reads nothing back from the device. ``noise`` is required where the step's noise
    coefficient is not zero. All tensors share one dense layout."""
    coef, flags = diffusion_step_coefficients(kind, t, tables, eta, clip)
    if coef[5] != 0.0 and noise is None:
        raise ValueError(f"diffusion_reverse_step: the {kind} step at t = {t}, eta = {eta} adds noise; "
                         "pass it")
    if coef[5] == 0.0:
        noise = None
    return ops.diffusion_reverse_step(x.detach(), eps.detach(),
                                      None if eps_uncond is None else eps_uncond.detach(),
                                      noise, coef, scale, flags)


class _MseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        ctx.save_for_backward(pred, target)
        return ops.mse_fwd(pred, target)

    @staticmethod
    def backward(ctx, g):
        pred, target = ctx.saved_tensors
        return ops.mse_bwd(pred, target, g.contiguous()), None


def mse_loss(pred, target):
    """``torch.nn.MSELoss()``: the mean of ``(pred - target)^2`` over all elements, a 0-d device
    tensor. Forward: one launch, fp64 partial sums per block folded in index order by the block
    that finishes last. Backward: one launch (gradient of ``pred`` only: the target is data). The
    MAE reconstruction loss's kernels (``mae_reconstruction_loss``) index patch tokens and need a
    copy to be reached from an image, so this is a kernel of its own. A ``target`` in the other
    dense layout than ``pred`` (row-major noise against a channels-last prediction) is copied to
    the prediction's layout first."""
    target = target.detach()
    if pred.is_cuda and target.is_cuda and pred.dim() in (4, 5) and pred.shape == target.shape:
        fmt = torch.channels_last_3d if pred.dim() == 5 else torch.channels_last
        if pred.is_contiguous(memory_format=fmt) and not pred.is_contiguous():
            target = target.contiguous(memory_format=fmt)
        elif pred.is_contiguous() and not target.is_contiguous():
            target = target.contiguous()
    return _MseFn.apply(pred, target).reshape(())


# ---- ensemble classifiers and the Gaussian-process head (csrc/ensemble.hip) ---------------------------
gp_route = ops.gp_route


class _GpPhiFn(torch.autograd.Function):
    """(logits, phi) of the fused route: one launch forward, at most two backward. W and b are
    buffers: no gradient."""

    @staticmethod
    def forward(ctx, x, gamma, beta, W, b, weights, scale, eps):
        phi, logits, mean, rstd = ops.gp_phi_fwd(x, gamma, beta, W, b, weights, scale, eps)
        ctx.save_for_backward(x, gamma, beta, W, b, weights, phi, mean, rstd)
        ctx.consts = (scale, eps)
        ctx.set_materialize_grads(False)
        return logits, phi

    @staticmethod
    def backward(ctx, dlogits, dphi):
        x, gamma, beta, W, b, weights, phi, mean, rstd = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx, dgamma, dbeta, dweights = ops.gp_phi_bwd(
            x, gamma, beta, W, b, weights, phi, mean, rstd, dlogits, dphi, *ctx.consts,
            need_x=need[0], need_norm=need[1] or need[2], need_weights=need[5])
        return dx, dgamma, dbeta, None, None, dweights, None, None


class _GpCosFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, b, scale):
        ctx.save_for_backward(t, b)
        ctx.scale = scale
        return ops.gp_cos(t, b, scale)

    @staticmethod
    def backward(ctx, dphi):
        t, b = ctx.saved_tensors
        return ops.gp_cos(t, b, ctx.scale, dphi=dphi.contiguous()), None, None


def gp_phi(x, gamma, beta, W, b, weights, scale, eps=1e-5, route=None):
    """(logits [N, o], phi [N, r]) of the Gaussian-process layer on rows x [N, i]: x^ = LayerNorm(x)
    (``gamma`` / ``beta`` None: x), phi = scale cos(b - W x^), logits = phi weights^T. ``route``:
    None asks ``gp_route``; "fused" is one launch, "composed" the layer norm and the two GEMMs of
    ``layer_norm`` / ``linear`` around the cos epilogue."""
    if x.dim() != 2:
        raise NotImplementedError(f"gp_phi: rows [N, in_channels] expected, got {tuple(x.shape)}: "
                                  "inputs of rank above 2 are not built")
    R, I = int(W.shape[-2]), int(W.shape[-1])
    route = gp_route(x.shape[0], I, R) if route is None else route
    x = x.contiguous()
    if route == "fused":
        return _GpPhiFn.apply(x, gamma, beta, W, b, weights, float(scale), float(eps))
    if route != "composed":
        raise ValueError(f"gp_phi: route {route!r} is neither 'fused' nor 'composed'")
    xh = x if gamma is None else layer_norm(x, gamma, beta, eps)
    phi = _GpCosFn.apply(linear(xh, W.reshape(R, I)), b, float(scale))
    return linear(phi, weights), phi


class _EnsemblePoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *members):
        out, arg = ops.ensemble_pool_fwd(members)
        ctx.save_for_backward(arg)
        ctx.shapes = [tuple(m.shape) for m in members]
        return out

    @staticmethod
    def backward(ctx, g):
        (arg,) = ctx.saved_tensors
        return tuple(ops.ensemble_pool_bwd(g, arg, ctx.shapes, ctx.needs_input_grad))


def ensemble_pool(members):
    """``torch.concat([m.flatten(start_dim=2).max(-1).values (or m itself when [B, C]) for m in
    members], 1)``: one launch each way for up to ``ops.ENSEMBLE_MAX`` members; more are composed
    from ``channel_max`` and the concat copy."""
    members = [m.contiguous() if m.dim() == 2 else
               m.contiguous(memory_format=torch.channels_last if m.dim() == 4
                            else torch.channels_last_3d) for m in members]
    if len(members) <= ops.ENSEMBLE_MAX:
        return _EnsemblePoolFn.apply(*members)
    pooled = [m if m.dim() == 2 else channel_max(m) for m in members]
    B = pooled[0].shape[0]
    return _CatFn.apply(*[p.reshape(B, -1, 1, 1, 1) for p in pooled]).reshape(B, -1)


class _EnsembleAverageFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *logits):
        y = ops.ensemble_average_fwd(logits)
        ctx.save_for_backward(y)
        ctx.K = len(logits)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return tuple(ops.ensemble_average_bwd(y, dy, ctx.K, ctx.needs_input_grad))


def ensemble_average(logits):
    """sigmoid (one column) or softmax over dim 1 of ``sum(logits) / len(logits)`` for logit tensors
    [B, C]; one launch each way, up to ``ops.ENSEMBLE_MAX`` members."""
    logits = [x.contiguous() for x in logits]
    if len(logits) > ops.ENSEMBLE_MAX:
        raise NotImplementedError(f"ensemble_average: {len(logits)} members, at most "
                                  f"{ops.ENSEMBLE_MAX} are built")
    return _EnsembleAverageFn.apply(*logits)


# ---- batch-ensemble layers (csrc/batch_ensemble.hip) -----------------------------------------------------
# The eval mean's "batched" route puts members side by side in one batch; a chunk of members is sized
# so that the expanded batch stays inside this many bytes (docs/LABBOOK.md, "Batch ensembles").
BE_BATCH_BUDGET_BYTES = 256 << 20
BE_ROUTES = ("batched", "loop")


def _be_dense(what, x):
    """Rows [B, C] as they are (dense), activations as dense channels-last memory."""
    if x.dim() == 2:
        return x.contiguous()
    return _as_channels_last(what, x)


def be_indices(idx, n, batch, device):
    """The int32 [batch] device tensor ``be_scale`` reads, from host indices (a sequence or a numpy
    array of ``batch`` entries). A negative entry wraps as torch indexing does; one outside
    ``[-n, n)`` raises ``IndexError`` here, on the host, before any kernel. One upload, without a
    host synchronisation."""
    host = np.asarray(idx)
    if host.ndim != 1 or host.dtype.kind not in "iu":
        raise TypeError(f"be_indices: a sequence of integers expected, got {idx!r}")
    assert len(host) == batch, "len(idx) must be == X.shape[0]"
    host = host.astype(np.int64)
    bad = (host < -n) | (host >= n)
    if bad.any():
        raise IndexError(f"index {int(host[bad][0])} is out of bounds for dimension 0 with size {n}")
    staged = torch.from_numpy(np.where(host < 0, host + n, host).astype(np.int32))
    if torch.device(device).type != "cuda":
        return staged.to(device)
    # through pinned memory: the copy is queued behind the stream and the host does not wait
    return staged.pin_memory().to(device, non_blocking=True)


class _BeScaleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, table, idx):
        ctx.save_for_backward(x, table, idx)
        return ops.be_expand(x, table, idx)

    @staticmethod
    def backward(ctx, dy):
        x, table, idx = ctx.saved_tensors
        dy = _be_dense("be_scale backward", dy)
        dx, dt = ops.be_tgrad(dy, x, int(table.shape[0]), table=table, idx=idx,
                              need_x=ctx.needs_input_grad[0], need_t=ctx.needs_input_grad[1])
        return dx, dt, None


def be_scale(x, table, idx=None):
    """``y[b, c, v] = x[b, c, v] * table[idx[b], c]`` for an activation ``x`` [B, C, *spatial]
    (channels-last memory) or rows [B, C], a table [n, C] and ``idx`` an int32 [B] device tensor
    (``be_indices``); ``idx=None``: row 0 for every item, broadcast inside the kernel. One launch
    forward. Backward: one pass over ``x`` and ``dy`` writes ``dx = dy * table[idx[b]]`` and fp64
    partial sums of ``dy * x``, a small fold sums them into ``dtable`` per member over the items that
    drew it, in item order (a member nobody drew: an exact 0 row). An index outside ``[0, n)`` in a
    hand-made ``idx`` is never read through: its item comes out NaN."""
    return _BeScaleFn.apply(_be_dense("be_scale", x), table, idx)


class _BeExpandFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pre, m0, m1):
        ctx.save_for_backward(x, pre)
        ctx.members = (m0, m1)
        return ops.be_expand(x, pre, None, m0, m1)

    @staticmethod
    def backward(ctx, dy):
        x, pre = ctx.saved_tensors
        m0, m1 = ctx.members
        dy = _be_dense("be_members_expand backward", dy)
        dx = ops.be_members_sum(dy, pre, m0, m1) if ctx.needs_input_grad[0] else None
        dpre = None
        if ctx.needs_input_grad[1]:
            dpre = ops.be_tgrad(dy, x, int(pre.shape[0]), m0, m1)[1]
        return dx, dpre, None, None


def be_members_expand(x, pre, m0, m1):
    """``out[(m - m0) * B + b] = x[b] * pre[m]`` for the members ``m0 <= m < m1``: ``x`` is read once
    and ``m1 - m0`` copies are written, one launch. Differentiable: the input gradient is a members
    sum with table ``pre``, the table gradient the fixed-order fp64 reduction of ``be_scale``."""
    return _BeExpandFn.apply(_be_dense("be_members_expand", x), pre, int(m0), int(m1))


class _BeMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, post, acc, m0, m1, n):
        ctx.save_for_backward(y, post)
        ctx.members = (m0, m1, n)
        return ops.be_members_sum(y, post, m0, m1, acc, 1.0 / n if m1 == n else None)

    @staticmethod
    def backward(ctx, dout):
        y, post = ctx.saved_tensors
        m0, m1, n = ctx.members
        scale = 1.0 / n if m1 == n else 1.0
        dout = _be_dense("be_members_mean backward", dout)
        dy = ops.be_expand(dout, post, None, m0, m1, scale) if ctx.needs_input_grad[0] else None
        dpost = None
        if ctx.needs_input_grad[1]:
            dpost = ops.be_tgrad(y, dout, n, m0, m1, scale)[1]
        dacc = None
        if ctx.needs_input_grad[2]:
            dacc = dout if m1 != n else ops.be_expand(dout, None, None, 0, 1, scale)
        return dy, dpost, dacc, None, None, None


def be_members_mean(y, post, m0, m1, n, acc=None):
    """``out[b] = acc[b] + sum_{m0 <= m < m1} post[m] * y[(m - m0) * B + b]``, a single fma chain in
    member order (from 0 without ``acc``), times ``1 / n`` once, in the call whose ``m1 == n``: the
    mean over ``n`` members does not depend on how they were cut into calls, bit for bit. One launch
    per call, no stack and no mean. Differentiable through the same kernels."""
    if tuple(post.shape)[0] != n:
        raise ValueError(f"be_members_mean: a table of {n} rows expected, got {tuple(post.shape)}")
    acc = None if acc is None else _be_dense("be_members_mean", acc)
    return _BeMeanFn.apply(_be_dense("be_members_mean", y), post, acc, int(m0), int(m1),
                           int(n))


def _be_mixes_items(mod):
    """True when ``mod`` holds a batch norm that takes its statistics from the batch it is given."""
    for m in mod.modules():
        if isinstance(m, torch.nn.modules.batchnorm._NormBase) and not isinstance(
                m, torch.nn.modules.instancenorm._InstanceNorm):
            if m.training or not m.track_running_stats or m.running_mean is None:
                return True
    return False


def be_chunk(n, B, item_bytes):
    """Members per launch of the "batched" route: as many as keep the expanded batch inside
    ``BE_BATCH_BUDGET_BYTES``, at least one."""
    return max(1, min(int(n), BE_BATCH_BUDGET_BYTES // max(1, int(B) * int(item_bytes))))


def be_route(n, B, item_bytes, mod):
    """The route of the eval mean over ``n`` members of a batch of ``B`` items of ``item_bytes`` each
    through ``mod``: "batched" (members side by side in one batch, ``mod`` run once per chunk) or
    "loop" (one member at a time). Batching is exact only where ``mod`` treats the items of a batch
    independently: a batch norm on batch statistics inside ``mod`` forces "loop"; so does a batch of
    which not even two members fit the byte budget."""
    if _be_mixes_items(mod) or n < 2:
        return "loop"
    return "batched" if be_chunk(n, B, item_bytes) >= 2 else "loop"


# ---- deconfounded classification (csrc/deconfound.hip) ---------------------------------------------------
class _SplitColumnsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, n):
        ctx.geom = (int(features.shape[0]), int(features.shape[1]), n, features.device)
        ctx.set_materialize_grads(False)
        return ops.deconf_split_fwd(features, n)

    @staticmethod
    def backward(ctx, da, db):
        B, F, n, dev = ctx.geom
        if da is None and db is None:
            return None, None
        da = None if da is None else da.contiguous()
        db = None if db is None else db.contiguous()
        return ops.deconf_split_bwd(da, db, B, F, n, dev), None


def split_columns(features, n):
    """``(features[:, :n], features[:, n:])`` of dense rows [B, F] as two dense tensors, one launch.
    Backward: one launch writes the whole [B, F] gradient from whichever halves have one (zeros for
    the other), no ``cat``. This is how a column slice reaches ``functional.linear``: a strided view
    is refused at the kernel boundary."""
    return _SplitColumnsFn.apply(features.contiguous(), int(n))


class _DeconfCorrFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, n_conf):
        loss, saved = ops.deconf_corr_fwd(features, n_conf)
        ctx.save_for_backward(features, saved)
        ctx.n_conf = n_conf
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        features, saved = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None
        g = g.to(torch.float32).reshape(1).contiguous()
        return ops.deconf_corr_bwd(features, ctx.n_conf, saved, g), None


def deconf_correlation_loss(features, n_conf):
    """``DeconfoundedNetPL.correlation_loss``: columns ``[0, n_conf)`` of ``features`` [B, F] against
    columns ``[n_conf, F)``, both centred over the batch, ``r = clamp(<a, b> / clamp(|a| |b|,
    min=1e-8), -1, 1)``, the mean of ``r^2`` over the pairs; a 0-d tensor. One launch forward, one
    backward; the ``[B, n_conf, F - n_conf]`` product is never written (kept: mean and norm per
    column, the ratio per pair, in fp64). Clamp gradients are torch's (passed on the closed
    interval). One deviation: the gradient of ``sqrt`` at an exactly zero centred norm is 0, where
    the reference's whole gradient becomes NaN: a constant column has ``r = 0`` with every partner
    and receives an exact 0 gradient."""
    return _DeconfCorrFn.apply(features.contiguous(), int(n_conf))


def deconf_route(n_conf, cat_classes=(), n_cont=0, structure=()):
    """The route of the confounder heads' loss: "fused" (``deconf_heads_loss`` in one launch) for
    linear heads within ``n_conf <= 1024``, at most 8 categorical heads of at most 64 classes and at
    most 64 regression outputs; "composed" (``split_columns``, the heads' own forward,
    ``cross_entropy`` and ``mse_loss``) beyond a limit or with a non-empty ``structure``."""
    if len(structure or ()) > 0:
        return "composed"
    return ops.deconf_route(n_conf, cat_classes, n_cont)


class _DeconfHeadsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, n_conf, n_cat, has_cont, cat_targets, cont_target, conf_mult, *params):
        cat_heads = [(params[2 * h], params[2 * h + 1]) for h in range(n_cat)]
        cont_head = (params[2 * n_cat], params[2 * n_cat + 1]) if has_cont else None
        out = ops.deconf_heads_fwd(features, n_conf, cat_heads, cat_targets, cont_head, cont_target,
                                   conf_mult)
        ctx.save_for_backward(features, cat_targets, cont_target, *params)
        ctx.cfg = (n_conf, n_cat, has_cont, conf_mult)
        ctx.set_materialize_grads(False)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_cat, g_cont):
        features, cat_targets, cont_target, *params = ctx.saved_tensors
        n_conf, n_cat, has_cont, conf_mult = ctx.cfg
        none = (None,) * (7 + len(params))
        if g_cat is None and g_cont is None:
            return none
        cat_heads = [(params[2 * h], params[2 * h + 1]) for h in range(n_cat)]
        cont_head = (params[2 * n_cat], params[2 * n_cat + 1]) if has_cont else None
        g_cat = None if g_cat is None or not n_cat else g_cat.to(torch.float32).reshape(1).contiguous()
        g_cont = (None if g_cont is None or not has_cont
                  else g_cont.to(torch.float32).reshape(1).contiguous())
        dx, dcat, dcont = ops.deconf_heads_bwd(
            features, n_conf, cat_heads, cat_targets, cont_head, cont_target, conf_mult, g_cat, g_cont,
            need_x=ctx.needs_input_grad[0], need_w=any(ctx.needs_input_grad[7:]))
        grads = []
        for pair in dcat + ([dcont] if dcont is not None else []):
            grads += list(pair)
        if not grads:
            grads = [None] * len(params)
        grads = [g if need else None for g, need in zip(grads, ctx.needs_input_grad[7:])]
        return (dx, None, None, None, None, None, None, *grads)


def deconf_heads_loss(features, n_conf, cat_heads, cat_targets, cont_head, cont_target, conf_mult=1.0):
    """``(cat_loss | None, cont_loss | None)`` of the default linear confounder heads on
    ``features[:, :n_conf]``, read in place: ``cat_heads`` a list of ``(W [K, n_conf], b [K])``,
    ``cat_targets`` ONE int64 ``[n_heads, B]`` device table, ``cont_head`` ``(W [n_cont, n_conf],
    b)`` with ``cont_target`` [B, n_cont]; either kind may be absent (empty list / None).
    ``cat_loss = conf_mult * sum_h CE_h / n_heads`` (mean cross entropy per head), ``cont_loss =
    conf_mult * mse``. A label outside ``[0, K)`` is never used as an index: the loss is NaN.
    Fused route (``deconf_route``): one launch forward, two backward (d features, every dW and db).
    Beyond its limits the same values come from ``split_columns``, ``linear``, ``cross_entropy`` and
    ``mse_loss``."""
    cat_heads = list(cat_heads or [])
    if not cat_heads and cont_head is None:
        return None, None
    n_conf = int(n_conf)
    if features.dim() != 2 or not 0 < n_conf < features.shape[1]:
        raise ValueError(f"deconf_heads_loss: features [B, F] and n_conf in (0, F) expected, got "
                         f"{tuple(features.shape)} and n_conf {n_conf}")
    n_cont = int(cont_head[0].shape[0]) if cont_head is not None else 0
    if deconf_route(n_conf, [int(W.shape[0]) for W, _ in cat_heads], n_cont) == "composed":
        conf, _ = split_columns(features, n_conf)
        cat_loss = cont_loss = None
        if cat_heads:
            cat_loss = sum(cross_entropy(linear(conf, W, b), cat_targets[h]) / len(cat_heads)
                           for h, (W, b) in enumerate(cat_heads)) * conf_mult
        if cont_head is not None:
            pred = linear(conf, cont_head[0], cont_head[1])
            cont_loss = mse_loss(pred, cont_target.to(pred)) * conf_mult
        return cat_loss, cont_loss
    params = [t for pair in cat_heads for t in pair] + (list(cont_head) if cont_head is not None else [])
    if cont_head is not None:
        cont_target = cont_target.detach().to(device=features.device, dtype=torch.float32).contiguous()
    cat, cont = _DeconfHeadsFn.apply(features.contiguous(), n_conf, len(cat_heads),
                                     cont_head is not None,
                                     None if not cat_heads else cat_targets,
                                     cont_target if cont_head is not None else None,
                                     float(conf_mult), *params)
    return (cat if cat_heads else None), (cont if cont_head is not None else None)


# ---- adaptive prediction sets (modules/conformal_prediction/conformal.py; csrc/bootstrap.hip) ------------
def aps_route(pred):
    """ "kernel" for probabilities [N, C] on the GPU with C <= ``ops.APS_MAX_CLASSES``, otherwise
    "composite" (CPU tensors, wider rows): the same rule in torch ops."""
    return ops.aps_route(pred.shape[1]) if pred.is_cuda else "composite"


def _aps_cumulative_composite(pred):
    order = torch.sort(pred, dim=1, descending=True, stable=True).indices
    prefix = torch.take_along_dim(pred, order, dim=1).double().cumsum(1).float()
    return torch.empty_like(prefix).scatter_(1, order, prefix)


def aps_cumulative(pred, labels=None):
    """``(cum [N, C], scores [N] | None)``: ``cum[i, c]`` is the cumulative probability of row i at
    the rank of class c in the stable descending order (of equal probabilities the lower index
    first); every prefix is summed in fp64 and rounded to fp32, which is what the reference's CPU
    ``cumsum`` does -- ``qhat`` is frequently exactly 1.0 and the sets test ``cum <= qhat``, so a
    plain fp32 running sum gives other sets. ``scores[i] = cum[i, labels[i]]``. No gradient."""
    pred = pred.detach().float()
    if pred.dim() != 2:
        raise ValueError(f"aps_cumulative: probabilities [N, C] expected, got {tuple(pred.shape)}")
    if labels is not None:
        labels = labels.detach().reshape(-1).to(device=pred.device, dtype=torch.int64)
        if labels.shape[0] != pred.shape[0]:
            raise ValueError(f"aps_cumulative: {labels.shape[0]} labels for {pred.shape[0]} rows")
    if aps_route(pred) == "kernel":
        return ops.aps_cumulative(pred.contiguous(), labels)
    cum = _aps_cumulative_composite(pred)
    if labels is None:
        return cum, None
    ok = (labels >= 0) & (labels < pred.shape[1])
    picked = torch.take_along_dim(cum, torch.where(ok, labels, torch.zeros_like(labels))[:, None], 1)
    return cum, torch.where(ok, picked[:, 0], torch.full_like(picked[:, 0], float("nan")))


def aps_scores(pred, labels):
    """The conformal score of every calibration row: the cumulative probability down to, and
    including, its own label (``AdaptivePredictionSets.calculate``)."""
    return aps_cumulative(pred, labels)[1]


def aps_sets(pred, qhat):
    """bool [N, C]: the classes whose cumulative probability is at most ``qhat`` (a float or a
    one-element tensor), and always the argmax class (the first maximal index)."""
    cum, _ = aps_cumulative(pred)
    sets = cum <= torch.as_tensor(qhat, dtype=torch.float32, device=cum.device)
    sets.scatter_(1, torch.argmax(pred.detach(), 1, keepdim=True), True)
    return sets


# ---- semi-supervised U-Net losses beyond the local contrastive one (csrc/semisl.hip) ---------------------
def semisl_route(kind, C=1, K=1, reduction="mean", ignore_index=-100):
    """The route of a semi-supervised loss, "fused" (csrc/semisl.hip) or "composed" (the same rule in
    torch ops; CPU tensors and tensors that are not fp32 always take it). Limits of the fused routes:

    * ``"anchor"`` (``loco_anchor_loss``): ``C % 4 == 0`` and ``C <= 1024`` (the kernels loop over
      channel quads, so no width spills);
    * ``"nn"`` (``nn_queue_loss``): ``C % 4 == 0``, ``C <= 64`` (two blocks per CU's LDS) and ``K <= 64``;
    * ``"pseudo_label"`` (``pseudo_label_ce``): ``K <= 64``, ``reduction`` "mean" or "sum" and the default
      ``ignore_index`` (probability targets never read it); ``weight`` and ``label_smoothing`` are fused.
    """
    if kind == "pseudo_label" and (reduction not in ("mean", "sum") or ignore_index != -100):
        return "composed"
    return ops.semisl_route(kind, C, K)


def _semisl_rows(x):
    """Dense NDHWC rows [B, V, C] of features [B, C, *spatial] (a view of channels-last memory)."""
    B, C = x.shape[0], x.shape[1]
    if x.dim() == 5:
        return ops.ndhwc(x).permute(0, 2, 3, 4, 1).reshape(B, -1, C)
    return x.flatten(2).transpose(1, 2).contiguous()


def _semisl_unrows(rows, shape):
    """The gradient rows [B, V, C] under the logical shape [B, C, *spatial]."""
    return rows.reshape(shape[0], *shape[2:], shape[1]).movedim(-1, 1)


def loco_anchor_loss_composite(x, a1, a2, temperature=0.1):
    """``LocalContrastiveLossWithAnchors.forward`` as the reference writes it
    (semi_supervised_segmentation/losses.py:576-585), in torch ops."""
    F = torch.nn.functional
    x, a1, a2 = x.flatten(start_dim=2), a1.flatten(start_dim=2), a2.flatten(start_dim=2)
    sim_1 = F.cosine_similarity(x, a1, dim=1) / temperature
    sim_2 = F.cosine_similarity(x, a2, dim=1) / temperature
    return F.kl_div(F.softmax(sim_1, dim=1), F.softmax(sim_2, dim=1), reduction="none").sum(-1)


class _LocoAnchorFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, a1, a2, temperature):
        shape = x.shape
        x, a1, a2 = _semisl_rows(x), _semisl_rows(a1), _semisl_rows(a2)
        loss, sim1, sim2, stats = ops.loco_anchor_fwd(x, a1, a2, temperature)
        ctx.save_for_backward(x, a1, a2, sim1, sim2, stats)
        ctx.conf = (temperature, shape)
        return loss

    @staticmethod
    def backward(ctx, g):
        temperature, shape = ctx.conf
        dx, da1, da2 = ops.loco_anchor_bwd(*ctx.saved_tensors, g, temperature,
                                           ctx.needs_input_grad[1], ctx.needs_input_grad[2])
        return (_semisl_unrows(dx, shape) if ctx.needs_input_grad[0] else None,
                None if da1 is None else _semisl_unrows(da1, shape),
                None if da2 is None else _semisl_unrows(da2, shape), None)


def loco_anchor_loss(x, a1, a2, temperature=0.1):
    """Per-item anchor loss [B] of features and two anchor maps [B, C, *spatial]
    (``LocalContrastiveLossWithAnchors.forward``, semi_supervised_segmentation/losses.py:547-585):
    ``sim_k[b, v] = cos(x[b, :, v], a_k[b, :, v]) / temperature``, ``p = softmax_v(sim_1)``,
    ``q = softmax_v(sim_2)`` over the voxels of an item, ``loss[b] = sum_v (xlogy(q, q) - q p)`` --
    ``F.kl_div`` with a probability, not a log-probability, as its input, as the reference calls it.
    Differentiable in all three inputs; the fused route writes two floats per voxel."""
    if tuple(a1.shape) != tuple(x.shape) or tuple(a2.shape) != tuple(x.shape) or x.dim() < 3:
        raise ValueError(f"loco_anchor_loss: features and anchors [B, C, *spatial] of one shape expected, "
                         f"got {tuple(x.shape)}, {tuple(a1.shape)}, {tuple(a2.shape)}")
    if not x.is_cuda or x.dtype != torch.float32 or semisl_route("anchor", C=x.shape[1]) == "composed":
        return loco_anchor_loss_composite(x, a1, a2, temperature)
    return _LocoAnchorFn.apply(x, a1, a2, float(temperature))


def nn_queue_loss_composite(x, y, past, past_labels, temperature=0.1):
    """``NearestNeighbourLoss.forward`` past the queue (semi_supervised_segmentation/losses.py:425-444)
    in torch ops: ``past_labels`` is the one-hot [Q, K]; writes the [B, V, Q] tensors."""
    F = torch.nn.functional
    x = x.flatten(start_dim=2).permute(0, 2, 1)
    y = y.flatten(start_dim=2).permute(0, 2, 1)
    distances = 1 - F.cosine_similarity(x[:, :, None], past[None, None, :], -1)
    is_same = torch.sum(y[:, :, None] * past_labels[None, None, :], -1)
    same = torch.exp(-distances * is_same / temperature)
    other = torch.exp(-distances * (1 - is_same) / temperature)
    return torch.nanmean(same.nansum(-1) / other.nansum(-1))


class _NNQueueFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, past, past_class, temperature):
        shape = x.shape
        x = _semisl_rows(x)
        y = y.reshape(y.shape[0], y.shape[1], -1).contiguous().float()
        pastn = ops.nn_queue_normalize(past.contiguous())
        loss, S, O, stats = ops.nn_queue_loss_fwd(x, y, pastn, past_class, temperature)
        ctx.save_for_backward(x, y, pastn, past_class, S, O, stats)
        ctx.conf = (temperature, shape)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        temperature, shape = ctx.conf
        dx = ops.nn_queue_loss_bwd(*ctx.saved_tensors, g, temperature)
        return _semisl_unrows(dx, shape), None, None, None, None


def nn_queue_loss(x, y, past, past_class, temperature=0.1):
    """Nearest-neighbour loss (0-d) of features ``x`` [B, C, *spatial] and labels ``y``
    [B, K, *spatial] (any float data) against the queued rows ``past`` [Q, C] of classes ``past_class``
    (integers [Q]): per voxel ``d_q = 1 - cos(x_v, past_q)``, ``m_q = y[b, past_class[q], v]``,
    ``S = sum_q exp(-d_q m_q / T)``, ``O = sum_q exp(-d_q (1 - m_q) / T)``; the mean of ``S / O`` over
    the voxels whose ratio is not NaN, a NaN term counting 0 in either sum
    (``NearestNeighbourLoss.forward``, semi_supervised_segmentation/losses.py:425-444). Differentiable
    in ``x``. The fused route keeps two floats per voxel and never writes a [B, V, Q] tensor. One
    deviation: the gradient at a voxel whose ratio is NaN is an exact 0 (torch gives 0 * NaN there)."""
    if x.dim() < 3 or y.dim() != x.dim() or y.shape[0] != x.shape[0] \
            or tuple(y.shape[2:]) != tuple(x.shape[2:]):
        raise ValueError(f"nn_queue_loss: x [B, C, *spatial] and y [B, K, *spatial] expected, got "
                         f"{tuple(x.shape)} and {tuple(y.shape)}")
    if past.dim() != 2 or past.shape[1] != x.shape[1] or past_class.shape != past.shape[:1]:
        raise ValueError(f"nn_queue_loss: past [Q, {x.shape[1]}] and past_class [Q] expected, got "
                         f"{tuple(past.shape)} and {tuple(past_class.shape)}")
    if past.shape[0] == 0:
        return torch.zeros([], device=x.device)
    K = y.shape[1]
    if not x.is_cuda or x.dtype != torch.float32 or semisl_route("nn", C=x.shape[1], K=K) == "composed":
        labels = torch.nn.functional.one_hot(past_class.to(device=x.device, dtype=torch.int64), K)
        return nn_queue_loss_composite(x, y, past.to(x.device), labels, temperature)
    past_class = past_class.to(device=x.device, dtype=torch.int32).contiguous()
    return _NNQueueFn.apply(x, y, past.detach(), past_class, float(temperature))


class _PseudoLabelCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, proba, threshold, weight, label_smoothing, mean):
        shape = pred.shape
        pred = pred.reshape(shape[0], shape[1], -1).contiguous()
        proba = proba.reshape(shape[0], shape[1], -1).contiguous()
        weight = None if weight is None else weight.contiguous()
        loss = ops.pseudo_label_ce_fwd(pred, proba, threshold, weight, label_smoothing, mean)
        ctx.save_for_backward(pred, proba, weight)
        ctx.conf = (threshold, label_smoothing, mean, shape)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return (None,) * 6
        pred, proba, weight = ctx.saved_tensors
        threshold, label_smoothing, mean, shape = ctx.conf
        d = ops.pseudo_label_ce_bwd(pred, proba, threshold, weight, label_smoothing, mean, g)
        return (d.reshape(shape),) + (None,) * 5


def pseudo_label_ce(pred, proba, threshold, weight=None, label_smoothing=0.0, reduction="mean"):
    """Cross entropy of the logits ``pred`` [B, K, *spatial] against the 0/1 pseudo-labels
    ``proba > threshold`` (strict, compared in fp32 as torch compares a tensor with a number) taken as
    PROBABILITY targets -- zero, one or several hot classes per voxel -- which is
    ``F.cross_entropy(pred, (proba > threshold).float(), weight, label_smoothing=..., reduction=...)``
    (``PseudoLabelCrossEntropy.forward``, semi_supervised_segmentation/losses.py:465-477). "mean"
    divides the sum by B V, with or without ``weight``. Differentiable in ``pred``. The fused route
    forms the log-softmax and the targets in registers: one launch each way."""
    if tuple(proba.shape) != tuple(pred.shape) or pred.dim() < 2:
        raise ValueError(f"pseudo_label_ce: logits and probabilities [B, K, *spatial] of one shape "
                         f"expected, got {tuple(pred.shape)} and {tuple(proba.shape)}")
    fused = pred.is_cuda and pred.dtype == torch.float32 and pred.numel() > 0 \
        and semisl_route("pseudo_label", K=pred.shape[1], reduction=reduction) == "fused"
    if not fused:
        return torch.nn.functional.cross_entropy(pred, (proba > threshold).float(), weight,
                                                 reduction=reduction,
                                                 label_smoothing=float(label_smoothing))
    if weight is not None:
        weight = weight.detach().to(device=pred.device, dtype=torch.float32)
    return _PseudoLabelCEFn.apply(pred, proba.detach().float(), float(threshold), weight,
                                  float(label_smoothing), reduction == "mean")


# ---- spectral normalisation (modules.layers.spectral_norm._SpectralNorm) -----------------------------------
def spectral_norm_route(h, w):
    """The route of ``spectral_normalize`` for an ``h x w`` matrix: "block" (one workgroup keeps the
    matrix, both vectors and the fp64 products in LDS: one launch each way whatever n is), "grid" (rows
    over workgroups, the last ticket folds: 2 n + 1 launches forward, 2 backward; up to 32768 rows and
    columns) or "composed" (torch operators) beyond."""
    return ops.spectral_norm_route(h, w)


class _SpectralNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, u, v, n_iter, eps, dim):
        out, sigma, u_used, v_used = ops.spectral_norm_fwd(weight, u, v, n_iter, eps, dim)
        # the output itself, sigma on the device and the vectors THIS access used: a later access
        # advances the buffers without changing this one's gradient
        ctx.save_for_backward(out, sigma, u_used, v_used)
        ctx.dim = dim
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return (None,) * 6
        out, sigma, u_used, v_used = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        return (ops.spectral_norm_bwd(g, out, u_used, v_used, sigma, ctx.dim),) + (None,) * 5


def spectral_normalize(weight, u, v, n_power_iterations=1, eps=1e-12, dim=0, training=True):
    """``W / sigma`` of torch's ``_SpectralNorm.forward``: when ``training``, ``n_power_iterations``
    times ``u <- normalize(W v, eps)``, ``v <- normalize(W^T u, eps)`` written IN PLACE into the given
    buffers (same storage), then ``sigma = u^T W v`` with ``u`` and ``v`` as constants. The matrix is
    the weight with ``dim`` in front, read in place; the result has the weight's layout. Backward:
    ``dL/dW = (G - <G, W_sn> u v^T) / sigma`` with the vectors of THIS access. A zero weight gives NaN,
    as torch does. Routes: ``spectral_norm_route``; CPU tensors, other dtypes and "composed" shapes
    run torch's own operators."""
    dim = dim if dim >= 0 else dim + weight.dim()
    outer, h, inner = ops.spectral_norm_matrix(weight.shape, dim)
    fused = weight.is_cuda and weight.dtype == torch.float32 and u.dtype == torch.float32 \
        and spectral_norm_route(h, outer * inner) != "composed"
    if not fused:
        mat = weight if dim == 0 else weight.permute(dim, *(d for d in range(weight.dim()) if d != dim))
        mat = mat.flatten(1)
        # on the device the products are summed in fp64 here too (and rounded where torch stores or
        # returns them); on the CPU this is torch's own arithmetic, bit for bit
        wide = weight.is_cuda and weight.dtype == torch.float32
        up = (lambda t: t.double()) if wide else (lambda t: t)
        if training:
            with torch.no_grad():
                big = up(mat)
                for _ in range(int(n_power_iterations)):
                    u.copy_(torch.nn.functional.normalize(torch.mv(big, up(v)), dim=0, eps=eps))
                    v.copy_(torch.nn.functional.normalize(torch.mv(big.H, up(u)), dim=0, eps=eps))
        uc, vc = u.clone(), v.clone()
        sigma = torch.vdot(up(uc), torch.mv(up(mat), up(vc)))
        return (weight / sigma).to(weight.dtype)
    n_iter = int(n_power_iterations) if training else 0
    if training and n_iter < 1:
        raise ValueError(f"Expected n_power_iterations to be positive, but got "
                         f"n_power_iterations={n_power_iterations}")
    return _SpectralNormFn.apply(weight.contiguous(), u, v, n_iter, float(eps), int(dim))
