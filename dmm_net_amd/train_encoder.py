"""bf16 channels-last TRAINING form of the encoder (reference a10 as the trainer runs it; BASELINE configs[3]).

Counterpart of ``dmm/modules/model_encoder.py:86-162`` + ``base.py:18-69`` + ``vision.py:6-38`` under
``train.py:296-307`` (forward, ``loss.backward()``, optimiser step).  Same parameters as ``FeatureEncoder`` -- the fp32
``nn.Parameter`` objects of the wrapped encoder stay the masters the optimiser, the checkpoints and
``distributed.GradBucketer`` see -- evaluated the way that is fast on MI355X (12 frames of 255 x 448, ResNet-101: 31.25 ms
per training step with the stock fp32 modules, 15.4 ms here; ``profiles/r06_cfg4_train_encoder_steps.md`` has every step in
between):

* **forward and backward as HIP-graph replays.**  The stock step is ~2 100 launches of 5-50 us kernels and HOST bound (17.6 ms
  of kernels inside a 24.4 ms step under bf16 autocast).  The body is cut into a CHAIN of segments (stem | layer1 | layer2 |
  layer3 in parts | layer4) plus the heads; the forward between two taps and every segment's backward
  (``torch.autograd.grad`` over the segment) are captured once per input shape and replayed; segments hand activations and
  gradients to each other in static buffers.  Memset nodes of a capture are rewritten into kernel nodes (``graphs.SafeGraph``).
* **two streams.**  In the backward only the data gradients are on the critical chain.  A segment's weight gradients are
  recorded while its chain is captured and captured afterwards into a graph of their own that replays on a SIDE stream beside
  the next segment's chain; the heads of a pyramid level (forward and backward) are side-stream graphs too.  (Two graphs on
  two streams overlap on this runtime; forked branches inside one graph do not: ``tools/graph_branch_probe.py``.)
* **bf16 activations, channels-last, end to end; fp32 master weights.**  BatchNorm runs on bf16 activations with fp32
  parameters and statistics.  No autocast.
* **1x1 convolutions are matrix products** of the [B*H*W, Cin] activation matrix (2/3 of a bottleneck): forward and data
  gradient on hipBLASLt; 3x3 forward / data gradient on MIOpen (in the deterministic mode with
  ``set_deterministic_conv("own")``: on ``dmm_conv3x3_bf16``, ``csrc/dmm_conv.hip``; with ``"own_all"`` the 32-channel heads
  too, on ``dmm_conv3x3_narrow_bf16`` / ``dmm_wgrad3x3_narrow_bf16``; with ``"own_stem"`` the 7x7 stem as well, on
  ``dmm_conv7x7s2_stem_bf16`` / ``dmm_wgrad7x7s2_stem_bf16``, ``csrc/dmm_stem.hip``); EVERY weight gradient from ``dmm_wgrad*_bf16``
  (``csrc/dmm_wgrad.hip``: MFMA, split over the rows, fp32 straight into the master's gradient, no atomics) -- hipBLASLt's pick
  for these products has no split-K (66 us each), MIOpen's bf16 solvers bring a zeroing and a cast launch each.
* **BatchNorm (+ residual) (+ ReLU) as two launches each way** (``dmm_bn_*`` in ``csrc/dmm_encoder_train.hip``) where the
  stock path issues 5-6 (three MIOpen BatchNorm kernels + add + clamp; backward likewise).

Gradient hand-over.  Parameter gradients are NOT returned through autograd (350 inputs to one node).  Each segment is an
autograd node chained to its neighbours by a token, and also takes the segment's HUB leaf: a leaf's AccumulateGrad runs once
per backward pass after its last user -- the moment every forward in flight (the reference's trainer calls the encoder once
per frame of a clip and backpropagates once, ``trainer.py:95-131``; each such forward owns a plan) has produced the segment's
gradients.  The hub's hook sums them, sets / accumulates ``p.grad`` and calls the parameters' post-accumulate-grad hooks, like
AccumulateGrad does -- ``GradBucketer(overlap=True)`` and plain optimisers work unchanged.  A segment is handed over one
segment late (the hand-over waits for its side-stream graph).  As with DDP's bucket views, a gradient may alias a static
buffer of the captured step: it is valid until the encoder's next forward (which moves a gradient that is still in place --
gradient accumulation -- into a tensor of its own first); do not hold on to the tensor object itself across steps.

Not supported: double backward, ``retain_graph`` replays of the same forward, forward hooks on the wrapped modules, changing
``requires_grad`` of a parameter after the first forward of a shape (the captured backward computes the gradients of the
parameters that required one at capture time).  In-place parameter updates (optimiser steps, ``load_state_dict``) are seen
by the replays; ``.to()`` / ``.cuda()`` drop the captured plans.  Fallbacks inside the same segments: the 7x7 stem and widths
that are not multiples of 64 take the stock convolution ops, ``dtype=float32`` the stock BatchNorm as well (the mode the tests
pin the plumbing with).  Off the GPU (or with ``graphs=False``) the same segment functions run eagerly under autograd.
"""
from __future__ import annotations

from contextlib import contextmanager
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from .determinism import get_deterministic_conv, is_deterministic, library_flags
from .encoder import _NO_CTX, Bottleneck, FeatureEncoder, ResNetBody
from .graphs import CaptureFailed, SafeGraph

_CL = torch.channels_last
_CAPTURE_LOCK = __import__("threading").Lock()     # plan captures set module-level scratch (_CAPTURE) and put the process
#                                                    into HIP's global capture mode: one at a time (nn.DataParallel threads)


# ---- scratch of a graph capture: the BatchNorm statistics' arena, the deferred weight-gradient launches ------------------
class _Arena:
    """fp32 scratch the statistics kernels accumulate into (they need zeroed [2, C] blocks): inside a captured segment ONE
    zeroing launch at the head of the graph clears the blocks of all its layers -- a ``torch.zeros`` per layer and direction
    was 238 launches of ~4 us per ResNet-101 step (profiles/r06_cfg4_train_encoder_steps.md).  A capture is traced
    once, so handing out consecutive slices while it runs fixes every layer's block for all replays."""

    def __init__(self, device, floats: int = 1 << 20):
        self.buf = torch.empty(int(floats), dtype=torch.float32, device=device)     # (zeroed by the scope, once per replay)
        self.off = 0

    def take(self, n: int) -> torch.Tensor:
        n = (n + 63) & ~63
        if self.off + n > self.buf.numel():
            raise RuntimeError("TrainEncoder: statistics arena exhausted")
        t = self.buf[self.off:self.off + n]
        self.off += n
        return t


class _Capture:
    """What the ops of ONE graph capture share: ``arena`` (the statistics scratch of the graph, or None) and ``records``
    (``overlap_wgrad``: the weight-gradient launches of a segment's backward chain, recorded with their operands kept alive
    instead of launched, and captured afterwards into a SECOND graph that replays on a side stream beside the next
    segment's chain; None: they are launched where the backward reaches them)."""

    def __init__(self, arena: Optional[_Arena], defer: bool):
        self.arena, self.records = arena, ([] if defer else None)


# The capture that is running, or None.  Process-global ON PURPOSE, guarded by _CAPTURE_LOCK (captures never run side by
# side): the backward nodes that ``torch.autograd.grad`` runs inside a capture execute on autograd's device worker thread,
# not on the capturing thread -- a thread-local or a ``contextvars`` variable would be unset where ``_zeroed`` and ``_wgrad``
# read it.
_CAPTURE: Optional[_Capture] = None


@contextmanager
def _capture_scope(arena: Optional[_Arena] = None, defer: bool = False):
    """Entered INSIDE a graph capture, for its length.  -> the ``_Capture``."""
    global _CAPTURE
    cap = _CAPTURE = _Capture(arena, defer)
    try:
        if arena is not None:
            arena.buf.zero_()                # a fill KERNEL (captured: replayed at the head of the graph)
        yield cap
    finally:
        _CAPTURE = None


def _zeroed(n: int, device) -> torch.Tensor:
    cap = _CAPTURE
    if cap is not None and cap.arena is not None and cap.arena.buf.device == device:
        return cap.arena.take(n)
    return torch.zeros(n, dtype=torch.float32, device=device)


# ---- deterministic mode (dmm_net_amd.determinism): resolved once per TrainEncoder call and pinned while it builds / runs ----
_DET: Optional[bool] = None              # set by TrainEncoder while its forward (eager or plan build) runs
_OWN_SETTINGS = ("own", "own_all", "own_stem")     # ``set_deterministic_conv`` values that take the 3x3 convolutions off MIOpen


def _det_now() -> bool:
    return _DET if _DET is not None else is_deterministic()


class _det_scope:
    """Pins the mode for the ops of one TrainEncoder call (its plan build included: warm-up and captures) and, when on, runs
    its library calls under cudnn.deterministic."""

    def __init__(self, det: bool):
        self.det, self.flags = det, library_flags(det)

    def __enter__(self):
        global _DET
        self.old, _DET = _DET, self.det
        self.flags.__enter__()

    def __exit__(self, *exc):
        global _DET
        _DET = self.old
        return self.flags.__exit__(*exc)


def _own_conv_now() -> bool:
    """The deterministic mode's 3x3 convolutions on ``dmm_conv3x3_bf16`` (``set_deterministic_conv("own")`` / ``"own_all"`` /
    ``"own_stem"``) instead of MIOpen."""
    return _det_now() and get_deterministic_conv() in _OWN_SETTINGS


def _narrow_conv_now() -> bool:
    """The deterministic mode's NARROW 3x3 convolutions (``_narrow_ok``) on ``dmm_conv3x3_narrow_bf16`` /
    ``dmm_wgrad3x3_narrow_bf16`` (``set_deterministic_conv("own_all")`` / ``"own_stem"``) instead of unfold + GEMM."""
    return _det_now() and get_deterministic_conv() in ("own_all", "own_stem")


def _stem_conv_now() -> bool:
    """The deterministic mode's 7x7 stem (``_stem_ok``) on ``dmm_conv7x7s2_stem_bf16`` / ``dmm_wgrad7x7s2_stem_bf16``
    (``set_deterministic_conv("own_stem")``) instead of unfold + GEMM."""
    return _det_now() and get_deterministic_conv() == "own_stem"


def _det_ws(nbytes: int, device) -> torch.Tensor:
    """Slab workspace of a deterministic reduction (the BatchNorm statistics', a weight gradient's): written whole by the
    launch that fills it, so never zeroed."""
    return torch.empty((max(int(nbytes), 16),), dtype=torch.uint8, device=device)


def _stats_channels_ok(C: int) -> bool:
    """The channel envelope of the statistics kernels (``dmm_bn_*_grouped_bf16``): C % 8 == 0 and C / 8 a divisor of 256 (eight
    channels per thread, whole rows per 256-thread workgroup)."""
    c8 = C // 8
    return C % 8 == 0 and 0 < c8 <= 256 and 256 % c8 == 0


def _bn_scratch(det: bool, R: int, C: int, groups: int, device):
    """What differs between the two forms of the ``dmm_bn_*_grouped_bf16`` entries: -> (the entry-name infix, the scratch
    arguments, which sit at the same position in both forms, the tensor behind them).  Atomic: the [groups, 2, C] sums,
    zeroed; deterministic: the slab of per-workgroup partials the consuming launch folds, with its byte count -- sized here
    and nowhere else."""
    if det:
        from . import _lib
        ws = _det_ws(int(_lib.load().dmm_bn_det_workspace_bytes(R, C, groups)), device)
        return "_det", (ws.data_ptr(), ws.numel()), ws
    sums = _zeroed(groups * 2 * C, device)
    return "", (sums.data_ptr(),), sums


# ---- BatchNorm (+ residual) (+ ReLU), training mode, bf16 NHWC: two launches each way -------------------------------
class _BNActFn(torch.autograd.Function):
    """y = act(BN_train(x) (+ residual)) on a channels-last bf16 activation; statistics, scale and shift in fp32.
    forward = ``dmm_bn_stats_bf16`` (per-channel sum / sum of squares) + ``dmm_bn_apply_bf16`` (normalise, residual, ReLU,
    running statistics); backward = ``dmm_bn_bwd_reduce_bf16`` (sum g, sum g*xhat with g = dy * [y > 0]) +
    ``dmm_bn_bwd_dx_bf16`` (dx, and g as the residual branch's gradient)."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps, relu, residual, groups=1, fork=False):
        from . import _lib
        assert x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous(memory_format=_CL)
        B, C, H, W = x.shape
        assert B % groups == 0, (B, groups)
        R = B * H * W
        stream = torch.cuda.current_stream(x.device).cuda_stream
        det = _det_now()
        form, scratch, _keep = _bn_scratch(det, R, C, groups, x.device)
        y = torch.empty_like(x, memory_format=_CL)
        saved = torch.empty((groups, 2, C), dtype=torch.float32, device=x.device)  # mean, invstd of every statistics group
        res = None
        if residual is not None:
            assert residual.shape == x.shape and residual.dtype == x.dtype
            res = residual.contiguous(memory_format=_CL)
        rm = None if running_mean is None else running_mean.data_ptr()
        rv = None if running_var is None else running_var.data_ptr()
        _lib.call(f"dmm_bn_stats{form}_grouped_bf16", x.device, x.data_ptr(), R, C, groups, *scratch, stream)
        _lib.call(f"dmm_bn_apply{form}_grouped_bf16", x.device, x.data_ptr(), None if res is None else res.data_ptr(), R, C,
                  groups, *scratch, weight.data_ptr(), bias.data_ptr(), rm, rv, float(momentum), float(eps), int(relu),
                  y.data_ptr(), saved.data_ptr(), stream)
        ctx.save_for_backward(x, y, weight, bias, saved)
        ctx.relu, ctx.has_res, ctx.groups, ctx.det = bool(relu), residual is not None, groups, det
        # fork: the output as TWO tensors (the second an alias) for its two consumers -- a residual block's first convolution and
        # its identity branch --, so that their gradients arrive separately and are added inside the backward kernels
        return (y, y.view_as(y)) if fork else y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy, dy2=None):
        from . import _lib
        x, y, weight, bias, saved = ctx.saved_tensors
        # no residual in front of the ReLU: the mask is recomputed from x (the forward's own fma), y is not read
        mode = 0 if not ctx.relu else (1 if ctx.has_res else 2)
        B, C, H, W = x.shape
        R = B * H * W
        if dy is None:                                    # (only the alias was used)
            dy, dy2 = dy2, None
        dy = dy.contiguous(memory_format=_CL)
        if dy2 is not None:
            dy2 = dy2.to(dy.dtype).contiguous(memory_format=_CL)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        groups = ctx.groups
        form, scratch, _keep = _bn_scratch(ctx.det, R, C, groups, x.device)
        dx = torch.empty_like(x, memory_format=_CL)
        dres = torch.empty_like(x, memory_format=_CL) if ctx.has_res else None
        dw = torch.empty((C,), dtype=torch.float32, device=x.device)
        db = torch.empty((C,), dtype=torch.float32, device=x.device)
        head = (dy.data_ptr(), None if dy2 is None else dy2.data_ptr(), x.data_ptr(), y.data_ptr(), R, C, groups,
                saved.data_ptr(), weight.data_ptr(), bias.data_ptr())
        _lib.call(f"dmm_bn_bwd_reduce{form}_grouped_bf16", x.device, *head, mode, *scratch, stream)
        _lib.call(f"dmm_bn_bwd_dx{form}_grouped_bf16", x.device, *head, *scratch, mode, dx.data_ptr(),
                  None if dres is None else dres.data_ptr(), dw.data_ptr(), db.data_ptr(), stream)
        return dx, dw, db, None, None, None, None, None, dres, None, None


class _TapSplit(torch.autograd.Function):
    """x -> (x for the body, x for the heads), two aliases whose gradients autograd accumulates separately; backward adds the
    two sums once -- the form of the plan's segment hand-over (deterministic mode: eager steps equal replays bit for bit)."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x), x.view_as(x)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_body, g_head):
        if g_body is None or g_head is None:
            return g_head if g_body is None else g_body
        return g_body + g_head


def _bn_fusable(bn: nn.BatchNorm2d) -> bool:
    return bn.affine and bn.track_running_stats and bn.momentum is not None and _stats_channels_ok(bn.num_features)


def _bn_act(x, bn: nn.BatchNorm2d, relu: bool, residual=None, fused: bool = True, counted: bool = False, groups: int = 1,
            fork: bool = False):
    """BatchNorm2d module ``bn`` (its fp32 parameters and running statistics) on a bf16 channels-last activation,
    followed by the optional residual add and ReLU.  ``fused`` and training and on the device: the two-launch HIP form
    (``counted``: the caller has already advanced ``num_batches_tracked`` for its whole segment in one launch).
    ``groups`` > 1 (training): the batch is ``groups`` consecutive sub-batches, each normalised with its OWN statistics and
    counted as a call of its own by the running statistics -- what ``groups`` calls of the module on the sub-batches do."""
    if fused and bn.training and x.is_cuda and x.dtype == torch.bfloat16 and _bn_fusable(bn):
        if not counted:
            with torch.no_grad():
                bn.num_batches_tracked.add_(groups)
        return _BNActFn.apply(x.contiguous(memory_format=_CL), bn.weight, bn.bias, bn.running_mean, bn.running_var,
                              bn.momentum, bn.eps, relu, residual, groups, fork)
    if groups > 1 and bn.training:
        y = torch.cat([bn(c) for c in x.chunk(groups, 0)], 0)
    else:
        y = bn(x)
    if residual is not None:
        y = y + residual
    y = F.relu(y) if relu else y
    return (y, y) if fork else y                          # (``fork``: the output for two consumers; only the fused form makes it two tensors)


# ---- weight gradients: launched where the backward reaches them, or collected for a graph of their own -------------------
_DGRAD_AS_FORWARD = True                 # (module switch for the A/B in tools/cfg4_probe.py)
_DET_AS_GEMM = ("forward", "dgrad")     # (module switch for the A/B in tools/cfg4_probe.py: which of _DetConvFn's convolutions
#                                          are an unfold + one GEMM under set_deterministic_conv("own"))


def _wgrad_launch(rec):
    """One weight gradient, ``rec`` = (kind, dy, x, dims, dw): "1x1" (rows, co, ci), "3x3" (B, H, W, ci, co, stride, Ho, Wo),
    "3x3n" (B, H, W, ci, co; the narrow kernel, sized and launched by its wrapper in ``ops``), "7x7s" (B, H, W; the stem kernel,
    likewise) -> dw, overwritten."""
    from . import _lib, ops
    kind, dy, x, dims, dw = rec
    if kind == "3x3n":
        ops.wgrad3x3_narrow_bf16(dy, x, out=dw)
        return
    if kind == "7x7s":
        ops.wgrad7x7s2_stem_bf16(dy, x, out=dw)
        return
    need = _lib.load().dmm_wgrad_workspace_bytes
    dev = x.device
    stream = torch.cuda.current_stream(dev).cuda_stream
    if kind == "1x1":
        rows, co, ci = dims
        ws = _det_ws(need(rows, co, ci), dev)
        _lib.call("dmm_wgrad_bf16", dev, dy.data_ptr(), x.data_ptr(), rows, co, ci, co, ci, dw.data_ptr(), ws.data_ptr(),
                  ws.numel(), stream)
    else:
        B, H, W, ci, co, stride, Ho, Wo = dims
        ws = _det_ws(need(B * Ho * Wo, co, 9 * ci), dev)
        _lib.call("dmm_wgrad3x3_bf16", dev, dy.data_ptr(), x.data_ptr(), B, H, W, ci, co, stride, dw.data_ptr(),
                  ws.data_ptr(), ws.numel(), stream)


def _wgrad(rec):
    """A weight gradient where the backward reaches it: launched, or recorded for the running capture's second graph."""
    cap = _CAPTURE
    if cap is not None and cap.records is not None:
        cap.records.append(rec)
    else:
        _wgrad_launch(rec)


# ---- convolutions ----------------------------------------------------------------------------------------------------
def _wgrad_ok(m: nn.Conv2d) -> bool:
    return (m.groups == 1 and m.dilation == (1, 1) and m.in_channels % 64 == 0 and m.out_channels % 64 == 0
            and m.stride in ((1, 1), (2, 2)))


def _narrow_ok(m: nn.Conv2d) -> bool:
    """A 3x3 / padding 1 / stride 1 convolution whose widths are multiples of 32 and that ``_wgrad_ok`` does not take (one of
    them is no multiple of 64): the 32-channel level-2 heads."""
    return (m.kernel_size == (3, 3) and m.padding == (1, 1) and m.stride == (1, 1) and m.groups == 1 and m.dilation == (1, 1)
            and m.in_channels % 32 == 0 and m.out_channels % 32 == 0 and not _wgrad_ok(m))


def _stem_ok(m: nn.Conv2d) -> bool:
    """The ResNet stem: 7x7 / stride 2 / padding 3, 3 -> 64, no groups, no dilation."""
    return (m.kernel_size == (7, 7) and m.stride == (2, 2) and m.padding == (3, 3) and m.groups == 1 and m.dilation == (1, 1)
            and m.in_channels == 3 and m.out_channels == 64)


def _conv_route(m: nn.Module, linear_1x1: bool = True, own_wgrad: bool = True) -> Optional[str]:
    """The route of convolution module ``m`` on a bf16 activation on the device: "1x1" (``_Conv1x1Fn``), "3x3" (``_Conv3x3Fn``),
    "narrow" (``_ConvNarrowFn``: only under the narrow setting, ``_narrow_conv_now``), "stem" (``_ConvStemFn``: only under the
    stem setting, ``_stem_conv_now``, and for an input that requires no gradient), or None (the stock ops).  ``_conv`` takes
    it, and ``TrainEncoder._tick`` prepares the weight copies of exactly the 1x1 / 3x3 / narrow modules it names."""
    if not (own_wgrad and isinstance(m, nn.Conv2d)):
        return None
    if not _wgrad_ok(m):
        if _narrow_ok(m) and _narrow_conv_now():
            return "narrow"
        return "stem" if _stem_ok(m) and _stem_conv_now() else None
    if linear_1x1 and m.kernel_size == (1, 1) and m.padding == (0, 0) and m.bias is None:
        return "1x1"
    return "3x3" if m.kernel_size == (3, 3) and m.padding == (1, 1) else None


def _dgrad_on_flipped(own: bool, stride: int, co: int, ci: int) -> bool:
    """A 3x3 convolution's data gradient runs as the FORWARD convolution of dy with the flipped, transposed weight: always on
    the own kernels; on MIOpen at stride 1 with as many channels in as out (conv2 of a bottleneck), where dX = conv(dY,
    W'[ci, co, kh, kw] = W[co, ci, 2 - kh, 2 - kw]) is the same convolution problem -- MIOpen's forward kernel for it takes
    28 us where its backward-data kernel takes 50 (profiles/r06_kernel_stats_config4_bf16.csv), on the backward's critical
    chain."""
    return own or (_DGRAD_AS_FORWARD and stride == 1 and co == ci)


def _flipped(w):
    """W'[ci, co, kh, kw] = W[co, ci, K - 1 - kh, K - 1 - kw], channels-last: the weight of a data gradient run as a forward."""
    return torch.flip(w, (2, 3)).transpose(0, 1).contiguous(memory_format=_CL)


def _bf16_weights(weight, bias, shadow, flip: bool):
    """-> (w, wt, b) of a 3x3 convolution: the bf16 channels-last copy of the fp32 master, its flipped copy or None, the bf16
    bias or None.  ``shadow`` = (w, wt): both made for the caller's whole segment in one launch (``TrainEncoder._tick``), wt
    None where the data gradient does not run on it; ``flip``: make a missing wt here (in the forward, off the backward's
    critical chain)."""
    w, wt = shadow if shadow is not None else (weight.detach().to(dtype=torch.bfloat16, memory_format=_CL), None)
    if wt is None and flip:
        wt = _flipped(w)
    return w, wt, None if bias is None else bias.detach().to(torch.bfloat16)


def _subsample(x, stride: int):
    """x[:, :, ::stride, ::stride] of a channels-last activation as a tensor of its own: one 16-byte-per-thread launch for stride 2
    in bf16 (the stock strided copy moves 2 bytes per thread: 52 us for layer2's downsample input at config 4, 5 with this)."""
    B, C, H, W = x.shape
    if stride == 2 and x.is_cuda and x.dtype == torch.bfloat16 and C % 8 == 0 and x.is_contiguous(memory_format=_CL):
        from . import _lib
        y = torch.empty((B, C, (H + 1) // 2, (W + 1) // 2), dtype=x.dtype, device=x.device, memory_format=_CL)
        _lib.call("dmm_subsample2_bf16", x.device, x.data_ptr(), B, H, W, C, y.data_ptr(),
                  torch.cuda.current_stream(x.device).cuda_stream)
        return y
    return x[:, :, ::stride, ::stride].contiguous(memory_format=_CL)


def _upsample_zero(dy, full, stride: int):
    """The gradient of ``_subsample``: a ``full``-shaped tensor with dy at the sampled positions and zero elsewhere, written once."""
    B, C, H, W = full
    if stride == 2 and dy.is_cuda and dy.dtype == torch.bfloat16 and C % 8 == 0:
        from . import _lib
        dy = dy.contiguous(memory_format=_CL)
        dx = torch.empty(full, dtype=dy.dtype, device=dy.device, memory_format=_CL)
        _lib.call("dmm_upsample2_zero_bf16", dy.device, dy.data_ptr(), B, H, W, C, dx.data_ptr(),
                  torch.cuda.current_stream(dy.device).cuda_stream)
        return dx
    dx = torch.zeros(full, dtype=dy.dtype, device=dy.device).to(memory_format=_CL)
    dx[:, :, ::stride, ::stride] = dy
    return dx


class _Conv1x1Fn(torch.autograd.Function):
    """1x1 convolution of a channels-last bf16 activation with an fp32 MASTER weight: y = X W^T on the [B*H*W, Cin] activation
    matrix (hipBLASLt); backward: dX = dY W (hipBLASLt) and dW = dY^T X straight into an fp32 gradient for the master
    (``dmm_wgrad_bf16``: MFMA, split over the rows) -- no bf16 weight gradient, no cast launch.  stride 2 = a row subsample."""

    @staticmethod
    def forward(ctx, x, weight, stride, shadow=None):
        co, ci = weight.shape[0], weight.shape[1]
        ctx.full = None
        if stride != 1:
            ctx.full = tuple(x.shape)
            x = _subsample(x, stride)
        B, _, H, W = x.shape
        # shadow: the bf16 copy of the weight the caller refreshed for its whole segment in one multi-tensor launch
        w = shadow if shadow is not None else weight.detach().view(co, ci).to(torch.bfloat16)
        y = torch.mm(x.permute(0, 2, 3, 1).reshape(B * H * W, ci), w.t())
        ctx.save_for_backward(x, w)
        ctx.stride = stride
        return y.view(B, H, W, co).permute(0, 3, 1, 2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        from . import _lib
        x, w = ctx.saved_tensors
        B, ci, H, W = x.shape
        co = w.shape[0]
        dy = dy.contiguous(memory_format=_CL)
        dy_rows = dy.permute(0, 2, 3, 1).reshape(B * H * W, co)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.mm(dy_rows, w).view(B, H, W, ci).permute(0, 3, 1, 2)
            if ctx.full is not None:
                dx = _upsample_zero(dx, ctx.full, ctx.stride)
        dw = torch.empty((co, ci, 1, 1), dtype=torch.float32, device=x.device)
        _wgrad(("1x1", dy_rows, x, (B * H * W, co, ci), dw))
        return dx, dw, None, None


class _Conv3x3Fn(torch.autograd.Function):
    """3x3 / padding 1 convolution (stride 1 or 2) of a channels-last bf16 activation with an fp32 MASTER weight: forward and
    data gradient on MIOpen, the weight gradient by ``dmm_wgrad3x3_bf16`` (implicit patch matrix, MFMA, fp32 out) -- MIOpen's
    bf16 weight-gradient solvers cost a zeroing and a cast launch each and clear their workspace with a memset node.

    ``own`` (the deterministic mode with ``set_deterministic_conv("own")``, resolved in the forward and kept for the backward):
    forward, bias add and data gradient by ``dmm_conv3x3_bf16`` -- under cudnn.deterministic MIOpen answers with its naive
    reference kernel.  The data gradient is then ALWAYS the forward convolution of dy with the flipped, transposed weight; at
    stride 2, of dy spread over zeros to the input's size, at stride 1 (``ops.conv3x3_dgrad_bf16``)."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, shadow=None):
        own = _own_conv_now()
        flip = _dgrad_on_flipped(own, stride, weight.shape[0], weight.shape[1])
        w, wt, b = _bf16_weights(weight, bias, shadow, flip and x.requires_grad and (own or shadow is None))
        if not flip:
            wt = None
        if own:
            from . import ops
            y = ops.conv3x3_bf16(x, w, b, stride)
        else:
            y = F.conv2d(x, w, b, stride, 1)
        ctx.save_for_backward(x, w, wt if wt is not None else w)
        ctx.stride, ctx.has_bias, ctx.flipped, ctx.det, ctx.own = stride, bias is not None, wt is not None, _det_now(), own
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, w, wt = ctx.saved_tensors
        B, ci, H, W = x.shape
        co = w.shape[0]
        dy = dy.contiguous(memory_format=_CL)
        dx = None
        if ctx.needs_input_grad[0] and ctx.own:
            from . import ops
            dx = ops.conv3x3_dgrad_bf16(dy, wt, (H, W), ctx.stride)
        elif ctx.needs_input_grad[0]:
            with library_flags(ctx.det):
                if ctx.flipped:
                    dx = F.conv2d(dy, wt, None, 1, 1)
                else:
                    dx = torch.ops.aten.convolution_backward(dy, x, w, None, [ctx.stride] * 2, [1, 1], [1, 1], False, [0, 0], 1,
                                                             [True, False, False])[0]
        Ho, Wo = dy.shape[2], dy.shape[3]
        dw = torch.empty((co, ci, 3, 3), dtype=torch.float32, device=x.device)      # the master's own layout
        _wgrad(("3x3", dy, x, (B, H, W, ci, co, ctx.stride, Ho, Wo), dw))
        db = _channel_sums(dy, ctx.det) if ctx.has_bias else None
        return dx, dw, db, None, None


class _ConvNarrowFn(torch.autograd.Function):
    """A narrow 3x3 / padding 1 / stride 1 convolution (``_narrow_ok``) of a channels-last bf16 activation with an fp32 MASTER
    weight in the deterministic mode under ``set_deterministic_conv("own_all")`` (resolved by ``_conv`` in the forward; the
    backward needs no setting): forward, bias add and data gradient by ``dmm_conv3x3_narrow_bf16`` -- the data gradient is the
    forward convolution of dy with the flipped, transposed weight --, the weight gradient by ``dmm_wgrad3x3_narrow_bf16``
    (deferred and captured like the others), the bias gradient by the deterministic statistics kernel."""

    @staticmethod
    def forward(ctx, x, weight, bias, shadow=None):
        from . import ops
        w, wt, b = _bf16_weights(weight, bias, shadow, x.requires_grad)
        y = ops.conv3x3_narrow_bf16(x, w, b)
        ctx.save_for_backward(x, wt if wt is not None else w)
        ctx.has_bias, ctx.flipped, ctx.det = bias is not None, wt is not None, _det_now()
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        from . import ops
        x, wt = ctx.saved_tensors
        B, ci, H, W = x.shape
        co = dy.shape[1]
        dy = dy.contiguous(memory_format=_CL)
        dx = None
        if ctx.needs_input_grad[0]:
            if not ctx.flipped:                              # (x began to require a gradient after the forward: not a TrainEncoder flow)
                wt = _flipped(wt)
            dx = ops.conv3x3_narrow_dgrad_bf16(dy, wt)
        dw = torch.empty((co, ci, 3, 3), dtype=torch.float32, device=x.device)      # the master's own layout
        _wgrad(("3x3n", dy, x, (B, H, W, ci, co), dw))
        db = _channel_sums(dy, ctx.det) if ctx.has_bias else None
        return dx, dw, db, None


class _ConvStemFn(torch.autograd.Function):
    """The 7x7 / stride 2 / padding 3 stem (``_stem_ok``) of a channels-last bf16 image with an fp32 MASTER weight in the
    deterministic mode under ``set_deterministic_conv("own_stem")`` (resolved by ``_conv`` in the forward; the backward needs no
    setting): forward and bias add by ``dmm_conv7x7s2_stem_bf16``, the weight gradient -- fp32 from the kernel, in the
    master's layout -- by ``dmm_wgrad7x7s2_stem_bf16`` (deferred and captured like the others), the bias gradient by the
    deterministic statistics kernel.  No data gradient: ``_conv`` sends an input that requires one to ``_DetConvFn``."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        from . import ops
        w, _, b = _bf16_weights(weight, bias, None, False)
        y = ops.conv7x7s2_stem_bf16(x, w, b)
        ctx.save_for_backward(x)
        ctx.has_bias, ctx.det = bias is not None, _det_now()
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        if ctx.needs_input_grad[0]:
            raise RuntimeError("_ConvStemFn has no data gradient: the image must not require one")
        dy = dy.contiguous(memory_format=_CL)
        dw = torch.empty((64, 3, 7, 7), dtype=torch.float32, device=x.device)        # the master's own layout
        _wgrad(("7x7s", dy, x, (x.shape[0], x.shape[2], x.shape[3]), dw))
        db = _channel_sums(dy, ctx.det) if ctx.has_bias else None
        return None, dw, db


def _channel_sums(dy, det: bool = False):
    """sum over (batch, rows, columns) of a channels-last bf16 gradient in fp32 (a bias gradient): the statistics kernel's first
    row -- one launch where ``dy.float().sum((0, 2, 3))`` is a cast of the whole tensor and a reduction.  ``det``: the
    deterministic statistics kernel and a fold launch (no consumer kernel folds this slab)."""
    B, C, H, W = dy.shape
    if dy.is_cuda and dy.dtype == torch.bfloat16 and _stats_channels_ok(C):
        from . import _lib
        R, stream = B * H * W, torch.cuda.current_stream(dy.device).cuda_stream
        form, scratch, stats = _bn_scratch(det, R, C, 1, dy.device)
        _lib.call(f"dmm_bn_stats{form}_grouped_bf16", dy.device, dy.data_ptr(), R, C, 1, *scratch, stream)
        if det:
            stats = torch.empty((2 * C,), dtype=torch.float32, device=dy.device)
            _lib.call("dmm_bn_fold_det", dy.device, *scratch, R, C, 1, stats.data_ptr(), stream)
        return stats[:C]
    return dy.float().sum((0, 2, 3))


def _conv(x, m: nn.Conv2d, dtype, linear_1x1: bool = True, own_wgrad: bool = True, shadow=None):
    """Convolution ``m`` (fp32 master weight) on a channels-last activation in the compute dtype.  On the device in bf16: a
    1x1 convolution is the product of the activation matrix with W^T (hipBLASLt forward and data gradient), a 3x3 one runs on
    MIOpen, and both take their weight gradient from ``dmm_wgrad*_bf16``; anything else (the 7x7 stem, widths that are not a
    multiple of 64, fp32 mode, the CPU) goes through the stock ops with a differentiable cast of the weight -- except, in the
    deterministic mode under ``set_deterministic_conv("own_all")``, a narrow 3x3 convolution (``_narrow_ok``), which runs on
    ``_ConvNarrowFn``, and, under ``"own_stem"``, the 7x7 stem (``_stem_ok``) of an input that requires no gradient, which runs
    on ``_ConvStemFn``."""
    route = _conv_route(m, linear_1x1, own_wgrad) if x.is_cuda and dtype == torch.bfloat16 and x.dtype == dtype else None
    if route == "1x1":
        return _Conv1x1Fn.apply(x.contiguous(memory_format=_CL), m.weight, m.stride[0], shadow)
    if route == "3x3":
        return _Conv3x3Fn.apply(x.contiguous(memory_format=_CL), m.weight, m.bias, m.stride[0], shadow)
    if route == "narrow":
        return _ConvNarrowFn.apply(x.contiguous(memory_format=_CL), m.weight, m.bias, shadow)
    if route == "stem" and not x.requires_grad:
        return _ConvStemFn.apply(x.contiguous(memory_format=_CL), m.weight, m.bias)
    b = None if m.bias is None else m.bias.to(dtype)
    if linear_1x1 and m.kernel_size == (1, 1) and m.padding == (0, 0) and m.groups == 1 and m.dilation == (1, 1):
        if m.stride != (1, 1):
            x = x[:, :, ::m.stride[0], ::m.stride[1]].contiguous(memory_format=_CL)
        w = m.weight.view(m.out_channels, m.in_channels).to(dtype)
        return F.linear(x.permute(0, 2, 3, 1), w, b).permute(0, 3, 1, 2)
    w = m.weight.to(dtype=dtype, memory_format=_CL)
    if x.is_cuda and _det_now():
        return _DetConvFn.apply(x, w, b, m.stride, m.padding, m.dilation, m.groups)
    return F.conv2d(x, w, b, m.stride, m.padding, m.dilation, m.groups)


def _conv_as_gemm(x, w, b, stride, padding):
    """conv2d(x, w, b, stride, padding) of a plain convolution as unfold + one matrix product -> channels-last."""
    co, ci, kh, kw = w.shape
    B, _, H, W = x.shape
    Ho = (H + 2 * padding[0] - kh) // stride[0] + 1
    Wo = (W + 2 * padding[1] - kw) // stride[1] + 1
    cols = F.unfold(x, (kh, kw), 1, padding, stride).transpose(1, 2).reshape(B * Ho * Wo, ci * kh * kw)
    y = torch.mm(cols, w.reshape(co, ci * kh * kw).t())
    if b is not None:
        y = y + b
    return y.view(B, Ho, Wo, co).permute(0, 3, 1, 2)


class _DetConvFn(torch.autograd.Function):
    """The stock convolution (7x7 stem, head convolutions outside the own-kernel envelope) in the deterministic mode.  Its
    backward, which autograd runs after the TrainEncoder call has returned, must not reach MIOpen's split-K weight-gradient
    solvers (two eager steps differed in the stem's and the level-2 head's gradients), nor their cudnn.deterministic form
    (MIOpen's naive reference kernel on gfx950: ~130 ms per call at config 4).  So: the weight gradient is an unfold + ONE
    GEMM (hipBLASLt), the data gradient of a stride-1 convolution the forward convolution of dy with the flipped, transposed
    weight, the bias gradient a torch reduction -- the convolutions under cudnn.deterministic, like the rest of the mode's
    library calls.

    With ``set_deterministic_conv("own")`` (and the settings above it) the forward of a plain convolution (no groups, no dilation) and its stride-1 data
    gradient (the forward convolution of dy) are an unfold + ONE GEMM too, the product the weight gradient already takes: the
    7x7 stem and the 32-channel heads leave MIOpen's naive kernel (profiles/r08_deterministic_conv.md)."""

    @staticmethod
    def forward(ctx, x, w, b, stride, padding, dilation, groups):
        ctx.save_for_backward(x, w)
        ctx.conf = (tuple(stride), tuple(padding), tuple(dilation), groups, b is not None)
        ctx.own = get_deterministic_conv() in _OWN_SETTINGS
        if ctx.own and "forward" in _DET_AS_GEMM and groups == 1 and tuple(dilation) == (1, 1):
            return _conv_as_gemm(x, w, b, tuple(stride), tuple(padding))
        with library_flags(True):
            return F.conv2d(x, w, b, stride, padding, dilation, groups)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        stride, padding, dilation, groups, has_b = ctx.conf
        need = ctx.needs_input_grad
        co, cig, kh, kw = w.shape
        dx = dw = db = None
        plain = groups == 1 and dilation == (1, 1)
        if need[0]:
            if plain and stride == (1, 1) and padding[0] <= kh - 1 and padding[1] <= kw - 1:
                wt = _flipped(w)
                if ctx.own and "dgrad" in _DET_AS_GEMM:
                    dx = _conv_as_gemm(dy, wt, None, (1, 1), (kh - 1 - padding[0], kw - 1 - padding[1]))
                else:
                    with library_flags(True):
                        dx = F.conv2d(dy, wt, None, 1, (kh - 1 - padding[0], kw - 1 - padding[1]))
            else:
                with library_flags(True):
                    dx = torch.ops.aten.convolution_backward(dy, x, w, None, list(stride), list(padding), list(dilation),
                                                             False, [0, 0], groups, [True, False, False])[0]
        if need[1]:
            if plain:
                B, _, Ho, Wo = dy.shape
                cols = F.unfold(x, (kh, kw), dilation, padding, stride)                     # [B, ci*kh*kw, Ho*Wo]
                cols = cols.transpose(1, 2).reshape(B * Ho * Wo, cig * kh * kw)
                dyr = dy.permute(0, 2, 3, 1).reshape(B * Ho * Wo, co)
                dw = torch.mm(dyr.t(), cols).view(co, cig, kh, kw)
            else:
                with library_flags(True):
                    dw = torch.ops.aten.convolution_backward(dy, x, w, None, list(stride), list(padding), list(dilation),
                                                             False, [0, 0], groups, [False, True, False])[1]
        if has_b and need[2]:
            # 16-bit gradients are summed in fp32; wider ones in their own precision (an fp32 sum of fp64 terms loses digits)
            wide = dy.float() if dy.element_size() < 4 else dy
            db = wide.sum((0, 2, 3)).to(dy.dtype)
        return dx, dw, db, None, None, None, None


class TrainEncoder(nn.Module):
    """``TrainEncoder(FeatureEncoder(...))``: same ``forward(img) -> feature dict`` (model_encoder.py:157-160), same
    parameters (``self.src`` is the wrapped encoder: build the optimiser / save checkpoints from it as before), training
    mode, bf16 channels-last, HIP-graph replays.  ``backbone_feature`` comes back as fp32 NCHW (what the ROI feature
    kernel's backward takes); ``refine_input_feat`` / ``body_feature`` as bf16 channels-last.

    ``skips_need_grad``: the decoder's inputs (``refine_input_feat``: ``sk_k`` + ``bn_k``) take part in the backward.  A
    trainer with the refine decoder leaves it on; a step that never sends a gradient there (bench.py's config 4: no decoder)
    switches it off so that the backward graph does not run those four convolutions on zeros.

    A/B switches (each measured in ``profiles/r06_cfg4_train_encoder_steps.md``; the defaults are the fast settings):
    ``graphs`` (False: the same segment functions eagerly), ``linear_1x1`` (False: 1x1 convolutions on MIOpen too),
    ``fused_bn`` (False: ``torch.nn.BatchNorm2d`` + add + relu), ``own_wgrad`` (False: the libraries' weight gradients),
    ``overlap_wgrad`` (False: one stream -- weight gradients inline in the chain, heads on the main stream), ``layer3_parts``
    (segments layer3 is cut into), ``miopen_find`` (let MIOpen search its solvers during the warm-up of a new shape; the
    shapes of BASELINE configs[3] ship in ``dmm_net_amd/miopen_db``)."""

    def __init__(self, encoder: FeatureEncoder, dtype=torch.bfloat16, graphs: bool = True, linear_1x1: bool = True,
                 fused_bn: bool = True, own_wgrad: bool = True, overlap_wgrad: bool = True, skips_need_grad: bool = True,
                 miopen_find: bool = False, warmup: int = 2, layer3_parts: int = 3):
        super().__init__()
        if not isinstance(encoder.base, ResNetBody):
            raise NotImplementedError("TrainEncoder is the bf16 channels-last training form of the ResNet bodies")
        self.src = encoder
        self.dtype, self.graphs, self.linear_1x1, self.fused_bn = dtype, bool(graphs), bool(linear_1x1), bool(fused_bn)
        self.own_wgrad = bool(own_wgrad)
        self.overlap_wgrad = bool(overlap_wgrad) and self.own_wgrad
        self.skips_need_grad, self.miopen_find, self.warmup = bool(skips_need_grad), bool(miopen_find), int(warmup)
        # the body as a CHAIN of segments: stem | layer1 | layer2 | layer3 in ``layer3_parts`` runs of blocks | layer4, then the
        # heads.  (name, the blocks it runs, which of the four taps x2..x5 its output is, or None.)  Finer segments = a finer
        # pipeline between the backward chain and the weight-gradient graphs on the side stream: the exposed tail is the FIRST
        # segment's weight gradients, and a segment's weight gradients should not outlast the next segment's chain (layer3 is
        # half of a ResNet-101: as ONE segment its 2.5 ms of weight gradients ran beside 1.7 ms of chain).
        body = encoder.base
        l3 = list(body.layer3)
        n3 = max(1, min(int(layer3_parts), len(l3)))
        cuts = [round(i * len(l3) / n3) for i in range(n3 + 1)]
        chain = [("stem", ["stem"], None), ("layer1", list(body.layer1), 0), ("layer2", list(body.layer2), 1)]
        chain += [(f"layer3_{i}" if n3 > 1 else "layer3", l3[cuts[i]:cuts[i + 1]], 2 if i == n3 - 1 else None) for i in range(n3)]
        chain.append(("layer4", list(body.layer4), 3))
        self.segments = tuple(c[0] for c in chain) + ("heads",)
        # The call state and the caches: plain attributes (lists, dicts, tuples and ints -- ``nn.Module.__setattr__`` only takes
        # Parameters, Modules and registered buffers aside), so none of it is module state.
        self._chain = chain
        self._plans = {}                         # (shape, device, mode) -> [_Plan]
        self._hubs = {}                          # device index -> {segment: hub leaf}
        self._pending = {}                       # segment -> plans whose backward of it ran in the current backward pass
        self._late = None                        # (segment, plans) whose hand-over waits for the next segment's (``_flush``)
        self._ticked = {}                        # id(module) -> covered by the running segment's _tick (rebuilt per call)
        self._bn_groups = 1                      # the running call's ``bn_groups``
        self._shadows = {}                       # id(1x1 conv) -> its persistent bf16 weight copy
        self._wcast = {}                         # ids of a segment's 1x1 convs -> the device table of ``_cast_1x1``
        self._wprep = {}                         # ids of a segment's 3x3 convs + the setting -> ``_prep_3x3``'s table and copies
        self._storage = None                     # the addresses of parameters and buffers the plans were captured with

    def _invalidate(self, hubs: bool):
        """Drops what a change of the parameters' storage makes stale: the captured graphs (which hold the old addresses) and
        the bf16 weight copies with their tables; ``hubs``: the hub leaves too (``_apply``: the module may change device)."""
        for d in (self._plans, self._shadows, self._pending, self._wprep, self._wcast) + ((self._hubs,) if hubs else ()):
            d.clear()

    def _apply(self, fn, *args, **kwargs):
        # .to() / .cuda() / .float() re-create the parameters' storage, maybe on another device; the next forward captures again
        self._invalidate(hubs=True)
        return super()._apply(fn, *args, **kwargs)

    # ---- the encoder in segments (plain functions of tensors; parameters come from self.src) ------------------------
    def _cbr(self, x, conv, bn, relu, residual=None, fork=False):
        t = self._ticked
        y = _conv(x, conv, self.dtype, self.linear_1x1, self.own_wgrad, t.get(id(conv)))
        return _bn_act(y, bn, relu, residual, self.fused_bn, counted=id(bn) in t, groups=self._bn_groups, fork=fork)

    def _tick(self, name: str, x: torch.Tensor, mods=None):
        """Per-segment housekeeping in ONE launch each instead of one per layer: ``num_batches_tracked += 1`` of every
        BatchNorm that takes the fused kernels (116 launches per ResNet-101 step before), and the bf16 copies of the 1x1
        weights (70), and of the 3x3 ones.  ``_ticked`` tells ``_cbr`` which modules were covered."""
        t = self._ticked
        if not (x.is_cuda and self.dtype == torch.bfloat16 and self.training):
            return
        mods = [m for mod in (self._seg_modules()[name] if mods is None else mods) for m in mod.modules()]
        if self.fused_bn:
            bns = [m for m in mods if isinstance(m, nn.BatchNorm2d) and m.training and _bn_fusable(m)]
            if bns:
                with torch.no_grad():
                    torch._foreach_add_([m.num_batches_tracked for m in bns], self._bn_groups)
                for m in bns:
                    t[id(m)] = True
        routes = [(m, _conv_route(m, self.linear_1x1, self.own_wgrad)) for m in mods]     # (where ``_conv`` will send them)
        convs = [m for m, r in routes if r == "1x1"]
        if convs:
            dst = []
            for m in convs:
                w = self._shadows.get(id(m))
                if w is None or w.device != m.weight.device:
                    w = self._shadows[id(m)] = torch.empty((m.out_channels, m.in_channels), dtype=torch.bfloat16,
                                                           device=m.weight.device)
                dst.append(w)
                t[id(m)] = w
            self._cast_1x1(convs, dst)
        convs = [m for m, r in routes if r in ("3x3", "narrow")]
        if convs:                                            # (the narrow heads share their level's one wprep launch)
            self._prep_3x3(convs, t)

    def _cast_1x1(self, convs, dst):
        """The bf16 copies of a segment's 1x1 weights by ONE launch over a device table (``torch._foreach_copy_`` with a dtype
        change: 20-38 us per segment); inside a capture without a table yet, the multi-tensor copy."""
        from . import _lib
        memo = self._wcast
        key = tuple(id(m) for m in convs)
        ptrs = tuple(m.weight.data_ptr() for m in convs) + tuple(d.data_ptr() for d in dst)
        got = memo.get(key)
        ok = all(m.weight.is_contiguous() and m.weight.numel() % 8 == 0 and m.weight.data_ptr() % 16 == 0 for m in convs) \
            and all(d.data_ptr() % 16 == 0 for d in dst)        # (16-byte pieces; e.g. parameters that are views of a flat buffer)
        if not ok or ((got is None or got[0] != ptrs) and torch.cuda.is_current_stream_capturing()):
            with torch.no_grad():
                torch._foreach_copy_(dst, [m.weight.detach().view(m.out_channels, m.in_channels) for m in convs])
            return
        dev = convs[0].weight.device
        if got is None or got[0] != ptrs:
            rec, blk = [], 0
            for m, d in zip(convs, dst):
                n = m.weight.numel()
                rec += [m.weight.data_ptr(), d.data_ptr(), n, blk]
                blk += (n + 8191) // 8192
            got = memo[key] = (ptrs, _lib.small_to_device(rec, torch.int64, dev), blk)
        _lib.call("dmm_cast_many_bf16", dev, got[1].data_ptr(), len(convs), got[2], torch.cuda.current_stream(dev).cuda_stream)

    def _prep_3x3(self, convs, t):
        """bf16 channels-last copies of the 3x3 weights of one segment (and the flipped + transposed ones their data gradients
        run on as forward convolutions) by ONE launch over a device table -- a cast, a layout copy and a flip launch per
        convolution before: 99 launches of ~5.5 us in a ResNet-101 forward."""
        from . import _lib
        memo = self._wprep
        own = _own_conv_now()                           # every data gradient runs on the flipped weight, whatever the shape
        # (tables of one setting are not reused under another)
        key = tuple(id(m) for m in convs) + (own, _narrow_conv_now(), _stem_conv_now())
        ptrs = tuple(m.weight.data_ptr() for m in convs)
        got = memo.get(key)
        if got is None or got[0] != ptrs:
            if torch.cuda.is_current_stream_capturing():
                # no table yet and no upload inside a capture: per-convolution copies.  Copies an earlier tick of these
                # modules left in ``t`` (the warm-up's) go: nothing in THIS graph would refresh them, and its replays would
                # read the weights of the day of the capture
                for m in convs:
                    t.pop(id(m), None)
                return
            dev = convs[0].weight.device
            rec, pairs, tile = [], [], 0
            for m in convs:
                co, ci = m.out_channels, m.in_channels
                w = torch.empty((co, ci, 3, 3), dtype=torch.bfloat16, device=dev, memory_format=_CL)
                wt = None
                if _dgrad_on_flipped(own, m.stride[0], co, ci):
                    wt = torch.empty((ci, co, 3, 3), dtype=torch.bfloat16, device=dev, memory_format=_CL)
                rec += [m.weight.data_ptr(), w.data_ptr(), 0 if wt is None else wt.data_ptr(), co | (ci << 32), tile]
                tile += (co // 32) * (ci // 32)
                pairs.append((w, wt))
            table = _lib.small_to_device(rec, torch.int64, dev)
            got = memo[key] = (ptrs, table, pairs, tile)
        _, table, pairs, tiles = got
        dev = convs[0].weight.device
        _lib.call("dmm_wprep3x3_bf16", dev, table.data_ptr(), len(convs), tiles, torch.cuda.current_stream(dev).cuda_stream)
        for m, pr in zip(convs, pairs):
            t[id(m)] = pr

    def _block(self, x, blk, fork=False):
        """One residual block.  ``x``: a tensor, or the PAIR (x, alias) a predecessor made with ``fork`` -- the first convolution
        takes one, the identity branch (or the downsample convolution) the other, so that the two gradients reach the
        predecessor's BatchNorm separately and are added inside its backward kernels (autograd's own add of them: one launch
        over the whole tensor per block).  ``fork``: return such a pair for the next block."""
        xa, xb = x if isinstance(x, tuple) else (x, x)
        idt = xb if blk.downsample is None else self._cbr(xb, blk.downsample[0], blk.downsample[1], False)
        if isinstance(blk, Bottleneck):
            out = self._cbr(xa, blk.conv1, blk.bn1, True)
            out = self._cbr(out, blk.conv2, blk.bn2, True)
            return self._cbr(out, blk.conv3, blk.bn3, True, idt, fork=fork)
        out = self._cbr(xa, blk.conv1, blk.bn1, True)
        return self._cbr(out, blk.conv2, blk.bn2, True, idt, fork=fork)

    def _layer(self, x, layer):
        for q, blk in enumerate(layer):
            x = self._block(x, blk, fork=q + 1 < len(layer))
        return x

    def _seg_body(self, name: str, x):
        """One body segment of the chain: (the stem when it is the first,) its blocks in order.  -> (output,)"""
        body = self.src.base
        self._tick(name, x)
        ops_ = next(c[1] for c in self._chain if c[0] == name)
        for q, op in enumerate(ops_):
            if isinstance(op, str):                                      # "stem": conv1 -> bn1 -> relu -> maxpool
                x = x.to(self.dtype).contiguous(memory_format=_CL)
                x = body.maxpool(self._cbr(x, body.conv1, body.bn1, True))
            else:
                # (the segment's last block hands ONE tensor on: its consumers are other graphs)
                x = self._block(x, op, fork=q + 1 < len(ops_) and not isinstance(ops_[q + 1], str))
        return (x,)

    def _head(self, x, head):
        out = self._cbr(x, head[0], head[1], True)                       # base.py:43-54: conv -> BN -> ReLU -> conv -> BN
        return self._cbr(out, head[3], head[4], False)

    def _head_level(self, k: int, x):
        """The heads of ONE pyramid level (k = 2..5) on that level's tap: ``prop_k`` (-> fp32 NCHW: what the ROI feature kernel,
        forward and backward, works on) and the decoder's skip projection ``bn_k(sk_k(x))``.  -> (prop, skip).  The level ticks
        for itself, eagerly and in a plan's capture alike: the warm-up of a plan then makes the weight tables the level's
        captured graph launches from (``_prep_3x3`` uploads none inside a capture)."""
        s = self.src
        self._tick("heads", x, mods=self._head_modules(k))
        prop = self._head(x, getattr(s, f"prop{k}"))
        with (torch.enable_grad() if self.skips_need_grad else torch.no_grad()):
            skip = self._cbr(x, getattr(s, f"sk{k}"), getattr(s, f"bn{k}"), False)
        return prop.float().contiguous(), skip

    def _head_modules(self, k: int):
        s = self.src
        return [getattr(s, f"prop{k}"), getattr(s, f"sk{k}"), getattr(s, f"bn{k}")]

    def _head_params(self, k: int) -> List[nn.Parameter]:
        mods = self._head_modules(k)
        if not self.skips_need_grad:
            mods = mods[:1]
        return [p for m in mods for p in m.parameters() if p.requires_grad]

    def _seg_heads(self, x2, x3, x4, x5):
        lv = [self._head_level(k, x) for k, x in ((2, x2), (3, x3), (4, x4), (5, x5))]
        return self._heads_order(lv)

    @staticmethod
    def _heads_order(levels):
        """[``_head_level(k)`` = (prop_k, skip_k) for k = 2..5] -> the heads' outputs as ``_pack`` takes them: props 2..5, skips
        5..2."""
        return tuple(p for p, _ in levels) + tuple(sk for _, sk in reversed(levels))

    def _seg_modules(self) -> Dict[str, List[nn.Module]]:
        s, body = self.src, self.src.base
        out = {}
        for name, ops, _ in self._chain:
            mods = []
            for op in ops:
                mods += [body.conv1, body.bn1] if isinstance(op, str) else [op]
            out[name] = mods
        out["heads"] = [s.prop2, s.prop3, s.prop4, s.prop5, s.sk2, s.sk3, s.sk4, s.sk5, s.bn2, s.bn3, s.bn4, s.bn5]
        return out

    def _seg_params(self) -> Dict[str, List[nn.Parameter]]:
        out = {}
        for name, mods in self._seg_modules().items():
            if name == "heads":
                out[name] = [p for k in (2, 3, 4, 5) for p in self._head_params(k)]
            else:
                out[name] = [p for m in mods for p in m.parameters() if p.requires_grad]
        return out

    def _arena_floats(self, name: str, backward: bool) -> int:
        """Upper bound of what a segment's graph takes from its arena: [2, C] per BatchNorm and per convolution bias (+ 64
        floats of rounding per request), the same forward and backward (the weight-gradient kernels overwrite their
        outputs: nothing to zero)."""
        n = 0
        for mod in self._seg_modules()[name]:
            for m in mod.modules():
                if isinstance(m, nn.BatchNorm2d):
                    n += self._bn_groups * 2 * m.num_features + 64
                elif isinstance(m, nn.Conv2d) and m.bias is not None:
                    n += 2 * m.out_channels + 64            # (its bias gradient: the statistics kernel's sums)
        return n + 1024

    @staticmethod
    def _pack(taps, heads):
        return {"backbone_feature": tuple(heads[:4]), "refine_input_feat": tuple(heads[4:]), "body_feature": tuple(taps)}

    def _eager(self, img):
        x, taps = img, [None] * 4
        for name, _, tap in self._chain:
            (x,) = self._seg_body(name, x)
            if tap is not None:
                if _det_now() and x.requires_grad and tap < 3:
                    # a tap's gradient as the captured plan forms it: (the body's terms) + (the heads' terms), one add --
                    # autograd would add the four terms in its arrival order, and bf16 sums are not associative
                    x, taps[tap] = _TapSplit.apply(x)
                else:
                    taps[tap] = x
        return self._pack(taps, self._seg_heads(*taps))

    # ---- entry ---------------------------------------------------------------------------------------------------------
    def forward(self, img: torch.Tensor, bn_groups: int = 1) -> Dict[str, Tuple[torch.Tensor, ...]]:
        """``bn_groups`` = G > 1 (training): ``img`` is G consecutive sub-batches and every BatchNorm takes its batch statistics
        per sub-batch -- the features, gradients and running statistics of G calls on the sub-batches in order (the reference's
        trainer calls the encoder once per frame step of a clip, trainer.py:95-131; a clip's frames stacked along the batch
        with G = frames is the same computation in one pass: convolutions never mix images)."""
        assert img.dim() == 4 and img.shape[1] == 3, img.shape           # model_encoder.py:91-92
        bn_groups = int(bn_groups) if self.training else 1
        assert bn_groups >= 1 and img.shape[0] % bn_groups == 0, (img.shape[0], bn_groups)
        self._bn_groups = bn_groups
        self._ticked.clear()
        self._late = None                        # (a hand-over left behind by a backward pass that raised)
        det = is_deterministic()
        if not (self.graphs and img.is_cuda and self.training and torch.is_grad_enabled()):
            with _det_scope(det):
                return self._eager(img)
        # the captured graphs hold the ADDRESSES of parameters and buffers: storage that was swapped since (``p.data = ...``,
        # ``load_state_dict(assign=True)``; ``.to()`` goes through ``_apply``) makes every plan stale -- captured again
        fp = tuple(t.data_ptr() for t in self.src.parameters()) + tuple(t.data_ptr() for t in self.src.buffers())
        if fp != self._storage:
            if self._storage is not None:
                self._invalidate(hubs=False)             # (the hub leaves hold no address of a parameter: they stay)
            self._storage = fp
        # (the mode is part of the key: a graph captured in one mode never replays in the other)
        conv = get_deterministic_conv() if det else "library"
        key = (tuple(img.shape), img.dtype, img.device.index, self.skips_need_grad, bn_groups, conv,
               conv in _OWN_SETTINGS, det)
        plans = self._plans.setdefault(key, [])
        # a plan's static buffers belong to ONE forward until its backward has run: a second forward of the same shape before
        # that (the trainer's clip: one encoder call per frame, one backward; trainer.py:95-131) takes / captures another plan
        plan = next((p for p in plans if not p.busy), None)
        if plan is None:
            try:
                with _CAPTURE_LOCK, _det_scope(det):
                    plan = _Plan(self, img)
            except CaptureFailed as e:
                # a capture was invalidated (an API call of another thread of the process the runtime does not tolerate beside a
                # capture, even in thread-local mode): this call runs the same functions eagerly, the next call of the shape
                # captures again.  The calling thread's stream is intact (graphs.SafeGraph).
                import warnings
                warnings.warn(f"TrainEncoder: graph capture failed ({str(e)[:200]}); this call runs eagerly", RuntimeWarning)
                torch.cuda.synchronize(img.device)
                self._ticked.clear()
                with _det_scope(det):
                    return self._eager(img)
            plans.append(plan)
        return plan.run(img)

    def _hubs_for(self, device):
        hubs = self._hubs.get(device.index)
        if hubs is None:
            hubs = self._hubs[device.index] = {}
            for name in self.segments:
                h = hubs[name] = torch.zeros((), device=device, requires_grad=True)
                h.register_post_accumulate_grad_hook(lambda t, name=name: self._flush(name, t))
        return hubs

    def _flush(self, name: str, hub: torch.Tensor):
        """The hub leaf of ``name`` has received its gradient: every plan that took part in this backward pass has replayed the
        segment's backward graph(s).  Their parameter gradients are summed (into the first plan's static buffers) and handed
        over: ``p.grad`` set / accumulated, post-accumulate-grad hooks called -- once per parameter and backward pass, like
        autograd's own AccumulateGrad.  With the weight gradients on a side stream the hand-over of a segment happens ONE
        SEGMENT LATE (the current stream has to wait for that segment's side-stream graph, and must not do so before the next
        segment's chain -- which the side stream runs beside -- has been enqueued); the first segment of the network, whose
        backward runs last, is handed over together with its predecessor."""
        hub.grad = None
        plans = self._pending.pop(name, [])
        late, self._late = self._late, None
        if late is not None:
            self._hand_over(*late)
        if not plans:
            return
        if any(p.side is not None and (name in p.wgrad or name == "heads") for p in plans) and name != self.segments[0]:
            self._late = (name, plans)
        else:
            self._hand_over(name, plans)

    def _hand_over(self, name: str, plans):
        for p in plans:
            p.wait_wgrad(name)
        params, base = plans[0].params[name], plans[0].pgrads[name]
        for other in plans[1:]:
            pairs = [(b, g) for b, g in zip(base, other.pgrads[name]) if b is not None and g is not None]
            if pairs:
                torch._foreach_add_([b for b, _ in pairs], [g for _, g in pairs])
        plans[0].aliased = True
        _deliver(params, base)


def _leaf(t):
    return t.detach().requires_grad_(True)


class _Plan:
    """The captured graphs of one input shape: forward graphs along ``enc.segments`` (stem -> layer1 -> layer2 -> layer3 in parts
    -> layer4 -> heads; each reads its predecessor's static outputs in place), backward graphs in the reverse order (each reads its successors' static input
    gradients in place), all in one memory pool and captured in the order they replay."""

    def __init__(self, enc: TrainEncoder, img: torch.Tensor):
        self.enc, self.dev = enc, img.device
        self.params = enc._seg_params()
        self.static_img = img.detach().clone()
        self.pool = torch.cuda.graph_pool_handle()
        # BatchNorm's running statistics are put back afterwards (the warm-up and the captures are not training steps)
        bns = [m for m in enc.src.modules() if isinstance(m, nn.BatchNorm2d)]
        keep = [(m.running_mean.clone(), m.running_var.clone(), m.num_batches_tracked.clone()) for m in bns]
        try:
            self._build()
        finally:                                          # (also when a capture failed: the caller falls back to the eager step)
            for (rm, rv, nb), m in zip(keep, bns):
                with torch.no_grad():
                    m.running_mean.copy_(rm), m.running_var.copy_(rv), m.num_batches_tracked.copy_(nb)

    def _build(self):
        self._warm_up()
        levels = self._capture_forward()                   # [(prop, skip)] of the four pyramid levels
        self._capture_backward(levels)
        self.tap_of = {name: tap for name, _, tap in self.enc._chain}
        self.token = torch.zeros((), device=self.dev)      # what the segment nodes hand each other (autograd ordering only)
        self.zero = torch.zeros((), device=self.dev)       # their gradient: the data moves in the static buffers
        self.busy = False
        self.aliased = False                               # some p.grad may still BE one of this plan's static buffers
        # what the rewrite found: {segment: (memset nodes, memcpy nodes) turned into kernel nodes} per direction
        tot = lambda gs: tuple(sum(g.rewritten[q] for g in gs) for q in (0, 1))
        self.rewritten = {"fwd": {"body": tot(self.fwd_body), "heads": tot(self.fwd_head)},
                          "bwd": dict({k: g.rewritten for k, g in self.bwd.items()}, heads=tot(self.bwd_head)),
                          "wgrad": {k: tot(gs) for k, gs in self.wgrad.items()}}

    def _warm_up(self):
        """Eager steps, off the capture: MIOpen / hipBLASLt pick their kernels, the allocator reaches its size."""
        enc, dev = self.enc, self.dev
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        old = torch.backends.cudnn.benchmark
        # (deterministic mode: no find pass -- the replayed step must pick MIOpen's solvers the way an eager step does, so that
        # the two agree bit for bit)
        torch.backends.cudnn.benchmark = old or (enc.miopen_find and not _det_now())
        try:
            with torch.cuda.stream(side):
                for _ in range(max(enc.warmup, 1)):
                    out = enc._eager(self.static_img)
                    leaves = [t for t in out["backbone_feature"] + out["refine_input_feat"] if t.requires_grad]
                    torch.autograd.grad(leaves, [p for ps in self.params.values() for p in ps],
                                        [torch.zeros_like(t) for t in leaves], allow_unused=True)
                    del out, leaves
        finally:
            torch.backends.cudnn.benchmark = old
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)

    def _arena(self, floats: int) -> _Arena:
        """The statistics scratch of one captured graph, kept alive with the plan."""
        self.arenas.append(_Arena(self.dev, floats))
        return self.arenas[-1]

    def _capture_forward(self):
        """The forward captures, in replay order; a segment's input is a DETACHED view of its predecessor's output that
        requires grad, so that every segment owns a separate autograd graph.  The BODY is captured as one graph per tap
        interval (stem + layer1 | layer2 | layer3 | layer4: what the forward needs between two taps; the finer segments only
        matter to the backward), the heads as one graph per pyramid level: a level's heads only need that level's tap, so
        their graph replays on the SIDE stream beside the deeper body graphs (two graphs on two streams overlap on this
        runtime, tools/graph_branch_probe.py); likewise their backward runs beside the body's backward chain.  Everything
        that replays on the side stream allocates from a pool of its own.  -> [(prop, skip)] of the four levels; leaves the
        segments' static inputs and outputs in ``ins`` / ``outs``."""
        enc, chain = self.enc, self.enc._chain
        self.ins, self.outs, self.arenas = {}, {}, []
        self.side = torch.cuda.Stream(device=self.dev) if enc.overlap_wgrad else None
        self.pool_s = torch.cuda.graph_pool_handle()      # the side stream's graphs (head levels, weight gradients)
        head_floats = enc._arena_floats("heads", False)
        self.fwd_body, self.fwd_head = [], []             # per tap interval: the body graph, the level's heads graph
        taps, hin, lv, x, k_ = [None] * 4, [None] * 4, [None] * 4, self.static_img, 0
        while k_ < len(chain):
            g = SafeGraph()
            end = next(q for q in range(k_, len(chain)) if chain[q][2] is not None) + 1      # (the chain ends with a tap: layer4)
            todo = chain[k_:end]                                                             # the segments up to the next tap
            with g.capture(pool=self.pool), _capture_scope(self._arena(sum(enc._arena_floats(n, False) for n, _, _ in todo))):
                for (name, _, tap) in todo:
                    inp = x if name == chain[0][0] else _leaf(x)
                    (x,) = enc._seg_body(name, inp)
                    self.ins[name], self.outs[name] = (inp,), (x,)
            tap = todo[-1][2]
            taps[tap] = x
            k_ += len(todo)
            self.fwd_body.append(g)
            gh_ = SafeGraph()
            hin[tap] = _leaf(x)
            with gh_.capture(pool=self.pool_s), _capture_scope(self._arena(head_floats)):
                lv[tap] = enc._head_level(tap + 2, hin[tap])
            self.fwd_head.append(gh_)
        self.heads = enc._heads_order(lv)
        self.ins["heads"], self.outs["heads"] = tuple(hin), self.heads
        self.taps = taps
        self.ev_tap = [torch.cuda.Event() for _ in range(4)]
        self.ev_heads_fwd = torch.cuda.Event()
        return lv

    def _capture_bwd(self, name, outs, make_gouts, inputs, ps, chain_pool):
        """One backward chain.  -> (gradients of ``inputs``, gradients of ``ps``, chain graph, recorded weight-gradient launches
        or None).  ``make_gouts``: called INSIDE the capture (sums of gradient buffers of two consumers are part of the graph)."""
        wrt = [t for t in inputs if t.requires_grad] + ps
        g = SafeGraph()
        enc = self.enc
        with g.capture(pool=chain_pool), _capture_scope(self._arena(enc._arena_floats(name, True)), enc.overlap_wgrad) as cap:
            grads = list(torch.autograd.grad(outs, wrt, make_gouts(), allow_unused=True))
            # a gradient is handed over in its PARAMETER's layout (the multi-tensor optimisers refuse anything else:
            # "params, grads ... must have same dtype, device, and layout"): the stock convolutions' weight gradients
            # come back channels-last strided (the 7x7 stem, widths the library's kernels do not take)
            for q, (t, g_) in enumerate(zip(wrt, grads)):
                if g_ is not None and isinstance(t, nn.Parameter) and (g_.stride() != t.stride() or g_.dtype != t.dtype):
                    grads[q] = torch.empty_like(t).copy_(g_)
        n_in = len(wrt) - len(ps)
        return grads[:n_in], list(grads[n_in:]), g, cap.records

    def _capture_wgrad(self, name, records):
        """The weight gradients a chain's capture recorded, as a graph of the side stream's pool (None without any).  The
        recorded operands (dY, X) are kept alive for the plan's lifetime -- the chain of the next segment must not reuse their
        memory while the side stream reads it."""
        if not records:
            return None
        gw = SafeGraph()
        with gw.capture(pool=self.pool_s), _capture_scope():
            for rec in records:
                _wgrad_launch(rec)
        self.keep.setdefault(name, []).extend(records)
        return gw

    def _capture_backward(self, levels):
        """The backward captures, reverse order.  Gradients that arrive from outside: one static buffer per head output that
        requires grad.  Gradients between segments: the tensors autograd.grad returned in the successor's capture.

        Weight gradients on a side stream (``overlap_wgrad``): a segment's backward is captured as TWO graphs -- the chain
        (BatchNorm backward, data gradients, everything the next layer down waits for) and, from the launches recorded while
        that capture ran, the weight gradients.  On replay the second graph runs on a side stream beside the NEXT segment's
        chain."""
        enc, chain, heads, hin = self.enc, self.enc._chain, self.heads, self.ins["heads"]
        self.gout = [torch.zeros_like(o) if o.requires_grad else None for o in heads]
        self.bwd, self.pgrads, self.wgrad, self.keep = {}, {}, {}, {}
        self.ev_chain = {n: torch.cuda.Event() for n in enc.segments}
        self.ev_wgrad = {n: torch.cuda.Event() for n in enc.segments}
        # the heads, level by level, deepest first (the order the body's backward needs their tap gradients in)
        self.bwd_head, self.ev_bh = [None] * 4, [torch.cuda.Event() for _ in range(4)]
        gh, hgrads, hrec = [None] * 4, {}, []
        where = {id(o): n for n, o in enumerate(heads)}
        for tap in (3, 2, 1, 0):
            outs_ = [o for o in levels[tap] if o.requires_grad]
            gbuf = [self.gout[where[id(o)]] for o in outs_]
            ps = enc._head_params(tap + 2)
            (gin,), pg, g, records = self._capture_bwd("heads", outs_, lambda gbuf=gbuf: list(gbuf), (hin[tap],), ps, self.pool_s)
            gh[tap], self.bwd_head[tap] = gin, g
            hgrads.update({id(p_): g_ for p_, g_ in zip(ps, pg)})
            hrec.append(records)
        self.pgrads["heads"] = [hgrads.get(id(p_)) for p_ in self.params["heads"]]
        # (captured in the order they replay on the side stream -- the four chains, then the four weight-gradient graphs: graphs
        # that share a pool replay in their capture order)
        hw = [g for g in (self._capture_wgrad("heads", r) for r in hrec) if g is not None]
        if hw:
            self.wgrad["heads"] = hw
        # a tap feeds the next body segment AND the heads: its gradient is the sum of the two static buffers (one add, captured
        # at the head of the segment's backward)
        g_next = None
        for k_ in range(len(chain) - 1, -1, -1):
            name, _, tap = chain[k_]
            terms = [t for t in (g_next, gh[tap] if tap is not None else None) if t is not None]
            make = (lambda terms=terms: [terms[0] + terms[1]]) if len(terms) == 2 else (lambda terms=terms: [terms[0]])
            gin, pg, g, records = self._capture_bwd(name, list(self.outs[name]), make, self.ins[name] if k_ > 0 else (),
                                                    self.params[name], self.pool)
            self.bwd[name], self.pgrads[name] = g, pg
            gw = self._capture_wgrad(name, records)
            if gw is not None:
                self.wgrad[name] = [gw]
            g_next = gin[0] if k_ > 0 else None

    def _unalias(self, names):
        """A ``p.grad`` that still IS one of this plan's static gradient buffers of the segments ``names`` moves into a tensor
        of its own (gradient accumulation: the usual flow, gradients set to None or re-pointed at bucket views between steps,
        never finds one)."""
        for name in names:
            for p, g in zip(self.params[name], self.pgrads[name]):
                if g is not None and p.grad is not None and p.grad.data_ptr() == g.data_ptr():
                    p.grad = p.grad.clone()

    def run(self, img):
        enc = self.enc
        if self.aliased:
            # the last backward handed this plan's static gradient buffers out as ``p.grad``.  The pool reuses that memory for
            # activations of the FORWARD graphs (a replayed step needs the two at different times), so a gradient that is still
            # in place now -- no zero_grad / optimiser step in between -- moves out first
            self._unalias(enc.segments)
            self.aliased = False
        self.static_img.copy_(img)
        main = torch.cuda.current_stream(img.device)
        for t in range(4):
            self.fwd_body[t].replay()
            if self.side is None:
                self.fwd_head[t].replay()
            else:                                          # this level's heads beside the deeper body graphs
                self.ev_tap[t].record(main)
                self.side.wait_event(self.ev_tap[t])
                with torch.cuda.stream(self.side):
                    self.fwd_head[t].replay()
        if self.side is not None:
            self.ev_heads_fwd.record(self.side)
            main.wait_event(self.ev_heads_fwd)
        self.busy = True
        hubs = enc._hubs_for(img.device)
        token = None
        for name in enc.segments[:-1]:
            token = _SegFn.apply(self, name, token, hubs[name])
        outs = _SegFn.apply(self, "heads", token, hubs["heads"])
        # (the body's own levels are handed out detached: inside the graphs they are inputs of the heads, not autograd leaves
        # of the caller)
        return enc._pack([t.detach() for t in self.taps], outs)

    def backward_segment(self, name: str, grads: Sequence[Optional[torch.Tensor]] = ()):
        if name == "heads":
            k = 0
            for g in self.gout:
                if g is None:
                    continue
                gi = grads[k] if k < len(grads) else None
                if gi is None:
                    g.zero_()
                elif gi.data_ptr() != g.data_ptr():
                    g.copy_(gi)
                k += 1
        # gradient accumulation (a second backward before zero_grad): a gradient that still IS this graph's static buffer
        # would be overwritten by the replay
        self._unalias((name,))
        main, side, heads = torch.cuda.current_stream(self.dev), self.side, name == "heads"
        if not heads:
            tap = self.tap_of[name]
            if side is not None and tap is not None:
                main.wait_event(self.ev_bh[tap])
            self.bwd[name].replay()
        if heads or name in self.wgrad:
            # what runs on the side stream: a segment's weight-gradient graphs, beside the next segment's chain -- and in front of
            # them the heads' whole backward, deepest level first (the body's chain only waits for the level whose tap gradient
            # it needs next)
            if side is not None:
                self.ev_chain[name].record(main)           # (heads: the incoming gradients are in their static buffers)
                side.wait_event(self.ev_chain[name])
            with (torch.cuda.stream(side) if side is not None else _NO_CTX):
                for tap in ((3, 2, 1, 0) if heads else ()):
                    self.bwd_head[tap].replay()
                    if side is not None:
                        self.ev_bh[tap].record(side)
                for gw in self.wgrad.get(name, ()):
                    gw.replay()
                if side is not None:
                    self.ev_wgrad[name].record(side)
        self.enc._pending.setdefault(name, []).append(self)

    def wait_wgrad(self, name: str):
        """The current stream waits for this plan's weight-gradient graph of ``name`` (a no-op without one)."""
        if self.side is not None and (name in self.wgrad or name == "heads"):
            torch.cuda.current_stream(self.dev).wait_event(self.ev_wgrad[name])


def _deliver(params, grads):
    """What autograd's AccumulateGrad does for a leaf, then its post-accumulate-grad hooks (GradBucketer's among them)."""
    acc_dst, acc_src = [], []
    for p, g in zip(params, grads):
        if g is None:
            continue
        if p.grad is None:
            p.grad = g.detach()
        else:
            acc_dst.append(p.grad), acc_src.append(g)
    if acc_dst:
        torch._foreach_add_(acc_dst, acc_src)
    for p, g in zip(params, grads):
        hooks = getattr(p, "_post_accumulate_grad_hooks", None)
        if g is not None and hooks:
            for h in list(hooks.values()):
                h(p)


class _Lease:
    """A plan is in flight from its forward until the backward of its first segment has run -- or until the autograd graph
    that holds this object is freed without a backward."""

    def __init__(self, plan):
        self.plan = plan

    def release(self):
        if self.plan is not None:
            self.plan.busy = False
            self.plan = None

    def __del__(self):
        self.release()


class _SegFn(torch.autograd.Function):
    """One segment of a plan as an autograd node.  The nodes of a plan are chained by a token (stem -> layer1 -> layer2 -> layer3_* -> layer4 ->
    heads; the heads' node returns the real outputs), so autograd runs their backwards last segment first; the data itself
    moves between the captured graphs in their static buffers.  Every node also takes the encoder's HUB leaf of its segment:
    autograd runs a leaf's AccumulateGrad once per backward pass, after the LAST node that uses it -- with several forwards
    in flight (the trainer calls the encoder once per frame of a clip and backpropagates once, trainer.py:95-131) that is
    the moment all of them have produced this segment's parameter gradients, and the hub's hook hands their sum over."""

    @staticmethod
    def forward(ctx, plan, name, token, hub):
        ctx.plan, ctx.name, ctx.has_token = plan, name, token is not None
        ctx.lease = _Lease(plan) if name == plan.enc.segments[0] else None
        ctx.set_materialize_grads(False)
        if name != "heads":
            return plan.token.detach()
        outs = tuple(o.detach() for o in plan.heads)
        ctx.mark_non_differentiable(*[o for o, g in zip(outs, plan.gout) if g is None])
        return outs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        plan, name = ctx.plan, ctx.name
        plan.backward_segment(name, [g for g, s in zip(grads, plan.gout) if s is not None] if name == "heads" else ())
        if ctx.lease is not None:
            ctx.lease.release()
        return None, None, (plan.zero if ctx.has_token else None), plan.zero
