"""The recurrent refine decoder of DMM-Net and its per-frame driver.

Counterparts in the reference:

* ``RSISMask``  -- ``dmm/modules/base.py:71-188`` with the cells of ``dmm/modules/clstm.py:68-131`` (``ConvLSTMCellMask``):
  same constructor attributes, the same parameter names and shapes (``clstm_list.{0..3}.Gates.{weight,bias}``,
  ``conv_out.{weight,bias}``: a reference checkpoint's decoder ``state_dict`` loads with ``strict=True``), the same
  ``forward(skip_feats, prev_mask_list, prev_state_spatial, prev_hidden_temporal) -> (out_mask, hidden_list)``.
* ``RefineStep``  -- the object loop of ``Evaler.inference_timestep`` (``dmm/modules/evaluator.py:179-212``) behind the
  ``refine`` contract of ``video.FrameLoop``.
* ``RefineTrainStep``  -- the object loop of ``Trainer.refine`` with its loss (``dmm/modules/trainer.py:236-306``): the
  training counterpart of ``RefineStep``, on ``mask_pyramid_fn`` / ``upsample_bilinear_fn`` / ``refine_train_finish_fn``
  (HIP forward and backward, include/dmm_match.h (12f)-(12h)) around the fused training form below.

Three execution forms behind the one ``forward``:

* the STOCK form: the reference's arithmetic op for op in torch.  Runs wherever torch runs and under autograd; taken when
  gradients are required (unless ``fused_train`` is set, below), in ``train()`` mode with ``dropout > 0``, for
  ``kernel_size == 1``, ``prev_mask_d != 1``, non-fp32 or CPU tensors.  With the default ``fused_train = False`` training
  through the decoder works this way and is not accelerated.
* the FUSED TRAINING form (``decoder.fused_train = True``, opt-in; HIP tensors, fp32 -- or the bf16 operand set of
  ``train_dtype``, below --, 3x3, a gradient required, no active dropout): the algebra of the fused form below under autograd.  The convolutions (on differentiable slices of
  ``Gates.weight``), the bilinear upsample, ``cat`` and the 'mul' product are torch ops; the cell is ``clstm_gates_fn``:
  ``dmm_clstm_gates_f32`` forward, ``dmm_clstm_gates_bwd_f32`` backward, which recomputes the gates from the cell's inputs
  instead of keeping the forward's intermediates.  One shared convolution share per level and direction instead of three
  full ones, one pointwise launch per level instead of about thirty.
* the FUSED form (HIP tensors, fp32, no grad, 3x3): the three cell evaluations of a level get the same input, the same
  spatial state and the same temporal hidden and differ in the one-channel mask plane only; a convolution is linear in
  its input channels, so

      Gates(cat[x, m_k, h_s, h_t]) = [W_x * x + W_hs * h_s + W_ht * h_t + b] + W_m * m_k          (k = 0, 2, 1)

  The bracket is ONE convolution per level instead of three; ``W_m * m_k`` is a 36-weight stencil per hidden channel and
  lives in the pointwise kernel (``dmm_clstm_gates_f32``) with the gate non-linearities, the state update and the mean
  over k.  Of the bracket, the skip map's share of ``W_x * x`` is the same for every object of a frame (computed once per
  frame by ``RefineStep``), the ``W_ht * h_t`` share does not depend on the object chain (one batched convolution for all
  objects); only ``W_hs * h_s`` and the share of the upsampled hidden of the level above are computed per object.  The
  convolutions stay on the library (``F.conv2d`` -> MIOpen); what lies between them is ``csrc/dmm_decoder.hip``.  A
  reordering of fp32 sums, not an approximation.

  ``decoder.compute_dtype = torch.bfloat16`` (opt-in; the default is fp32) runs this form on bf16 ACTIVATIONS, behind an
  encoder that hands out bf16 maps: the skip maps, the hiddens and every convolution's input and output are bf16, the library
  convolutions run in bf16 on weights cast once (``weight_slices``), and the kernels between them are the 16-bit entries
  (include/dmm_match.h (12i)-(12k)): fp32 arithmetic on widened values, one rounding at each 16-bit store.  The mask
  pyramid, the stencil weights, the cells, ``outs`` and the mask history stay fp32; the parameters stay fp32 masters.
  Calls that require a gradient ignore the setting: the training forms have a switch of their own.

``decoder.train_dtype = torch.bfloat16`` (opt-in; the default is fp32) runs the FUSED TRAINING form, and ``RefineTrainStep`` on
it, on bf16 ACTIVATIONS behind an encoder that trains in bf16 (``TrainEncoder``): the skip maps and the spatial and temporal
hiddens are bf16, the mask planes and the cells fp32 (any other set raises a ``DmmError`` that names it: no silent casts).  The
library convolutions run in bf16 on bf16 casts of the differentiable fp32 weight slices, cast once per frame; the cell, the
upsample and the trainer's finish run on the 16-bit entries forward and backward (include/dmm_match.h (12i), (12j),
(12l)-(12o)); the mask pyramid, its backward and the loss stay fp32.  The parameters stay fp32 masters and receive fp32
gradients: every convolution's weight gradient is widened before it is added to another's (``_ConvStacked``), the bias
gradients and the mask stencil's are fp32 sums.  With the default ``train_dtype`` every route is what it was.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

_SKIP_MODES = ("concat", "sum", "mul", "none")
_UP_MODE = {"write": 0, "add": 1, "mul": 2}
_ACT_SUFFIX = {torch.float32: "f32", torch.bfloat16: "bf16"}     # the storage types of the activations (dmm_match.h (12i)-(12k))


def _act_entry(stem: str, dtype, what: str):
    """The entry ``stem`` + the suffix of the activations' dtype; anything but fp32 / bf16 raises."""
    if dtype not in _ACT_SUFFIX:
        raise _lib.DmmError(f"{stem}*: {what} must be float32 or bfloat16, not {dtype}")
    return stem + _ACT_SUFFIX[dtype]


# ------------------------------------------------------------------------------------------------------------------
# launchers of csrc/dmm_decoder.hip (tensor in, tensor out; the module and the tests share them)
# ------------------------------------------------------------------------------------------------------------------
def _need_device(t: torch.Tensor):
    if not t.is_cuda:
        raise _lib.DmmError("the fused decoder kernels need tensors on an MI355X device (the stock form runs on the CPU)")


def _stream(t: torch.Tensor):
    return torch.cuda.current_stream(t.device).cuda_stream


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _batch_stride(t: torch.Tensor):
    """The batch stride the entries are handed: torch may report anything for a dimension of size 1, so the batch stride of
    a B == 1 tensor is the sample size."""
    return t.stride(0) if t.shape[0] > 1 else math.prod(t.shape[1:])


def _plane_strides(t: torch.Tensor, H: int, W: int):
    """[B, O, H*W] or [B, O, H, W] fp32 with dense planes -> (tensor, batch stride, object stride)."""
    assert t.dtype == torch.float32 and t.dim() in (3, 4), (t.shape, t.dtype)
    dense = t.stride(-1) == 1 and (t.dim() == 3 or t.stride(2) == W)
    if not dense:
        t = t.contiguous()
    return t, t.stride(0), t.stride(1)


def pyramid_sizes(H: int, W: int):
    """Sizes after 5, 4, 3, 2 nested ceil-mode 2x2 pools: coarsest first, the order of ``refine_input_feat``."""
    return [(-(-H // (1 << k)), -(-W // (1 << k))) for k in (5, 4, 3, 2)]


def _check_on_pyramid(feats, H: int, W: int):
    for f, s in zip(feats, pyramid_sizes(H, W)):
        assert tuple(f.shape[-2:]) == s, ("refine_input_feat does not sit on the mask pyramid", f.shape, s)


def mask_pyramid(prev_mask, y_mask, init_pred, n_obj: int, H: int, W: int, out: Optional[Sequence[torch.Tensor]] = None):
    """evaluator.py:188-195 for objects 0..n_obj-1 in one launch -> 4 tensors [n_obj, B, 3, h_l, w_l], coarsest first."""
    _need_device(prev_mask)
    prev_mask, sbp, sop = _plane_strides(prev_mask, H, W)
    y_mask, sby, soy = _plane_strides(y_mask, H, W)
    init_pred, sbi, soi = _plane_strides(init_pred, H, W)
    B = prev_mask.shape[0]
    assert n_obj <= min(prev_mask.shape[1], y_mask.shape[1], init_pred.shape[1])
    if out is None:
        out = [torch.empty((n_obj, B, 3, h, w), dtype=torch.float32, device=prev_mask.device) for h, w in pyramid_sizes(H, W)]
    _lib.call("dmm_mask_pyramid_f32", prev_mask.device, _ptr(prev_mask), _ptr(y_mask), _ptr(init_pred),
              sbp, sop, sby, soy, sbi, soi, B, n_obj, H, W, *[_ptr(o) for o in out], _stream(prev_mask))
    return list(out)


def _dense_samples(t: torch.Tensor):
    """Is every [C, h, w] sample of t [B, C, h, w] dense (whatever the batch stride)?"""
    h, w = t.shape[2:]
    return t.stride(3) == 1 and t.stride(2) == w and t.stride(1) == h * w


def _dense_batch(t: torch.Tensor):
    """[B, C, h, w] with dense [C, h, w] samples -> (tensor, batch stride)."""
    if not _dense_samples(t):
        t = t.contiguous()
    return t, _batch_stride(t)


def _addends(pre: Sequence[Optional[torch.Tensor]], shape=None, dtype=torch.float32):
    """The up to three addends of the cell's pre-activation (None entries skipped), each of ``dtype`` and of ``shape`` =
    [B, 4*Hd, h, w] (default: the first one's) -> (pointers, batch strides, the tensors behind the pointers), the first two
    padded to three."""
    pre = [p for p in pre if p is not None]
    assert 1 <= len(pre) <= 3
    shape = tuple(pre[0].shape if shape is None else shape)
    ptrs, strides, keep = [], [], []
    for p in pre:
        if p.dtype != dtype:
            raise _lib.DmmError(f"clstm_gates: an addend of the pre-activation is {p.dtype}, the hidden it feeds {dtype}")
        assert tuple(p.shape) == shape, (p.shape, shape)
        p, sb = _dense_batch(p)
        keep.append(p)
        ptrs.append(p.data_ptr())
        strides.append(sb)
    ptrs += [None] * (3 - len(ptrs))
    strides += [0] * (3 - len(strides))
    return ptrs, strides, keep


def clstm_gates(pre: Sequence[Optional[torch.Tensor]], masks, w_mask, cell_prev, hidden, cell, hidden_copy=None):
    """``dmm_clstm_gates_f32`` / ``_bf16`` by ``hidden``'s dtype: pre = up to three addends [B, 4*Hd, h, w]; masks [B, 3, h, w];
    w_mask [4*Hd, 9]; cell_prev [B, Hd, h, w] or None; writes ``hidden`` / ``cell`` (dense) and, when given, ``hidden_copy`` (a
    channel slice of the next evaluation's convolution input).  The addends and ``hidden_copy`` have ``hidden``'s dtype;
    masks, w_mask, cell_prev and cell are fp32 in either form."""
    _need_device(masks)
    B, Hd, h, w = hidden.shape
    entry = _act_entry("dmm_clstm_gates_", hidden.dtype, "hidden")
    ptrs, strides, keep = _addends(pre, (B, 4 * Hd, h, w), hidden.dtype)
    for name, t in (("masks", masks), ("w_mask", w_mask), ("cell_prev", cell_prev), ("cell", cell)):
        if t is not None and t.dtype != torch.float32:
            raise _lib.DmmError(f"clstm_gates: {name} is {t.dtype}; the mask planes, the stencil and the cell state are float32")
    if hidden_copy is not None and hidden_copy.dtype != hidden.dtype:
        raise _lib.DmmError(f"clstm_gates: hidden_copy is {hidden_copy.dtype}, hidden {hidden.dtype}")
    masks, sbm = _dense_batch(masks)
    assert tuple(masks.shape) == (B, 3, h, w) and w_mask.is_contiguous() and tuple(w_mask.shape) == (4 * Hd, 9)
    assert hidden.is_contiguous() and cell.is_contiguous() and tuple(cell.shape) == (B, Hd, h, w)
    if cell_prev is not None:
        cell_prev = cell_prev.contiguous()
        assert tuple(cell_prev.shape) == (B, Hd, h, w)
    sbc = 0
    if hidden_copy is not None:
        assert tuple(hidden_copy.shape) == (B, Hd, h, w) and _dense_samples(hidden_copy)
        sbc = _batch_stride(hidden_copy)
    _lib.call(entry, masks.device, *ptrs, *strides, _ptr(masks), sbm, _ptr(w_mask), _ptr(cell_prev),
              B, Hd, h, w, _ptr(hidden), _ptr(cell), _ptr(hidden_copy), sbc, _stream(masks))
    return hidden, cell


def clstm_gates_bwd(pre: Sequence[Optional[torch.Tensor]], masks, w_mask, cell_prev, d_hidden, d_cell,
                    need=(True, True, True)):
    """``dmm_clstm_gates_bwd_f32`` / ``_bf16`` by the addends' dtype: the inputs of ``clstm_gates`` and the upstream gradients
    ``d_hidden`` / ``d_cell`` ([B, Hd, h, w]; either may be None = zeros, not both) -> ``(d_pre, d_cell_prev, d_masks,
    d_w_mask)``.  ``d_pre`` [B, 4*Hd, h, w] is the gradient of the sum of the addends, so of each of them; ``need`` says which
    of ``d_cell_prev``, ``d_masks`` [B, 3, h, w], ``d_w_mask`` [4*Hd, 9] are wanted (the others are None and cost nothing).
    ``d_hidden`` and ``d_pre`` have the addends' dtype; masks, w_mask, cell_prev, ``d_cell`` and the other three gradients are
    fp32 in either form.  The gates are recomputed from the inputs; bit-reproducible."""
    _need_device(masks)
    first = next(p for p in pre if p is not None)
    entry = _act_entry("dmm_clstm_gates_bwd_", first.dtype, "the addends of the pre-activation")
    ptrs, strides, keep = _addends(pre, dtype=first.dtype)
    B, C4, h, w = keep[0].shape
    Hd = C4 // 4
    assert C4 == 4 * Hd, keep[0].shape
    need_cell, need_masks, need_w = (bool(n) for n in need)
    assert not need_cell or cell_prev is not None, "d_cell_prev without cell_prev"
    if d_hidden is not None and d_hidden.dtype != first.dtype:
        raise _lib.DmmError(f"clstm_gates_bwd: d_hidden is {d_hidden.dtype}, the addends of the pre-activation {first.dtype}")
    for name, t in (("masks", masks), ("w_mask", w_mask), ("cell_prev", cell_prev), ("d_cell", d_cell)):
        if t is not None and t.dtype != torch.float32:
            raise _lib.DmmError(f"clstm_gates_bwd: {name} is {t.dtype}; the mask planes, the stencil, the cell state and its "
                                "gradient are float32")
    masks, sbm = _dense_batch(masks)
    w_mask = w_mask.contiguous()
    assert tuple(masks.shape) == (B, 3, h, w) and tuple(w_mask.shape) == (4 * Hd, 9)
    state = []
    for t in (cell_prev, d_hidden, d_cell):
        if t is not None:
            assert tuple(t.shape) == (B, Hd, h, w), (t.shape, (B, Hd, h, w))
            t = t.contiguous()
        state.append(t)
    cell_prev, d_hidden, d_cell = state
    assert d_hidden is not None or d_cell is not None
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=masks.device)
    d_pre = torch.empty((B, 4 * Hd, h, w), dtype=first.dtype, device=masks.device)
    d_cell_prev = new(B, Hd, h, w) if need_cell else None
    d_masks = new(B, 3, h, w) if need_masks else None
    d_w_mask = new(4 * Hd, 9) if need_w else None
    ws, ws_bytes = None, 0
    if need_masks or need_w:
        ws_bytes = int(_lib.load().dmm_clstm_gates_bwd_workspace_bytes(B, Hd, h, w))
        ws = torch.empty((max(ws_bytes, 4) // 4,), dtype=torch.float32, device=masks.device)
    _lib.call(entry, masks.device, *ptrs, *strides, _ptr(masks), sbm, _ptr(w_mask), _ptr(cell_prev),
              B, Hd, h, w, _ptr(d_hidden), _ptr(d_cell), _ptr(d_pre), _ptr(d_cell_prev), _ptr(d_masks), _ptr(d_w_mask), _ptr(ws),
              ws_bytes, _stream(masks))
    return d_pre, d_cell_prev, d_masks, d_w_mask


class ClstmGatesFn(torch.autograd.Function):
    """The fused cell under autograd: ``apply(pre0, pre1, pre2, masks, w_mask, cell_prev) -> (hidden, cell)`` (``pre1``,
    ``pre2``, ``cell_prev`` may be None).  Forward: ``clstm_gates`` into fresh tensors; backward: ``clstm_gates_bwd``.
    Saves its inputs only: the backward recomputes the gates.  On bf16 addends ``hidden`` and the addends' gradient are bf16;
    the cell, the mask planes, the stencil and their gradients are fp32."""

    @staticmethod
    def forward(ctx, pre0, pre1, pre2, masks, w_mask, cell_prev):
        B, C4, h, w = pre0.shape
        hidden, cell = pre0.new_empty((B, C4 // 4, h, w)), pre0.new_empty((B, C4 // 4, h, w), dtype=torch.float32)
        clstm_gates([pre0, pre1, pre2], masks, w_mask.contiguous(), cell_prev, hidden, cell)
        ctx.save_for_backward(pre0, pre1, pre2, masks, w_mask, cell_prev)
        ctx.set_materialize_grads(False)
        return hidden, cell

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_hidden, d_cell):
        pre0, pre1, pre2, masks, w_mask, cell_prev = ctx.saved_tensors
        if d_hidden is None and d_cell is None:
            return (None,) * 6
        g = ctx.needs_input_grad
        d_pre, d_cell_prev, d_masks, d_w_mask = clstm_gates_bwd([pre0, pre1, pre2], masks, w_mask, cell_prev, d_hidden, d_cell,
                                                                need=(g[5], g[3], g[4]))
        pre_grads = tuple(d_pre if (p is not None and g[n]) else None for n, p in enumerate((pre0, pre1, pre2)))
        return pre_grads + (d_masks, d_w_mask, d_cell_prev)


def clstm_gates_fn(pre: Sequence[Optional[torch.Tensor]], masks, w_mask, cell_prev):
    """``ClstmGatesFn`` with the addends as a sequence (up to three, None entries skipped) -> ``(hidden, cell)``.  Every
    addend that requires a gradient receives the same ``d_pre`` tensor; ``w_mask``'s gradient has its shape [4*Hd, 9]."""
    pre = [p for p in pre if p is not None]
    assert 1 <= len(pre) <= 3
    pre += [None] * (3 - len(pre))
    return ClstmGatesFn.apply(pre[0], pre[1], pre[2], masks, w_mask, cell_prev)


class _WeightSlices(torch.autograd.Function):
    """``apply(weight, bounds) -> contiguous weight[:, bounds[k]:bounds[k + 1]]`` for every k.  Its backward assembles the
    weight's gradient with ONE ``cat`` of the slices' gradients (zeros for a slice the call did not use) where one
    differentiable slice each would cost a zero-filled tensor of the whole weight's size and an add per slice (a tenth of the
    fused training step at config 4's sizes, profiles/r11_decoder_train.md).  The slices are disjoint, so every element of
    the gradient is the same single value (or sum of two, where a slice is used twice) either way."""

    @staticmethod
    def forward(ctx, weight, bounds):
        ctx.bounds, ctx.rest = bounds, tuple(weight.shape[2:])
        ctx.set_materialize_grads(False)
        return tuple(weight[:, a:b].contiguous() for a, b in zip(bounds[:-1], bounds[1:]))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        ref = next((g for g in grads if g is not None), None)
        if ref is None:
            return None, None
        parts = [g if g is not None else ref.new_zeros((ref.shape[0], b - a) + ctx.rest)
                 for g, a, b in zip(grads, ctx.bounds[:-1], ctx.bounds[1:])]
        return torch.cat(parts, 1), None


class _LevelSlices(dict):
    """One level's slices (``RSISMask._cut_slices``) with ``low``: the memo of the bf16 casts the bf16 training form's
    convolutions run on (``RSISMask._conv``), so a slice is cast once per frame however many objects use it."""

    def __init__(self, **slices):
        super().__init__(**slices)
        self.low = {}


def _chain_weight(d):
    """``cat`` = [up | hs] of one level's slices (``RSISMask._cut_slices``; levels >= 1), made on first use and kept with them:
    the training form needs it only once an object has a spatial state, and then once for every object of the frame."""
    if d["cat"] is None:
        d["cat"] = torch.cat([d["up"], d["hs"]], 1)
    return d["cat"]


class _ConvStacked(torch.autograd.Function):
    """``apply(x, weight, bias, chunks)``: ONE 3x3 / padding 1 convolution of ``x`` = ``chunks`` equal groups of samples
    stacked along the batch (the objects of a frame), and one data-gradient call for all of them; the gradients of ``weight``
    and ``bias`` are taken group by group and added in group order.  Summed in a single library call over every group's
    pixels, conv_out's weight gradient came out 2 - 3 times further from fp64 than the trainer's per-object convolutions
    leave it (profiles/r12_refine_train.md); this way it carries their error.

    The bf16 training form (``x`` bf16, ``weight`` / ``bias`` the fp32 masters): the library runs in ``x``'s dtype on casts of
    the two -- ``low``, an optional ``(weight, bias)`` pair cast by the caller once per frame, else cast here -- and every
    group's weight gradient is widened to fp32 BEFORE it meets another's: the sum over the groups here, and autograd's sum over
    the uses of a weight slice, are fp32 sums.  The bias gradient is an fp32 sum of the bf16 ``dy`` (rounded to bf16 by the
    library it reached 1.68 of the stock form's error where tests/test_gpu_decoder_train_bf16.py allows 2;
    profiles/r16_decoder_train_bf16.md).
    ``chunks = 1`` is the plain convolution of that form."""

    @staticmethod
    def forward(ctx, x, weight, bias, chunks, low=None):
        if weight.dtype != x.dtype:
            w, b = low if low is not None else (weight.to(x.dtype), None if bias is None else bias.to(x.dtype))
        else:
            w, b = weight, bias
        ctx.save_for_backward(x, w)
        ctx.chunks, ctx.has_bias, ctx.master = int(chunks), bias is not None, weight.dtype
        return F.conv2d(x, w, b, padding=1)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        bias_sizes = [weight.shape[0]] if ctx.has_bias else None
        bwd = lambda g, inp, mask: torch.ops.aten.convolution_backward(g, inp, weight, bias_sizes, [1, 1], [1, 1], [1, 1],
                                                                       False, [0, 0], 1, mask)
        dy = dy.contiguous()
        dx = bwd(dy, x, [True, False, False])[0] if need_x else None
        dw = db = None
        low = weight.dtype != ctx.master                                  # the bias gradient is then summed in fp32 here
        if need_w or need_b:
            for xc, dc in zip(x.chunk(ctx.chunks, 0), dy.chunk(ctx.chunks, 0)):
                _, a, c = bwd(dc, xc, [False, need_w, need_b and not low])
                if need_w:
                    a = a.to(ctx.master)
                    dw = a if dw is None else dw + a
                if need_b:
                    c = dc.sum((0, 2, 3), dtype=ctx.master) if low else c
                    db = c if db is None else db + c
        return dx, dw, db, None, None


def upsample_bilinear_into(src, dst, c0: int = 0, mode: str = "write"):
    """``dmm_upsample_bilinear_into_f32`` / ``_bf16`` by the dtype of ``src`` and ``dst`` (the same one):
    UpsamplingBilinear2d(src [B,C,h,w]) to dst's size, combined into dst[:, c0:c0+C] ([B, C', H, W] dense) by ``mode``
    ('write' | 'add' | 'mul')."""
    _need_device(src)
    entry = _act_entry("dmm_upsample_bilinear_into_", src.dtype, "src")
    if dst.dtype != src.dtype:
        raise _lib.DmmError(f"upsample_bilinear_into: src is {src.dtype}, dst {dst.dtype}")
    src, sbs = _dense_batch(src)
    B, C, h, w = src.shape
    Bd, Cd, H, W = dst.shape
    assert Bd == B and _dense_samples(dst), (src.shape, dst.shape, dst.stride())
    _lib.call(entry, src.device, _ptr(src), sbs, B, C, h, w, _ptr(dst), _batch_stride(dst), Cd, int(c0),
              H, W, _UP_MODE[mode], _stream(src))
    return dst


def refine_finish(logits, valid_i32, outs, mask_hist, n_obj: int):
    """``dmm_refine_finish_f32`` / ``_bf16`` by the logits' dtype: logits [B, n_obj, h, w] (any batch / object strides, dense
    planes) -> outs [B,O,H,W] fp32 (sigmoid of the upsampled logits, zero rows beyond n_obj) and mask_hist[b, t] (fp32) where
    valid_i32[b, t]."""
    _need_device(outs)
    entry = _act_entry("dmm_refine_finish_", logits.dtype, "logits")
    B, O, H, W = outs.shape
    assert outs.is_contiguous() and outs.dtype == torch.float32
    assert mask_hist is None or (mask_hist.is_contiguous() and tuple(mask_hist.shape) == (B, O, H, W) and
                                 mask_hist.dtype == torch.float32)
    assert valid_i32 is None or (valid_i32.dtype == torch.int32 and valid_i32.is_contiguous() and
                                 tuple(valid_i32.shape) == (B, O))
    h, w = logits.shape[-2:]
    assert logits.shape[0] == B and logits.shape[1] >= n_obj and logits.stride(3) == 1 and logits.stride(2) == w
    _lib.call(entry, outs.device, _ptr(logits), logits.stride(0), logits.stride(1), h, w, _ptr(valid_i32),
              B, O, int(n_obj), H, W, _ptr(outs), _ptr(mask_hist), _stream(outs))
    return outs


# ------------------------------------------------------------------------------------------------------------------
# what the refine step of training runs around the decoder (include/dmm_match.h (12f)-(12h)): launchers, the autograd
# functions over them, and for each its torch-op twin -- the same function in the ops the trainer uses
# ------------------------------------------------------------------------------------------------------------------
def mask_pyramid_bwd(prev_mask, init_pred, d_outs, n_obj: int, H: int, W: int, need=(True, True), out=None):
    """``dmm_mask_pyramid_bwd_f32``: the planes the forward read and the gradients of its four outputs (coarsest first,
    [n_obj, B, 3, h_l, w_l]; None = zeros) -> ``(d_prev, d_init)`` in the inputs' shapes; ``need`` says which is wanted (the
    other is None).  Rows of objects >= n_obj are zero.  ``out``: a pair of tensors to write into instead of fresh ones
    ([B, >= n_obj, H*W | H, W], dense planes, any batch / object strides; rows >= n_obj are then left alone)."""
    _need_device(prev_mask)
    prev_c, sbp, sop = _plane_strides(prev_mask, H, W)
    init_c, sbi, soi = _plane_strides(init_pred, H, W)
    B = prev_c.shape[0]
    assert n_obj <= min(prev_c.shape[1], init_c.shape[1])
    ds = []
    for d, (h, w) in zip(d_outs, pyramid_sizes(H, W)):
        if d is not None:
            assert tuple(d.shape) == (n_obj, B, 3, h, w) and d.dtype == torch.float32, (d.shape, (n_obj, B, 3, h, w))
            d = d.contiguous()
        ds.append(d)
    res = []
    for k, like in enumerate((prev_mask, init_pred)):
        g = None
        if need[k] and out is not None:
            g = out[k]
            assert g.dtype == torch.float32 and g.shape[0] == B and g.shape[1] >= n_obj and g.stride(-1) == 1 and \
                (g.dim() == 3 or g.stride(2) == W) and g[0, 0].numel() == H * W, (g.shape, g.stride())
        elif need[k]:
            g = torch.empty((B, like.shape[1], H * W), dtype=torch.float32, device=like.device)
            if like.shape[1] > n_obj:
                g[:, n_obj:].zero_()
        res.append(g)
    strides = lambda g: (0, H * W) if g is None else (g.stride(0), max(g.stride(1), H * W))
    _lib.call("dmm_mask_pyramid_bwd_f32", prev_c.device, _ptr(prev_c), _ptr(init_c), sbp, sop, sbi, soi, B, int(n_obj),
              H, W, *[_ptr(d) for d in ds], _ptr(res[0]), *strides(res[0]), _ptr(res[1]), *strides(res[1]), _stream(prev_c))
    if out is None:
        res = [None if g is None else g.view(like.shape) for g, like in zip(res, (prev_mask, init_pred))]
    return tuple(res)


class MaskPyramidFn(torch.autograd.Function):
    """``mask_pyramid`` under autograd: ``apply(prev_mask, y_mask, init_pred, n_obj, H, W)`` -> the four levels.  Gradients
    go to ``prev_mask`` and ``init_pred`` (``mask_pyramid_bwd``); the reference mask is data."""

    @staticmethod
    def forward(ctx, prev_mask, y_mask, init_pred, n_obj, H, W):
        outs = mask_pyramid(prev_mask, y_mask, init_pred, n_obj, H, W)
        ctx.save_for_backward(prev_mask, init_pred)
        ctx.dims = (int(n_obj), int(H), int(W))
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *d_outs):
        g = ctx.needs_input_grad
        if all(d is None for d in d_outs) or not (g[0] or g[2]):
            return (None,) * 6
        prev_mask, init_pred = ctx.saved_tensors
        d_prev, d_init = mask_pyramid_bwd(prev_mask, init_pred, d_outs, *ctx.dims, need=(g[0], g[2]))
        return d_prev, None, d_init, None, None, None


def mask_pyramid_fn(prev_mask, y_mask, init_pred, n_obj: int, H: int, W: int):
    """trainer.py:256-265 for objects 0..n_obj-1 in one launch, differentiable in ``prev_mask`` and ``init_pred`` -> 4 tensors
    [n_obj, B, 3, h_l, w_l], coarsest first."""
    return list(MaskPyramidFn.apply(prev_mask, y_mask, init_pred, n_obj, H, W))


def mask_pyramid_torch(prev_mask, y_mask, init_pred, n_obj: int, H: int, W: int):
    """The twin of ``mask_pyramid_fn``: the trainer's nested ``max_pool2d`` calls on all objects at once (any device, dtype)."""
    B = prev_mask.shape[0]
    m = torch.stack([t[:, :n_obj].reshape(B, n_obj, H, W) for t in (prev_mask, y_mask, init_pred)], 2)
    m = m.transpose(0, 1).reshape(n_obj * B, 3, H, W)
    pool = lambda x: F.max_pool2d(x, (2, 2), ceil_mode=True)
    m = pool(m)
    pyr = []
    for _ in range(4):
        m = pool(m)
        pyr.append(m.view(n_obj, B, 3, *m.shape[-2:]))
    return pyr[::-1]


def upsample_bilinear_bwd(d_dst, c0: int, C: int, h: int, w: int):
    """``dmm_upsample_bilinear_bwd_f32`` / ``_bf16`` by ``d_dst``'s dtype: the gradient of channels c0 .. c0 + C of d_dst
    [B, C', H, W] (what 'write' mode of ``upsample_bilinear_into`` wrote) -> d_src [B, C, h, w] of the same dtype.  H >= h and
    W >= w; anything else raises."""
    _need_device(d_dst)
    entry = _act_entry("dmm_upsample_bilinear_bwd_", d_dst.dtype, "d_dst")
    d_dst, sbd = _dense_batch(d_dst)
    B, Cd, H, W = d_dst.shape
    d_src = torch.empty((B, C, h, w), dtype=d_dst.dtype, device=d_dst.device)
    _lib.call(entry, d_dst.device, _ptr(d_dst), sbd, B, int(C), H, W, Cd, int(c0),
              _ptr(d_src), C * h * w, int(h), int(w), _stream(d_dst))
    return d_src


class UpsampleBilinearFn(torch.autograd.Function):
    """``apply(src, size)``: ``upsample_bilinear_into`` ('write') into a fresh tensor of ``src``'s dtype (fp32 or bf16); backward
    ``upsample_bilinear_bwd``."""

    @staticmethod
    def forward(ctx, src, size):
        B, C, h, w = src.shape
        H, W = int(size[0]), int(size[1])
        if H < h or W < w:
            raise _lib.DmmError(f"upsample_bilinear_fn: {h}x{w} -> {H}x{W} is not an upsample (its backward covers H >= h, W >= w)")
        dst = torch.empty((B, C, H, W), dtype=src.dtype, device=src.device)
        upsample_bilinear_into(src, dst, 0, "write")
        ctx.src_size = (h, w)
        return dst

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_dst):
        return upsample_bilinear_bwd(d_dst, 0, d_dst.shape[1], *ctx.src_size), None


def upsample_bilinear_fn(src, size):
    """UpsamplingBilinear2d (align_corners = True) of src [B, C, h, w] to ``size``, HIP forward and backward (no atomics)."""
    return UpsampleBilinearFn.apply(src, tuple(size))


def upsample_bilinear_torch(src, size):
    """The twin of ``upsample_bilinear_fn``."""
    return F.interpolate(src, size=tuple(size), mode="bilinear", align_corners=True)


def _logit_planes(logits):
    h, w = logits.shape[-2:]
    if not (logits.stride(3) == 1 and logits.stride(2) == w):
        logits = logits.contiguous()
    return logits


def refine_train_finish(logits, O: int, H: int, W: int):
    """``dmm_refine_train_finish_f32`` / ``_bf16`` by the logits' dtype: logits [B, n_obj, h, w] (any batch / object strides,
    dense planes) -> outs [B, O, H, W] fp32 = sigmoid of the NEAREST interpolation (torch's default mode, trainer.py:275), zero
    rows beyond n_obj."""
    _need_device(logits)
    entry = _act_entry("dmm_refine_train_finish_", logits.dtype, "logits")
    assert logits.dim() == 4 and logits.shape[1] <= O
    logits = _logit_planes(logits)
    B, n_obj, h, w = logits.shape
    outs = torch.empty((B, O, H, W), dtype=torch.float32, device=logits.device)
    _lib.call(entry, logits.device, _ptr(logits), logits.stride(0), logits.stride(1), h, w, B, int(O),
              n_obj, int(H), int(W), _ptr(outs), _stream(logits))
    return outs


def refine_train_finish_bwd(logits, d_outs):
    """``dmm_refine_train_finish_bwd_f32`` / ``_bf16`` by the logits' dtype: the forward's logits and d_outs [B, O, H, W] fp32
    -> d_logits [B, n_obj, h, w] of the logits' dtype."""
    _need_device(logits)
    entry = _act_entry("dmm_refine_train_finish_bwd_", logits.dtype, "logits")
    if d_outs.dtype != torch.float32:
        raise _lib.DmmError(f"refine_train_finish_bwd: d_outs is {d_outs.dtype}; the probabilities and their gradient are float32")
    logits = _logit_planes(logits)
    B, n_obj, h, w = logits.shape
    assert d_outs.dim() == 4 and d_outs.shape[0] == B and d_outs.shape[1] >= n_obj
    d_outs = d_outs.contiguous()
    O, H, W = d_outs.shape[1:]
    d_logits = torch.empty((B, n_obj, h, w), dtype=logits.dtype, device=logits.device)
    _lib.call(entry, logits.device, _ptr(logits), logits.stride(0), logits.stride(1), h, w,
              _ptr(d_outs), B, O, n_obj, H, W, _ptr(d_logits), n_obj * h * w, h * w, _stream(logits))
    return d_logits


class RefineTrainFinishFn(torch.autograd.Function):
    """``apply(logits, O, H, W)``: ``refine_train_finish``; backward ``refine_train_finish_bwd`` (recomputes the sigmoid)."""

    @staticmethod
    def forward(ctx, logits, O, H, W):
        ctx.save_for_backward(logits)
        return refine_train_finish(logits, O, H, W)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_outs):
        (logits,) = ctx.saved_tensors
        return refine_train_finish_bwd(logits, d_outs), None, None, None


def refine_train_finish_fn(logits, O: int, H: int, W: int):
    """trainer.py:275-287, 302-304 for all objects: logits [B, n_obj, h, w] -> padded probabilities [B, O, H, W]."""
    return RefineTrainFinishFn.apply(logits, int(O), int(H), int(W))


def refine_train_finish_torch(logits, O: int, H: int, W: int):
    """The twin of ``refine_train_finish_fn`` (bf16 logits are widened before the sigmoid: the probabilities are fp32)."""
    x = F.interpolate(logits, (H, W))
    p = torch.sigmoid(x.float() if x.dtype == torch.bfloat16 else x)
    outs = p.new_zeros((p.shape[0], O, H, W))
    outs[:, :p.shape[1]] = p
    return outs


# ------------------------------------------------------------------------------------------------------------------
# the module
# ------------------------------------------------------------------------------------------------------------------
class ConvLSTMCellMask(nn.Module):
    """clstm.py:68-131: one ``Gates`` convolution over cat[input, prev_mask, hidden_spatial, hidden_temporal]."""

    def __init__(self, args, input_size: int, hidden_size: int, kernel_size: int, padding: int):
        super().__init__()
        self.input_size, self.hidden_size = int(input_size), int(hidden_size)
        self.Gates = nn.Conv2d(self.input_size + 2 * self.hidden_size + int(args.prev_mask_d), 4 * self.hidden_size,
                               kernel_size, padding=padding)

    def forward(self, input_, prev_mask, prev_state_spatial, hidden_state_temporal):
        B = input_.shape[0]
        size = (B, self.hidden_size) + tuple(input_.shape[2:])
        if prev_state_spatial is None:
            prev_state_spatial = (input_.new_zeros(size), input_.new_zeros(size))
        if hidden_state_temporal is None:
            hidden_state_temporal = input_.new_zeros(size)
        h_s, c_s = prev_state_spatial
        gates = self.Gates(torch.cat([input_, prev_mask, h_s, hidden_state_temporal], 1))
        i, r, o, g = gates.chunk(4, 1)
        i, r, o, g = torch.sigmoid(i), torch.sigmoid(r), torch.sigmoid(o), torch.tanh(g)
        cell = (r * c_s) + (i * g)
        return [o * torch.tanh(cell), cell]


class RSISMask(nn.Module):
    """The recurrent decoder (base.py:71-188).  ``args``: hidden_size, kernel_size, dropout, skip_mode, prev_mask_d
    (``use_gpu`` is accepted and ignored: states are allocated on the input's device)."""

    def __init__(self, args):
        super().__init__()
        self.hidden_size = args.hidden_size
        self.kernel_size = args.kernel_size
        self.dropout = args.dropout
        self.skip_mode = args.skip_mode
        self.prev_mask_d = int(getattr(args, "prev_mask_d", 1))
        padding = 0 if self.kernel_size == 1 else 1
        hs = int(self.hidden_size)
        self.skip_dims_out = [hs, int(hs / 2), int(hs / 4), int(hs / 8)]
        self.clstm_list = nn.ModuleList()
        for i, out_dim in enumerate(self.skip_dims_out):
            in_dim = hs if i == 0 else self.skip_dims_out[i - 1] * (2 if self.skip_mode == "concat" else 1)
            self.clstm_list.append(ConvLSTMCellMask(args, in_dim, out_dim, self.kernel_size, padding))
        self.conv_out = nn.Conv2d(self.skip_dims_out[-1], 1, self.kernel_size, padding=padding)
        self.fused = True                    # False: always the stock form (A/B timing, tests)
        self.fused_train = False             # True: calls that require a gradient take the fused training form
        self._compute_dtype = torch.float32  # the activations' dtype of the fused (no-grad) form: ``compute_dtype``
        self._train_dtype = torch.float32    # the activations' dtype of the fused training form: ``train_dtype``
        self._slices = None                  # (key, per-level weight slices, conv_out's pair) of the fused form
        self.conv_calls = 0                  # convolutions issued by the fused form (diagnostic, like dmm_launch_count)

    @property
    def compute_dtype(self):
        """The dtype of the fused inference form's activations: ``torch.float32`` (default) or, opt-in, ``torch.bfloat16``
        (module docstring).  The parameters stay fp32 either way; calls that require a gradient ignore it."""
        return self._compute_dtype

    @compute_dtype.setter
    def compute_dtype(self, dtype):
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"RSISMask.compute_dtype is torch.float32 or torch.bfloat16, not {dtype!r}")
        self._compute_dtype = dtype

    @property
    def train_dtype(self):
        """The dtype of the fused TRAINING form's activations (``fused_train = True``, a gradient required): ``torch.float32``
        (default) or, opt-in, ``torch.bfloat16`` (module docstring).  The parameters stay fp32 masters with fp32 gradients;
        calls that require no gradient ignore it (``compute_dtype`` is theirs)."""
        return self._train_dtype

    @train_dtype.setter
    def train_dtype(self, dtype):
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"RSISMask.train_dtype is torch.float32 or torch.bfloat16, not {dtype!r}")
        self._train_dtype = dtype

    # ---- dispatch ------------------------------------------------------------------------------------------------
    def _route(self, tensors: Sequence[torch.Tensor]) -> str:
        """'fused' (no gradient), 'train' (a gradient is required and ``fused_train`` is on) or 'stock'.  With
        ``compute_dtype = torch.bfloat16`` (no gradient) or ``train_dtype = torch.bfloat16`` (a gradient) the form takes bf16
        tensors beside fp32 ones (which tensor has to be which: ``_check_bf16_operands``); in every other case all of them
        are fp32."""
        if not self.fused or self.skip_mode not in _SKIP_MODES or int(self.kernel_size) != 3 or self.prev_mask_d != 1:
            return "stock"
        if self.training and self.dropout > 0:
            return "stock"
        params = list(self.parameters())
        grad = torch.is_grad_enabled() and any(t.requires_grad for t in list(tensors) + params)
        if grad and not self.fused_train:
            return "stock"
        if not all(t.is_cuda and t.dtype == torch.float32 for t in params):
            return "stock"
        act = self._train_dtype if grad else self._compute_dtype
        taken = (torch.float32,) if act == torch.float32 else (torch.float32, torch.bfloat16)
        if not all(t.is_cuda and t.dtype in taken for t in tensors):
            return "stock"
        return "train" if grad else "fused"

    def _act_dtype(self, route: str):
        """The activations' dtype of a fused route: ``train_dtype`` for 'train', ``compute_dtype`` for 'fused'."""
        return self._train_dtype if route == "train" else self._compute_dtype

    @staticmethod
    def _check_bf16_operands(low, full, setting="compute_dtype"):
        """The operand set of a bf16 fused form: ``low`` (skip maps, hiddens) bf16, ``full`` (mask planes, cells) fp32."""
        if not all(t.dtype == torch.bfloat16 for t in low) or not all(t.dtype == torch.float32 for t in full):
            raise _lib.DmmError(f"RSISMask with {setting} = torch.bfloat16 takes bfloat16 skip maps, spatial hiddens and "
                                "temporal hiddens and float32 mask planes and cells; got "
                                f"{sorted({str(t.dtype) for t in low})} and {sorted({str(t.dtype) for t in full})}")

    def fused_ok(self, tensors: Sequence[torch.Tensor]) -> bool:
        """Does the fused inference form cover this call?  (Anything else is the stock form -- same results, torch ops --
        or, with ``fused_train``, the fused training form.)"""
        return self._route(tensors) == "fused"

    def forward(self, skip_feats, prev_mask_list, prev_state_spatial, prev_hidden_temporal):
        ts = list(skip_feats) + list(prev_mask_list)
        if prev_state_spatial is not None:
            ts += [t for st in prev_state_spatial for t in st]
        if prev_hidden_temporal is not None:
            ts += list(prev_hidden_temporal)
        route = self._route(ts)
        if route != "stock" and self._act_dtype(route) == torch.bfloat16:
            low = list(skip_feats) + ([] if prev_hidden_temporal is None else list(prev_hidden_temporal))
            full = list(prev_mask_list)
            if prev_state_spatial is not None:
                low += [st[0] for st in prev_state_spatial]
                full += [st[1] for st in prev_state_spatial]
            self._check_bf16_operands(low, full, "train_dtype" if route == "train" else "compute_dtype")
        if route == "fused":
            return self._forward_fused(skip_feats, prev_mask_list, prev_state_spatial, prev_hidden_temporal)
        if route == "train":
            return self._forward_fused_train(skip_feats, prev_mask_list, prev_state_spatial, prev_hidden_temporal)
        return self.forward_stock(skip_feats, prev_mask_list, prev_state_spatial, prev_hidden_temporal)

    # ---- stock form: base.py:115-188 op for op ----------------------------------------------------------------------
    def forward_stock(self, skip_feats, prev_mask_list, prev_state_spatial, prev_hidden_temporal):
        clstm_in = skip_feats[0]
        skips = skip_feats[1:]
        hidden_list = []
        for i, cell in enumerate(self.clstm_list):
            m = prev_mask_list[i]
            st = None if prev_state_spatial is None else prev_state_spatial[i]
            ht = None if prev_hidden_temporal is None else prev_hidden_temporal[i]
            a = cell(clstm_in, m[:, 0:1], st, ht)                 # prev_mask
            b = cell(clstm_in, m[:, 2:], st, ht)                  # init_pred
            c = cell(clstm_in, m[:, 1:2], st, ht)                 # y_mask
            state = [(a[0] + b[0] + c[0]) / 3, (a[1] + b[1] + c[1]) / 3]
            hidden_list.append(state)
            hidden = state[0]
            if self.dropout > 0:
                hidden = F.dropout2d(hidden, self.dropout, training=self.training)
            if i < len(skips):
                skip = skips[i]
                hidden = F.interpolate(hidden, size=tuple(skip.shape[-2:]), mode="bilinear", align_corners=True)
                if self.skip_mode == "concat":
                    clstm_in = torch.cat([hidden, skip], 1)
                elif self.skip_mode == "sum":
                    clstm_in = hidden + skip
                elif self.skip_mode == "mul":
                    clstm_in = hidden * skip
                elif self.skip_mode == "none":
                    clstm_in = hidden
                else:
                    raise Exception("Skip connection mode not supported !")
            else:
                clstm_in = F.interpolate(hidden, size=(hidden.shape[-2] * 2, hidden.shape[-1] * 2), mode="bilinear",
                                         align_corners=True)
        return self.conv_out(clstm_in), hidden_list

    # ---- fused form ------------------------------------------------------------------------------------------------------
    def _cut_slices(self, train: bool):
        """The slice layout of ``Gates.weight`` ([4*Hd, Cin + 1 + 2*Hd, 3, 3], input channels in the order x, mask, h_s,
        h_t), per level a dict: ``up`` = the share of the upsampled hidden of the level above (levels >= 1), ``skip`` = the
        skip map's share (all of x at level 0; levels >= 1: the second half of x = [up | skip] under 'concat', all of x
        under 'sum', none under 'mul' / 'none'), ``m`` [4*Hd, 9], ``hs``, ``ht``, ``bias`` and ``cat`` = [up | hs] (one chain
        convolution on cat[x, h_s]; None at level 0).  ``train``: cut from the parameters themselves, so the slices carry
        one ``_WeightSlices`` node per level, and ``cat`` is left to ``_chain_weight``; otherwise from the detached
        parameters, ``cat`` included."""
        out = []
        for i, cell in enumerate(self.clstm_list):
            Wt, bias, Hd, cin = cell.Gates.weight, cell.Gates.bias, cell.hidden_size, cell.input_size
            if not train:
                Wt, bias = Wt.detach(), bias.detach()
            cup = cin if i == 0 or self.skip_mode != "concat" else self.skip_dims_out[i - 1]
            w_x, w_x2, w_m, w_hs, w_ht = _WeightSlices.apply(Wt, (0, cup, cin, cin + 1, cin + 1 + Hd, cin + 1 + 2 * Hd))
            d = _LevelSlices(m=w_m.reshape(4 * Hd, 9), hs=w_hs, ht=w_ht, bias=bias, up=None, skip=w_x, cat=None)
            if i > 0:
                d["up"] = w_x
                d["skip"] = w_x2 if self.skip_mode == "concat" else w_x if self.skip_mode == "sum" else None
                if not train:
                    _chain_weight(d)
            out.append(d)
        return out

    def weight_slices(self):
        """The no-grad cut of ``_cut_slices`` (the fused form's), ``cat`` present.  Made once and kept against the
        parameters' versions and storages and ``compute_dtype``: with bf16 set, the same layout with the convolution weights
        and the bias cast to bf16 (once, here); ``m``, the mask stencil the gate kernel reads, stays fp32."""
        return self._cached_slices()[1]

    def head_weights(self):
        """``conv_out``'s (weight, bias) as the fused form applies them: the parameters, or their bf16 casts kept with
        ``weight_slices()``."""
        return self._cached_slices()[2]

    def _cached_slices(self):
        key = (self._compute_dtype,) + tuple((p.data_ptr(), p._version, p.device) for p in self.parameters())
        if self._slices is None or self._slices[0] != key:
            sl = self._cut_slices(train=False)
            head = (self.conv_out.weight.detach(), self.conv_out.bias.detach())
            if self._compute_dtype != torch.float32:
                cast = lambda t: None if t is None else t.to(self._compute_dtype)
                sl = [{k: (v if k == "m" else cast(v)) for k, v in d.items()} for d in sl]
                head = tuple(cast(t) for t in head)
            self._slices = (key, sl, head)
        return self._slices

    def train_slices(self):
        """The differentiable cut of ``_cut_slices`` (the fused training form's).  One ``_WeightSlices`` node per level: a
        caller that evaluates several objects of a frame on the same slices (``RefineTrainStep``) pays the assembly of the
        weight's gradient once per frame."""
        return self._cut_slices(train=True)

    def _conv(self, x, w, b=None, low=None):
        """One 3x3 / padding 1 library convolution.  ``x`` bf16 on fp32 ``w`` / ``b`` -- the bf16 training form on its fp32
        master slices -- runs in bf16 on casts of the two and hands the slices fp32 gradients (``_ConvStacked``); ``low``: a
        level's memo of such casts (``_cut_slices``), so a slice is cast once per frame however many objects use it."""
        self.conv_calls += 1
        if w.dtype == x.dtype:
            return F.conv2d(x, w, b, padding=1)
        pair = None
        if low is not None:
            pair = low.get((id(w), id(b)))
            if pair is None:
                with torch.no_grad():
                    pair = low[(id(w), id(b))] = (w.to(x.dtype), None if b is None else b.to(x.dtype))
        return _ConvStacked.apply(x, w, b, 1, pair)

    def skip_terms(self, skip_feats, slices=None):
        """The object-independent share of every level's pre-activation: conv(skip map, W_skip) + bias (None where the
        level has no such term: 'mul' / 'none' above level 0).  Once per frame.  ``slices``: default ``weight_slices()``."""
        sl = self.weight_slices() if slices is None else slices
        return [None if d["skip"] is None else self._conv(f, d["skip"], d["bias"], getattr(d, "low", None))
                for d, f in zip(sl, skip_feats)]

    def temporal_terms(self, hidden_temporal, slices=None):
        """conv(h_t, W_ht) per level; ``hidden_temporal[i]`` may stack every object of the frame along the batch."""
        sl = self.weight_slices() if slices is None else slices
        return [self._conv(h, d["ht"], None, getattr(d, "low", None)) for d, h in zip(sl, hidden_temporal)]

    def _level(self, i, d, skip_term, temporal_term, skip, masks, state_spatial, hidden, cell, up_src, chain_in=None,
               holds_state=False, hidden_copy=None):
        """One level of one object: the chain convolution + the gate launch into ``hidden`` / ``cell``.  ``up_src``: the
        hidden of the level above (None at level 0).  ``chain_in`` (levels >= 1): the chain convolution's input, written
        here -- [B, Cup, h, w] without a spatial state, [B, Cup + Hd, h, w] = [up | h_s] with one; ``holds_state``: its upper
        channels hold the state's hidden already (otherwise it is copied there).  ``hidden_copy``: where the gate launch
        leaves this level's hidden a second time."""
        chain = None
        bias_in_chain = None if skip_term is not None else d["bias"]
        if i == 0:
            if state_spatial is not None:
                chain = self._conv(state_spatial[0], d["hs"])
        else:
            cup = self.skip_dims_out[i - 1]
            if state_spatial is not None and not holds_state:
                chain_in[:, cup:].copy_(state_spatial[0])
            if self.skip_mode == "mul":
                chain_in[:, :cup].copy_(skip)
                upsample_bilinear_into(up_src, chain_in, 0, "mul")
            else:
                upsample_bilinear_into(up_src, chain_in, 0, "write")
            chain = self._conv(chain_in, d["up"] if state_spatial is None else d["cat"], bias_in_chain)
        pre = [skip_term, temporal_term, chain]
        cell_prev = None if state_spatial is None else state_spatial[1]
        clstm_gates(pre, masks, d["m"], cell_prev, hidden, cell, hidden_copy)
        return hidden, cell

    def _forward_fused(self, skip_feats, prev_mask_list, prev_state_spatial, prev_hidden_temporal):
        sl = self.weight_slices()
        skip_terms = self.skip_terms(skip_feats)
        temporal = [None] * 4 if prev_hidden_temporal is None else self.temporal_terms(prev_hidden_temporal)
        hidden_list, up_src = [], None
        for i, d in enumerate(sl):
            f = skip_feats[i]
            B, (h, w) = f.shape[0], f.shape[-2:]
            Hd = self.skip_dims_out[i]
            st = None if prev_state_spatial is None else prev_state_spatial[i]
            chain_in = None
            if i > 0:
                chain_in = f.new_empty((B, self.skip_dims_out[i - 1] + (0 if st is None else Hd), h, w))
            hidden, cell = f.new_empty((B, Hd, h, w)), f.new_empty((B, Hd, h, w), dtype=torch.float32)
            self._level(i, d, skip_terms[i], temporal[i], f, prev_mask_list[i], st, hidden, cell, up_src, chain_in)
            hidden_list.append([hidden, cell])
            up_src = hidden
        h, w = up_src.shape[-2:]
        top = up_src.new_empty((up_src.shape[0], self.skip_dims_out[-1], 2 * h, 2 * w))
        upsample_bilinear_into(up_src, top, 0, "write")
        return self._conv(top, *self.head_weights()), hidden_list

    # ---- fused training form ---------------------------------------------------------------------------------------------

    def _forward_fused_train(self, skip_feats, prev_mask_list, prev_state_spatial, prev_hidden_temporal, slices=None,
                             skip_terms=None, temporal_terms=None, bilinear=None, head=True):
        """The fused algebra under autograd: per level the addends (skip term with the bias, temporal term, chain term on
        cat[up, h_s] / up / h_s) are library convolutions on differentiable slices of ``Gates.weight``, the upsample, ``cat``
        and the 'mul' product are torch ops, and the cell is ``clstm_gates_fn`` (HIP forward and backward).  The activations'
        dtype is the skip maps': on the bf16 operand set of ``train_dtype`` every op here is the same op in bf16 (``_conv``
        on the fp32 master slices), the cells and the mask planes fp32.

        The optional arguments let a driver hand over what does not depend on the object (``RefineTrainStep``); the defaults
        compute everything here.  ``slices``: ``train_slices()`` taken once per frame; ``skip_terms``: per level
        conv(skip map, W_skip) + bias (None where the level has no such term) -- ``skip_feats`` is then read for the sizes
        and the 'mul' product only; ``temporal_terms``: per level conv(h_t, W_ht) of this object, used INSTEAD of
        ``prev_hidden_temporal``; ``bilinear(x, size)``: the upsample; ``head=False``: return the last level's hidden in
        place of ``conv_out`` of its upsample (the driver runs both once for all objects)."""
        if bilinear is None:
            bilinear = lambda x, size: F.interpolate(x, size=size, mode="bilinear", align_corners=True)
        if slices is None:
            slices = self.train_slices()
        if skip_terms is None:
            skip_terms = self.skip_terms(skip_feats, slices)
        if temporal_terms is None:
            temporal_terms = [None] * 4 if prev_hidden_temporal is None else self.temporal_terms(prev_hidden_temporal, slices)
        hidden_list, up = [], None
        for i, d in enumerate(slices):
            f = skip_feats[i]
            st = None if prev_state_spatial is None else prev_state_spatial[i]
            chain_bias = None if skip_terms[i] is not None else d["bias"]
            chain, low = None, getattr(d, "low", None)
            if i == 0:
                if st is not None:
                    chain = self._conv(st[0], d["hs"], None, low)
            else:
                x = bilinear(up, tuple(f.shape[-2:]))
                if self.skip_mode == "mul":
                    x = f * x
                if st is None:
                    chain = self._conv(x, d["up"], chain_bias, low)
                else:
                    chain = self._conv(torch.cat([x, st[0]], 1), _chain_weight(d), chain_bias, low)
            hidden, c = clstm_gates_fn([skip_terms[i], temporal_terms[i], chain], prev_mask_list[i], d["m"],
                                       None if st is None else st[1])
            hidden_list.append([hidden, c])
            up = hidden
        if not head:
            return up, hidden_list
        top = bilinear(up, (up.shape[-2] * 2, up.shape[-1] * 2))
        return self._conv(top, self.conv_out.weight, self.conv_out.bias), hidden_list


# ------------------------------------------------------------------------------------------------------------------
# the per-frame driver
# ------------------------------------------------------------------------------------------------------------------
class RefineState:
    """What ``RefineStep`` carries from frame to frame: ``n_obj`` (valid_num_obj_max, read from ``valid`` once per clip)
    and ``thid`` = per object the list of per-level temporal hiddens (the reference's prev_thid_list; None before the first
    frame has run, and for ever under ``only_spatial``).  In the fused form the hiddens are views of the step's own
    buffers: they are rewritten in place by the next frame (after their temporal convolutions have been taken)."""

    def __init__(self, n_obj: int, thid=None):
        self.n_obj, self.thid = int(n_obj), thid

    def __len__(self):
        return 0 if self.thid is None else len(self.thid)

    def __getitem__(self, t):
        return self.thid[t]


def _stock_objects(decode, feats, pyr, prev_thid, n_obj: int, only_temporal: bool):
    """The object loop of the evaluator (evaluator.py:183-200) and of the trainer (trainer.py:245-273), op for op: object t is
    decoded on the spatial state of object t - 1 (on none under ``only_temporal``, once there are temporal hiddens) and on its
    own temporal hiddens of the last frame.  ``decode``: the decoder entry to call; ``pyr``: the four mask levels of all objects
    ([n_obj, B, 3, h_l, w_l], coarsest first).  -> (``out_mask`` per object, ``thid``)."""
    assert prev_thid is None or len(prev_thid) == n_obj, (len(prev_thid), n_obj)
    hidden_spatial, thid, out_masks = None, [], []
    for t in range(n_obj):
        hidden_temporal = None
        if prev_thid is not None:
            hidden_temporal = prev_thid[t]
            if only_temporal:
                hidden_spatial = None
        out_mask, hidden = decode(feats, [p[t] for p in pyr], hidden_spatial, hidden_temporal)
        hidden_spatial = hidden
        thid.append([hc[0] for hc in hidden])
        out_masks.append(out_mask)
    return out_masks, thid


class RefineStep:
    """``refine(features, prev_mask, y_mask, init_pred, mask_hist_new, valid, state) -> (outs, mask_hist_new, state)`` for
    ``video.FrameLoop``: evaluator.py:179-212.  ``prev_mask`` / ``y_mask`` [B,O,HW], ``init_pred`` / ``mask_hist_new``
    [B,O,H,W], ``valid`` [B,O]; ``outs`` [B,O,HW], zero for objects >= valid_num_obj_max; ``mask_hist_new[b, t]`` is
    written only where ``valid[b, t]``.

    Fused form (the decoder's ``fused_ok``): one pyramid launch, the hoisted skip convolutions, one batched temporal
    convolution per level, per object and level one chain convolution + one gate launch + one upsample launch, one
    upsample + ``conv_out`` for all objects, one finish launch.  ``valid_num_obj_max`` is read when ``state is None``
    (frame 0 of a clip) and kept in the state: afterwards no host sync, and every buffer is kept by shape, so the step can
    be captured into a graph and replayed.  ``mask_hist_new`` is then updated in place (FrameLoop hands over a tensor of
    its own for that).

    With ``decoder.compute_dtype = torch.bfloat16`` (and HIP tensors, no gradient) the same step runs on bf16 activations:
    the feature maps are taken as bf16 (a bf16 encoder's pass through untouched, others are cast), the hidden buffers -- so
    the temporal state in ``RefineState`` -- and every convolution are bf16; the pyramid, the cells, ``outs`` and
    ``mask_hist_new`` stay fp32.  The same convolution and launch counts, buffers kept by shape and dtype."""

    def __init__(self, decoder: RSISMask, only_spatial: bool = False, only_temporal: bool = False):
        self.decoder, self.only_spatial, self.only_temporal = decoder, bool(only_spatial), bool(only_temporal)
        self._bufs = {}

    def __call__(self, features, prev_mask, y_mask, init_pred, mask_hist_new, valid, state):
        low = (torch.float16, torch.bfloat16)
        maps = list(features["refine_input_feat"])
        B, O = init_pred.shape[:2]
        H, W = init_pred.shape[-2:]
        if state is None:
            # valid_num_obj_max (evaluator.py:179): the clip's one host read of the decoder
            state = RefineState(max(1, int((valid.sum(0) > 0).sum())))
        n_obj = min(state.n_obj, O)
        init_pred = init_pred.float() if init_pred.dtype in low else init_pred
        planes = [prev_mask, y_mask, init_pred, mask_hist_new]
        dt = getattr(self.decoder, "compute_dtype", torch.float32)
        if dt != torch.float32 and maps[0].is_cuda:
            # the opt-in 16-bit form: a bf16 encoder's maps pass through untouched, others are cast; the planes stay fp32
            feats = [f if f.dtype == dt else f.to(dt) for f in maps]
            if self.decoder.fused_ok(feats + planes):
                return self._fused(feats, prev_mask, y_mask, init_pred, mask_hist_new, valid, state, n_obj, B, O, H, W)
        feats = [f.float() if f.dtype in low else f for f in maps]   # a bf16 encoder's maps: the default arithmetic is fp32
        ts = feats + planes
        if self.decoder.fused_ok(ts):
            return self._fused(feats, prev_mask, y_mask, init_pred, mask_hist_new, valid, state, n_obj, B, O, H, W)
        return self._stock(feats, prev_mask, y_mask, init_pred, mask_hist_new, valid, state, n_obj, B, O, H, W)

    # ---- evaluator.py:179-212 in torch -----------------------------------------------------------------------------------
    def _stock(self, feats, prev_mask, y_mask, init_pred, mask_hist_new, valid, state, n_obj, B, O, H, W):
        prev_thid = state.thid
        pyr = mask_pyramid_torch(*[m.to(feats[0].dtype) for m in (prev_mask, y_mask, init_pred)], n_obj, H, W)
        out_masks, thid = _stock_objects(self.decoder.forward_stock, feats, pyr, prev_thid, n_obj, self.only_temporal)
        logits =[F.interpolate(o, size=(H, W), mode="bilinear", align_corners=True) for o in out_masks]
        for t, up in enumerate(logits):
            for b in range(B):
                # (:202-205 video by video, as the reference evaluates it; the gate stays on the device)
                mask_hist_new[b, t:t + 1] = torch.where(valid[b, t] != 0, torch.sigmoid(up[b]).to(mask_hist_new.dtype),
                                                        mask_hist_new[b, t:t + 1])
        probs = torch.sigmoid(torch.cat(logits, 1))                             # [B, n_obj, H, W]
        outs = probs.new_zeros((B, O, H * W))
        outs[:, :n_obj] = probs.view(B, n_obj, H * W)
        return outs, mask_hist_new, RefineState(state.n_obj, prev_thid if self.only_spatial else thid)

    # ---- the fused step ----------------------------------------------------------------------------------------------------
    def _buffers(self, feats, n_obj, B, O, H, W):
        dec = self.decoder
        dev = feats[0].device
        act = feats[0].dtype                                      # the activations: fp32, or the decoder's compute_dtype
        key = (dev, act, n_obj, B, O, H, W, dec.skip_mode, tuple(tuple(f.shape) for f in feats))
        b = self._bufs.get(key)
        if b is not None:
            return b
        _check_on_pyramid(feats, H, W)
        sizes = pyramid_sizes(H, W)
        new = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
        new_act = lambda *shape: torch.zeros(shape, dtype=act, device=dev)
        dims = dec.skip_dims_out
        h3, w3 = sizes[-1]
        b = {"pyr": [new(n_obj, B, 3, h, w) for h, w in sizes],
             # hidden / cell of every object and level: the spatial chain of this frame, the temporal state of the next
             "hid": [new_act(n_obj, B, dims[i], *sizes[i]) for i in range(4)],
             "cell": [new(n_obj, B, dims[i], *sizes[i]) for i in range(4)],
             "cat": [None] + [new_act(B, dims[i - 1] + dims[i], *sizes[i]) for i in range(1, 4)],
             "up": [None] + [new_act(B, dims[i - 1], *sizes[i]) for i in range(1, 4)],
             "top": new_act(n_obj * B, dims[-1], 2 * h3, 2 * w3),
             "outs": new(B, O, H, W), "valid": torch.zeros((B, O), dtype=torch.int32, device=dev)}
        self._bufs[key] = b
        return b

    def _fused(self, feats, prev_mask, y_mask, init_pred, mask_hist_new, valid, state, n_obj, B, O, H, W):
        dec = self.decoder
        bufs = self._buffers(feats, n_obj, B, O, H, W)
        sl = dec.weight_slices()
        dims = dec.skip_dims_out
        if not mask_hist_new.is_contiguous():
            mask_hist_new = mask_hist_new.contiguous()
        bufs["valid"].copy_(valid)
        mask_pyramid(prev_mask, y_mask, init_pred, n_obj, H, W, out=bufs["pyr"])
        skip_terms = dec.skip_terms(feats)
        # the temporal terms read last frame's hiddens from the very buffers this frame's object loop overwrites: taken
        # for every object and level BEFORE the loop (one batched convolution per level)
        have_t = state.thid is not None
        temporal = None
        if have_t:
            temporal = dec.temporal_terms([bufs["hid"][i].view(n_obj * B, dims[i], *bufs["hid"][i].shape[-2:])
                                           for i in range(4)])
        spatial = None                                            # [(hidden, cell)] per level of the previous object
        for t in range(n_obj):
            if have_t and self.only_temporal:
                spatial = None
            up_src, cur = None, []
            for i, d in enumerate(sl):
                hidden, cell = bufs["hid"][i][t], bufs["cell"][i][t]
                chain_in = next_copy = None
                if i > 0:
                    chain_in = bufs["up"][i] if spatial is None else bufs["cat"][i]
                    # this object's hidden goes, besides its own slot, into the next object's convolution input, which
                    # therefore holds its spatial state already
                    if t + 1 < n_obj and not (have_t and self.only_temporal):
                        next_copy = bufs["cat"][i][:, dims[i - 1]:]
                tt = None if temporal is None else temporal[i][t * B:(t + 1) * B]
                dec._level(i, d, skip_terms[i], tt, feats[i], bufs["pyr"][i][t], None if spatial is None else spatial[i],
                           hidden, cell, up_src, chain_in, holds_state=True, hidden_copy=next_copy)
                cur.append((hidden, cell))
                up_src = hidden
            spatial = cur
        upsample_bilinear_into(bufs["hid"][3].view(n_obj * B, dims[3], *bufs["hid"][3].shape[-2:]), bufs["top"], 0, "write")
        logits = dec._conv(bufs["top"], *dec.head_weights())                        # [n_obj * B, 1, 2h, 2w]
        logits = logits.view(n_obj, B, *logits.shape[-2:]).transpose(0, 1)          # [B, n_obj, 2h, 2w] (strided view)
        refine_finish(logits, bufs["valid"], bufs["outs"], mask_hist_new, n_obj)
        if self.only_spatial:
            thid = state.thid
        else:
            thid = [[bufs["hid"][i][t] for i in range(4)] for t in range(n_obj)]
        return bufs["outs"].view(B, O, H * W), mask_hist_new, RefineState(state.n_obj, thid)


class RefineTrainStep:
    """The refine step of TRAINING: the object loop of ``Trainer.refine`` (``dmm/modules/trainer.py:236-306``) with its loss.

    ``step(features, prev_mask, ref_mask, init_pred, y_mask, sw_mask, valid, state)
        -> (loss, {'hard_iou', 'loss_miou'}, outs_pad [B,O,HW], state)``

    ``features``: the encoder's dict (its ``'refine_input_feat'`` is read) or the four skip maps themselves; ``prev_mask`` /
    ``ref_mask`` / ``y_mask`` [B,O,HW], ``init_pred`` [B,O,H,W], ``sw_mask`` / ``valid`` [B,O].  ``loss`` is ``iou_weight`` *
    the soft-IoU loss of the first ``n_obj`` planes, ``hard_iou`` the trainer's ``hard_iou0`` (``hard_all`` of
    ``losses.mask_step_losses``, which computes both).  ``state`` is a ``RefineState``: ``n_obj`` is the trainer's
    ``valid_num_obj`` -- the number of columns of ``valid`` with any entry set -- read ONCE per clip, when ``state is None``
    (one host read); a caller that runs with ``skip_empty_starting_frame = False`` passes ``RefineState(O)`` of its own.
    ``thid`` carries the temporal hiddens WITH their graph: gradients cross frames through them and through
    ``prev_mask = outs``, so the step keeps no persistent buffers (unlike ``RefineStep``).  The trainer's
    ``num_template_not_empty == 0`` branch (trainer.py:213-216: no refine at all, zero loss terms) stays the caller's.

    Two routes, decided once per call with the decoder's ``_route``:

    * ``_stock``: the trainer's loop op for op on ``decoder.forward`` (``_stock_objects``; the nested pools of the masks are
      taken for all objects at once, which selects the same values) -- CPU tensors, active dropout, any dtype, and every
      decoder that cannot train on its fused form (``fused_train`` off, 1x1 kernels, ...).
    * ``_fused`` (``decoder.fused_train = True``, HIP fp32 tensors): one ``mask_pyramid_fn`` for all objects, the skip terms
      once per frame, one batched temporal convolution per level for all objects, per object the chain convolutions,
      ``clstm_gates_fn`` and ``upsample_bilinear_fn``, then one upsample, one ``conv_out`` and one ``refine_train_finish_fn``
      for all objects.  ``kernels`` names which of the three pieces run on their HIP functions; setting one to False routes
      that piece alone through its torch twin (the same function in torch ops).

    With ``decoder.train_dtype = torch.bfloat16`` (and ``fused_train``, HIP tensors, a gradient required) ``_fused`` runs on
    bf16 ACTIVATIONS, behind an encoder that trains in bf16: the skip maps and the hiddens in ``thid`` are bf16 (anything else
    raises the named ``DmmError``: no silent casts), every convolution runs in bf16 and the kernels between them are the 16-bit
    entries (include/dmm_match.h (12i), (12j), (12l)-(12o)).  ``prev_mask`` / ``ref_mask`` / ``init_pred``, the pyramid, the
    cells, ``outs_pad`` and the loss stay fp32; the parameters stay fp32 masters and receive fp32 gradients, every
    convolution's weight gradient widened before it is added to another's.  The same convolution and launch counts.
    """

    def __init__(self, decoder: RSISMask, only_temporal: bool = False, iou_weight: float = 1.0):
        self.decoder, self.only_temporal, self.iou_weight = decoder, bool(only_temporal), float(iou_weight)
        self.kernels = {"pyramid": True, "upsample": True, "finish": True}
        self.last_route = None                                    # 'fused' | 'stock': the route of the last call (diagnostic)

    def __call__(self, features, prev_mask, ref_mask, init_pred, y_mask, sw_mask, valid, state):
        feats = list(features["refine_input_feat"] if isinstance(features, dict) else features)
        B, O = init_pred.shape[:2]
        H, W = init_pred.shape[-2:]
        if state is None:
            state = RefineState(int((valid.sum(0) > 0).sum()))    # valid_num_obj (trainer.py:146): the clip's one host read
        n_obj = min(state.n_obj, O)
        if n_obj <= 0:
            raise ValueError("RefineTrainStep: no valid object (the trainer's num_template_not_empty == 0 branch is the caller's)")
        dec = self.decoder
        planes = [prev_mask, ref_mask, init_pred]
        hiddens = [] if state.thid is None else [h for hs in state.thid for h in hs]
        route = dec._route(feats + planes + hiddens)
        fused = dec.fused_train and route in ("train", "fused")
        self.last_route = "fused" if fused else "stock"
        if fused and dec._act_dtype(route) == torch.bfloat16 and (route == "train" or feats[0].dtype != torch.float32):
            # (without a gradient the step takes all-fp32 tensors under compute_dtype = bf16 as it always has)
            dec._check_bf16_operands(feats + hiddens, planes, "train_dtype" if route == "train" else "compute_dtype")
        run = self._fused if fused else self._stock
        probs, thid = run(feats, prev_mask, ref_mask, init_pred, state.thid, n_obj, B, O, H, W)      # [B, O, HW]
        from .losses import mask_step_losses
        loss_miou, _, hard_all, _, _ = mask_step_losses(y_mask, probs, sw_mask, valid, n_obj)
        return self.iou_weight * loss_miou, {"hard_iou": hard_all, "loss_miou": loss_miou}, probs, RefineState(state.n_obj, thid)

    # ---- trainer.py:245-287, 302-304 in torch ---------------------------------------------------------------------------
    def _stock(self, feats, prev_mask, ref_mask, init_pred, prev_thid, n_obj, B, O, H, W):
        pyr = mask_pyramid_torch(*[m.to(feats[0].dtype) for m in (prev_mask, ref_mask, init_pred)], n_obj, H, W)
        out_masks, thid = _stock_objects(self.decoder, feats, pyr, prev_thid, n_obj, self.only_temporal)
        out_masks = [F.interpolate(o, (H, W)).view(B, -1) for o in out_masks]
        probs = torch.sigmoid(torch.cat(out_masks, 1).view(B, n_obj, -1))
        outs_pad = probs.new_zeros((B, O, H * W))
        outs_pad[:, :n_obj] = probs
        return outs_pad, thid

    # ---- the fused step --------------------------------------------------------------------------------------------------
    def _fused(self, feats, prev_mask, ref_mask, init_pred, prev_thid, n_obj, B, O, H, W):
        dec, k = self.decoder, self.kernels
        _check_on_pyramid(feats, H, W)
        pyramid =mask_pyramid_fn if k["pyramid"] else mask_pyramid_torch
        bilinear = upsample_bilinear_fn if k["upsample"] else upsample_bilinear_torch
        finish = refine_train_finish_fn if k["finish"] else refine_train_finish_torch
        pyr = pyramid(prev_mask, ref_mask, init_pred, n_obj, H, W)
        sl = dec.train_slices()
        skip_terms = dec.skip_terms(feats, sl)
        temporal = None
        if prev_thid is not None:
            assert len(prev_thid) == n_obj, (len(prev_thid), n_obj)
            # one convolution per level over the hiddens of every object, stacked along the batch
            temporal = dec.temporal_terms([torch.cat([prev_thid[t][i] for t in range(n_obj)], 0) for i in range(4)], sl)
        hidden_spatial, thid, tops = None, [], []
        for t in range(n_obj):
            tt = None
            if temporal is not None:
                tt = [x[t * B:(t + 1) * B] for x in temporal]
                if self.only_temporal:
                    hidden_spatial = None
            up, hidden = dec._forward_fused_train(feats, [p[t] for p in pyr], hidden_spatial, None, slices=sl,
                                                  skip_terms=skip_terms, temporal_terms=tt, bilinear=bilinear, head=False)
            thid.append([hc[0] for hc in hidden])
            hidden_spatial = hidden
            tops.append(up)
        top = torch.cat(tops, 0)                                                    # [n_obj * B, Hd / 8, h, w]
        top = bilinear(top, (top.shape[-2] * 2, top.shape[-1] * 2))
        dec.conv_calls += 1
        logits = _ConvStacked.apply(top, dec.conv_out.weight, dec.conv_out.bias, n_obj, None)   # [n_obj * B, 1, 2h, 2w]
        logits = logits.view(n_obj, B, *logits.shape[-2:]).transpose(0, 1)          # [B, n_obj, 2h, 2w] (strided view)
        return finish(logits, O, H, W).view(B, O, H * W), thid
