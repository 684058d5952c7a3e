"""The float64 reference of the own 3x3 convolution (``dmm_conv3x3_bf16``, include/dmm_match.h (10d)) and what its tests share:
the cases, their inputs (generated on the host, so the same values on every machine), ``F.conv2d`` in float64 on those bf16
values with dx by autograd, and the elementwise bound of a bf16 result.

Bound.  The kernel accumulates in fp32, adds the bias in fp32 and rounds ONCE, so an element is off by half a bf16 ulp of the
reference (2^-9 |ref|) plus the fp32 summation error, which depends on the order: |got - ref| <= 2^-8 |ref| + 1e-3 max|ref| is
the measure ``test_gpu_train_encoder_ref._elementwise`` uses, without its ``pre`` term (no second rounding here).  An
emulation on the host (fp32 accumulation, bias in fp32, one rounding) reached 0.755 of it over these cases."""
import functools
import math

import torch
import torch.nn.functional as F

ULP = 2.0 ** -8                          # bf16: 8 significant bits
CL = torch.channels_last

# (ci, co, stride, B, H, W): each has its own way to go wrong
CASES = [
    (64, 64, 1, 2, 17, 23),              # odd sizes; tiles cross row ends and the image boundary
    (64, 128, 1, 3, 5, 7),               # three images inside one pixel tile
    (128, 128, 2, 2, 17, 23),            # stride 2 at odd sizes
    (128, 64, 2, 2, 16, 24),             # stride 2 at even sizes: right and bottom padding unused
    (192, 192, 1, 2, 9, 13),             # widths that are not a power of two
    (2048, 128, 1, 2, 8, 14),            # K = 18 432 with tiny M: the split-K fold
    (64, 64, 1, 2, 1, 1),                # every tap but one is padding
    (64, 64, 2, 2, 2, 3),                # tiny image at stride 2
    (256, 64, 2, 1, 1, 5),               # single row at stride 2
    (64, 64, 1, 1, 40, 40),              # more than one tile of pixels
]


def case_id(case):
    return "ci{}_co{}_s{}_{}x{}x{}".format(*case)


def out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def flipped(w):
    """wt[ci, co, a, b] = w[co, ci, 2 - a, 2 - b]: the weight whose forward convolution is the data gradient."""
    return torch.flip(w, (2, 3)).transpose(0, 1).contiguous(memory_format=CL)


def spread(dy, H, W, stride):
    """dy at the sampled positions of a [B, C, H, W] plane of zeros."""
    full = torch.zeros((dy.shape[0], dy.shape[1], H, W), dtype=dy.dtype, device=dy.device)
    full[:, :, ::stride, ::stride] = dy
    return full


@functools.lru_cache(maxsize=None)
def inputs(case):
    """bf16 host tensors of a case: x (a ReLU's output), w ~ N(0, 1 / (9 ci)), bias ~ N(0, 0.25), dy ~ N(0, 1)."""
    ci, co, stride, B, H, W = case
    g = torch.Generator().manual_seed(1000 * ci + 10 * co + stride + B + H + W)
    Ho, Wo = out_hw(H, W, stride)
    x = torch.randn((B, ci, H, W), generator=g).relu().bfloat16().contiguous(memory_format=CL)
    w = (torch.randn((co, ci, 3, 3), generator=g) / math.sqrt(9 * ci)).bfloat16().contiguous(memory_format=CL)
    b = (torch.randn((co,), generator=g) * 0.5).bfloat16()
    dy = torch.randn((B, co, Ho, Wo), generator=g).bfloat16().contiguous(memory_format=CL)
    return x, w, b, dy


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> (y without bias, dx) in float64 from the case's bf16 values; computed once, shared, never written to."""
    stride = case[2]
    x, w, _, dy = inputs(case)
    x64 = x.double().contiguous().requires_grad_(True)
    y = F.conv2d(x64, w.double().contiguous(), None, stride, 1)
    dx, = torch.autograd.grad(y, x64, dy.double().contiguous())
    return y.detach(), dx.detach()


def elementwise(got, ref):
    """max over elements of |got - ref| / (2^-8 |ref| + 1e-3 max|ref|): <= 1 is the bound of a once-rounded bf16 result."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    tol = ULP * ref.abs() + 1e-3 * float(ref.abs().max())
    return float(((got - ref).abs() / tol.clamp_min(1e-300)).max())


def record(name, v):
    from conftest import record_achieved
    record_achieved("conv3x3/" + name, v)
