"""The float64 reference of the 7x7 / stride 2 / padding 3 stem convolution (``dmm_conv7x7s2_stem_bf16`` /
``dmm_wgrad7x7s2_stem_bf16``, include/dmm_match.h (10f)) and what its tests share: the cases, their inputs (generated on the host,
so the same values on every machine) and ``F.conv2d(..., 2, 3)`` in float64 on those bf16 values with dw by autograd.

Bounds, both the project's own.  y: ``conv_ref.elementwise(...) <= 1``, the bound of a once-rounded bf16 result (fp32
accumulation, the bias added in fp32, one rounding).  dw (fp32 out): ``conv_narrow_ref.dw_error(...) <= DW_BOUND`` = 1e-4, the
bound every own weight-gradient kernel is held to.  ``emulate`` is that arithmetic on the host (fp32 ``F.conv2d``, the bias in
fp32, one rounding; dw by fp32 autograd): over these cases it reached at most 0.752 of the y bound (with and without bias)
and 6.2e-7 for dw, so the reference arithmetic alone stays inside both (tests/test_conv_stem_cpu.py holds it to them)."""
import functools
import math

import torch
import torch.nn.functional as F

from conv_narrow_ref import DW_BOUND, dw_error  # noqa: F401  (shared with the tests that import this module)
from conv_ref import CL, elementwise, record  # noqa: F401

# (B, H, W): each has its own way to go wrong
CASES = [
    (2, 17, 23),                         # odd sizes: three padding rows / columns at the far edges; 138-byte rows alternate 4-byte phase
    (2, 16, 24),                         # even sizes: two padding rows / columns at the far edges
    (3, 5, 7),                           # images smaller than the window; three images inside one pixel tile
    (2, 1, 1),                           # 48 of 49 taps are padding
    (1, 1, 9),                           # a single row
    (1, 2, 3),                           # a tiny image
    (1, 6, 6),                           # a tiny image
    (1, 80, 80),                         # 1 600 output pixels: more than one pixel tile, more than one slab in the weight gradient
    (2, 33, 131),                        # Wo = 66: tile boundaries inside rows at odd offsets
    (1, 7, 449),                         # a 225-pixel output row; odd W
]


def case_id(case):
    return "{}x{}x{}".format(*case)


def out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


@functools.lru_cache(maxsize=None)
def inputs(case):
    """bf16 host tensors of a case: x ~ N(0, 1) (a normalised image), w ~ N(0, 1 / 147), bias ~ N(0, 0.25), dy ~ N(0, 1)."""
    B, H, W = case
    g = torch.Generator().manual_seed(7000 + 100 * B + 10 * H + W)
    Ho, Wo = out_hw(H, W)
    x = torch.randn((B, 3, H, W), generator=g).bfloat16().contiguous(memory_format=CL)
    w = (torch.randn((64, 3, 7, 7), generator=g) / math.sqrt(147)).bfloat16().contiguous(memory_format=CL)
    b = (torch.randn((64,), generator=g) * 0.5).bfloat16()
    dy = torch.randn((B, 64, Ho, Wo), generator=g).bfloat16().contiguous(memory_format=CL)
    return x, w, b, dy


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> (y without bias, dw) in float64 from the case's bf16 values; computed once, shared, never written to."""
    x, w, _, dy = inputs(case)
    w64 = w.double().contiguous().requires_grad_(True)
    y = F.conv2d(x.double().contiguous(), w64, None, 2, 3)
    dw, = torch.autograd.grad(y, w64, dy.double().contiguous())
    return y.detach(), dw.detach()


def emulate(case, bias):
    """The kernels' arithmetic on the host: fp32 accumulation, the bias added in fp32, one rounding -> (y bf16, dw fp32)."""
    x, w, b, dy = inputs(case)
    w32 = w.float().contiguous().requires_grad_(True)
    y = F.conv2d(x.float().contiguous(), w32, b.float() if bias else None, 2, 3)
    dw, = torch.autograd.grad(y, w32, dy.float().contiguous())
    return y.detach().bfloat16(), dw.detach()
