"""The float64 reference of the narrow 3x3 convolutions (``dmm_conv3x3_narrow_bf16`` / ``dmm_wgrad3x3_narrow_bf16``,
include/dmm_match.h (10e)) and what their tests share: the cases, their inputs (generated on the host as ``conv_ref.inputs``
generates them, so the same values on every machine) and ``F.conv2d`` in float64 on those bf16 values with dx and dw by
autograd.

Bounds.  y and dx: ``conv_ref.elementwise(...) <= 1``, the bound of a once-rounded bf16 result (fp32 accumulation, the bias
added in fp32, one rounding); a host emulation of that arithmetic reached at most 0.733 (y) and 0.723 (dx) of it over these
cases.  dw (fp32 out): max|dw - ref| <= 1e-4 max|ref|, the bound the route tests hold ``dmm_wgrad3x3_bf16`` to; the fp32
emulation reached at most 4.5e-7."""
import functools
import math

import torch
import torch.nn.functional as F

from conv_ref import CL, elementwise, flipped, record  # noqa: F401  (shared with the tests that import this module)

DW_BOUND = 1e-4

# (ci, co, B, H, W): the smallest shapes at which each mechanism can go wrong
CASES = [
    (256, 32, 2, 17, 23),                # the 32-channel output tile; odd sizes, tiles crossing row ends and image boundaries
    (32, 128, 2, 17, 23),                # a 32-channel input: 9 taps of 32 channels, an odd count of half stages
    (32, 32, 3, 5, 7),                   # both sides narrow; three images inside one pixel tile
    (96, 160, 2, 9, 13),                 # odd multiples of 32 on both sides; the 64-tile tail in co
    (544, 32, 2, 8, 14),                 # ci = 17 x 32: a long reduction with a half stage at its end
    (64, 32, 2, 16, 24),                 # ci a multiple of 64 beside a narrow co, even sizes
    (32, 32, 2, 1, 1),                   # every tap but one is padding
    (32, 64, 1, 1, 5),                   # a single row
    (32, 32, 1, 40, 40),                 # more than one pixel tile of one image; more than one row slab in the weight gradient
]


def case_id(case):
    return "ci{}_co{}_{}x{}x{}".format(*case)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """bf16 host tensors of a case: x (a ReLU's output), w ~ N(0, 1 / (9 ci)), bias ~ N(0, 0.25), dy ~ N(0, 1)."""
    ci, co, B, H, W = case
    g = torch.Generator().manual_seed(1000 * ci + 10 * co + B + H + W)
    x = torch.randn((B, ci, H, W), generator=g).relu().bfloat16().contiguous(memory_format=CL)
    w = (torch.randn((co, ci, 3, 3), generator=g) / math.sqrt(9 * ci)).bfloat16().contiguous(memory_format=CL)
    b = (torch.randn((co,), generator=g) * 0.5).bfloat16()
    dy = torch.randn((B, co, H, W), generator=g).bfloat16().contiguous(memory_format=CL)
    return x, w, b, dy


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> (y without bias, dx, dw) in float64 from the case's bf16 values; computed once, shared, never written to."""
    x, w, _, dy = inputs(case)
    x64 = x.double().contiguous().requires_grad_(True)
    w64 = w.double().contiguous().requires_grad_(True)
    y = F.conv2d(x64, w64, None, 1, 1)
    dx, dw = torch.autograd.grad(y, [x64, w64], dy.double().contiguous())
    return y.detach(), dx.detach(), dw.detach()


def dw_error(got, ref):
    """max|got - ref| / max|ref|."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max()) / float(ref.abs().max())
