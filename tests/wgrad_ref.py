"""The float64 reference of the weight-gradient kernels (``dmm_wgrad_bf16`` / ``dmm_wgrad3x3_bf16``, csrc/dmm_wgrad.hip) and what
their tests share: the cases, two families of inputs (generated on the host as ``conv_ref.inputs`` generates them, so the same
values on every machine), the reference with the sum of the terms' magnitudes beside it, and the bounds.

Cases.  A row is (shape, groups, reduce): the shape, and as LITERALS the number of slab groups ``wgrad_plan`` gives it and the
second launch it reaches -- ``None``: one group of a plain product is stored straight into dw, no second launch; else S, the
threads per output of ``wgrad_reduce_kernel<S, T9>`` (T9 = the 3x3 entry's [co, ci, 3, 3] layout).  The kernel form follows from the
widths by the three lines of ``wgrad_plan`` that ``form`` restates, the tables are grouped by it; tests/test_wgrad_ref_cpu.py holds
every literal to the library's host planner and shows that the tables reach every form, every direct store and every S of both
reduce layouts.  The shapes are the smallest that reach a mechanism: rows below one 16-row step, one 32-row stage, one 256-row
round; a slab of 2 rows; images smaller than one stage of 64 output pixels, so that the branch-free pixel cursor of the staged
kernels steps over several images per stage; Wo == 1 and Ho == 1; column tiles that hold two taps or end beyond the last column.

Families.  ``"int"``: x and dy are integers in [-3, 3] times 2^(c % 13 - 6) per channel c.  Every value is a bf16, every product is
exact, every partial sum of an output is an integer below 2^24 times ONE power of two: fp32 accumulation is exact in any order,
so the kernels must return the float64 reference bit for bit -- for outputs whose magnitudes span 2^24.  A dropped, doubled or
misplaced row, tap, channel or slab shows as a wrong bit; this family carries the indexing.  ``"relu"``: x = relu(randn) 2^(c % 13 - 6),
dy = randn 2^(c % 11 - 5), rounded to bf16 -- what the layers see (a ReLU's output against a gradient, per-channel scales orders of
magnitude apart); it shows arithmetic that loses precision, which integers cannot.

Bounds.  ``scaled(got, ref, A)`` = max |got - ref| / A over the elements with A > 0, A the same sum over the magnitudes: an
error relative to what was summed, per element, so a small output beside large ones is judged by its own terms.
``bound_worst(n)`` = n 2^-23 bounds it for ANY fp32 summation order of n exact products whether an addition rounds to nearest or
truncates: at most n - 1 additions lie above a product, each off by at most 2^-23 of its result, and no partial result exceeds
A(1 + (n - 1) 2^-23).  Derived, not measured.  A host fp32 product (``host_fp32``) of every ``"relu"`` case reached at most
0.167 of it (3x3 (1, 1, 5, 256, 128, 2): 3 rows, where ONE rounding to nearest is a sixth of the bound; 0.124 at 4 rows, 0.097 at 2
rows -- the ratio falls with the row count, the bound grows with n and a rounding error with about sqrt(n))."""
import functools

import torch
import torch.nn.functional as F

FAMILIES = ("int", "relu")

# ---- 1x1: (rows, co, ci), groups, reduce -------------------------------------------------------------------------------------------
CASES_1X1 = {
    "wave": [                                       # 64 x 64 tiles, one wave per slab (wgrad_bf16_kernel<false>)
        ((1, 64, 64), 1, None),                     # one row: 15 of 16 rows of the only step are masked
        ((37, 64, 64), 1, None),                    # three steps, the last with 5 rows
        ((600, 64, 64), 2, 2),
        ((2100, 192, 64), 5, 4),
        ((5000, 64, 64), 10, 8),
        ((9000, 64, 64), 18, 16),
        ((515, 192, 320), 2, 2),                    # 15 tiles; the last wave of the second group owns no row
        ((515, 832, 1280), 2, 1),                   # a table of 2^20 outputs: the float4 reduce without fold
    ],
    "lds": [                                        # 128 x 128 tiles staged through LDS (wgrad_lds_kernel<false>)
        ((1, 128, 128), 1, None),                   # less than one 32-row stage
        ((31, 128, 128), 1, None),
        ((130, 128, 128), 2, 2),                    # the second slab has 2 rows
        ((700, 128, 128), 6, 4),
        ((1100, 128, 128), 9, 8),
        ((4200, 128, 128), 33, 16),
        ((300, 256, 512), 3, 2),
        ((260, 2048, 512), 3, 1),                   # the float4 reduce without fold
    ],
    "tile64x128": [                                 # wgrad_tile_kernel<false, 4, 64, 128>
        ((1, 64, 128), 1, None),
        ((300, 64, 128), 2, 2),
        ((777, 64, 192), 4, 4),                     # a half-empty column tile
        ((2100, 64, 128), 9, 8),
        ((8200, 64, 128), 33, 16),
        ((300, 64, 16384), 2, 1),
    ],
    "tile128x64": [                                 # wgrad_tile_kernel<false, 4, 128, 64>: below one 256-row round, and above
        ((1, 128, 64), 1, None),
        ((300, 384, 64), 2, 2),
        ((800, 128, 64), 4, 4),
        ((2100, 128, 64), 9, 8),
        ((8200, 128, 64), 33, 16),
        ((300, 16384, 64), 2, 1),
    ],
}

# ---- 3x3: (B, H, W, ci, co, stride), groups, reduce ----------------------------------------------------------------------------
CASES_3X3 = {
    "tile_patch": [                                 # co == 64: wgrad_tile_kernel<true, 4, 64, 128>
        ((2, 1, 1, 64, 64, 1), 1, 1),               # every tap but one is padding; 2 rows
        ((2, 5, 3, 64, 64, 2), 1, 1),
        ((3, 9, 13, 64, 64, 1), 2, 2),
        ((1, 40, 40, 64, 64, 1), 7, 4),
        ((1, 43, 43, 64, 64, 1), 8, 8),
        ((2, 64, 64, 64, 64, 1), 32, 16),
        ((5, 3, 3, 128, 64, 1), 1, 1),
        ((150, 1, 2, 64, 64, 1), 2, 2),             # 64 images per step of 128 output pixels: this kernel's cursor over whole images
        ((2, 2, 3, 192, 64, 2), 1, 1),              # 13.5 column tiles and two taps in a tile
    ],
    "lds_patch": [                                  # wgrad_lds_kernel<true>: the pixel cursor with two carries
        ((70, 1, 1, 128, 128, 1), 1, 1),            # 64 images per stage
        ((20, 2, 2, 128, 128, 1), 1, 1),            # 16 images per stage
        ((9, 3, 2, 128, 128, 2), 1, 1),             # Wo == 1 (18 rows: the cursor's start, no step)
        ((40, 3, 2, 128, 128, 2), 1, 1),            # Wo == 1 over 80 rows: 32 images per step
        ((40, 1, 3, 128, 128, 1), 1, 1),            # Ho == 1
        ((1, 1, 5, 256, 128, 2), 1, 1),             # 3 rows
        ((2, 17, 23, 128, 128, 2), 2, 2),
        ((2, 17, 23, 128, 128, 1), 7, 4),
        ((1, 40, 40, 128, 128, 1), 13, 8),
        ((2, 33, 41, 128, 128, 1), 22, 16),
        ((2, 5, 7, 256, 384, 1), 1, 1),
        ((2, 8, 14, 512, 512, 1), 1, 1),            # S1 with the 9-tap layout on a large table
    ],
    "wave_patch": [                                 # wgrad_bf16_kernel<true>
        ((30, 1, 1, 64, 128, 1), 1, 1),
        ((2, 9, 13, 64, 128, 1), 1, 1),
        ((2, 17, 23, 64, 128, 2), 1, 1),
        ((2, 9, 13, 192, 192, 1), 1, 1),
        ((2, 17, 23, 64, 128, 1), 2, 2),
        ((2, 33, 41, 64, 128, 1), 6, 4),
        ((1, 70, 70, 64, 128, 1), 10, 8),
        ((1, 89, 91, 64, 128, 1), 16, 16),
    ],
}

ALL_1X1 = [row for rows in CASES_1X1.values() for row in rows]
ALL_3X3 = [row for rows in CASES_3X3.values() for row in rows]
STRIDED_1X1 = [(600, 64, 64), (130, 128, 128), (300, 64, 128), (300, 384, 64)]        # one per kernel form, run on strided operands too


def is_3x3(case):
    return len(case) == 6


def case_id(case):
    return "{}x{}x{}x{}x{}s{}".format(*case) if is_3x3(case) else "{}x{}x{}".format(*case)


def out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def dims(case):
    """-> (rows, co, cv): the product the planner sees; cv = 9 ci for the 3x3 entry."""
    if is_3x3(case):
        B, H, W, ci, co, stride = case
        Ho, Wo = out_hw(H, W, stride)
        return B * Ho * Wo, co, 9 * ci
    return case


def form(case):
    """The kernel form ``wgrad_plan`` picks, restated from its three lines."""
    _, co, cv = dims(case)
    ci_patch = case[3] if is_3x3(case) else 0
    wide = co % 128 == 0 and cv % 128 == 0 and ci_patch % 128 == 0
    if wide:
        name = "lds"
    elif co == 64 and cv >= 128 and cv % 64 == 0:
        name = "tile" if ci_patch else "tile64x128"
    elif cv == 64 and co % 128 == 0 and not ci_patch:
        name = "tile128x64"
    else:
        name = "wave"
    return name + "_patch" if ci_patch else name


def reduce_form(case, groups):
    """The second launch of ``wgrad_launch`` for ``groups`` slab groups: None (direct store) or S, restated from its loop."""
    _, co, cv = dims(case)
    if groups == 1 and not is_3x3(case):
        return None
    outs = co * cv // (9 if is_3x3(case) else 4)
    S = 1
    while S < 16 and 2 * S <= groups and outs * S < 256 * 1024:
        S *= 2
    return S


def _scale(channels, period, shift):
    return torch.pow(2.0, (torch.arange(channels) % period - shift).double())


@functools.lru_cache(maxsize=None)
def inputs(case, family):
    """bf16 host tensors (dy, x) of a case: [rows, co] and [rows, ci], or channels-last [B, co, Ho, Wo] and [B, ci, H, W]."""
    g = torch.Generator().manual_seed(sum(int(v) * 31 ** k for k, v in enumerate(case)) % (2 ** 31) + FAMILIES.index(family))
    if is_3x3(case):
        B, H, W, ci, co, stride = case
        Ho, Wo = out_hw(H, W, stride)
        sdy, sx = (B, Ho, Wo, co), (B, H, W, ci)
    else:
        rows, co, ci = case
        sdy, sx = (rows, co), (rows, ci)
    if family == "int":
        dy = torch.randint(-3, 4, sdy, generator=g).double() * _scale(co, 13, 6)
        x = torch.randint(-3, 4, sx, generator=g).double() * _scale(ci, 13, 6)
    else:
        dy = torch.randn(sdy, generator=g).double() * _scale(co, 11, 5)
        x = torch.randn(sx, generator=g).relu().double() * _scale(ci, 13, 6)
    dy16, x16 = dy.bfloat16(), x.bfloat16()
    if family == "int":
        assert torch.equal(dy16.double(), dy) and torch.equal(x16.double(), x)
    if is_3x3(case):
        dy16, x16 = dy16.permute(0, 3, 1, 2), x16.permute(0, 3, 1, 2)        # channels-last [B, C, H, W] views of the NHWC data
    return dy16, x16


def taps(x, Ho, Wo, stride):
    """The nine shifted and strided slices of the zero-padded x [B, ci, H, W], as [rows, ci] matrices in (kh, kw) order."""
    B, ci, H, W = x.shape
    xp = torch.zeros((B, ci, H + 2, W + 2), dtype=x.dtype, device=x.device)
    xp[:, :, 1:H + 1, 1:W + 1] = x
    out = []
    for kh in range(3):
        for kw in range(3):
            s = xp[:, :, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride]
            out.append(s.permute(0, 2, 3, 1).reshape(B * Ho * Wo, ci).contiguous())
    return out


def product(dy, x, case, dtype=torch.float64):
    """dw of the case from (dy, x) in ``dtype`` on their device: dy^T x, or one such product per tap -> [co, ci, 3, 3]."""
    dy, x = dy.to(dtype), x.to(dtype)
    if not is_3x3(case):
        return dy.t().contiguous() @ x.contiguous()
    B, H, W, ci, co, stride = case
    Ho, Wo = out_hw(H, W, stride)
    dyt = dy.permute(1, 0, 2, 3).reshape(co, B * Ho * Wo).contiguous()
    return torch.stack([dyt @ s for s in taps(x, Ho, Wo, stride)], 2).view(co, ci, 3, 3)


@functools.lru_cache(maxsize=None)
def reference(case, family):
    """-> (dw64, A): the float64 product of the case's bf16 values and the same sum over the absolute values; computed once,
    shared, never written to."""
    dy, x = inputs(case, family)
    return product(dy, x, case), product(dy.abs(), x.abs(), case)


def host_fp32(case, family):
    """An fp32 evaluation of the same sums on the host (torch's CPU product: some other order than the kernels')."""
    dy, x = inputs(case, family)
    return product(dy, x, case, torch.float32)


def conv2d_autograd(case, family):
    """float64 ``F.conv2d`` autograd's weight gradient of a 3x3 case: what the nine-slice reference is held to on the CPU."""
    dy, x = inputs(case, family)
    ci, co, stride = case[3], case[4], case[5]
    w = torch.zeros((co, ci, 3, 3), dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x.double().contiguous(), w, None, stride, 1)
    dw, = torch.autograd.grad(y, w, dy.double().contiguous())
    return dw


def scaled(got, ref, A):
    """max |got - ref| / A over the elements with A > 0 (where A == 0 every term is zero and so is ref)."""
    got, ref, A = got.detach().double().cpu(), ref.detach().double().cpu(), A.detach().double().cpu()
    ok = A > 0
    if not bool(ok.any()):
        return 0.0
    return float(((got - ref).abs()[ok] / A[ok]).max())


def bound_worst(n):
    return n * 2.0 ** -23


FLOOR = 2.0 ** -24                       # one fp32 rounding relative to A: the floor of the yardstick rule


def yardstick(q_stock):
    """The project's rule (``held`` in tests/test_gpu_decoder.py): no further from float64 than twice the stock fp32 evaluation
    of the same values on the same device, with one rounding as its floor."""
    return 2 * max(q_stock, FLOOR)
