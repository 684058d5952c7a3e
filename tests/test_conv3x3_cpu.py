"""The own 3x3 convolution of the deterministic mode, without a GPU: the identity its stride-2 data gradient rests on, the C
entry's argument validation (nothing is launched), the workspace size, and the setting that selects it."""
import ctypes
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import dmm_net_amd
from conv_ref import flipped, out_hw, spread
from dmm_net_amd import _lib
from dmm_net_amd.train_encoder import _Conv3x3Fn, _conv


@pytest.fixture(autouse=True)
def _restore():
    yield
    dmm_net_amd.set_deterministic_conv("library")
    dmm_net_amd.set_deterministic(None)


@pytest.mark.parametrize("H,W", [(8, 12), (9, 13), (8, 13), (9, 12), (1, 5), (2, 3), (1, 1)])
@pytest.mark.parametrize("stride", [1, 2])
def test_data_gradient_is_a_stride_1_convolution_of_the_spread_gradient_in_fp64(H, W, stride):
    """dx = conv_stride1(dy spread over zeros to [B, co, H, W], wt), wt[ci, co, a, b] = w[co, ci, 2 - a, 2 - b]: equal to
    autograd's dx up to the order of the same fp64 terms (the spread's zeros add exact zeros)."""
    g = torch.Generator().manual_seed(H * 31 + W)
    ci, co, B = 5, 3, 2
    x = torch.randn((B, ci, H, W), generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn((co, ci, 3, 3), generator=g, dtype=torch.float64)
    y = F.conv2d(x, w, None, stride, 1)
    assert tuple(y.shape[2:]) == out_hw(H, W, stride)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    dx, = torch.autograd.grad(y, x, dy)
    got = F.conv2d(spread(dy, H, W, stride), flipped(w), None, 1, 1)
    assert got.shape == dx.shape
    assert float((got - dx).abs().max()) <= 1e-13 * max(1.0, float(dx.abs().max()))


def _lib_loaded():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_conv3x3_entry_validates_its_arguments_without_gpu():
    """Every rejected call answers DMM_ERR_BAD_ARG before anything is launched; B == 0 is nothing to do."""
    L = _lib_loaded()
    OK, BAD = _lib.DMM_OK, _lib.DMM_ERR_BAD_ARG
    one = ctypes.c_void_p(4096)                           # a non-null, 16-byte aligned address nobody dereferences

    def st(B=2, H=8, W=14, ci=64, co=64, stride=1, x=one, w=one, bias=None, y=one, ws=None, ws_bytes=0):
        return L.dmm_conv3x3_bf16(x, w, bias, B, H, W, ci, co, stride, y, ws, ws_bytes, None)

    for kw in (dict(stride=0), dict(stride=3), dict(stride=-1), dict(ci=32), dict(ci=96), dict(co=32), dict(co=65), dict(ci=0),
               dict(co=0), dict(H=0), dict(W=0), dict(B=-1), dict(x=None), dict(w=None), dict(y=None),
               dict(x=ctypes.c_void_p(4098)), dict(bias=ctypes.c_void_p(4100))):
        assert st(**kw) == BAD, kw
    assert st(B=0) == OK and st(B=0, x=None, w=None, y=None) == OK
    assert st(B=0, stride=3) == BAD and st(B=0, ci=32) == BAD                     # sizes before "nothing to do"
    # a shape whose reduction is split: the workspace is needed, null or short answers before any launch
    big = dict(ci=2048, co=128, H=8, W=14, B=2)
    need = L.dmm_conv3x3_workspace_bytes(2, 8, 14, 2048, 128, 1)
    assert need > 0
    assert st(**big) == BAD and st(**big, ws=one, ws_bytes=need - 1) == BAD and st(**big, ws=one, ws_bytes=0) == BAD
    assert st(**big, ws=ctypes.c_void_p(4104), ws_bytes=need) == BAD              # (alignment)


def test_conv3x3_workspace_bytes():
    L = _lib_loaded()
    ws = L.dmm_conv3x3_workspace_bytes
    # split reductions (few pixels per image, a long K): positive, 16-byte aligned, at least one fp32 partial per split
    for B, H, W, ci, co, s in ((2, 8, 14, 2048, 128, 1), (12, 8, 14, 512, 512, 1), (12, 16, 28, 256, 256, 1), (12, 32, 56, 512, 512, 2)):
        n = ws(B, H, W, ci, co, s)
        Ho, Wo = out_hw(H, W, s)
        assert n > 0 and n % 16 == 0 and n >= 2 * 4 * B * Ho * Wo * co and n % (4 * B * Ho * Wo * co) == 0, (B, H, W, ci, co, s)
    # grows with the batch by exactly the batch: the number of splits does not depend on it
    assert ws(6, 8, 14, 512, 512, 1) == 3 * ws(2, 8, 14, 512, 512, 1)
    # shapes whose pixel tiles fill the chip need none; rejected arguments answer 0
    assert ws(12, 64, 112, 64, 64, 1) == 0
    for bad in ((2, 8, 14, 2048, 128, 3), (2, 8, 14, 2048, 100, 1), (2, 8, 14, 96, 128, 1), (0, 8, 14, 2048, 128, 1),
                (2, 0, 14, 2048, 128, 1)):
        assert ws(*bad) == 0, bad


def test_setting_defaults_to_library_and_rejects_other_values():
    assert dmm_net_amd.get_deterministic_conv() == "library"
    dmm_net_amd.set_deterministic_conv("own")
    assert dmm_net_amd.get_deterministic_conv() == "own"
    for bad in ("Own", "miopen", "", None, True, 1):
        with pytest.raises(ValueError):
            dmm_net_amd.set_deterministic_conv(bad)
    assert dmm_net_amd.get_deterministic_conv() == "own"                          # a rejected value changes nothing
    dmm_net_amd.set_deterministic_conv("library")
    assert dmm_net_amd.get_deterministic_conv() == "library"


def test_setting_takes_effect_only_in_the_mode():
    from dmm_net_amd.train_encoder import _own_conv_now
    dmm_net_amd.set_deterministic_conv("own")
    with dmm_net_amd.deterministic(False):
        assert not _own_conv_now()
    with dmm_net_amd.deterministic(True):
        assert _own_conv_now()
        dmm_net_amd.set_deterministic_conv("library")
        assert not _own_conv_now()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cpu_path_of_conv_is_untouched_by_the_setting(dtype):
    """Off the GPU ``_conv`` runs the stock convolution whatever the setting: same bits, same autograd route."""
    torch.manual_seed(4)
    m = nn.Conv2d(64, 64, 3, 2, 1, bias=True)
    x = torch.randn(2, 64, 9, 11).to(dtype).contiguous(memory_format=torch.channels_last)
    outs = []
    for which in ("library", "own"):
        dmm_net_amd.set_deterministic_conv(which)
        with dmm_net_amd.deterministic(True):
            xg = x.clone().requires_grad_(True)
            m.zero_grad(set_to_none=True)
            y = _conv(xg, m, dtype)
            assert not isinstance(y.grad_fn, _Conv3x3Fn._backward_cls) and "Conv3x3" not in type(y.grad_fn).__name__
            y.float().sum().backward()
            outs.append((y.detach(), xg.grad, m.weight.grad.clone(), m.bias.grad.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    ref = F.conv2d(x, m.weight.to(dtype=dtype, memory_format=torch.channels_last), m.bias.to(dtype), 2, 1)
    assert torch.equal(outs[0][0], ref)
