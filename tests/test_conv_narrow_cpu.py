"""The narrow 3x3 convolutions of the deterministic mode (include/dmm_match.h (10e)), without a GPU: the C entries' argument
validation (nothing is launched), the weight gradient's workspace size, and the ``"own_all"`` setting that selects them."""
import ctypes
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import dmm_net_amd
from dmm_net_amd import _lib
from dmm_net_amd.train_encoder import _conv, _narrow_conv_now, _narrow_ok, _own_conv_now, _wgrad_ok


@pytest.fixture(autouse=True)
def _restore():
    yield
    dmm_net_amd.set_deterministic_conv("library")
    dmm_net_amd.set_deterministic(None)


def _lib_loaded():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


ONE = ctypes.c_void_p(4096)                               # a non-null, 16-byte aligned address nobody dereferences


def test_conv_entry_validates_its_arguments_without_gpu():
    """Every rejected call answers DMM_ERR_BAD_ARG before anything is launched; B == 0 is nothing to do."""
    L = _lib_loaded()
    OK, BAD = _lib.DMM_OK, _lib.DMM_ERR_BAD_ARG

    def st(B=2, H=8, W=14, ci=32, co=32, x=ONE, w=ONE, bias=None, y=ONE):
        return L.dmm_conv3x3_narrow_bf16(x, w, bias, B, H, W, ci, co, y, None)

    for kw in (dict(ci=16), dict(ci=48), dict(co=16), dict(co=48), dict(co=33), dict(ci=0), dict(co=0), dict(ci=-32), dict(H=0),
               dict(W=0), dict(H=-1), dict(B=-1), dict(x=None), dict(w=None), dict(y=None), dict(x=ctypes.c_void_p(4098)),
               dict(w=ctypes.c_void_p(4104)), dict(y=ctypes.c_void_p(4100)), dict(bias=ctypes.c_void_p(4100)),
               dict(B=2 ** 31 - 1, H=2 ** 15, W=2 ** 15)):                # more than 2^31 - 1 pixel tiles
        assert st(**kw) == BAD, kw
    assert st(B=0) == OK and st(B=0, x=None, w=None, y=None) == OK
    assert st(B=0, ci=64, co=96) == OK and st(B=0, ci=256, co=128) == OK          # multiples of 64 are taken too
    assert st(B=0, ci=48) == BAD and st(B=0, H=0) == BAD                          # sizes before "nothing to do"


def test_wgrad_entry_validates_its_arguments_without_gpu():
    """Bad sizes and null pointers answer DMM_ERR_BAD_ARG, a null or short workspace DMM_ERR_WORKSPACE -- all before a launch."""
    L = _lib_loaded()
    BAD, WS = _lib.DMM_ERR_BAD_ARG, _lib.DMM_ERR_WORKSPACE
    need = L.dmm_wgrad3x3_narrow_workspace_bytes(2, 8, 14, 32, 32)
    assert need > 0
    dw = ctypes.cast(ONE, ctypes.POINTER(ctypes.c_float))

    def st(B=2, H=8, W=14, ci=32, co=32, dy=ONE, x=ONE, dw=dw, ws=ONE, ws_bytes=need):
        return L.dmm_wgrad3x3_narrow_bf16(dy, x, B, H, W, ci, co, dw, ws, ws_bytes, None)

    for kw in (dict(ci=16), dict(ci=48), dict(co=16), dict(co=48), dict(ci=0), dict(co=0), dict(H=0), dict(W=0), dict(B=-1),
               dict(dy=None), dict(x=None), dict(dw=None), dict(dy=ctypes.c_void_p(4098)), dict(x=ctypes.c_void_p(4097)),
               dict(B=0, ci=48), dict(B=0, dw=None)):
        assert st(**kw) == BAD, kw
    for kw in (dict(ws=None), dict(ws=None, ws_bytes=0), dict(ws_bytes=0), dict(ws_bytes=need - 1)):
        assert st(**kw) == WS, kw
    assert st(ws=ctypes.c_void_p(4104)) == BAD                                    # (the workspace's alignment)


def test_wgrad_workspace_bytes():
    L = _lib_loaded()
    ws = L.dmm_wgrad3x3_narrow_workspace_bytes
    # positive, 16-byte aligned, a whole number of fp32 [co, 9 ci] partial tables
    for B, H, W, ci, co in ((2, 17, 23, 256, 32), (2, 17, 23, 32, 128), (3, 5, 7, 32, 32), (2, 9, 13, 96, 160), (2, 1, 1, 32, 32),
                            (12, 64, 112, 256, 32), (12, 64, 112, 32, 128), (1, 40, 40, 32, 32), (1, 40, 40, 64, 64)):
        n = ws(B, H, W, ci, co)
        assert n > 0 and n % 16 == 0 and n % (4 * co * 9 * ci) == 0, (B, H, W, ci, co)
    # row slabs are folded where there are rows enough: more than one table
    assert ws(1, 40, 40, 32, 32) >= 2 * 4 * 32 * 9 * 32
    assert ws(12, 64, 112, 256, 32) >= 2 * 4 * 32 * 9 * 256
    assert ws(2, 1, 1, 32, 32) == 4 * 32 * 9 * 32                                 # two rows: one slab
    # a function of its arguments alone: asked again, around other calls, the answer is the same
    first = [ws(2, 17, 23, 256, 32), ws(12, 64, 112, 32, 128)]
    ws(1, 40, 40, 32, 32)
    assert [ws(2, 17, 23, 256, 32), ws(12, 64, 112, 32, 128)] == first
    # rejected arguments answer 0
    for bad in ((2, 8, 14, 16, 32), (2, 8, 14, 32, 48), (2, 8, 14, 0, 32), (2, 8, 14, 32, 0), (0, 8, 14, 32, 32), (-1, 8, 14, 32, 32),
                (2, 0, 14, 32, 32), (2, 8, 0, 32, 32)):
        assert ws(*bad) == 0, bad


def test_setting_accepts_own_all_and_still_rejects_other_values():
    assert dmm_net_amd.get_deterministic_conv() == "library"
    dmm_net_amd.set_deterministic_conv("own_all")
    assert dmm_net_amd.get_deterministic_conv() == "own_all"
    for bad in ("Own", "miopen", "", None, True, 1, "own-all", "OWN_ALL", "all"):
        with pytest.raises(ValueError):
            dmm_net_amd.set_deterministic_conv(bad)
    assert dmm_net_amd.get_deterministic_conv() == "own_all"                      # a rejected value changes nothing
    dmm_net_amd.set_deterministic_conv("own")
    assert dmm_net_amd.get_deterministic_conv() == "own"
    dmm_net_amd.set_deterministic_conv("library")
    assert dmm_net_amd.get_deterministic_conv() == "library"


def test_settings_take_effect_only_in_the_mode():
    for which, narrow in (("own", False), ("own_all", True)):
        dmm_net_amd.set_deterministic_conv(which)
        with dmm_net_amd.deterministic(False):
            assert not _own_conv_now() and not _narrow_conv_now()
        with dmm_net_amd.deterministic(True):
            assert _own_conv_now() and _narrow_conv_now() == narrow
    dmm_net_amd.set_deterministic_conv("library")
    with dmm_net_amd.deterministic(True):
        assert not _own_conv_now() and not _narrow_conv_now()


def test_narrow_predicate():
    yes = [nn.Conv2d(256, 32, 3, 1, 1), nn.Conv2d(32, 128, 3, 1, 1), nn.Conv2d(32, 32, 3, 1, 1, bias=False), nn.Conv2d(96, 160, 3, 1, 1)]
    no = [nn.Conv2d(64, 64, 3, 1, 1), nn.Conv2d(256, 128, 3, 1, 1),              # _wgrad_ok: the wide kernels' own
          nn.Conv2d(256, 16, 3, 1, 1), nn.Conv2d(48, 32, 3, 1, 1),                # a multiple of 16 only
          nn.Conv2d(256, 32, 3, 2, 1), nn.Conv2d(256, 32, 3, 1, 0), nn.Conv2d(256, 32, 1, 1, 0), nn.Conv2d(256, 32, 5, 1, 1),
          nn.Conv2d(256, 32, 3, 1, 1, groups=2), nn.Conv2d(256, 32, 3, 1, 2, dilation=2), nn.Conv2d(3, 64, 7, 2, 3)]
    assert all(_narrow_ok(m) and not _wgrad_ok(m) for m in yes)
    assert not any(_narrow_ok(m) for m in no)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cpu_path_of_a_narrow_conv_is_untouched_by_the_setting(dtype):
    """Off the GPU ``_conv`` runs the stock convolution whatever the setting: same bits, same autograd route."""
    torch.manual_seed(4)
    m = nn.Conv2d(32, 64, 3, 1, 1, bias=True)
    assert _narrow_ok(m)
    x = torch.randn(2, 32, 9, 11).to(dtype).contiguous(memory_format=torch.channels_last)
    outs, nodes = [], []
    for which in ("library", "own", "own_all"):
        dmm_net_amd.set_deterministic_conv(which)
        with dmm_net_amd.deterministic(True):
            xg = x.clone().requires_grad_(True)
            m.zero_grad(set_to_none=True)
            y = _conv(xg, m, dtype)
            nodes.append(type(y.grad_fn).__name__)
            y.float().sum().backward()
            outs.append((y.detach(), xg.grad, m.weight.grad.clone(), m.bias.grad.clone()))
    assert nodes[0] == nodes[1] == nodes[2] and "Narrow" not in nodes[0] and "Conv3x3" not in nodes[0], nodes
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1])) and all(torch.equal(a, b) for a, b in zip(outs[0], outs[2]))
    ref = F.conv2d(x, m.weight.to(dtype=dtype, memory_format=torch.channels_last), m.bias.to(dtype), 1, 1)
    assert torch.equal(outs[0][0], ref)
