"""The 7x7 / stride 2 stem convolution of the deterministic mode (include/dmm_match.h (10f)), without a GPU: the ``"own_stem"``
setting that selects it, the route predicates, the C entries' argument validation (nothing is launched), the weight gradient's
workspace size, and the reference file's own emulation against its bounds."""
import ctypes
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import dmm_net_amd
from conv_stem_ref import CASES, DW_BOUND, case_id, dw_error, elementwise, emulate, inputs, reference
from dmm_net_amd import _lib
from dmm_net_amd.train_encoder import _conv, _conv_route, _narrow_conv_now, _own_conv_now, _stem_conv_now, _stem_ok


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


def test_setting_accepts_own_stem_and_still_rejects_other_values():
    assert dmm_net_amd.get_deterministic_conv() == "library"
    dmm_net_amd.set_deterministic_conv("own_stem")
    assert dmm_net_amd.get_deterministic_conv() == "own_stem"
    for bad in ("Own_stem", "stem", "", None, True, 1, "own-stem", "OWN_STEM", "own_all_stem", "all"):
        with pytest.raises(ValueError):
            dmm_net_amd.set_deterministic_conv(bad)
    assert dmm_net_amd.get_deterministic_conv() == "own_stem"                     # a rejected value changes nothing
    for which in ("own_all", "own", "library"):
        dmm_net_amd.set_deterministic_conv(which)
        assert dmm_net_amd.get_deterministic_conv() == which


def test_settings_take_effect_only_in_the_mode():
    for which, narrow, stem in (("own", False, False), ("own_all", True, False), ("own_stem", True, True)):
        dmm_net_amd.set_deterministic_conv(which)
        with dmm_net_amd.deterministic(False):
            assert not _own_conv_now() and not _narrow_conv_now() and not _stem_conv_now()
        with dmm_net_amd.deterministic(True):
            assert _own_conv_now() and _narrow_conv_now() == narrow and _stem_conv_now() == stem
    dmm_net_amd.set_deterministic_conv("library")
    with dmm_net_amd.deterministic(True):
        assert not _own_conv_now() and not _narrow_conv_now() and not _stem_conv_now()


def test_stem_predicate_and_route():
    stem = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
    no = [nn.Conv2d(3, 64, 7, 1, 3), nn.Conv2d(4, 64, 7, 2, 3), nn.Conv2d(3, 32, 7, 2, 3), nn.Conv2d(3, 64, 7, 2, 2),
          nn.Conv2d(3, 63, 7, 2, 3, groups=3), nn.Conv2d(3, 64, 3, 2, 1), nn.Conv2d(3, 64, 7, 2, 6, dilation=2),
          nn.Conv2d(3, 128, 7, 2, 3), nn.Conv2d(64, 64, 7, 2, 3)]
    assert _stem_ok(stem) and _stem_ok(nn.Conv2d(3, 64, 7, 2, 3, bias=True))
    assert not any(_stem_ok(m) for m in no)
    for which, route in (("library", None), ("own", None), ("own_all", None), ("own_stem", "stem")):
        dmm_net_amd.set_deterministic_conv(which)
        with dmm_net_amd.deterministic(True):
            assert _conv_route(stem) == route, which
            assert all(_conv_route(m) != "stem" for m in no)
        with dmm_net_amd.deterministic(False):
            assert _conv_route(stem) is None


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cpu_path_of_the_stem_is_untouched_by_the_setting(dtype):
    """Off the GPU ``_conv`` runs the stock convolution whatever the setting: same bits, same autograd route."""
    torch.manual_seed(4)
    m = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
    assert _stem_ok(m)
    x = torch.randn(2, 3, 17, 23).to(dtype).contiguous(memory_format=torch.channels_last)
    outs, nodes = [], []
    for which in ("library", "own", "own_all", "own_stem"):
        dmm_net_amd.set_deterministic_conv(which)
        with dmm_net_amd.deterministic(True):
            m.zero_grad(set_to_none=True)
            y = _conv(x, m, dtype)
            nodes.append(type(y.grad_fn).__name__)
            y.float().sum().backward()
            outs.append((y.detach(), m.weight.grad.clone()))
    assert len(set(nodes)) == 1 and "Stem" not in nodes[0] and "DetConv" not in nodes[0], nodes
    assert all(torch.equal(a, b) for o in outs[1:] for a, b in zip(outs[0], o))
    ref = F.conv2d(x, m.weight.to(dtype=dtype, memory_format=torch.channels_last), None, 2, 3)
    assert torch.equal(outs[0][0], ref)


def test_conv_entry_validates_its_arguments_without_gpu():
    """Every rejected call answers DMM_ERR_BAD_ARG before anything is launched; B == 0 is nothing to do."""
    L = _lib_loaded()
    OK, BAD = _lib.DMM_OK, _lib.DMM_ERR_BAD_ARG

    def st(B=2, H=17, W=23, x=ONE, w=ONE, bias=None, y=ONE):
        return L.dmm_conv7x7s2_stem_bf16(x, w, bias, B, H, W, y, None)

    for kw in (dict(B=-1), dict(H=0), dict(W=0), dict(H=-3), dict(W=-1), dict(x=None), dict(w=None), dict(y=None),
               dict(x=ctypes.c_void_p(4097)), dict(w=ctypes.c_void_p(4104)), dict(w=ctypes.c_void_p(4098)),
               dict(y=ctypes.c_void_p(4100)), dict(bias=ctypes.c_void_p(4097)), dict(B=0, H=0), dict(B=0, W=-1),
               dict(B=2 ** 31 - 1, H=2 ** 18, W=2 ** 18)):                         # more than 2^56 elements
        assert st(**kw) == BAD, kw
    assert st(B=0) == OK and st(B=0, x=None, w=None, y=None) == OK


def test_wgrad_entry_validates_its_arguments_without_gpu():
    """Bad sizes, null and misaligned pointers answer DMM_ERR_BAD_ARG, a null or short workspace DMM_ERR_WORKSPACE -- all before
    a launch, in the order of the narrow entry."""
    L = _lib_loaded()
    BAD, WS = _lib.DMM_ERR_BAD_ARG, _lib.DMM_ERR_WORKSPACE
    need = L.dmm_wgrad7x7s2_stem_workspace_bytes(2, 17, 23)
    assert need > 0

    def f32(addr):
        return ctypes.cast(ctypes.c_void_p(addr), ctypes.POINTER(ctypes.c_float))

    def st(B=2, H=17, W=23, dy=ONE, x=ONE, dw=f32(4096), ws=ONE, ws_bytes=need):
        return L.dmm_wgrad7x7s2_stem_bf16(dy, x, B, H, W, dw, ws, ws_bytes, None)

    for kw in (dict(B=-1), dict(H=0), dict(W=0), dict(dy=None), dict(x=None), dict(dw=None), dict(dw=f32(4098)),
               dict(dy=ctypes.c_void_p(4100)), dict(dy=ctypes.c_void_p(4104)), dict(x=ctypes.c_void_p(4097)),
               dict(B=0, H=0), dict(B=0, dw=None), dict(B=0, dw=f32(4097)), dict(B=2 ** 31 - 1, H=2 ** 18, W=2 ** 18),
               dict(dy=None, ws=None), dict(x=None, ws_bytes=0)):                  # (the pointers before the workspace)
        assert st(**kw) == BAD, kw
    for kw in (dict(ws=None), dict(ws=None, ws_bytes=0), dict(ws_bytes=0), dict(ws_bytes=need - 1),
               dict(ws=ctypes.c_void_p(4098), ws_bytes=need - 1)):                # (short before misaligned)
        assert st(**kw) == WS, kw
    assert st(ws=ctypes.c_void_p(4098)) == BAD                                    # (the workspace's alignment)
    assert st(x=ctypes.c_void_p(4098), ws_bytes=0) == WS                          # (x needs only 2-byte alignment)


def test_wgrad_workspace_bytes():
    L = _lib_loaded()
    ws = L.dmm_wgrad7x7s2_stem_workspace_bytes
    table = 4 * 64 * 147                                                          # one fp32 [64, 147] partial table
    for case in CASES + [(12, 255, 448), (4, 128, 224), (1, 2049, 3)]:
        n = ws(*case)
        assert n > 0 and n % 4 == 0 and n % table == 0, case
    assert ws(2, 1, 1) == table                                                   # two pixels: one slab
    assert ws(1, 80, 80) >= 2 * table and ws(12, 255, 448) >= 2 * table           # pixel slabs are folded where there are pixels enough
    assert ws(12, 255, 448) <= 16 << 20
    # a function of its arguments alone: asked again, around other calls, the answer is the same
    first = [ws(2, 17, 23), ws(12, 255, 448)]
    ws(1, 80, 80)
    assert [ws(2, 17, 23), ws(12, 255, 448)] == first
    # rejected arguments and B == 0 answer 0
    for bad in ((0, 17, 23), (-1, 17, 23), (2, 0, 23), (2, 17, 0), (2, -17, 23), (0, 0, 0)):
        assert ws(*bad) == 0, bad


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_emulation_holds_the_bounds(case):
    """fp32 accumulation, the bias in fp32 and one rounding -- the arithmetic the kernels are asked for -- stays inside both
    bounds on the host, so the bounds ask nothing the number formats do not give."""
    ry, rdw = reference(case)
    b = inputs(case)[2]
    for bias in (False, True):
        y, dw = emulate(case, bias)
        ref = ry + b.double().view(1, -1, 1, 1) if bias else ry
        ey, edw = elementwise(y, ref), dw_error(dw, rdw)
        print(f"conv7x7 stem emulation {case_id(case)} bias={bias}: y {ey:.3f} dw {edw:.3e}")
        assert ey <= 1.0 and edw <= DW_BOUND, (ey, edw)
