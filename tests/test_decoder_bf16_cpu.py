"""The bf16 form of the refine decoder without a GPU (dmm_net_amd/decoder.py, include/dmm_match.h (12i)-(12k)): the
``compute_dtype`` switch, the routes it must leave alone (CPU tensors, calls that require a gradient), the bf16 weight slices
and their cache, and the three 16-bit entries' answers to calls they refuse -- the same as their fp32 siblings', before any
HIP call."""
import copy
import ctypes
import os

import pytest
import torch

from dmm_net_amd import _lib
from dmm_net_amd.decoder import RSISMask, RefineStep
from test_decoder_cpu import CASES, case_inputs, chain_inputs, flat_outputs, load_decoder, make_args
from conftest import golden

BF16 = torch.bfloat16


def test_compute_dtype_accepts_fp32_and_bf16_only():
    dec = RSISMask(make_args("concat"))
    assert dec.compute_dtype == torch.float32                        # the default: nothing changes unless asked
    dec.compute_dtype = BF16
    assert dec.compute_dtype == BF16
    for bad in (torch.float16, torch.float64, torch.int32, "bf16", None):
        with pytest.raises(ValueError, match="compute_dtype"):
            dec.compute_dtype = bad
    assert dec.compute_dtype == BF16                                 # a refused value leaves the setting alone
    dec.compute_dtype = torch.float32
    assert dec.compute_dtype == torch.float32
    # the parameters are fp32 masters whatever the setting, and a reference checkpoint still loads strictly
    dec2, g = load_decoder("concat")
    dec2.compute_dtype = BF16
    dec2.load_state_dict(copy.deepcopy(dec2.state_dict()), strict=True)
    assert all(p.dtype == torch.float32 for p in dec2.parameters())
    assert copy.deepcopy(dec2).compute_dtype == BF16


@pytest.mark.parametrize("mode", ["concat", "sum"])
def test_cpu_route_is_stock_and_bit_equal_to_the_default(mode):
    dec, g = load_decoder(mode)
    dec16 = copy.deepcopy(dec)
    dec16.compute_dtype = BF16
    with torch.no_grad():
        for case in CASES:
            args = case_inputs(g, mode, case)
            assert dec16._route(args[0] + args[1]) == "stock" and not dec16.fused_ok(args[0] + args[1])
            want, got = flat_outputs(dec(*args)), flat_outputs(dec16(*args))
            for k in want:
                assert got[k].dtype == torch.float32 and torch.equal(got[k], want[k]), (case, k)
            low = [t.to(BF16) for t in args[0]]                      # bf16 tensors on the CPU: still the stock route
            assert dec16._route(low + args[1]) == "stock"
    assert dec16.conv_calls == 0                                     # the fused form never ran


def test_refine_step_on_the_cpu_is_unchanged_by_compute_dtype():
    dec, _ = load_decoder("concat")
    dec16 = copy.deepcopy(dec)
    dec16.compute_dtype = BF16
    g = golden("g23_refine_decoder_chain")
    valid = torch.from_numpy(g["chain/valid"])
    res = []
    with torch.no_grad():
        for d in (dec, dec16):
            step, state, outs_all = RefineStep(d), None, []
            for t in range(2):
                feats, prev_mask, y_mask, init_pred, hist, H, W = chain_inputs(g, t)
                outs, hist_new, state = step(feats, prev_mask, y_mask, init_pred, hist, valid, state)
                outs_all += [outs, hist_new] + [h for hs in state.thid for h in hs]
            res.append(outs_all)
    assert len(res[0]) == len(res[1])
    for a, b in zip(*res):
        assert a.dtype == b.dtype == torch.float32 and torch.equal(a, b)


def test_route_with_a_gradient_ignores_compute_dtype():
    """A call that requires a gradient goes where it goes today: 'stock' by default, and 'stock' on the CPU with
    ``fused_train`` as well -- whatever ``compute_dtype`` says; the results are the default's, bit for bit."""
    dec, g = load_decoder("concat")
    dec16 = copy.deepcopy(dec)
    dec16.compute_dtype = BF16
    feats, masks, spatial, temporal = case_inputs(g, "concat", "st")
    for fused_train in (False, True):
        dec.fused_train = dec16.fused_train = fused_train
        x = [f.clone().requires_grad_(True) for f in feats]
        assert dec16._route(x + masks) == dec._route(x + masks) == "stock"
        assert dec16._route(feats + masks) == dec._route(feats + masks) == "stock"      # (the parameters require one)
        a, b = dec(x, masks, spatial, temporal), dec16(x, masks, spatial, temporal)
        assert torch.equal(a[0], b[0]) and a[0].requires_grad and b[0].requires_grad


SLICE_KEYS = ("skip", "up", "hs", "ht", "cat", "bias")


@pytest.mark.parametrize("mode", ["concat", "sum", "mul", "none"])
def test_bf16_weight_slices_are_the_fp32_cut_cast_once(mode):
    torch.manual_seed(3)
    dec = RSISMask(make_args(mode, hidden=16)).eval()
    full = dec.weight_slices()
    full_head = dec.head_weights()
    assert dec.weight_slices() is full and dec.head_weights() is full_head
    dec.compute_dtype = BF16
    low = dec.weight_slices()
    assert low is not full and len(low) == len(full) == 4
    for d16, d32 in zip(low, full):
        assert sorted(d16) == sorted(d32)
        for k in SLICE_KEYS:
            if d32[k] is None:
                assert d16[k] is None, k
            else:
                assert d16[k].dtype == BF16 and d16[k].shape == d32[k].shape and torch.equal(d16[k], d32[k].to(BF16)), k
        assert d16["m"].dtype == torch.float32 and torch.equal(d16["m"], d32["m"])       # the stencil stays fp32
    head = dec.head_weights()
    assert all(t.dtype == BF16 for t in head)
    assert torch.equal(head[0], dec.conv_out.weight.detach().to(BF16)) and torch.equal(head[1], dec.conv_out.bias.detach().to(BF16))
    # the identical objects on a second call
    again = dec.weight_slices()
    assert again is low and all(a[k] is b[k] for a, b in zip(again, low) for k in a) and dec.head_weights() is head
    # new ones after a parameter update ...
    with torch.no_grad():
        dec.clstm_list[1].Gates.weight.mul_(1.5)
    upd = dec.weight_slices()
    assert upd is not low and upd[1]["hs"] is not low[1]["hs"]
    cin, Hd = dec.clstm_list[1].input_size, dec.clstm_list[1].hidden_size
    assert torch.equal(upd[1]["hs"], dec.clstm_list[1].Gates.weight.detach()[:, cin + 1:cin + 1 + Hd].to(BF16))
    assert not torch.equal(upd[1]["hs"], low[1]["hs"])
    # ... and after a dtype switch, each way, each time the right set
    dec.compute_dtype = torch.float32
    back = dec.weight_slices()
    assert back is not upd and all(d[k] is None or d[k].dtype == torch.float32 for d in back for k in d)
    assert all(t.dtype == torch.float32 for t in dec.head_weights())
    dec.compute_dtype = BF16
    low2 = dec.weight_slices()
    assert low2 is not back and low2 is not upd
    for d16, d32 in zip(low2, back):
        for k in SLICE_KEYS:
            assert (d16[k] is None and d32[k] is None) or torch.equal(d16[k], d32[k].to(BF16)), k
        assert d16["m"].dtype == torch.float32


def test_launchers_refuse_cpu_tensors_before_any_call():
    """Nothing falls back: the 16-bit launchers need device tensors like the fp32 ones."""
    from dmm_net_amd import decoder as D
    x = torch.zeros(1, 2, 3, 4, dtype=BF16)
    with pytest.raises(_lib.DmmError, match="MI355X"):
        D.upsample_bilinear_into(x, torch.zeros(1, 2, 6, 8, dtype=BF16))
    with pytest.raises(_lib.DmmError, match="MI355X"):
        D.refine_finish(x, None, torch.zeros(1, 2, 6, 8), None, 2)
    with pytest.raises(_lib.DmmError, match="MI355X"):
        D.clstm_gates([torch.zeros(1, 8, 3, 4, dtype=BF16)], torch.zeros(1, 3, 3, 4), torch.zeros(8, 9), None,
                      torch.zeros(1, 2, 3, 4, dtype=BF16), torch.zeros(1, 2, 3, 4))
    with pytest.raises(_lib.DmmError, match="bfloat16 skip maps"):
        RSISMask._check_bf16_operands([torch.zeros(1)], [torch.zeros(1)])
    RSISMask._check_bf16_operands([torch.zeros(1, dtype=BF16)], [torch.zeros(1)])


# ---- the entries' answers before any HIP call ---------------------------------------------------------------------------------
def _lib_loaded():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _p(have=True):
    return ctypes.c_void_p(8) if have else None


def _gates(L, sfx, *, pre0=True, pre1=True, pre2=True, masks=True, wm=True, cp=True, hidden=True, cell=True, copy_=True, B=2,
           Hd=6, h=5, w=7, sb=None, sb_m=None, sb_c=None):
    hw = h * w
    sb = 4 * Hd * hw if sb is None else sb
    return getattr(L, "dmm_clstm_gates_" + sfx)(_p(pre0), _p(pre1), _p(pre2), sb, sb, sb, _p(masks), 3 * hw if sb_m is None else sb_m,
                                                _p(wm), _p(cp), B, Hd, h, w, _p(hidden), _p(cell), _p(copy_),
                                                Hd * hw if sb_c is None else sb_c, None)


def _upsample(L, sfx, *, src=True, dst=True, B=2, C=3, h=1, w=4, Cd=8, c0=2, H=7, W=9, mode=0, sb_s=None, sb_d=None):
    return getattr(L, "dmm_upsample_bilinear_into_" + sfx)(_p(src), C * h * w if sb_s is None else sb_s, B, C, h, w, _p(dst),
                                                           Cd * H * W if sb_d is None else sb_d, Cd, c0, H, W, mode, None)


def _finish(L, sfx, *, logits=True, valid=True, outs=True, hist=True, B=1, O=2, n_obj=2, h=2, w=2, H=5, W=7, sb=4, so=4):
    return getattr(L, "dmm_refine_finish_" + sfx)(_p(logits), sb, so, h, w, _p(valid), B, O, n_obj, H, W, _p(outs), _p(hist), None)


GATES_ROWS = [dict(pre0=False), dict(masks=False), dict(wm=False), dict(hidden=False), dict(cell=False), dict(B=-1), dict(Hd=0),
              dict(Hd=-4), dict(h=0), dict(w=-1), dict(sb=-1), dict(sb_m=3 * 35 - 1), dict(sb_c=6 * 35 - 1), dict(B=0),
              dict(B=0, pre0=False, hidden=False), dict(B=0, Hd=0), dict(B=-1, pre0=False), dict(Hd=4 * 65536, pre0=False),
              dict(Hd=4 * 65535 + 1), dict(B=1 << 20, h=1 << 12, w=1 << 12), dict(B=1 << 20, h=1 << 12, w=1 << 12, cell=False)]
UPSAMPLE_ROWS = [dict(src=False), dict(dst=False), dict(B=-1), dict(C=0), dict(h=0), dict(w=-2), dict(H=0), dict(W=-1), dict(Cd=0),
                 dict(c0=-1), dict(c0=6), dict(c0=5, C=4), dict(mode=-1), dict(mode=3), dict(sb_s=11), dict(sb_d=8 * 63 - 1),
                 dict(B=0), dict(B=0, src=False, dst=False), dict(B=0, mode=3), dict(B=0, c0=6), dict(src=False, mode=3),
                 dict(B=1 << 30, H=1 << 15, W=1 << 15, sb_d=1 << 40), dict(B=1 << 30, H=1 << 15, W=1 << 15, sb_d=1 << 40, src=False)]
FINISH_ROWS = [dict(logits=False), dict(outs=False), dict(valid=False), dict(valid=False, outs=False), dict(B=-1), dict(O=-1),
               dict(n_obj=-1), dict(n_obj=3), dict(h=0), dict(w=0), dict(H=0), dict(W=-3), dict(sb=-1), dict(so=-4), dict(B=0),
               dict(O=0, n_obj=0), dict(O=0, n_obj=1), dict(B=0, outs=False), dict(n_obj=0, logits=False, outs=False), dict(B=0, n_obj=3),
               dict(B=1 << 30, H=1 << 15, W=1 << 15), dict(B=1 << 30, H=1 << 15, W=1 << 15, outs=False)]
NOT_LAUNCHED = (_lib.DMM_ERR_BAD_ARG, _lib.DMM_ERR_UNSUPPORTED)


@pytest.mark.parametrize("fn,rows", [(_gates, GATES_ROWS), (_upsample, UPSAMPLE_ROWS), (_finish, FINISH_ROWS)],
                         ids=["gates", "upsample", "finish"])
def test_bf16_entries_answer_as_their_fp32_siblings_without_gpu(fn, rows):
    """Null needed pointer, negative / zero size, n_obj > O, channel range outside dst, bad mode, short strides, nothing to do,
    a grid beyond the launch limits: every row is answered before a launch (the pointers are the address 8, not memory), and
    the bf16 entry's answer is the fp32 entry's."""
    L = _lib_loaded()
    seen = set()
    for kw in rows:
        a, b = fn(L, "f32", **kw), fn(L, "bf16", **kw)
        nothing_to_do = kw.get("B") == 0 or kw.get("O") == 0
        assert a in NOT_LAUNCHED or (a == _lib.DMM_OK and nothing_to_do), (kw, a)
        assert b == a, (kw, a, b)
        seen.add(a)
    assert seen == {_lib.DMM_OK, _lib.DMM_ERR_BAD_ARG, _lib.DMM_ERR_UNSUPPORTED}
    assert _finish(L, "bf16", n_obj=3) == _lib.DMM_ERR_BAD_ARG and _upsample(L, "bf16", c0=6) == _lib.DMM_ERR_BAD_ARG
    assert _upsample(L, "bf16", mode=3) == _lib.DMM_ERR_BAD_ARG and _gates(L, "bf16", pre0=False) == _lib.DMM_ERR_BAD_ARG


def test_bf16_entries_are_bound_with_void_pointers():
    L = _lib_loaded()
    for name in ("dmm_clstm_gates_bf16", "dmm_upsample_bilinear_into_bf16", "dmm_refine_finish_bf16"):
        assert name in _lib.SYMBOLS and getattr(L, name).restype is ctypes.c_int
        twin = getattr(L, name.replace("_bf16", "_f32"))
        assert getattr(L, name).argtypes == twin.argtypes, name
