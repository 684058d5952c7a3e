"""Training the refine decoder on its fused form, the parts that need no GPU: the closed-form backward of the cell
(tests/decoder_bwd_ref.py, what ``dmm_clstm_gates_bwd_f32`` implements) against fp64 autograd of the cell's forward, the
entry's answers to calls it refuses before anything touches the device, and ``fused_train`` on CPU tensors (stock form)."""
import copy
import ctypes

import pytest
import torch

from decoder_bwd_ref import gates_bwd_closed_form
from dmm_net_amd import _lib
from dmm_net_amd.decoder import RSISMask, pyramid_sizes
from test_decoder_cpu import CASES, flat_outputs, make_args
from test_gpu_decoder import gates_torch


@pytest.mark.parametrize("B,Hd,h,w", [(2, 6, 5, 7), (1, 1, 1, 1)])
@pytest.mark.parametrize("n_pre,with_cell", [(3, True), (1, False), (2, True)])
@pytest.mark.parametrize("ups", ["hc", "h", "c"])
def test_closed_form_equals_fp64_autograd(B, Hd, h, w, n_pre, with_cell, ups):
    """Both sides are fp64 evaluations of the same derivative, gradients are O(1): 1e-12 leaves four digits of room above
    the roundings of the ~4 * Hd * 9 * B * h * w term sums and catches any wrong gate, plane, tap or sign (>= 1e-3)."""
    g = torch.Generator().manual_seed(100 * B + Hd)
    R = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    pre = [R(B, 4 * Hd, h, w).requires_grad_(True) for _ in range(n_pre)]
    masks = torch.rand(B, 3, h, w, generator=g, dtype=torch.float64).requires_grad_(True)
    w_mask = (R(4 * Hd, 9) * 0.3).requires_grad_(True)
    cell_prev = R(B, Hd, h, w).requires_grad_(True) if with_cell else None
    d_hidden = R(B, Hd, h, w) if "h" in ups else None
    d_cell = R(B, Hd, h, w) if "c" in ups else None
    hidden, cell = gates_torch(pre, masks, w_mask, cell_prev)
    outs, ups_ = [], []
    if d_hidden is not None:
        outs.append(hidden), ups_.append(d_hidden)
    if d_cell is not None:
        outs.append(cell), ups_.append(d_cell)
    leaves = pre + [masks, w_mask] + ([cell_prev] if with_cell else [])
    want = torch.autograd.grad(outs, leaves, ups_)
    with torch.no_grad():
        d_pre, d_cell_prev, d_masks, d_w = gates_bwd_closed_form(pre, masks, w_mask, cell_prev, d_hidden, d_cell)
    got = [d_pre] * n_pre + [d_masks, d_w] + ([d_cell_prev] if with_cell else [])
    assert (d_cell_prev is None) == (not with_cell)
    for a, b in zip(got, want):
        assert a.shape == b.shape and float((a - b).abs().max()) < 1e-12


def _status(L, *, B=2, Hd=6, h=5, w=7, pre0=True, sb=(840, 840, 840), masks=True, sb_masks=105, w_mask=True, cell_prev=True,
            d_hidden=True, d_cell=True, d_pre=True, d_cell_prev=True, d_masks=True, d_w_mask=True, ws=True, ws_bytes=1 << 30):
    """The entry's status for a call that must be answered before the device is touched (every pointer is the address 8)."""
    p = lambda have: ctypes.c_void_p(8) if have else None
    return L.dmm_clstm_gates_bwd_f32(p(pre0), None, None, *sb, p(masks), sb_masks, p(w_mask), p(cell_prev), B, Hd, h, w,
                                     p(d_hidden), p(d_cell), p(d_pre), p(d_cell_prev), p(d_masks), p(d_w_mask), p(ws), ws_bytes,
                                     None)


def test_gates_bwd_entry_validates_its_arguments_without_gpu():
    L = _lib.load()
    OK, BAD, UNSUPPORTED, WORKSPACE = _lib.DMM_OK, _lib.DMM_ERR_BAD_ARG, _lib.DMM_ERR_UNSUPPORTED, _lib.DMM_ERR_WORKSPACE
    st = lambda **kw: _status(L, **kw)
    for kw in (dict(B=-1), dict(Hd=0), dict(Hd=-4), dict(h=0), dict(w=-1), dict(pre0=False), dict(masks=False),
               dict(w_mask=False), dict(d_pre=False), dict(d_hidden=False, d_cell=False), dict(cell_prev=False),
               dict(sb=(-1, 0, 0)), dict(sb=(840, -1, 0)), dict(sb=(840, 0, -1)), dict(sb_masks=104), dict(ws=False),
               dict(ws=False, d_masks=False), dict(ws=False, d_w_mask=False)):
        assert st(**kw) == BAD, kw
    none = dict(pre0=False, masks=False, w_mask=False, d_hidden=False, d_cell=False, d_pre=False, ws=False)
    assert st(B=0) == OK and st(B=0, **none) == OK                       # nothing to do, whatever the pointers
    assert st(B=0, h=0) == BAD                                           # sizes before "nothing to do"
    assert st(B=1 << 16, h=1 << 8, w=1 << 8, sb_masks=3 << 16) == UNSUPPORTED       # B * h * w beyond 2^31 - 1
    assert st(Hd=4 * 65535 + 1) == UNSUPPORTED                                      # more than 65535 channel groups
    need = L.dmm_clstm_gates_bwd_workspace_bytes(2, 6, 5, 7)
    # 2 channel groups x B x 27 taps x h * w  +  1 position block x 36 * Hd, fp32
    assert need == 4 * (2 * 2 * 27 * 35 + 1 * 36 * 6)
    assert st(ws_bytes=need - 4) == WORKSPACE and st(ws_bytes=0) == WORKSPACE
    assert st(B=1 << 16, h=1 << 8, w=1 << 8, sb_masks=3 << 16, ws_bytes=0) == UNSUPPORTED      # the grid before the workspace
    assert st(pre0=False, ws_bytes=0) == BAD and st(sb_masks=104, ws_bytes=0) == BAD           # arguments before both
    size = L.dmm_clstm_gates_bwd_workspace_bytes
    assert size(4, 16, 64, 112) == 4 * (4 * 4 * 27 * 7168 + 112 * 36 * 16)
    assert size(0, 6, 5, 7) == 0 and size(2, 0, 5, 7) == 0 and size(2, 6, -1, 7) == 0 and size(1 << 16, 6, 1 << 8, 1 << 8) == 0
    assert _lib.SYMBOLS.count("dmm_clstm_gates_bwd_f32") == 1 and L.dmm_clstm_gates_bwd_workspace_bytes.restype is ctypes.c_size_t


def test_weight_slices_give_the_gradient_of_plain_slicing():
    """``_WeightSlices``: contiguous slices whose backward is one ``cat``; an unused slice, an empty slice and a slice used
    twice give bit for bit what differentiable ``weight[:, a:b]`` slices give."""
    from dmm_net_amd.decoder import _WeightSlices
    bounds = (0, 3, 3, 4, 9, 14)
    res = []
    for own in (True, False):
        torch.manual_seed(4)
        wt = torch.randn(8, 14, 3, 3).requires_grad_(True)
        parts = _WeightSlices.apply(wt, bounds) if own else [wt[:, a:b] for a, b in zip(bounds[:-1], bounds[1:])]
        assert all(p.shape[1] == b - a for p, a, b in zip(parts, bounds[:-1], bounds[1:]))
        assert not own or all(p.is_contiguous() for p in parts)
        loss = (parts[0] * torch.randn(8, 3, 3, 3)).sum() + (parts[0] * parts[2]).sum() + (parts[4] ** 2).sum()   # 3 unused, 1 empty
        res.append((torch.autograd.grad(loss, wt)[0], [p.detach() for p in parts]))
    assert torch.equal(res[0][0], res[1][0]) and float(res[0][0][:, 4:9].abs().max()) == 0.0
    assert all(torch.equal(a, b) for a, b in zip(res[0][1], res[1][1]))


def _inputs(mode, seed=3, B=2, hidden=16, H=61, W=45):
    torch.manual_seed(seed)
    dec = RSISMask(make_args(mode, hidden=hidden)).eval()
    sizes = pyramid_sizes(H, W)
    ch = [hidden, hidden, hidden // 2, hidden // 4]
    feats = [torch.randn((B, c) + s) for c, s in zip(ch, sizes)]
    masks = [torch.rand((B, 3) + s) for s in sizes]
    spatial = [[torch.randn((B, d) + s) for _ in range(2)] for d, s in zip(dec.skip_dims_out, sizes)]
    temporal = [torch.randn((B, d) + s) for d, s in zip(dec.skip_dims_out, sizes)]
    return dec, feats, masks, spatial, temporal


@pytest.mark.parametrize("case", list(CASES))
def test_fused_train_on_cpu_tensors_is_the_stock_form(case):
    """``fused_train`` is an opt-in for HIP tensors: on the CPU the call is the stock form, bit for bit, with or without it."""
    dec, feats, masks, spatial, temporal = _inputs("concat")
    assert dec.fused_train is False
    sp, tm = CASES[case]
    res = []
    for flag in (False, True):
        d = copy.deepcopy(dec)
        d.fused_train = flag
        leaves = [t.clone().requires_grad_(True) for t in feats + masks]
        n0 = d.conv_calls
        out = flat_outputs(d(leaves[:4], leaves[4:], spatial if sp else None, temporal if tm else None))
        assert d.conv_calls == n0 and not d.fused_ok(leaves)              # neither fused form ran
        torch.manual_seed(9)
        loss = sum((v * torch.randn_like(v)).sum() for v in out.values())
        grads = torch.autograd.grad(loss, leaves + list(d.parameters()))
        res.append((out, grads))
    for k in res[0][0]:
        assert torch.equal(res[0][0][k], res[1][0][k]), k
    for a, b in zip(res[0][1], res[1][1]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("mode", ["concat", "sum", "mul", "none"])
def test_the_two_cuts_of_the_slice_layout_agree(mode):
    """``weight_slices()`` (no grad, memoised, ``cat`` made with it) and ``train_slices()`` (one autograd node per level, ``cat``
    on first use) are one layout: same keys, same None entries, equal tensors; the hoisted convolutions take either."""
    from dmm_net_amd.decoder import _chain_weight
    dec, feats, _, _, temporal = _inputs(mode)
    ws, ts = dec.weight_slices(), dec.train_slices()
    assert len(ws) == len(ts) == 4 and dec.weight_slices() is ws                        # the memo holds while nothing changes
    for i, (w, t) in enumerate(zip(ws, ts)):
        assert list(w) == list(t) and sorted(w) == ["bias", "cat", "hs", "ht", "m", "skip", "up"]
        assert (w["cat"] is None) == (i == 0) and t["cat"] is None                      # the training form's: not made yet
        if i > 0:
            want = torch.cat([t["up"], t["hs"]], 1)
            assert torch.equal(w["cat"], want) and w["cat"].is_contiguous()
            c = _chain_weight(t)
            assert c is t["cat"] and _chain_weight(t) is c and torch.equal(c, want)     # made once, kept with the slices
        assert (w["up"] is None) == (i == 0) and (w["skip"] is None) == (i > 0 and mode in ("mul", "none"))
        assert (mode == "sum" and i > 0) == (w["skip"] is w["up"] and w["up"] is not None)
        for k in w:
            assert (w[k] is None) == (t[k] is None), (i, k)
            if w[k] is not None:
                assert torch.equal(w[k], t[k]) and w[k].is_contiguous() and t[k].is_contiguous(), (i, k)
                assert not w[k].requires_grad and t[k].requires_grad, (i, k)            # only the training slices
    for name, terms, arg in (("skip", dec.skip_terms, feats), ("temporal", dec.temporal_terms, temporal)):
        n0 = dec.conv_calls
        plain, train = terms(arg), terms(arg, slices=ts)
        assert dec.conv_calls - n0 == 2 * sum(p is not None for p in plain)
        for a, b in zip(plain, train):
            assert (a is None) == (b is None), name
            if a is not None:
                assert torch.equal(a, b) and a.grad_fn is None and b.grad_fn is not None, name
    assert [p is None for p in dec.skip_terms(feats)] == [False] + [mode in ("mul", "none")] * 3
    # the memo's key follows an in-place update of a parameter
    with torch.no_grad():
        dec.clstm_list[2].Gates.weight.mul_(0.5)
    again = dec.weight_slices()
    assert again is not ws and torch.equal(again[2]["hs"], ws[2]["hs"] * 0.5) and torch.equal(again[1]["hs"], ws[1]["hs"])
    assert torch.equal(again[2]["cat"], torch.cat([again[2]["up"], again[2]["hs"]], 1))
    for w, t in zip(again, dec.train_slices()):
        assert all(torch.equal(w[k], t[k]) for k in w if k != "cat" and w[k] is not None)
