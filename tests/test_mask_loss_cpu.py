"""The fused mask loss without a GPU: the fp64 reference of tests/mask_loss_ref.py against a first-hand fixture of the
reference's criterion, the closed-form gradient against fp64 autograd, every status of the two entries in the order
include/dmm_match.h (13) states, and the module on CPU tensors (the stock form)."""
import ctypes

import numpy as np
import pytest
import torch

import mask_loss_ref as R
from conftest import golden
from dmm_net_amd import _lib, losses


@pytest.mark.parametrize("name", ["all", "none", "mixed"])
def test_reference_agrees_with_the_first_hand_fixture(name):
    """tests/golden/mask_loss.npz holds what the reference's softIoULoss / compute_iou_binary_mask_2D computed in fp32
    (gen_golden_mask_loss.py); the fp64 reference agrees to 1e-6 relative, the fp32 rounding of the fixture's own values."""
    z = golden("mask_loss").group(name)
    pred, target, sw = z["pred"][None], z["target"][None], z["sw"].reshape(1, -1)
    ref = R.reference(pred, target, sw, None, pred.shape[1])
    rel = lambda got, want: float(np.abs(got - want).max() / np.abs(want).max())
    assert rel(ref["loss"], z["loss"]) <= 1e-6
    assert rel(ref["cost"][0], z["cost"]) <= 1e-6
    assert rel(ref["dpred"][0], z["dpred"]) <= 1e-6
    assert rel(ref["hard"][0].astype(np.float64), z["hard"]) <= 1e-6
    assert z["pred"].shape[0] <= 6 and z["pred"].shape[1] <= 35


@pytest.mark.parametrize("weights", ["all", "none", "mixed", "one"])
def test_closed_form_gradient_equals_fp64_autograd(weights):
    pred, target, sw, _ = R.make_case(2, 5, 3, 35, weights=weights)
    n = 3
    p = torch.from_numpy(pred).double().requires_grad_(True)
    y = torch.from_numpy(target).double()
    pp, yy = p[:, :n].reshape(-1, 35), y[:, :n].reshape(-1, 35)
    cost = 1 - (pp * yy).sum(1) / ((pp + yy - pp * yy).sum(1) + 1e-6)
    sel = torch.from_numpy(R.selection(sw[:, :n]).reshape(-1))
    (cost[sel].mean() * 18.0).backward()
    got = R.closed_form_gradient(pred, target, sw, n, g=18.0)
    assert float(np.abs(got - p.grad.numpy()).max()) <= 1e-12
    assert not got[:, n:].any()


def _fwd(L, *, B=2, O=3, n_obj=2, HW=16, so=16, sb=48, dtype=0, pred=True, target=True, sw=True, cost=True, hard=True,
         scalars=True, ws=True, ws_bytes=1 << 20, sb_sw=3):
    p = lambda have: ctypes.c_void_p(8) if have else None
    return L.dmm_mask_iou_loss_fwd(p(pred), sb, so, p(target), dtype, sb, so, p(sw), sb_sw, None, B, O, n_obj, HW, p(cost),
                                   p(hard), p(scalars), p(ws), ws_bytes, None)


def _bwd(L, *, B=2, O=3, n_obj=2, HW=16, so=16, sb=48, dtype=0, target=True, d_loss=True, dpred=True, ws=True,
         ws_bytes=1 << 20, so_d=16):
    p = lambda have: ctypes.c_void_p(8) if have else None
    return L.dmm_mask_iou_loss_bwd(p(target), dtype, sb, so, p(d_loss), B, O, n_obj, HW, p(ws), ws_bytes, p(dpred), sb, so_d,
                                   None)


def test_every_status_in_the_stated_order_without_gpu():
    """Both entries answer before anything touches the device (every pointer is the address 8): bad sizes (1), nothing to do
    (0, pointers not looked at), null pointers (1), unsupported dtype (2), workspace null or short (4); where two faults
    coincide the earlier one is named."""
    L = _lib.load()
    OK, BAD, UNS, WS = _lib.DMM_OK, _lib.DMM_ERR_BAD_ARG, _lib.DMM_ERR_UNSUPPORTED, _lib.DMM_ERR_WORKSPACE
    need = L.dmm_mask_iou_loss_workspace_bytes(2, 2, 16)
    assert need >= 2 * 2 * (8 + 16) and L.dmm_mask_iou_loss_workspace_bytes(0, 2, 16) == 0
    assert L.dmm_mask_iou_loss_workspace_bytes(2, 0, 16) == 0 and L.dmm_mask_iou_loss_workspace_bytes(2, 2, 0) == 0
    C = _lib.MASK_LOSS_CHUNK
    per_chunk = L.dmm_mask_iou_loss_workspace_bytes(1, 2, C + 1) - L.dmm_mask_iou_loss_workspace_bytes(1, 2, C)
    assert per_chunk == 2 * 16                                                   # one 16-byte slot per (row, chunk)
    for f in (_fwd, _bwd):
        # 1. bad sizes, ahead of everything else
        for kw in (dict(B=-1), dict(O=-1), dict(n_obj=-1), dict(HW=-1), dict(n_obj=4), dict(so=15), dict(sb=-1)):
            assert f(L, target=False, dtype=7, ws=False, **kw) == BAD, (f.__name__, kw)
        # 2. nothing to do, before the pointers are looked at
        for kw in (dict(B=0), dict(HW=0, so=0)):
            assert f(L, target=False, dtype=7, ws=False, **kw) == OK, (f.__name__, kw)
        # 3. null pointers, ahead of dtype and workspace
        assert f(L, target=False, dtype=7, ws=False) == BAD
        # 4. unsupported, ahead of the workspace
        assert f(L, dtype=7, ws=False) == UNS and f(L, dtype=3, ws=False) == UNS
        assert f(L, B=6554, O=10, n_obj=10, sb=160, ws=False) == UNS             # more than 65535 planes
        # 5. the workspace
        assert f(L, ws=False) == WS and f(L, ws_bytes=need - 1) == WS
    assert _fwd(L, n_obj=0, pred=False, ws=False) == OK and _bwd(L, O=0, n_obj=0, dpred=False, ws=False) == OK
    assert _fwd(L, sb_sw=-1) == BAD and _bwd(L, so_d=15) == BAD
    for kw in (dict(pred=False), dict(sw=False), dict(cost=False), dict(hard=False), dict(scalars=False)):
        assert _fwd(L, dtype=7, ws=False, **kw) == BAD, kw
    for kw in (dict(d_loss=False), dict(dpred=False)):
        assert _bwd(L, dtype=7, ws=False, **kw) == BAD, kw


def test_module_on_cpu_tensors_is_the_stock_form():
    pred, target, sw, valid = R.make_case(2, 5, 3, 35, weights="mixed")
    t = torch.from_numpy
    p = t(pred).requires_grad_(True)
    got = losses.mask_step_losses(t(target), p, t(sw), t(valid), n_obj=3)
    got[0].backward()
    ref = R.reference(pred, target, sw, valid, 3)
    assert abs(float(got[0].detach()) - ref["loss"]) <= 1e-6 and np.abs(got[3].numpy() - ref["cost"]).max() <= 1e-6
    assert np.abs(p.grad.numpy() - ref["dpred"]).max() <= 1e-6 * np.abs(ref["dpred"]).max() + 1e-9
    assert np.abs(got[4].numpy() - ref["hard"]).max() <= 1e-6
    assert abs(float(got[1]) - float(ref["hard_valid"])) <= 1e-6 and abs(float(got[2]) - float(ref["hard_all"])) <= 1e-6
    # the criterion with the reference's call: the same value as the rows' selection mean, need_sigmoid must be false
    crit = losses.softIoULoss()
    y2, p2, sw2 = t(target[:, :3]).reshape(6, 35), t(pred[:, :3]).reshape(6, 35), t(sw[:, :3]).reshape(6, 1)
    assert torch.equal(crit(y2, p2, sw2, need_sigmoid=0), got[0].detach())
    with pytest.raises(AssertionError):
        crit(y2, p2, sw2)
    # no template valid: both hard figures are 0; no weight set: the mean over every row
    z = losses.mask_step_losses(t(target), t(pred), t(sw) * 0, t(valid) * 0)
    assert float(z[1]) == 0.0 and float(z[2]) == 0.0 and torch.equal(z[0], z[3].mean())
    import dmm_net_amd
    assert dmm_net_amd.softIoULoss is losses.softIoULoss and dmm_net_amd.mask_step_losses is losses.mask_step_losses
