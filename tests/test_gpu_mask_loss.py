"""The fused mask loss on the GPU (csrc/dmm_loss.hip, include/dmm_match.h (13)) against tests/mask_loss_ref.py.

The hard IoU figures are integer counts put through one fp32 formula with one addition order: BIT FOR BIT.  cost, loss and
dpred are held through fp64 by the decoder's rule: with e_stock = the stock fp32 form's own error against
the fp64 evaluation of the same inputs, on the same device, the kernels may be off by 2 * e_stock + 1 ulp of the largest
output.  Every achieved pair is recorded (conftest.record_achieved)."""
import numpy as np
import pytest
import torch

import mask_loss_ref as R
from conftest import record_achieved
from dmm_net_amd import _lib, losses, ops
from dmm_net_amd.graphs import SafeGraph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = _lib.MASK_LOSS_CHUNK
G = 18.0                                          # the trainer's loss_weight_iouraw: the upstream gradient of the loss


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def run(fn, y, p, sw, valid, n_obj):
    """(loss, hard_valid, hard_all, cost, hard, dpred) of ``fn`` = losses.mask_step_losses or its stock form, as numpy."""
    p = p.detach().requires_grad_(True)
    out = fn(y, p, sw, valid, n_obj)
    (out[0] * G).backward()
    return tuple(o.detach().cpu().numpy() for o in out) + (p.grad.detach().cpu().numpy(),)


def held(name, got, stock, ref64):
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    e_stock = float(np.abs(stock.astype(np.float64) - ref64).max())
    b = R.bound(e_stock, np.abs(ref64).max())
    print(f"{name}: err {err:.3e}  e_stock {e_stock:.3e}  bound {b:.3e}")
    record_achieved(f"mask_loss/{name}/err", err)
    record_achieved(f"mask_loss/{name}/e_stock", e_stock)
    assert err <= b, (name, err, e_stock, b)


def check(name, y, p, sw, valid, n_obj, pred_np, target_np, sw_np, valid_np):
    """One fused call held against the reference and the stock form; ``target_np`` holds the VALUES the kernels read."""
    got = run(losses.mask_step_losses, y, p, sw, valid, n_obj)
    stock = run(losses.mask_step_losses_stock, y.float(), p, sw, valid, n_obj)
    B, K = pred_np.shape[:2]
    HW = int(np.prod(pred_np.shape[2:]))
    ref = R.reference(pred_np.reshape(B, K, HW), target_np.reshape(B, -1, HW), sw_np, valid_np, n_obj, g=G)
    bits = lambda a: np.asarray(a, np.float32).view(np.uint32)
    assert np.array_equal(bits(got[4]), bits(ref["hard"])), name
    assert bits(got[1]) == bits(ref["hard_valid"]) and bits(got[2]) == bits(ref["hard_all"]), (name, got[1:3], ref["hard_valid"], ref["hard_all"])
    held(name + "/cost", got[3], stock[3], ref["cost"])
    dp, dp_stock = got[5].reshape(B, K, HW), stock[5].reshape(B, K, HW)
    if np.isfinite(ref["loss"]):
        held(name + "/loss", got[0], stock[0], np.float64(ref["loss"]))
    else:                                            # K == 0: the reference's mean of an empty selection
        assert np.isnan(got[0]) and np.isnan(stock[0]), name
    held(name + "/dpred", dp, dp_stock, ref["dpred"].reshape(B, K, HW))
    assert not dp[:, n_obj:].any(), name             # the planes that are not compared: exactly zero
    assert not dp[:, :n_obj][~ref["sel"]].any(), name  # rows that are not selected: exactly zero
    return got


CASES = [(hw, bon) for hw in R.HW_OF(CHUNK) for bon in R.BON]


@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"HW{hw}-B{b}O{o}n{n}" for hw, (b, o, n) in CASES])
def test_every_shape_against_the_reference(i):
    HW, (B, O, n) = CASES[i]
    w, v = R.WEIGHTS[i % 4], R.VALIDS[(i // 4) % 2]
    pred, target, sw, valid = R.make_case(B, O, n, HW, weights=w, valids=v, seed=i)
    check(f"HW{HW}_B{B}O{O}n{n}_{w}_{v}", dev(target), dev(pred), dev(sw), dev(valid), n, pred, target, sw, valid)


@pytest.mark.parametrize("w", R.WEIGHTS + ("frac",))
@pytest.mark.parametrize("v", R.VALIDS)
def test_weight_and_valid_patterns(w, v):
    """All set, none set, mixed, exactly one set, and weights in (0, 1) only (they truncate to "not selected": K = 0, the loss
    is the NaN of the reference's empty mean and the gradient is zero); valid flags mixed and all zero."""
    B, O, n, HW = 2, 5, 3, CHUNK + 1
    pred, target, sw, valid = R.make_case(B, O, n, HW, weights=w, valids=v, seed=77)
    got = check(f"patterns_{w}_{v}", dev(target), dev(pred), dev(sw), dev(valid), n, pred, target, sw, valid)
    if v == "zero":
        assert got[1] == 0.0 and got[2] == 0.0
    if w == "frac":
        assert not got[5].any()


@pytest.mark.parametrize("layout", ["dense", "target_slice", "plane_stride", "f16", "bf16"])
def test_layouts_at_a_multi_chunk_shape(layout):
    """Tensors that pass ``ops._plane_rows`` go in as they are: the target as a batch-strided slice, ``alloc_planes``
    strides (planes 7 x 1171 = 2 * CHUNK + 5 pixels: odd, only 4-byte-aligned rows), 16-bit targets."""
    B, O, n, H, W = 2, 5, 2, 7, (2 * CHUNK + 5) // 7
    HW = H * W
    assert HW == 2 * CHUNK + 5
    pred, target, sw, valid = R.make_case(B, O, n, HW, weights="mixed", seed=5)
    p, y = dev(pred), dev(target)
    if layout == "target_slice":
        big = torch.full((B, O + 3, HW), 0.7, device=DEV)
        big[:, :O] = y
        y = big[:, :O]
        assert not y.is_contiguous() and ops._loss_planes(y)[0].data_ptr() == y.data_ptr()
    elif layout == "plane_stride":
        ya, pa = ops.alloc_planes(B, O, H, W, torch.float32, DEV, fill=0.7), ops.alloc_planes(B, O, H, W, torch.float32, DEV, fill=0.7)
        ya.copy_(y.view(B, O, H, W))
        pa.copy_(p.view(B, O, H, W))
        y, p = ya, pa
        assert y.stride(1) > HW and ops._loss_planes(y)[0].data_ptr() == y.data_ptr()
    elif layout in ("f16", "bf16"):
        y = y.to(torch.float16 if layout == "f16" else torch.bfloat16)
        assert torch.equal(y.float(), dev(target))                     # the case's target values are exact in 16 bits
    check(f"layout_{layout}", y, p, dev(sw), dev(valid), n, pred, target, sw, valid)


def test_two_runs_and_a_graph_replay_are_bit_identical():
    """No float atomics: the same bits run after run; forward and backward capture into ONE graph (nothing reads the host)."""
    B, O, n, HW = 4, 5, 5, 2 * CHUNK + 5
    pred, target, sw, valid = R.make_case(B, O, n, HW, weights="mixed", seed=9)
    y, p, s, v = dev(target), dev(pred).requires_grad_(True), dev(sw), dev(valid)

    def step():
        out = losses.mask_step_losses(y, p, s, v, n)
        (dp,) = torch.autograd.grad(out[0] * G, p)
        return [o.detach() for o in out] + [dp]

    first, second = step(), step()
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    torch.cuda.synchronize()
    g = SafeGraph()
    with g.capture():
        held_out = step()
    for t in held_out:
        t.zero_()
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(first, held_out):
        assert torch.equal(a, b)


def test_launch_counts_and_module():
    """Forward 2 launches, backward 1; the criterion with the reference's call gives the same loss as the step function."""
    B, O, n, HW = 2, 3, 3, CHUNK + 1
    pred, target, sw, valid = R.make_case(B, O, n, HW, weights="mixed", seed=3)
    y, p, s, v = dev(target), dev(pred).requires_grad_(True), dev(sw), dev(valid)
    L = _lib.load()
    losses.mask_step_losses(y, p, s, v)[0].backward()                  # warm: sizes asked, workspace cached
    c0 = L.dmm_launch_count()
    out = losses.mask_step_losses(y, p, s, v)
    c1 = L.dmm_launch_count()
    out[0].backward()
    c2 = L.dmm_launch_count()
    assert (c1 - c0, c2 - c1) == (2, 1)
    with torch.no_grad():
        c0 = L.dmm_launch_count()
        quiet = losses.mask_step_losses(y, p, s, v)
        assert L.dmm_launch_count() - c0 == 2 and torch.equal(quiet[0], out[0].detach())
    crit = losses.softIoULoss()
    p2 = p.detach().view(B * O, HW).requires_grad_(True)
    loss = crit(y.view(B * O, HW), p2, s.view(-1, 1), need_sigmoid=0)
    loss.backward()
    assert torch.equal(loss.detach(), out[0].detach()) and torch.equal(p2.grad.view_as(p), p.grad / 2)
    with pytest.raises(AssertionError):
        crit(y.view(B * O, HW), p2, s.view(-1, 1))


def test_feature_gradients_through_matchmodel_equal_the_stock_loss():
    """MatchModel in train mode with targets at G2's shape (8 proposals x 3 templates, 64 x 64): the features' gradients of
    the frame step with ``mask_step_losses`` against the same step with the stock loss, within 1e-5 of the largest entry --
    DESIGN's figure for two runs of the mix backward's float atomics."""
    from dmm_net_amd import synth
    from dmm_net_amd.match_model import MatchModel
    fr = synth.make_config_frame(1, kind="structured", with_targets=True)
    cfgs = {"matching": {"algo": "relax"}, "relax_max_iter": 10, "relax_proj_iter": 5, "relax_learning_rate": 0.1,
            "score_weight": 0.3}
    model = MatchModel(cfgs, is_test=0)
    O, H, W = fr.targets.shape
    y = dev(fr.targets).view(1, O, H * W)
    sw = torch.ones((1, O), device=DEV)
    valid = torch.ones((1, O), dtype=torch.int32, device=DEV)
    grads = {}
    for name, fn in (("fused", losses.mask_step_losses), ("stock", losses.mask_step_losses_stock)):
        pf, tf = dev(fr.proposed_feature).requires_grad_(True), dev(fr.template_feature).requires_grad_(True)
        fo, _ms, _ds, _, loss = model(pf, dev(fr.proposed_mask), [tf], dev(fr.mask_last_occurence), dev(fr.proposal_score),
                                      dev(fr.targets))
        out = fn(y, fo.unsqueeze(0), sw, valid)
        (out[0] * G + loss["cost_loss"]).backward()
        grads[name] = (pf.grad.clone(), tf.grad.clone(), out)
    for k, which in enumerate(("proposed_feature", "template_feature")):
        a, b = grads["fused"][k], grads["stock"][k]
        largest = float(b.abs().max())
        err = float((a - b).abs().max())
        print(f"{which}: err {err:.3e} of largest {largest:.3e}")
        record_achieved(f"mask_loss/matchmodel/{which}/rel_err", err / largest)
        assert largest > 0 and err <= 1e-5 * largest, (which, err, largest)
    assert abs(float(grads["fused"][2][1]) - float(grads["stock"][2][1])) <= 1e-6
