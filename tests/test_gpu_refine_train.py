"""The refine step of training on the GPU: the kernels (12f)-(12h) of include/dmm_match.h against torch autograd of the ops
they replace, their repeatability, batch independence and guard bands, and ``RefineTrainStep`` against the fp64 evaluation
of its stock route.

Tolerances: the rule of tests/test_gpu_decoder.py (``held``): err <= 2 * max(e_stock, floor) + 1 ulp of max|ref|, both errors
against the fp64 evaluation on the same device.  The pyramid's backward with a gradient on one level is a pure scatter: bit
exact.  For the step, e_stock is the larger of the stock route's own fp32 error and the fp32 error of the trainer's loop
(tests/refine_train_ref.py) on the decoder's ``fused_train`` form with torch ops around it -- the same reordered algebra as
the step, with none of the step's code or of the new kernels in it.  Every pair is recorded."""
import copy

import pytest
import torch
import torch.nn.functional as F

import dmm_net_amd
import refine_train_ref as R
from dmm_net_amd import _lib, decoder as D
from dmm_net_amd.decoder import RSISMask, RefineTrainStep
from guarded import banded, guarded
from test_decoder_cpu import make_args
from test_gpu_decoder import DEV, held
from test_gpu_decoder_train import held_all
from test_refine_train_cpu import clip, loop_call, run_clip, step_call

pytestmark = pytest.mark.gpu


# ---- (12f) the pyramid's backward ------------------------------------------------------------------------------------------
def pyramid_case(H, W, kind, B=2, O=4, seed=1):
    """Planes as tests/test_gpu_decoder.py builds them: ``prev_mask`` strided, its planes only 4-byte aligned."""
    torch.manual_seed(seed)
    draw = (lambda *s: torch.rand(*s, device=DEV)) if kind == "random" else \
        (lambda *s: torch.randint(0, 3, s, device=DEV).float() / 2)
    big = draw(B, O + 1, H * W + 3)
    prev_mask = big[:, 1:, 3:]
    return prev_mask, draw(B, O, H * W), draw(B, O, H, W)


def pyramid_autograd(prev_mask, ref_mask, init_pred, d_outs, n_obj, H, W, dtype):
    """(d_prev [B,O,HW], d_init [B,O,H,W]) of the nested pools by torch autograd in ``dtype`` on the device."""
    prev = prev_mask.detach().to(dtype).clone().requires_grad_(True)
    init = init_pred.detach().to(dtype).clone().requires_grad_(True)
    outs = R.nested_pools(prev, ref_mask.to(dtype), init, n_obj, H, W)
    pick = [i for i, d in enumerate(d_outs) if d is not None]
    return torch.autograd.grad([outs[i] for i in pick], [prev, init], [d_outs[i].to(dtype) for i in pick])


@pytest.mark.parametrize("H,W,kind", [(h, w, k) for h, w in ((7, 9), (33, 17), (32, 33), (47, 66), (1, 1)) for k in ("random", "ties")]
                         + [(255, 448, "ties")])
def test_pyramid_bwd_kernel(H, W, kind):
    B, O, n_obj = 2, 4, 3
    prev_mask, ref_mask, init_pred = pyramid_case(H, W, kind)
    torch.manual_seed(2)
    d_all = [torch.randn(n_obj, B, 3, h, w, device=DEV) for h, w in D.pyramid_sizes(H, W)]
    tag = f"pyramid_bwd_{H}x{W}_{kind}"
    # the forward under the function is the forward
    fwd = D.mask_pyramid_fn(prev_mask, ref_mask, init_pred, n_obj, H, W)
    for a, b in zip(fwd, R.nested_pools(prev_mask, ref_mask, init_pred, n_obj, H, W)):
        assert torch.equal(a, b)
    # one level at a time: a pure scatter, bit for bit what torch routes
    for lvl in range(4):
        ds = [d if i == lvl else None for i, d in enumerate(d_all)]
        got = D.mask_pyramid_bwd(prev_mask, init_pred, ds, n_obj, H, W)
        want = pyramid_autograd(prev_mask, ref_mask, init_pred, ds, n_obj, H, W, torch.float32)
        for name, a, b in zip(("d_prev", "d_init"), got, want):
            assert a.shape == b.shape and torch.equal(a, b), (tag, lvl, name)
    # all four levels
    got = D.mask_pyramid_bwd(prev_mask, init_pred, d_all, n_obj, H, W)
    stock = pyramid_autograd(prev_mask, ref_mask, init_pred, d_all, n_obj, H, W, torch.float32)
    ref = pyramid_autograd(prev_mask, ref_mask, init_pred, d_all, n_obj, H, W, torch.float64)
    for name, a, s, r in zip(("d_prev", "d_init"), got, stock, ref):
        held(f"{tag}/{name}", a, s, r)
        assert float(a[:, n_obj:].abs().max()) == 0.0
    # three calls, bit identical; image 0 alone
    for _ in range(2):
        again = D.mask_pyramid_bwd(prev_mask, init_pred, d_all, n_obj, H, W)
        assert all(torch.equal(a, b) for a, b in zip(got, again))
    one = D.mask_pyramid_bwd(prev_mask[:1], init_pred[:1], [d[:, :1] for d in d_all], n_obj, H, W)
    assert all(torch.equal(a[:1], b) for a, b in zip(got, one))
    # under autograd, and a plane without a gradient is not asked for
    p, i = prev_mask.clone().requires_grad_(True), init_pred.clone().requires_grad_(True)
    outs = D.mask_pyramid_fn(p, ref_mask, i, n_obj, H, W)
    gp, gi = torch.autograd.grad(outs, [p, i], d_all)
    assert torch.equal(gp, got[0]) and torch.equal(gi, got[1])
    outs = D.mask_pyramid_fn(prev_mask, ref_mask, i, n_obj, H, W)
    (gi,) = torch.autograd.grad(outs, [i], d_all)
    assert torch.equal(gi, got[1])


@pytest.mark.parametrize("H,W", [(7, 9), (47, 66)])
def test_pyramid_bwd_stays_inside_its_buffers_and_leaves_an_unwanted_plane_alone(H, W):
    B, O, n_obj = 2, 4, 3
    prev_mask, ref_mask, init_pred = pyramid_case(H, W, "ties")
    torch.manual_seed(3)
    d_all = [torch.randn(n_obj, B, 3, h, w, device=DEV) for h, w in D.pyramid_sizes(H, W)]
    plain = D.mask_pyramid_bwd(prev_mask, init_pred, d_all, n_obj, H, W)
    with guarded() as g:
        args = [banded(prev_mask), banded(init_pred), [banded(d) for d in d_all]]
        got = D.mask_pyramid_bwd(*args, n_obj, H, W)
        torch.cuda.synchronize()
        assert g.check() == [] and g.outside(list(got)) == []
        # caller's planes with strides of their own (4-byte aligned), one of them not wanted
        wide = torch.full((B, O + 1, H * W + 3), 7.0, device=DEV)
        keep = torch.full((B, O, H, W), 7.0, device=DEV)
        D.mask_pyramid_bwd(*args, n_obj, H, W, need=(True, False), out=(wide[:, 1:, 3:], keep))
        torch.cuda.synchronize()
        assert g.check() == []
    for a, b in zip(got, plain):
        assert torch.equal(a, b) and not bool(torch.isnan(a).any())
    assert torch.equal(wide[:, 1:1 + n_obj, 3:], plain[0][:, :n_obj])
    assert float((wide[:, 0] - 7).abs().max()) == 0 and float((wide[:, 1:, :3] - 7).abs().max()) == 0
    assert float((wide[:, 1 + n_obj:] - 7).abs().max()) == 0                # rows beyond n_obj are the caller's
    assert float((keep - 7).abs().max()) == 0                               # no gradient wanted: not touched


# ---- (12g) the bilinear upsample's backward -----------------------------------------------------------------------------------
def bilinear_autograd(d_dst, h, w, dtype):
    B, C, H, W = d_dst.shape
    src = torch.zeros(B, C, h, w, device=DEV, dtype=dtype, requires_grad=True)        # (linear: the gradient ignores src)
    up = F.interpolate(src, size=(H, W), mode="bilinear", align_corners=True)
    return torch.autograd.grad(up, src, d_dst.to(dtype))[0]


@pytest.mark.parametrize("C", [1, 6])
@pytest.mark.parametrize("shape", [(2, 3, 3, 5), (8, 14, 16, 28), (1, 1, 2, 2), (5, 7, 5, 7)])
def test_upsample_bilinear_bwd_kernel(shape, C):
    h, w, H, W = shape
    B, c0, Cd = 2, 2, C + 5
    torch.manual_seed(4)
    wide = torch.randn(B, Cd, H, W, device=DEV)                          # the gradient of a wider tensor: a channel range of it
    d_dst = wide[:, c0:c0 + C]
    got = D.upsample_bilinear_bwd(wide, c0, C, h, w)
    stock, ref = bilinear_autograd(d_dst, h, w, torch.float32), bilinear_autograd(d_dst, h, w, torch.float64)
    tag = f"upsample_bwd_{h}x{w}_to_{H}x{W}_c{C}"
    held(tag, got, stock, ref)
    held(tag + "/closed_form", got, stock, R.bilinear_bwd_closed_form(d_dst.double(), h, w))
    for _ in range(2):
        assert torch.equal(D.upsample_bilinear_bwd(wide, c0, C, h, w), got)
    assert torch.equal(D.upsample_bilinear_bwd(wide[:1], c0, C, h, w), got[:1])
    with guarded() as g:
        again = D.upsample_bilinear_bwd(banded(wide), c0, C, h, w)
        torch.cuda.synchronize()
        assert g.check() == [] and g.outside([again]) == []
    assert torch.equal(again, got)
    # the function: forward = the 'write' kernel, backward = this one
    src = torch.randn(B, C, h, w, device=DEV, requires_grad=True)
    up = D.upsample_bilinear_fn(src, (H, W))
    dst = torch.empty(B, C, H, W, device=DEV)
    D.upsample_bilinear_into(src.detach(), dst, 0, "write")
    assert torch.equal(up, dst)
    (gs,) = torch.autograd.grad(up, src, d_dst)
    assert torch.equal(gs, got)


def test_upsample_bilinear_bwd_refuses_a_downsample():
    d = torch.randn(2, 3, 1, 1, device=DEV)
    with pytest.raises(_lib.DmmError):
        D.upsample_bilinear_bwd(d, 0, 3, 3, 4)
    with pytest.raises(_lib.DmmError):
        D.upsample_bilinear_fn(torch.randn(2, 3, 3, 4, device=DEV, requires_grad=True), (1, 1))


# ---- (12h) the finish of the training step ---------------------------------------------------------------------------------------
def finish_torch(logits, d_outs, n_obj, H, W, dtype):
    lg = logits.detach().to(dtype).contiguous().requires_grad_(True)
    p = torch.sigmoid(F.interpolate(lg, (H, W)))
    return p.detach(), torch.autograd.grad(p, lg, d_outs[:, :n_obj].to(dtype))[0]


@pytest.mark.parametrize("shape", [(16, 24, 29, 43), (128, 224, 255, 448), (8, 8, 7, 7)])
def test_refine_train_finish_kernels(shape):
    h, w, H, W = shape
    B, O, n_obj = 2, 4, 3
    torch.manual_seed(5)
    # conv_out's output for all objects, handed over as a strided view
    logits = (torch.randn(n_obj * B, 1, h, w, device=DEV) * 3).view(n_obj, B, h, w).transpose(0, 1)
    assert not logits.is_contiguous()
    d_outs = torch.randn(B, O, H, W, device=DEV)
    outs = D.refine_train_finish(logits, O, H, W)
    d_logits = D.refine_train_finish_bwd(logits, d_outs)
    (so, sg), (ro, rg) = finish_torch(logits, d_outs, n_obj, H, W, torch.float32), finish_torch(logits, d_outs, n_obj, H, W,
                                                                                                 torch.float64)
    tag = f"train_finish_{h}x{w}_to_{H}x{W}"
    held(tag + "/outs", outs[:, :n_obj], so, ro)
    held(tag + "/d_logits", d_logits, sg, rg)
    held(tag + "/d_logits/closed_form", d_logits, sg, R.train_finish_bwd_closed_form(logits.double(), d_outs.double()))
    assert float(outs[:, n_obj:].abs().max()) == 0.0                       # the padded rows: exactly zero
    for _ in range(2):
        assert torch.equal(D.refine_train_finish(logits, O, H, W), outs)
        assert torch.equal(D.refine_train_finish_bwd(logits, d_outs), d_logits)
    assert torch.equal(D.refine_train_finish(logits[:1], O, H, W), outs[:1])
    assert torch.equal(D.refine_train_finish_bwd(logits[:1], d_outs[:1]), d_logits[:1])
    with guarded() as g:
        lb, db = banded(logits), banded(d_outs)
        o2, g2 = D.refine_train_finish(lb, O, H, W), D.refine_train_finish_bwd(lb, db)
        torch.cuda.synchronize()
        assert g.check() == [] and g.outside([o2, g2]) == []
    assert torch.equal(o2, outs) and torch.equal(g2, d_logits)
    lg = logits.detach().clone().requires_grad_(True)
    o3 = D.refine_train_finish_fn(lg, O, H, W)
    (g3,) = torch.autograd.grad(o3, lg, d_outs)
    assert torch.equal(o3, outs) and torch.equal(g3, d_logits)


# ---- the step ------------------------------------------------------------------------------------------------------------------------
B_, O_, H_, W_, HID = 2, 4, 29, 43, 32
VALID = [[1, 1, 1, 0], [1, 0, 1, 0]]                                        # 3 objects; (video 1, object 1) is invalid


def step_setup(mode, seed):
    torch.manual_seed(seed)
    dec = RSISMask(make_args(mode, hidden=HID)).eval().to(DEV)
    with torch.no_grad():
        dec.conv_out.weight.mul_(10)                                      # (default weights leave every logit within +-0.3)
    dec.fused_train = True
    frames = clip(seed + 1, B_, O_, H_, W_, HID, 2, device=DEV)
    valid = torch.tensor(VALID, device=DEV)
    return dec, frames, valid, valid.float()


def run_forms(dec, frames, valid, sw, only_temporal):
    """-> (got, [stock route fp32, trainer's loop on fused_train fp32], fp64 stock route); each = run_clip's result."""
    step = RefineTrainStep(dec, only_temporal=only_temporal)
    got = run_clip(step_call(step, valid, sw), dec, frames, valid, sw)
    assert step.last_route == "fused"
    plain = copy.deepcopy(dec)
    plain.fused_train = False
    step_s = RefineTrainStep(plain, only_temporal=only_temporal)
    stock = run_clip(step_call(step_s, valid, sw), plain, frames, valid, sw)
    assert step_s.last_route == "stock"
    n0 = dec.conv_calls
    loop = run_clip(loop_call(valid, sw, 3, only_temporal), dec, frames, valid, sw)
    assert dec.conv_calls > n0                                             # the loop ran on the decoder's fused training form
    dec64 = copy.deepcopy(plain).double()
    frames64 = [{"feats": [t.double() for t in fr["feats"]], "y_mask": fr["y_mask"].double(),
                 "init_pred": fr["init_pred"].double()} for fr in frames]
    step64 = RefineTrainStep(dec64, only_temporal=only_temporal)
    ref = run_clip(step_call(step64, valid, sw), dec64, frames64, valid, sw)
    assert step64.last_route == "stock"
    return got, [stock, loop], ref


@pytest.mark.parametrize("mode,only_temporal", [("concat", False), ("sum", False), ("concat", True)])
def test_step_against_the_fp64_stock_route(mode, only_temporal):
    dec, frames, valid, sw = step_setup(mode, 81)
    got, stocks, ref = run_forms(dec, frames, valid, sw, only_temporal)
    tag = f"refine_train/{mode}{'_only_temporal' if only_temporal else ''}"
    held_all(tag + "/loss", got[0], [s[0] for s in stocks], ref[0])
    for f in range(2):
        held_all(f"{tag}/f{f}/outs_pad", got[1][f], [s[1][f] for s in stocks], ref[1][f])
        assert got[1][f].shape == (B_, O_, H_ * W_) and float(got[1][f][:, 3:].abs().max()) == 0.0
        assert sorted(got[3][f]) == ["hard_iou", "loss_miou"]
    assert sorted(got[2]) == sorted(ref[2]) and len(got[2]) == 2 * 5 + len(list(dec.parameters()))
    for k in got[2]:
        held_all(f"{tag}/grad/{k}", got[2][k], [s[2][k] for s in stocks], ref[2][k])


def test_step_twice_is_bit_identical_in_deterministic_mode():
    dec, frames, valid, sw = step_setup("concat", 91)
    runs = []
    with dmm_net_amd.deterministic(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        for _ in range(2):
            step = RefineTrainStep(dec)
            runs.append(run_clip(step_call(step, valid, sw), dec, frames, valid, sw))
            assert step.last_route == "fused"
    assert torch.equal(runs[0][0], runs[1][0])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k


def test_step_routes():
    dec, frames, valid, sw = step_setup("concat", 95)
    fr = frames[0]
    args = lambda to=None: [[t if to is None else t.to(to) for t in fr["feats"]]] + \
        [t if to is None else t.to(to) for t in (fr["y_mask"], fr["y_mask"], fr["init_pred"], fr["y_mask"])] + [sw, valid]
    step = RefineTrainStep(dec)
    loss, _, outs, state = step(*args(), None)
    assert step.last_route == "fused" and loss.requires_grad and state.n_obj == 3 and state[0][0].requires_grad
    # no gradient required: the same forward
    with torch.no_grad():
        loss0, _, outs0, state0 = step(*args(), None)
    assert step.last_route == "fused" and not loss0.requires_grad and torch.equal(outs0, outs) and torch.equal(loss0, loss)
    # one piece routed back to its torch twin, the other two stay
    for piece in ("pyramid", "upsample", "finish"):
        twin = RefineTrainStep(dec)
        twin.kernels[piece] = False
        l2, _, o2, _ = twin(*args(), None)
        assert twin.last_route == "fused" and l2.requires_grad
        # the same function: the pyramid is exact; the other two are fp32 evaluations of the same probabilities in (0, 1)
        # (their bounds are test_step_against_the_fp64_stock_route's; a wrong route is off by O(0.1))
        assert float((o2 - outs).detach().abs().max()) <= (0.0 if piece == "pyramid" else 1e-4), piece
    # fused_train off, active dropout, non-fp32 tensors, CPU tensors: the trainer's loop
    off = copy.deepcopy(dec)
    off.fused_train = False
    drop = RSISMask(make_args("concat", hidden=HID, dropout=0.5)).to(DEV).train()
    drop.fused_train = True
    for d, to in ((off, None), (drop, None), (copy.deepcopy(dec).double(), torch.float64), (copy.deepcopy(dec).cpu(), "cpu")):
        s = RefineTrainStep(d)
        a = args(to)
        if to == "cpu":
            a[-2:] = [sw.cpu(), valid.cpu()]
        n0 = d.conv_calls
        out = s(*a, None)
        assert s.last_route == "stock" and d.conv_calls == n0 and out[0].requires_grad
    drop.eval()
    s = RefineTrainStep(drop)
    s(*args(), None)
    assert s.last_route == "fused"
