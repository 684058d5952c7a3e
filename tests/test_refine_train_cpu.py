"""The refine step of training, the parts that need no GPU: the closed forms of tests/refine_train_ref.py (what the kernels
(12f)-(12h) of include/dmm_match.h implement) against fp64 torch autograd of the trainer's own ops, the entries' answers to
calls they refuse before anything touches the device, and ``RefineTrainStep`` on CPU tensors (stock route) against the
trainer's loop restated."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import refine_train_ref as R
from dmm_net_amd import _lib
from dmm_net_amd.decoder import RSISMask, RefineState, RefineTrainStep, pyramid_sizes
from test_decoder_cpu import make_args

SIZES = [(7, 9), (33, 17), (32, 33), (47, 66), (1, 1)]


def planes(kind, B, O, H, W, g, dtype=torch.float64):
    """'random': distinct values; 'ties': values from {0, 0.5, 1}, so nearly every window has several maxima."""
    if kind == "random":
        return torch.rand(B, O, H * W, generator=g, dtype=torch.float64).to(dtype)
    return (torch.randint(0, 3, (B, O, H * W), generator=g).to(dtype)) / 2


# ---- closed forms against fp64 autograd ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "ties"])
@pytest.mark.parametrize("size", SIZES)
def test_pyramid_closed_form_equals_fp64_autograd_of_the_nested_pools(size, kind):
    """Both sides route each output gradient to one pixel and add at most four of them: 1e-12 is far above the rounding of
    a four-term fp64 sum of O(1) values and far below any misrouted gradient."""
    H, W = size
    B, O, n_obj = 2, 4, 3
    g = torch.Generator().manual_seed(H * 100 + W)
    prev = planes(kind, B, O, H, W, g).requires_grad_(True)
    ref = planes(kind, B, O, H, W, g)
    init = planes(kind, B, O, H, W, g).view(B, O, H, W).requires_grad_(True)
    outs = R.nested_pools(prev, ref, init, n_obj, H, W)
    assert [tuple(o.shape[-2:]) for o in outs] == pyramid_sizes(H, W)
    d_outs = [torch.randn(o.shape, generator=g, dtype=torch.float64) for o in outs]
    for sel in ([0, 1, 2, 3], [0], [1], [2], [3]):
        ds = [d if i in sel else None for i, d in enumerate(d_outs)]
        want = torch.autograd.grad([outs[i] for i in sel], [prev, init], [d_outs[i] for i in sel], retain_graph=True)
        got = R.pyramid_bwd_closed_form(prev.detach(), init.detach(), ds, n_obj, H, W)
        for a, b in zip(got, want):
            b = b.reshape(B, O, H, W)
            assert float((a - b[:, :n_obj]).abs().max()) < 1e-12, (size, kind, sel)
            assert float(b[:, n_obj:].abs().max()) == 0.0


def test_zorder_is_not_row_major():
    """In a 4 x 4 window of equal values the winner is pixel (0, 0); with (0, 0) and (0, 1) lowered, pixel (1, 0) (code 2) wins
    over (0, 2) (code 4), which a row-major scan would take."""
    code = R.zorder_codes(2)
    assert code[1, 0] == 2 and code[0, 2] == 4 and code[0, 1] == 1 and code[3, 3] == 15
    p = torch.ones(1, 1, 4, 4, dtype=torch.float64)
    p[0, 0, 0, :2] = 0
    iy, ix = R.pyramid_winners(p, 2)
    assert (int(iy), int(ix)) == (1, 0)
    x = p.clone().requires_grad_(True)
    pool = lambda t: F.max_pool2d(t, (2, 2), ceil_mode=True)
    pool(pool(x)).sum().backward()
    assert float(x.grad[0, 0, 1, 0]) == 1.0 and float(x.grad.sum()) == 1.0


@pytest.mark.parametrize("shape", [(2, 3, 3, 5), (8, 14, 16, 28), (1, 1, 2, 2), (5, 7, 5, 7), (1, 4, 7, 9), (24, 33, 48, 66)])
def test_bilinear_closed_form_equals_fp64_autograd(shape):
    h, w, H, W = shape
    g = torch.Generator().manual_seed(h * 10 + W)
    src = torch.randn(2, 3, h, w, generator=g, dtype=torch.float64).requires_grad_(True)
    up = F.interpolate(src, size=(H, W), mode="bilinear", align_corners=True)
    d = torch.randn(up.shape, generator=g, dtype=torch.float64)
    (want,) = torch.autograd.grad(up, src, d)
    assert float((R.bilinear_bwd_closed_form(d, h, w) - want).abs().max()) < 1e-12
    # the forward's matrix is the same one
    my, mx = R.bilinear_matrix(h, H, torch.float64), R.bilinear_matrix(w, W, torch.float64)
    assert float((torch.einsum("Yy,bcyx,Xx->bcYX", my, src.detach(), mx) - up.detach()).abs().max()) < 1e-12
    # per source index the touching destination indices are one solid range, in fp32 as in fp64: what the gather relies on
    for n_in, n_out in ((h, H), (w, W)):
        for dt in (np.float32, np.float64):
            lo, hi, solid = R.gather_range(n_in, n_out, dt)
            assert solid and lo[0] == 0 and hi[-1] == n_out - 1


@pytest.mark.parametrize("shape", [(16, 24, 29, 43), (128, 224, 255, 448), (8, 8, 7, 7), (4, 4, 1, 1), (16, 20, 47, 66)])
def test_finish_closed_form_equals_fp64_autograd(shape):
    h, w, H, W = shape
    B, O, n_obj = 2, 4, 3
    g = torch.Generator().manual_seed(h + W)
    logits = (torch.randn(B, n_obj, h, w, generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    want_o = torch.sigmoid(F.interpolate(logits, (H, W)))
    got_o = R.train_finish_closed_form(logits.detach(), O, H, W)
    assert float((got_o[:, :n_obj] - want_o.detach()).abs().max()) < 1e-12 and float(got_o[:, n_obj:].abs().max()) == 0.0
    d = torch.randn(B, O, H, W, generator=g, dtype=torch.float64)
    (want,) = torch.autograd.grad(want_o, logits, d[:, :n_obj])
    assert float((R.train_finish_bwd_closed_form(logits.detach(), d) - want).abs().max()) < 1e-12


@pytest.mark.parametrize("pair", [(128, 255), (224, 448), (16, 29), (24, 43), (8, 7), (4, 1), (16, 47), (20, 66)])
def test_nearest_index_in_fp32_is_the_integer_quotient(pair):
    n_in, n_out = pair
    assert np.array_equal(R.nearest_index(n_in, n_out), (np.arange(n_out) * n_in) // n_out)


# ---- the entries' argument checks ------------------------------------------------------------------------------------------
P = lambda have=True: ctypes.c_void_p(8) if have else None


def test_pyramid_bwd_entry_validates_its_arguments_without_gpu():
    L = _lib.load()
    OK, BAD, UNSUPPORTED = _lib.DMM_OK, _lib.DMM_ERR_BAD_ARG, _lib.DMM_ERR_UNSUPPORTED

    def st(B=2, n_obj=3, H=7, W=9, prev=True, init=True, sp=(252, 63, 252, 63), d_prev=True, d_init=True, sd=(252, 63, 252, 63)):
        return L.dmm_mask_pyramid_bwd_f32(P(prev), P(init), *sp, B, n_obj, H, W, P(), P(), P(), P(), P(d_prev), sd[0], sd[1],
                                          P(d_init), sd[2], sd[3], None)

    for kw in (dict(B=-1), dict(n_obj=-1), dict(H=0), dict(W=-3), dict(prev=False), dict(init=False), dict(sp=(-1, 63, 252, 63)),
               dict(sp=(252, 63, 252, -1)), dict(sd=(252, 62, 252, 63)), dict(sd=(252, 63, 252, 62)), dict(sd=(-1, 63, 252, 63))):
        assert st(**kw) == BAD, kw
    assert st(B=0) == OK and st(n_obj=0) == OK and st(B=0, prev=False, init=False) == OK
    assert st(d_prev=False, d_init=False) == OK                          # no plane wanted: nothing to do
    assert st(B=0, H=0) == BAD                                           # sizes before "nothing to do"
    assert st(B=1 << 13, n_obj=3) == UNSUPPORTED                         # B * n_obj * 3 > 65535
    assert _lib.SYMBOLS.count("dmm_mask_pyramid_bwd_f32") == 1


def test_upsample_bwd_entry_validates_its_arguments_without_gpu():
    L = _lib.load()
    OK, BAD, UNSUPPORTED = _lib.DMM_OK, _lib.DMM_ERR_BAD_ARG, _lib.DMM_ERR_UNSUPPORTED

    def st(B=2, C=3, H=6, W=10, Cd=5, c0=1, h=3, w=5, d_dst=True, d_src=True, sbd=None, sbs=None):
        sbd = Cd * H * W if sbd is None else sbd
        sbs = C * h * w if sbs is None else sbs
        return L.dmm_upsample_bilinear_bwd_f32(P(d_dst), sbd, B, C, H, W, Cd, c0, P(d_src), sbs, h, w, None)

    for kw in (dict(B=-1), dict(C=0), dict(H=0), dict(w=0), dict(Cd=0), dict(c0=-1), dict(c0=3), dict(d_dst=False),
               dict(d_src=False), dict(sbd=299), dict(sbs=44)):
        assert st(**kw) == BAD, kw
    for kw in (dict(h=7), dict(w=11), dict(h=3, w=4, H=1, W=1), dict(B=0, h=7)):
        assert st(**kw) == UNSUPPORTED, kw                               # not an upsample: refused, whatever else
    assert st(B=0) == OK and st(B=0, d_dst=False, d_src=False) == OK
    assert st(B=1 << 20, C=1 << 10, h=1 << 10, w=1 << 10, H=1 << 10, W=1 << 10, Cd=1 << 10, c0=0, sbd=1 << 30, sbs=1 << 30) == UNSUPPORTED


def test_train_finish_entries_validate_their_arguments_without_gpu():
    L = _lib.load()
    OK, BAD, UNSUPPORTED = _lib.DMM_OK, _lib.DMM_ERR_BAD_ARG, _lib.DMM_ERR_UNSUPPORTED

    def fwd(B=2, O=4, n_obj=3, h=8, w=12, H=15, W=23, logits=True, outs=True, sl=(288, 96)):
        return L.dmm_refine_train_finish_f32(P(logits), sl[0], sl[1], h, w, B, O, n_obj, H, W, P(outs), None)

    def bwd(B=2, O=4, n_obj=3, h=8, w=12, H=15, W=23, logits=True, d_outs=True, d_logits=True, sl=(288, 96), sd=None):
        sd = (n_obj * h * w, h * w) if sd is None else sd
        return L.dmm_refine_train_finish_bwd_f32(P(logits), sl[0], sl[1], h, w, P(d_outs), B, O, n_obj, H, W, P(d_logits), sd[0],
                                                 sd[1], None)

    for f in (fwd, bwd):
        for kw in (dict(B=-1), dict(O=-1), dict(n_obj=-1), dict(n_obj=5), dict(h=0), dict(W=0), dict(logits=False),
                   dict(sl=(-1, 96)), dict(sl=(288, -1))):
            assert f(**kw) == BAD, (f.__name__, kw)
        assert f(B=0) == OK and f(B=0, logits=False) == OK and f(B=0, H=0) == BAD
        assert f(B=1 << 16, O=1 << 10, n_obj=1 << 10, h=1 << 10, w=1 << 10, H=1 << 10, W=1 << 10) == UNSUPPORTED
    assert fwd(outs=False) == BAD and fwd(O=0, n_obj=0) == OK
    assert bwd(d_outs=False) == BAD and bwd(d_logits=False) == BAD and bwd(sd=(288, 95)) == BAD and bwd(sd=(-1, 96)) == BAD
    assert bwd(n_obj=0, logits=False) == OK


# ---- the step on CPU tensors -------------------------------------------------------------------------------------------------
def clip(seed, B, O, H, W, hidden, T, device="cpu", dtype=torch.float32):
    """T frames of inputs for the step: skip maps, the reference / target masks, sample weights, init_pred."""
    g = torch.Generator().manual_seed(seed)
    sizes = pyramid_sizes(H, W)
    ch = [hidden, hidden, hidden // 2, hidden // 4]
    frames = []
    for _ in range(T):
        frames.append({"feats": [torch.randn((B, c) + s, generator=g).to(device, dtype) for c, s in zip(ch, sizes)],
                       "y_mask": (torch.rand(B, O, H * W, generator=g) > 0.6).to(device, dtype),
                       "init_pred": torch.rand(B, O, H, W, generator=g).to(device, dtype)})
    return frames


def run_clip(call, dec, frames, valid, sw_mask, n_obj=None):
    """Two or more frames as the trainer chains them: prev_mask = y_mask at frame 0, then last frame's ``outs`` (attached);
    the temporal hiddens carried with their graph.  ``call(dec, feats, prev_thid, init_pred, prev_mask, y_mask, ref_mask)`` ->
    (loss, logged, outs, thid).  -> (total loss, [outs], {name: gradient})."""
    leaves = {}
    for f, fr in enumerate(frames):
        for i, t in enumerate(fr["feats"]):
            leaves[f"f{f}/skip{i}"] = t.detach().clone().requires_grad_(True)
        leaves[f"f{f}/init_pred"] = fr["init_pred"].detach().clone().requires_grad_(True)
    ref_mask = frames[0]["y_mask"]
    prev_mask, thid, total, outs_all, logged_all = ref_mask, None, 0, [], []
    for f, fr in enumerate(frames):
        feats = [leaves[f"f{f}/skip{i}"] for i in range(4)]
        loss, logged, outs, thid = call(dec, feats, thid, leaves[f"f{f}/init_pred"], prev_mask, fr["y_mask"], ref_mask)
        total = total + loss
        prev_mask = outs
        outs_all.append(outs.detach())
        logged_all.append({k: v.detach() for k, v in logged.items()})
    params = dict(dec.named_parameters())
    names = list(leaves) + list(params)
    grads = torch.autograd.grad(total, list(leaves.values()) + list(params.values()))
    return total.detach(), outs_all, dict(zip(names, grads)), logged_all


def step_call(step, valid, sw_mask, state0=None):
    """``call`` of ``run_clip`` on a ``RefineTrainStep``; the state rides in a closure (``thid`` is what run_clip carries)."""
    box = {"state": state0}

    def call(dec, feats, thid, init_pred, prev_mask, y_mask, ref_mask):
        assert step.decoder is dec
        loss, logged, outs, box["state"] = step({"refine_input_feat": feats}, prev_mask, ref_mask, init_pred, y_mask, sw_mask,
                                                valid, box["state"])
        return loss, logged, outs, box["state"].thid
    return call


def loop_call(valid, sw_mask, n_obj, only_temporal=False, iou_weight=1.0):
    def call(dec, feats, thid, init_pred, prev_mask, y_mask, ref_mask):
        return R.trainer_refine(dec, feats, thid, init_pred, prev_mask, sw_mask, y_mask, valid, ref_mask, n_obj,
                                only_temporal=only_temporal, iou_weight=iou_weight)
    return call


@pytest.mark.parametrize("only_temporal", [False, True])
def test_step_on_cpu_tensors_is_the_trainers_loop(only_temporal):
    """2 frames x 3 objects (of O = 4), one invalid (video, object) pair: the step's stock route IS the loop -- same ops in
    the same order, so the same bits."""
    B, O, H, W, hidden = 2, 4, 29, 43, 16
    torch.manual_seed(5)
    dec = RSISMask(make_args("concat", hidden=hidden)).eval()
    dec.fused_train = True                                                 # an opt-in for HIP tensors: the CPU takes stock
    frames = clip(6, B, O, H, W, hidden, 2)
    valid = torch.tensor([[1, 1, 1, 0], [1, 0, 1, 0]])
    sw_mask = valid.float()
    step = RefineTrainStep(dec, only_temporal=only_temporal, iou_weight=0.7)
    got = run_clip(step_call(step, valid, sw_mask), dec, frames, valid, sw_mask)
    assert step.last_route == "stock"
    want = run_clip(loop_call(valid, sw_mask, 3, only_temporal, 0.7), dec, frames, valid, sw_mask)
    assert torch.equal(got[0], want[0])
    for a, b in zip(got[1], want[1]):
        assert a.shape == (B, O, H * W) and torch.equal(a, b) and float(a[:, 3:].abs().max()) == 0.0
    assert sorted(got[2]) == sorted(want[2])
    for k in got[2]:
        assert torch.equal(got[2][k], want[2][k]), k
    for a, b in zip(got[3], want[3]):
        assert sorted(a) == ["hard_iou", "loss_miou"] and all(torch.equal(a[k], b[k]) for k in a)


def test_step_state_and_refusals():
    B, O, H, W, hidden = 1, 3, 29, 43, 16
    torch.manual_seed(7)
    dec = RSISMask(make_args("sum", hidden=hidden)).eval()
    fr = clip(8, B, O, H, W, hidden, 1)[0]
    valid = torch.tensor([[1, 0, 0]])
    step = RefineTrainStep(dec)
    args = (fr["feats"], fr["y_mask"], fr["y_mask"], fr["init_pred"], fr["y_mask"], valid.float(), valid)
    loss, logged, outs, state = step(*args, None)
    assert state.n_obj == 1 and len(state) == 1 and len(state[0]) == 4 and state[0][0].requires_grad
    assert float(outs.detach()[:, 1:].abs().max()) == 0.0 and loss.requires_grad
    # the caller's own state: skip_empty_starting_frame = False evaluates every slot
    _, _, outs_all, state = step(*args, RefineState(O))
    assert state.n_obj == O and len(state) == O and float(outs_all.detach()[:, 1:].abs().min()) > 0.0
    # object 0 does not depend on how many follow (torch's sigmoid rounds a vector lane and a tail element differently)
    assert float((outs_all[:, :1] - outs[:, :1]).abs().max()) < 1e-6
    with pytest.raises(ValueError):
        step(*args[:-1], torch.zeros(1, 3, dtype=torch.long), None)       # no valid template: the caller's branch
    # dropout active, double precision: still the loop
    drop = RSISMask(make_args("concat", hidden=hidden, dropout=0.3)).train().double()
    out = RefineTrainStep(drop)([f.double() for f in fr["feats"]], fr["y_mask"].double(), fr["y_mask"].double(),
                                fr["init_pred"].double(), fr["y_mask"].double(), valid.float(), valid, None)
    assert out[2].dtype == torch.float64 and out[0].requires_grad


def test_forward_fused_train_defaults_are_unchanged():
    """The optional arguments of ``_forward_fused_train`` exist and default to 'compute everything here'."""
    import inspect
    sig = inspect.signature(RSISMask._forward_fused_train)
    for name, default in (("slices", None), ("skip_terms", None), ("temporal_terms", None), ("bilinear", None), ("head", True)):
        assert sig.parameters[name].default is default, name
    dec = copy.deepcopy(RSISMask(make_args("concat", hidden=16)))
    sl = dec.train_slices()
    assert [tuple(d["m"].shape) for d in sl] == [(64, 9), (32, 9), (16, 9), (8, 9)] and sl[0]["up"] is None
    assert sl[1]["skip"].shape[1] == 16 and sl[1]["up"].shape[1] == 16 and all(d["ht"].requires_grad for d in sl)


@pytest.mark.parametrize("with_bias", [True, False])
def test_stacked_convolution_is_the_convolution(with_bias):
    """``_ConvStacked``: the library's convolution forward; its gradients, the weight's and bias's taken group by group, are
    those of ``F.conv2d`` (fp64: the two differ by the order of a few hundred additions)."""
    from dmm_net_amd.decoder import _ConvStacked
    g = torch.Generator().manual_seed(3)
    x = torch.randn(6, 4, 5, 7, generator=g, dtype=torch.float64).requires_grad_(True)
    w = torch.randn(2, 4, 3, 3, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(2, generator=g, dtype=torch.float64).requires_grad_(True) if with_bias else None
    d = torch.randn(6, 2, 5, 7, generator=g, dtype=torch.float64)
    leaves = [x, w] + ([b] if with_bias else [])
    y0 = F.conv2d(x, w, b, padding=1)
    y1 = _ConvStacked.apply(x, w, b, 3)
    assert torch.equal(y0, y1)
    for a, c in zip(torch.autograd.grad(y1, leaves, d), torch.autograd.grad(y0, leaves, d)):
        assert a.shape == c.shape and float((a - c).abs().max()) < 1e-12
    (gw,) = torch.autograd.grad(_ConvStacked.apply(x.detach(), w, b, 3), [w], d)          # the input needs no gradient
    assert float((gw - torch.autograd.grad(F.conv2d(x.detach(), w, b, padding=1), [w], d)[0]).abs().max()) < 1e-12
