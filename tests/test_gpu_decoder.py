"""The refine decoder on the GPU: each kernel of csrc/dmm_decoder.hip against the torch ops it replaces, the fused
``RSISMask.forward`` against the reference fixture (G23) and, at the product's size, against the stock form, ``RefineStep``
fused against stock, graph capture, the frame loop with the decoder plugged in, and the launch counts.

Tolerances are not fixed numbers.  A fused result and the stock torch result are both fp32 evaluations of the same
expression; each is held against an fp64 evaluation of the same inputs on the same device: with e_stock = the stock
ops' own error against fp64, a kernel alone may be off by 2 * e_stock + 1 ulp of the largest output, the fused module by
2 * e_stock (2 * max(e_stock, e_ref) against the fixture, e_ref = the reference's recorded fp32 error).  The pyramid is a
maximum: bit exact.  Every achieved pair is recorded (conftest.record_achieved)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden, record_achieved
from dmm_net_amd import _lib, decoder as D, video
from dmm_net_amd.decoder import RSISMask, RefineStep, pyramid_sizes
from test_decoder_cpu import CASES, case_inputs, chain_inputs, flat_outputs, load_decoder, make_args

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def ulp(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def held(name, got, stock, ref64, slack_ulp=True, floor=0.0):
    """err(got) <= 2 * max(e_stock, floor) [+ 1 ulp of the largest output]; both against the fp64 evaluation."""
    err = float((got.double() - ref64).abs().max())
    e_stock = float((stock.double() - ref64).abs().max())
    bound = 2 * max(e_stock, floor) + (ulp(ref64.abs().max()) if slack_ulp else 0.0)
    print(f"{name}: err {err:.3e}  e_stock {e_stock:.3e}  bound {bound:.3e}")
    record_achieved(f"decoder/{name}/err", err)
    record_achieved(f"decoder/{name}/e_stock", e_stock)
    assert err <= bound, (name, err, e_stock, bound)


# ---- the kernels alone -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(95, 130), (255, 448), (33, 17), (7, 9)])
def test_mask_pyramid_is_bit_exact(size):
    H, W = size
    torch.manual_seed(1)
    B, O, n_obj = 2, 4, 3
    big = torch.rand(B, O + 1, H * W + 3, device=DEV)
    prev_mask = big[:, 1:, 3:]                                          # strided, planes only 4-byte aligned
    y_mask = (torch.rand(B, O, H * W, device=DEV) > 0.5).float()
    init_pred = torch.rand(B, O, H, W, device=DEV)
    got = D.mask_pyramid(prev_mask, y_mask, init_pred, n_obj, H, W)
    worst = 0.0
    for t in range(n_obj):
        m = torch.stack([prev_mask[:, t].reshape(B, H, W), y_mask[:, t].view(B, H, W), init_pred[:, t]], 1)
        m = F.max_pool2d(m, (2, 2), ceil_mode=True)
        for lvl in (3, 2, 1, 0):
            m = F.max_pool2d(m, (2, 2), ceil_mode=True)
            assert got[lvl][t].shape == m.shape
            worst = max(worst, float((got[lvl][t] - m).abs().max()))
            assert torch.equal(got[lvl][t], m), (size, t, lvl)
    record_achieved(f"decoder/pyramid_{H}x{W}/err", worst)


def gates_torch(pre, masks, w_mask, cell_prev):
    Hd = w_mask.shape[0] // 4
    g0 = pre[0]
    for p in pre[1:]:
        g0 = g0 + p
    hs, cs = [], []
    for k in (0, 2, 1):
        g = g0 + F.conv2d(masks[:, k:k + 1], w_mask.view(4 * Hd, 1, 3, 3), padding=1)
        gi, gr, go, gc = g.chunk(4, 1)
        cell = torch.sigmoid(gi) * torch.tanh(gc) if cell_prev is None else \
            torch.sigmoid(gr) * cell_prev + torch.sigmoid(gi) * torch.tanh(gc)
        hs.append(torch.sigmoid(go) * torch.tanh(cell))
        cs.append(cell)
    return (hs[0] + hs[1] + hs[2]) / 3, (cs[0] + cs[1] + cs[2]) / 3


@pytest.mark.parametrize("B,Hd,h,w,n_pre,with_cell", [(2, 32, 8, 14, 3, True), (3, 6, 5, 7, 1, False), (1, 16, 24, 33, 2, True),
                                                      (4, 16, 64, 112, 3, True)])
def test_clstm_gates_kernel(B, Hd, h, w, n_pre, with_cell):
    torch.manual_seed(2)
    pre = [torch.randn(B, 4 * Hd, h, w, device=DEV) for _ in range(n_pre)]
    masks = torch.rand(B, 3, h, w, device=DEV)
    w_mask = torch.randn(4 * Hd, 9, device=DEV) * 0.3
    cell_prev = torch.randn(B, Hd, h, w, device=DEV) if with_cell else None
    hidden, cell = torch.empty(B, Hd, h, w, device=DEV), torch.empty(B, Hd, h, w, device=DEV)
    wide = torch.zeros(B, Hd + 3, h, w, device=DEV)
    D.clstm_gates(pre, masks, w_mask, cell_prev, hidden, cell, hidden_copy=wide[:, 3:])
    sh, sc = gates_torch(pre, masks, w_mask, cell_prev)
    rh, rc = gates_torch([p.double() for p in pre], masks.double(), w_mask.double(),
                         None if cell_prev is None else cell_prev.double())
    tag = f"gates_{B}x{Hd}x{h}x{w}_{n_pre}"
    held(tag + "/hidden", hidden, sh, rh)
    held(tag + "/cell", cell, sc, rc)
    assert torch.equal(wide[:, 3:], hidden) and float(wide[:, :3].abs().max()) == 0.0


@pytest.mark.parametrize("mode", ["write", "add", "mul"])
@pytest.mark.parametrize("shape", [(2, 5, 3, 5, 6, 9), (1, 16, 24, 33, 48, 66), (3, 4, 8, 14, 16, 28), (2, 3, 1, 4, 7, 9)])
def test_upsample_bilinear_into_kernel(mode, shape):
    B, C, h, w, H, W = shape
    torch.manual_seed(3)
    src = torch.randn(B, C, h, w, device=DEV)
    c0, Cd = 2, C + 5
    base = torch.randn(B, Cd, H, W, device=DEV)
    dst = base.clone()
    D.upsample_bilinear_into(src, dst, c0, mode)
    comb = {"write": lambda d, u: u, "add": lambda d, u: d + u, "mul": lambda d, u: d * u}[mode]
    up = lambda x: F.interpolate(x, size=(H, W), mode="bilinear", align_corners=True)
    stock = comb(base[:, c0:c0 + C], up(src))
    ref = comb(base[:, c0:c0 + C].double(), up(src.double()))
    held(f"upsample_{mode}_{h}x{w}_to_{H}x{W}", dst[:, c0:c0 + C], stock, ref)
    assert torch.equal(dst[:, :c0], base[:, :c0]) and torch.equal(dst[:, c0 + C:], base[:, c0 + C:])


@pytest.mark.parametrize("shape", [(2, 4, 3, 24, 34, 47, 66), (4, 6, 5, 128, 224, 255, 448), (1, 2, 2, 2, 2, 5, 7)])
def test_refine_finish_kernel(shape):
    B, O, n_obj, h, w, H, W = shape
    torch.manual_seed(4)
    logits = (torch.randn(n_obj * B, 1, h, w, device=DEV) * 3).view(n_obj, B, h, w).transpose(0, 1)
    valid = (torch.rand(B, O, device=DEV) > 0.4).to(torch.int32)
    hist0 = torch.rand(B, O, H, W, device=DEV)
    hist, outs = hist0.clone(), torch.full((B, O, H, W), 7.0, device=DEV)
    D.refine_finish(logits, valid, outs, hist, n_obj)
    up = lambda x: torch.sigmoid(F.interpolate(x, size=(H, W), mode="bilinear", align_corners=True))
    stock, ref = up(logits.contiguous()), up(logits.contiguous().double())
    held(f"finish_{h}x{w}_to_{H}x{W}", outs[:, :n_obj], stock, ref)
    assert float(outs[:, n_obj:].abs().max()) == 0.0 if n_obj < O else True
    keep = (valid[:, :n_obj] != 0).view(B, n_obj, 1, 1)
    assert torch.equal(hist[:, :n_obj], torch.where(keep, outs[:, :n_obj], hist0[:, :n_obj]))
    assert torch.equal(hist[:, n_obj:], hist0[:, n_obj:])


# ---- the module ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["concat", "sum"])
@pytest.mark.parametrize("case", list(CASES))
def test_fused_forward_against_the_reference_fixture(mode, case):
    dec, g = load_decoder(mode, DEV)
    dec64 = copy.deepcopy(dec).double()
    with torch.no_grad():
        args = case_inputs(g, mode, case, DEV)
        assert dec.fused_ok(args[0] + args[1])
        n0 = dec.conv_calls
        got = flat_outputs(dec(*args))
        assert dec.conv_calls > n0                                      # the fused form ran
        stock = flat_outputs(dec.forward_stock(*args))
        ref = flat_outputs(dec64.forward_stock(*case_inputs(g, mode, case, DEV, torch.float64)))
    for k in got:
        fix64 = torch.from_numpy(g[f"{mode}/{case}/f64/{k}"]).to(DEV)
        assert float((ref[k] - fix64).abs().max()) < 1e-12, k           # the device's fp64 evaluation IS the fixture's
        held(f"fixture/{mode}/{case}/{k}", got[k], stock[k], fix64, slack_ulp=False,
             floor=float(g[f"{mode}/{case}/e_ref/{k}"]))


def product_inputs(mode, seed=7, B=4, hidden=128, H=255, W=448):
    torch.manual_seed(seed)
    dec = RSISMask(make_args(mode, hidden=hidden)).eval().to(DEV)
    sizes = pyramid_sizes(H, W)                                          # 8 x 14 .. 64 x 112
    ch = [hidden, hidden, hidden // 2, hidden // 4]
    feats = [torch.randn((B, c) + s, device=DEV) for c, s in zip(ch, sizes)]
    masks = [torch.rand((B, 3) + s, device=DEV) for s in sizes]
    spatial = [[0.5 * torch.randn((B, d) + s, device=DEV).tanh(), torch.randn((B, d) + s, device=DEV)]
               for d, s in zip(dec.skip_dims_out, sizes)]
    temporal = [0.5 * torch.randn((B, d) + s, device=DEV).tanh() for d, s in zip(dec.skip_dims_out, sizes)]
    return dec, feats, masks, spatial, temporal


@pytest.mark.parametrize("mode", ["concat", "sum", "mul", "none"])
def test_fused_forward_against_stock_at_product_size(mode):
    dec, feats, masks, spatial, temporal = product_inputs(mode)
    dec64 = copy.deepcopy(dec).double()
    dbl = lambda ts: None if ts is None else [t.double() for t in ts]
    with torch.no_grad():
        for case, (sp, tm) in CASES.items():
            s, t = (spatial if sp else None), (temporal if tm else None)
            got = flat_outputs(dec(feats, masks, s, t))
            stock = flat_outputs(dec.forward_stock(feats, masks, s, t))
            ref = flat_outputs(dec64.forward_stock(dbl(feats), dbl(masks), None if s is None else [dbl(x) for x in s], dbl(t)))
            for k in got:
                held(f"product/{mode}/{case}/{k}", got[k], stock[k], ref[k], slack_ulp=False)


def step_inputs(seed, B, O, H, W, hidden, T):
    g = torch.Generator(device="cpu").manual_seed(seed)
    sizes = pyramid_sizes(H, W)
    ch = [hidden, hidden, hidden // 2, hidden // 4]
    frames = []
    for _ in range(T):
        feats = {"refine_input_feat": tuple(torch.randn((B, c) + s, generator=g).to(DEV) for c, s in zip(ch, sizes))}
        frames.append((feats, (torch.rand(B, O, H * W, generator=g) > 0.6).float().to(DEV),
                       (torch.rand(B, O, H * W, generator=g) > 0.6).float().to(DEV),
                       torch.rand(B, O, H, W, generator=g).to(DEV), torch.rand(B, O, H, W, generator=g).to(DEV)))
    return frames


def run_steps(step, frames, valid, dtype=torch.float32):
    state, res = None, []
    with torch.no_grad():
        for feats, pm, ym, ip, hist in frames:
            f = {"refine_input_feat": tuple(x.to(dtype) for x in feats["refine_input_feat"])}
            outs, hist_new, state = step(f, pm.to(dtype), ym.to(dtype), ip.to(dtype), hist.clone().to(dtype), valid, state)
            res.append((outs.clone(), hist_new.clone()))
    return res, state


@pytest.mark.parametrize("kw", [{}, {"only_spatial": True}, {"only_temporal": True}])
def test_refine_step_fused_against_stock(kw):
    B, O, H, W, hidden, T = 2, 6, 95, 130, 32, 3
    torch.manual_seed(11)
    dec = RSISMask(make_args("concat", hidden=hidden)).eval().to(DEV)
    with torch.no_grad():
        dec.conv_out.weight.mul_(10)
    stock_dec = copy.deepcopy(dec)
    stock_dec.fused = False
    dec64 = copy.deepcopy(stock_dec).double()
    valid = torch.tensor([[1, 1, 0, 1, 1, 0], [1, 0, 1, 0, 1, 0]], device=DEV)     # 5 objects, ragged
    frames = step_inputs(12, B, O, H, W, hidden, T)
    fused, st = run_steps(RefineStep(dec, **kw), frames, valid)
    stock, _ = run_steps(RefineStep(stock_dec, **kw), frames, valid)
    ref, _ = run_steps(RefineStep(dec64, **kw), frames, valid, torch.float64)
    assert st.n_obj == 5 and ((st.thid is None) if kw.get("only_spatial") else len(st) == 5)
    tag = "step" + "".join("_" + k for k in kw)
    for t in range(T):
        held(f"{tag}/t{t}/outs", fused[t][0], stock[t][0], ref[t][0], slack_ulp=False)
        held(f"{tag}/t{t}/mask_hist_new", fused[t][1], stock[t][1], ref[t][1], slack_ulp=False)
        assert float(fused[t][0].view(B, O, -1)[:, 5:].abs().max()) == 0.0          # rows beyond n_obj
        hist_in = frames[t][4]
        dead = (valid == 0)
        assert torch.equal(fused[t][1][dead], hist_in[dead])                        # invalid pairs: bit-unchanged


def test_refine_step_graph_replay_equals_eager_without_syncs():
    B, O, H, W, hidden, T = 2, 4, 95, 130, 32, 5
    torch.manual_seed(21)
    dec = RSISMask(make_args("concat", hidden=hidden)).eval().to(DEV)
    valid = torch.tensor([[1, 1, 1, 0], [1, 0, 1, 0]], device=DEV)
    frames = step_inputs(22, B, O, H, W, hidden, T)
    eager, _ = run_steps(RefineStep(dec), frames, valid)
    step = RefineStep(dec)
    static = [tuple(x.clone() for x in frames[0][0]["refine_input_feat"])] + [x.clone() for x in frames[0][1:]]

    def load(t):
        for d, s in zip(static[0], frames[t][0]["refine_input_feat"]):
            d.copy_(s)
        for d, s in zip(static[1:], frames[t][1:]):
            d.copy_(s)

    def call(state):
        return step({"refine_input_feat": static[0]}, static[1], static[2], static[3], static[4], valid, state)

    with torch.no_grad():
        state = None
        for t in range(2):                                               # frame 0 (reads n_obj), frame 1 (temporal path)
            load(t)
            outs, hist, state = call(state)
            assert torch.equal(outs, eager[t][0]) and torch.equal(hist, eager[t][1])
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs, hist, state2 = call(state)
        assert state2.n_obj == state.n_obj
        torch.cuda.set_sync_debug_mode("error")
        try:
            kept = []
            for t in range(2, T):
                load(t)
                graph.replay()
                kept.append((outs.clone(), hist.clone()))
        finally:
            torch.cuda.set_sync_debug_mode("default")
        for t, (o, h) in zip(range(2, T), kept):
            assert torch.equal(o, eager[t][0]) and torch.equal(h, eager[t][1]), t
        # and the eager fused step itself issues no sync after frame 0
        step2, st = RefineStep(dec), None
        f0 = frames[0]
        _, _, st = step2(f0[0], f0[1], f0[2], f0[3], f0[4].clone(), valid, None)
        clones = [f[4].clone() for f in frames]
        torch.cuda.set_sync_debug_mode("error")
        try:
            for t in range(1, T):
                f = frames[t]
                _, _, st = step2(f[0], f[1], f[2], f[3], clones[t], valid, st)
        finally:
            torch.cuda.set_sync_debug_mode("default")


def test_one_chain_convolution_per_level_and_object():
    """Launch accounting of one steady-state frame: per object 4 chain convolutions (the stock form evaluates the cell's
    convolution 3 x 4 times per object), 4 hoisted + 4 batched temporal + 1 conv_out per frame; library launches: 1 pyramid
    + per object 4 gates + 3 upsamples, + 1 upsample + 1 finish."""
    B, O, H, W, hidden = 2, 4, 95, 130, 32
    torch.manual_seed(31)
    dec = RSISMask(make_args("concat", hidden=hidden)).eval().to(DEV)
    valid = torch.ones(B, O, dtype=torch.long, device=DEV)
    frames = step_inputs(32, B, O, H, W, hidden, 2)
    step = RefineStep(dec)
    with torch.no_grad():
        f = frames[0]
        _, _, st = step(f[0], f[1], f[2], f[3], f[4], valid, None)
        torch.cuda.synchronize()
        c0, l0 = dec.conv_calls, int(_lib.load().dmm_launch_count())
        f = frames[1]
        step(f[0], f[1], f[2], f[3], f[4], valid, st)
        convs, launches = dec.conv_calls - c0, int(_lib.load().dmm_launch_count()) - l0
    n = O
    chain = convs - (4 + 4 + 1)
    record_achieved("decoder/launches/convs_per_frame", convs)
    record_achieved("decoder/launches/kernels_per_frame", launches)
    assert chain == 4 * n - 1, (convs, chain)            # object 0 has no spatial state at level 0: no chain term there
    assert launches == 1 + n * (4 + 3) + 1 + 1, launches


# ---- the frame loop with the decoder plugged in --------------------------------------------------------------------------
class _ToyEncoder:
    """Batch-independent toy encoder: pooled grey image times per-channel gains; backbone levels at strides 4..32 and the
    decoder's four skip maps (strides 32..4, hidden / hidden / hidden/2 / hidden/4 channels)."""

    def __init__(self, hidden, C=8):
        self.mul = torch.linspace(0.5, 1.5, C, device=DEV).view(1, C, 1, 1)
        self.gain = [torch.linspace(-1.0, 1.0, c, device=DEV).view(1, c, 1, 1) for c in (hidden, hidden, hidden // 2, hidden // 4)]

    def __call__(self, x):
        g = x.mean(1, keepdim=True)
        lv = tuple(F.avg_pool2d(g, s, ceil_mode=True) * self.mul for s in (4, 8, 16, 32))
        sk = tuple(torch.sin(3 * F.avg_pool2d(g, s, ceil_mode=True) * (1 + gn.abs())) * gn
                   for s, gn in zip((32, 16, 8, 4), self.gain))
        return {"backbone_feature": lv, "refine_input_feat": sk}


def _raw_proposals(rng, n, H, W):
    from dmm_net_amd import proposals as prop
    x1, y1 = rng.uniform(0, W - 24, n), rng.uniform(0, H - 24, n)
    boxes = np.stack([x1, y1, np.minimum(x1 + rng.uniform(10, 60, n), W - 1), np.minimum(y1 + rng.uniform(10, 50, n), H - 1)], 1)
    bl = prop.SimpleBoxList(torch.from_numpy(boxes.astype(np.float32)), (W, H))
    bl.add_field("scores", torch.from_numpy(rng.random(n).astype(np.float32)))
    bl.add_field("mask", torch.from_numpy((rng.random((n, 1, 28, 28)) * 0.6 + 0.4).astype(np.float32)))
    return bl


def test_frame_loop_with_the_decoder_fused_against_stock():
    from dmm_net_amd.dmm_model import DMM_Model
    from dmm_net_amd.roi_features import FeatureExtractor
    rng = np.random.default_rng(41)
    B, T, O, H, W, hidden = 2, 4, 4, 96, 128, 32
    cfgs = {"matching": {"algo": "relax"}, "relax_max_iter": 40, "relax_proj_iter": 5, "relax_learning_rate": 0.1,
            "score_weight": 0.3}
    frames = torch.randn(B, T, 3, H, W, device=DEV)
    n_obj = [3, 2]
    props = [[_raw_proposals(rng, 30 + 5 * b + t, H, W) for t in range(T)] for b in range(B)]
    first = torch.zeros(B, O, H, W, device=DEV)
    for b in range(B):
        for o in range(n_obj[b]):
            y0, x0 = int(rng.integers(0, H - 30)), int(rng.integers(0, W - 30))
            first[b, o, y0:y0 + 25, x0:x0 + 28] = 1.0
    first = first.view(B, O, H * W)
    torch.manual_seed(42)
    dec = RSISMask(make_args("concat", hidden=hidden)).eval().to(DEV)
    with torch.no_grad():
        dec.conv_out.weight.mul_(20)                                     # default weights leave every logit within +-0.3
    stock_dec = copy.deepcopy(dec)
    stock_dec.fused = False

    class Refine64:
        """The stock step evaluated in fp64 inside the same loop; its fp64 ``outs`` are kept, the loop gets them rounded."""

        def __init__(self):
            self.step, self.outs = RefineStep(copy.deepcopy(stock_dec).double()), []

        def __call__(self, features, pm, ym, ip, hist, valid, state):
            f = {"refine_input_feat": tuple(x.double() for x in features["refine_input_feat"])}
            outs, hn, st = self.step(f, pm.double(), ym.double(), ip.double(), hist.double(), valid, state)
            self.outs.append(outs.clone())
            return outs.float(), hn.float(), st

    def run(refine):
        labels = {}
        lp = video.FrameLoop(_ToyEncoder(hidden), DMM_Model(cfgs, is_test=1, feature_extractor=FeatureExtractor()),
                             refine=refine, nms_thresh=0.4, max_proposals=20)
        hist = lp.run(frames, first, props, on_labels=lambda b, t, lab: labels.__setitem__((b, t), lab.clone()))
        return [h.clone() for h in hist], labels

    c0 = dec.conv_calls
    fh, fl = run(RefineStep(dec))
    assert dec.conv_calls > c0
    sh, sl = run(RefineStep(stock_dec))
    r64 = Refine64()
    run(r64)
    left_out = total = 0
    for t in range(T):
        if t > 0:                                                        # (frame 0 reports the annotation)
            held(f"frame_loop/t{t}/outs", fh[t], sh[t], r64.outs[t].view(B, O, H * W), slack_ulp=False)
        for b in range(B):
            m = sh[t][b, :n_obj[b]].view(n_obj[b], H * W)
            allv = torch.cat([(1 - m.max(0)[0])[None], m], 0)
            top2 = allv.topk(2, 0)[0]
            sure = (top2[0] - top2[1]) > 1e-4
            left_out += int((~sure).sum())
            total += H * W
            assert torch.equal(fl[(b, t)].view(-1)[sure], sl[(b, t)].view(-1)[sure]), (b, t)
    record_achieved("decoder/frame_loop/pixels_left_out", left_out / total)
    print(f"label pixels left out: {left_out} of {total}")
    assert left_out <= 0.01 * total
