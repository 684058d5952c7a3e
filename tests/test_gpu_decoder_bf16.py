"""The refine decoder's bf16 form on the GPU (``RSISMask.compute_dtype = torch.bfloat16``; include/dmm_match.h (12i)-(12k)).

The kernels: a 16-bit entry widens every 16-bit value on load, evaluates its fp32 sibling's expressions in the same order and
rounds every 16-bit output once, so ``entry_bf16(x) == entry_f32(x.float())`` -- 16-bit outputs after ``.to(bfloat16)``, fp32
outputs as they are -- BIT FOR BIT: no tolerance.  In every kernel case at least one 16-bit operand sits at a base that is only
2-byte aligned (one element sliced off a larger allocation), and the three entries run between guard bands at their smallest
shapes.

The module: the yardstick is the stock torch decoder run in bf16 on the same (bf16-rounded) inputs; both are held against an
fp64 evaluation of those inputs by the rule of test_gpu_decoder.py without its ulp slack: with e_stock16 = max|stock16 - ref64|,
max|got - ref64| <= 2 * e_stock16.  Both are 16-bit evaluations of the same expression in another rounding order (the fused form
rounds up to three convolution addends separately where the stock form rounds their sum once; it keeps the gate arithmetic and
the cell in fp32 where the stock form rounds after every op).  Every achieved pair is recorded under ``decoder_bf16/``."""
import copy

import numpy as np
import pytest
import torch

from conftest import record_achieved
from dmm_net_amd import _lib, decoder as D, video
from dmm_net_amd.decoder import RSISMask, RefineState, RefineStep, pyramid_sizes
from test_decoder_cpu import CASES, case_inputs, flat_outputs, load_decoder, make_args
from test_gpu_guard_bands import run_row

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16


def odd(t):
    """``t``'s values in a tensor of its shape whose base is only 2-byte (bf16) / 4-byte (fp32) aligned: one leading element
    sliced off a larger allocation."""
    big = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = big[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % (2 * t.element_size()) == t.element_size()
    return v


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def held16(name, got, stock16, ref64):
    """max|got - ref64| <= 2 * max|stock16 - ref64|: no floor, no ulp slack."""
    err = float((got.double() - ref64).abs().max())
    e_stock16 = float((stock16.double() - ref64).abs().max())
    print(f"{name}: err {err:.3e}  e_stock16 {e_stock16:.3e}  ratio {err / e_stock16 if e_stock16 else float('nan'):.3f}")
    record_achieved(f"decoder_bf16/{name}/err", err)
    record_achieved(f"decoder_bf16/{name}/e_stock16", e_stock16)
    assert err <= 2 * e_stock16, (name, err, e_stock16)


# ---- 1. each kernel against its fp32 sibling, bit for bit -----------------------------------------------------------------------
GATES = [(3, 6, 5, 7, 1, False), (1, 16, 24, 33, 2, True), (2, 32, 8, 14, 3, True)]


def gates_inputs(B, Hd, h, w, n_pre, with_cell, gen=None):
    r = lambda *s: torch.randn(s, device=DEV, generator=gen)
    pre = [r(B, 4 * Hd, h, w).to(BF16) for _ in range(n_pre)]
    masks = torch.rand((B, 3, h, w), device=DEV, generator=gen)
    w_mask = r(4 * Hd, 9) * 0.3
    cell_prev = r(B, Hd, h, w) if with_cell else None
    wide = r(B, Hd + 3, h, w).to(BF16)
    return pre, masks, w_mask, cell_prev, wide


@pytest.mark.parametrize("B,Hd,h,w,n_pre,with_cell", GATES)
def test_clstm_gates_bf16_equals_fp32_on_widened_inputs(B, Hd, h, w, n_pre, with_cell):
    torch.manual_seed(2)
    pre, masks, w_mask, cell_prev, wide0 = gates_inputs(B, Hd, h, w, n_pre, with_cell)
    pre16 = [odd(p) for p in pre]
    hidden16, cell16 = odd(torch.empty((B, Hd, h, w), dtype=BF16, device=DEV)), torch.empty((B, Hd, h, w), device=DEV)
    wide16 = odd(wide0)                                                   # hidden_copy: the upper channels of a wider tensor
    D.clstm_gates(pre16, masks, w_mask, cell_prev, hidden16, cell16, hidden_copy=wide16[:, 3:])
    hidden32, cell32 = torch.empty((B, Hd, h, w), device=DEV), torch.empty((B, Hd, h, w), device=DEV)
    wide32 = wide0.float()
    D.clstm_gates([p.float() for p in pre], masks, w_mask, cell_prev, hidden32, cell32, hidden_copy=wide32[:, 3:])
    assert same(hidden16, hidden32.to(BF16))
    assert same(cell16, cell32)                                           # the cell stays fp32: the very bits
    assert same(wide16[:, 3:], hidden16) and same(wide16[:, :3], wide0[:, :3])   # the lower channels: bit-unchanged
    assert torch.equal(wide32[:, 3:], hidden32)
    assert bool(torch.isfinite(hidden32).all()) and float(hidden32.abs().max()) > 0


UPSAMPLE = [(2, 3, 1, 4, 7, 9), (2, 5, 3, 5, 6, 9), (1, 16, 24, 33, 48, 66)]


@pytest.mark.parametrize("mode", ["write", "add", "mul"])
@pytest.mark.parametrize("shape", UPSAMPLE)
def test_upsample_bilinear_into_bf16_equals_fp32_on_widened_inputs(mode, shape):
    B, C, h, w, H, W = shape
    torch.manual_seed(3)
    src = torch.randn(B, C, h, w, device=DEV).to(BF16)
    c0, Cd = 2, C + 5
    base = torch.randn(B, Cd, H, W, device=DEV).to(BF16)
    dst16 = odd(base)
    D.upsample_bilinear_into(odd(src), dst16, c0, mode)
    dst32 = base.float()
    D.upsample_bilinear_into(src.float(), dst32, c0, mode)
    assert same(dst16[:, c0:c0 + C], dst32[:, c0:c0 + C].to(BF16))
    assert same(dst16[:, :c0], base[:, :c0]) and same(dst16[:, c0 + C:], base[:, c0 + C:])   # the other channels: bit-unchanged
    assert not same(dst16[:, c0:c0 + C], base[:, c0:c0 + C])


FINISH = [(1, 2, 2, 2, 2, 5, 7), (2, 4, 3, 24, 34, 47, 66)]


def finish_inputs(B, O, n_obj, h, w, H, W, gen=None):
    logits = (torch.randn((n_obj * B, 1, h, w), device=DEV, generator=gen) * 3).to(BF16)
    valid = torch.ones((B, O), dtype=torch.int32, device=DEV)
    valid[B - 1, n_obj - 1] = 0                                           # one invalid (video, object) pair
    hist0 = torch.rand((B, O, H, W), device=DEV, generator=gen)
    return logits, valid, hist0


@pytest.mark.parametrize("with_hist", [True, False])
@pytest.mark.parametrize("shape", FINISH)
def test_refine_finish_bf16_equals_fp32_on_widened_inputs(shape, with_hist):
    B, O, n_obj, h, w, H, W = shape
    torch.manual_seed(4)
    logits, valid, hist0 = finish_inputs(*shape)
    view = lambda t: t.view(n_obj, B, h, w).transpose(0, 1)               # the strided [B, n_obj] view RefineStep passes
    res = []
    for lg in (view(odd(logits)), view(logits.float())):
        outs = torch.full((B, O, H, W), 7.0, device=DEV)
        hist = hist0.clone() if with_hist else None
        D.refine_finish(lg, valid if with_hist else None, outs, hist, n_obj)
        res.append((outs, hist))
    (o16, h16), (o32, h32) = res
    assert same(o16, o32)
    assert float(o16[:, n_obj:].abs().max()) == 0.0 if n_obj < O else True       # rows t >= n_obj are zero
    assert float(o16[:, :n_obj].min()) >= 0.0 and float(o16[:, :n_obj].max()) <= 1.0 and float(o16[:, :n_obj].max()) > 0.0
    if with_hist:
        assert same(h16, h32)
        keep = (valid[:, :n_obj] != 0).view(B, n_obj, 1, 1)
        assert torch.equal(h16[:, :n_obj], torch.where(keep, o16[:, :n_obj], hist0[:, :n_obj]))
        assert torch.equal(h16[:, n_obj:], hist0[:, n_obj:])
        assert torch.equal(h16[B - 1, n_obj - 1], hist0[B - 1, n_obj - 1])


def test_launchers_refuse_mixed_dtypes():
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=DEV)
    pre16, pre32, masks, wm = z(1, 8, 3, 4, dt=BF16), z(1, 8, 3, 4), z(1, 3, 3, 4), z(8, 9)
    hid16, hid32, cell = z(1, 2, 3, 4, dt=BF16), z(1, 2, 3, 4), z(1, 2, 3, 4)
    for args in ((([pre32], masks, wm, None, hid16, cell), {}), (([pre16], masks, wm, None, hid32, cell), {}),
                 (([pre16], masks, wm, None, hid16, hid16.clone()), {}), (([pre16], masks.to(BF16), wm, None, hid16, cell), {}),
                 (([pre16], masks, wm, cell.to(BF16), hid16, cell), {}), (([pre16], masks, wm, None, hid16, cell), {"hidden_copy": hid32}),
                 (([pre16.half()], masks, wm, None, hid16.half(), cell), {})):
        with pytest.raises(_lib.DmmError):
            D.clstm_gates(*args[0], **args[1])
    with pytest.raises(_lib.DmmError):
        D.upsample_bilinear_into(z(1, 2, 3, 4, dt=BF16), z(1, 2, 6, 8))
    with pytest.raises(_lib.DmmError):
        D.upsample_bilinear_into(z(1, 2, 3, 4, dt=torch.float16), z(1, 2, 6, 8, dt=torch.float16))
    with pytest.raises(_lib.DmmError):
        D.refine_finish(z(1, 2, 3, 4, dt=torch.float16), None, z(1, 2, 6, 8), None, 2)


# ---- 2. the same three entries between guard bands --------------------------------------------------------------------------------
def test_clstm_gates_bf16_between_bands():
    B, Hd, h, w, n_pre, with_cell = GATES[0]
    gen = torch.Generator(device=DEV).manual_seed(2)
    pre, masks, w_mask, cell_prev, _ = gates_inputs(B, Hd, h, w, n_pre, with_cell, gen)

    def call(m, wm, *pres):
        hidden, cell = torch.empty((B, Hd, h, w), dtype=BF16, device=DEV), torch.empty((B, Hd, h, w), device=DEV)
        wide = torch.zeros((B, Hd + 3, h, w), dtype=BF16, device=DEV)
        D.clstm_gates(list(pres), m, wm, None, hidden, cell, hidden_copy=wide[:, 3:])
        return [hidden, cell, wide]
    run_row(f"decoder_bf16/gates_{B}x{Hd}x{h}x{w}", lambda wr: (wr(masks), wr(w_mask)) + tuple(wr(p) for p in pre), call)


@pytest.mark.parametrize("mode", ["write", "add", "mul"])
def test_upsample_bilinear_into_bf16_between_bands(mode):
    B, C, h, w, H, W = UPSAMPLE[0]
    gen = torch.Generator(device=DEV).manual_seed(3)
    src = torch.randn((B, C, h, w), generator=gen, device=DEV).to(BF16)
    base = torch.randn((B, C + 5, H, W), generator=gen, device=DEV).to(BF16)

    def call(s, b):
        out = []
        for c0 in (2, 5):                                                 # the last slice included (c0 + C = C')
            dst = torch.empty_like(b)
            dst.copy_(b)
            out.append(D.upsample_bilinear_into(s, dst, c0, mode))
        return out
    run_row(f"decoder_bf16/upsample_{mode}_{h}x{w}_to_{H}x{W}", lambda wr: (wr(src), wr(base)), call)


def test_refine_finish_bf16_between_bands():
    B, O, n_obj, h, w, H, W = FINISH[0]
    gen = torch.Generator(device=DEV).manual_seed(4)
    logits, valid, hist0 = finish_inputs(B, O, n_obj, h, w, H, W, gen)
    logits = logits.view(n_obj, B, h, w).transpose(0, 1)

    def call(lg, v, h0):
        outs = torch.full((B, O, H, W), 7.0, device=DEV)
        hist = torch.empty_like(h0)
        hist.copy_(h0)
        D.refine_finish(lg, v, outs, hist, n_obj)
        outs2 = torch.full((B, O, H, W), 7.0, device=DEV)
        D.refine_finish(lg, None, outs2, None, n_obj)
        return [outs, hist, outs2]
    run_row(f"decoder_bf16/finish_{h}x{w}_to_{H}x{W}", lambda wr: (wr(logits), wr(valid, 1), wr(hist0)), call)


# ---- 3. RSISMask.forward on the reference fixture ---------------------------------------------------------------------------------
def rounded_inputs(args):
    """(feats, masks, spatial, temporal) fp32 -> the bf16 form's operand set (maps and hiddens bf16; masks and cells fp32), the
    all-bf16 set of the stock yardstick and the fp64 widening of the first: the same numbers except the masks and cells the
    stock form has to round."""
    feats, masks, spatial, temporal = args
    r = lambda t: t.to(BF16)
    low = ([r(f) for f in feats], masks, None if spatial is None else [[r(h), c] for h, c in spatial],
           None if temporal is None else [r(t) for t in temporal])
    all16 = (low[0], [r(m) for m in masks], None if spatial is None else [[h, r(c)] for h, c in low[2]], low[3])
    d = lambda t: t.double()
    wide = ([d(f) for f in low[0]], [d(m) for m in masks], None if spatial is None else [[d(h), d(c)] for h, c in low[2]],
            None if temporal is None else [d(t) for t in low[3]])
    return low, all16, wide


@pytest.mark.parametrize("mode", ["concat", "sum"])
@pytest.mark.parametrize("case", list(CASES))
def test_bf16_fused_forward_against_the_reference_fixture(mode, case):
    dec, g = load_decoder(mode, DEV)
    dec16 = copy.deepcopy(dec).to(BF16)                                   # the yardstick: the stock torch decoder in bf16
    dec64 = copy.deepcopy(dec).double()
    dec.compute_dtype = BF16
    with torch.no_grad():
        low, all16, wide = rounded_inputs(case_inputs(g, mode, case, DEV))
        assert dec._route(low[0] + low[1]) == "fused"
        n0, l0 = dec.conv_calls, int(_lib.load().dmm_launch_count())
        res = dec(*low)
        assert dec.conv_calls > n0 and int(_lib.load().dmm_launch_count()) - l0 == 4 + 3 + 1      # the fused form ran
        out_mask, hidden_list = res
        assert out_mask.dtype == BF16 and all(h.dtype == BF16 and c.dtype == torch.float32 for h, c in hidden_list)
        got = flat_outputs(res)
        stock16 = flat_outputs(dec16.forward_stock(*all16))
        ref64 = flat_outputs(dec64.forward_stock(*wide))
    for k in got:
        held16(f"fixture/{mode}/{case}/{k}", got[k], stock16[k], ref64[k])


def test_bf16_forward_names_a_wrong_operand_set():
    dec, g = load_decoder("concat", DEV)
    dec.compute_dtype = BF16
    with torch.no_grad():
        args = case_inputs(g, "concat", "st", DEV)
        with pytest.raises(_lib.DmmError, match="bfloat16 skip maps"):
            dec(*args)                                                    # fp32 maps with bf16 set: named, not guessed
        low, all16, _ = rounded_inputs(args)
        with pytest.raises(_lib.DmmError, match="float32 mask planes"):
            dec(*all16)


# ---- 4. RefineStep over chained frames ------------------------------------------------------------------------------------------
STEP = dict(B=2, O=3, H=47, W=66, hidden=16)
VALID = [[1, 1, 1], [1, 0, 1]]                                            # 3 objects, one invalid (video, object) pair


def step_frames(seed, T, B, O, H, W, hidden):
    g = torch.Generator(device="cpu").manual_seed(seed)
    sizes = pyramid_sizes(H, W)
    ch = [hidden, hidden, hidden // 2, hidden // 4]
    frames = []
    for _ in range(T):
        feats = tuple(torch.randn((B, c) + s, generator=g).to(DEV).to(BF16) for c, s in zip(ch, sizes))
        frames.append((feats, (torch.rand(B, O, H * W, generator=g) > 0.6).float().to(DEV),
                       (torch.rand(B, O, H * W, generator=g) > 0.6).float().to(DEV),
                       torch.rand(B, O, H, W, generator=g).to(DEV), torch.rand(B, O, H, W, generator=g).to(DEV)))
    return frames


def step_decoder(seed, hidden):
    torch.manual_seed(seed)
    dec = RSISMask(make_args("concat", hidden=hidden)).eval().to(DEV)
    with torch.no_grad():
        dec.conv_out.weight.mul_(10)                                      # default weights leave every logit near zero
    return dec


def run_bf16(step, frames, valid):
    state, res = None, []
    with torch.no_grad():
        for feats, pm, ym, ip, hist in frames:
            outs, hist_new, state = step({"refine_input_feat": feats}, pm, ym, ip, hist.clone(), valid, state)
            res.append((outs.clone(), hist_new.clone()))
    return res, state


def run_stock16(step, frames, valid, n_obj):
    """The evaluator's loop on the bf16 stock decoder: ``RefineStep._stock`` with bf16 maps (it rounds the masks itself)."""
    B, O, H, W = (STEP[k] for k in "BOHW")
    state, res = RefineState(n_obj), []
    with torch.no_grad():
        for feats, pm, ym, ip, hist in frames:
            outs, hist_new, state = step._stock(list(feats), pm, ym, ip, hist.clone(), valid, state, n_obj, B, O, H, W)
            res.append((outs.clone(), hist_new.clone()))
    return res


def run_ref64(step, frames, valid):
    state, res = None, []
    with torch.no_grad():
        for feats, pm, ym, ip, hist in frames:
            f = {"refine_input_feat": tuple(x.double() for x in feats)}
            outs, hist_new, state = step(f, pm.double(), ym.double(), ip.double(), hist.double(), valid, state)
            res.append((outs.clone(), hist_new.clone()))
    return res


@pytest.mark.parametrize("kw", [{}, {"only_spatial": True}, {"only_temporal": True}])
def test_refine_step_bf16_against_the_bf16_stock_decoder(kw):
    B, O, H, W, hidden, T = STEP["B"], STEP["O"], STEP["H"], STEP["W"], STEP["hidden"], 3
    dec = step_decoder(11, hidden)
    stock = copy.deepcopy(dec)
    stock.fused = False
    dec16, dec64 = copy.deepcopy(stock).to(BF16), copy.deepcopy(stock).double()
    dec.compute_dtype = BF16
    valid = torch.tensor(VALID, device=DEV)
    frames = step_frames(12, T, B, O, H, W, hidden)
    c0 = dec.conv_calls
    fused, st = run_bf16(RefineStep(dec, **kw), frames, valid)
    assert dec.conv_calls > c0                                            # the fused form ran
    stock16 = run_stock16(RefineStep(dec16, **kw), frames, valid, 3)
    ref64 = run_ref64(RefineStep(dec64, **kw), frames, valid)
    assert st.n_obj == 3
    if kw.get("only_spatial"):
        assert st.thid is None
    else:
        assert len(st) == 3 and all(h.dtype == BF16 for hs in st.thid for h in hs)       # the temporal state is bf16
    tag = "step" + "".join("_" + k for k in kw)
    dead = (valid == 0)
    for t in range(T):
        assert fused[t][0].dtype == torch.float32 and fused[t][1].dtype == torch.float32
        held16(f"{tag}/t{t}/outs", fused[t][0], stock16[t][0], ref64[t][0])
        held16(f"{tag}/t{t}/mask_hist_new", fused[t][1], stock16[t][1], ref64[t][1])
        assert torch.equal(fused[t][1][dead], frames[t][4][dead])         # invalid pairs: bit-unchanged
    O_big = O + 1                                                         # rows beyond n_obj: exactly zero
    frames4 = step_frames(13, 1, B, O_big, H, W, hidden)
    valid4 = torch.tensor([v + [0] for v in VALID], device=DEV)
    wide, st4 = run_bf16(RefineStep(dec, **kw), frames4, valid4)
    assert st4.n_obj == 3 and float(wide[0][0].view(B, O_big, -1)[:, 3:].abs().max()) == 0.0
    assert float(wide[0][0].view(B, O_big, -1)[:, :3].abs().max()) > 0.0


# ---- 5. graph capture ---------------------------------------------------------------------------------------------------------------
def test_refine_step_bf16_graph_replay_equals_eager_without_syncs():
    B, O, H, W, hidden, T = STEP["B"], STEP["O"], STEP["H"], STEP["W"], STEP["hidden"], 5
    dec = step_decoder(21, hidden)
    dec.compute_dtype = BF16
    valid = torch.tensor(VALID, device=DEV)
    frames = step_frames(22, T, B, O, H, W, hidden)
    eager, _ = run_bf16(RefineStep(dec), frames, valid)
    step = RefineStep(dec)
    static = [tuple(x.clone() for x in frames[0][0])] + [x.clone() for x in frames[0][1:]]

    def load(t):
        for d, s in zip(static[0], frames[t][0]):
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
        assert state2.n_obj == state.n_obj and all(h.dtype == BF16 for hs in state2.thid for h in hs)
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
        # and the eager bf16 step itself issues no sync after frame 0
        step2 = RefineStep(dec)
        f0 = frames[0]
        _, _, st = step2({"refine_input_feat": f0[0]}, f0[1], f0[2], f0[3], f0[4].clone(), valid, None)
        clones = [f[4].clone() for f in frames]
        torch.cuda.set_sync_debug_mode("error")
        try:
            for t in range(1, T):
                f = frames[t]
                _, _, st = step2({"refine_input_feat": f[0]}, f[1], f[2], f[3], clones[t], valid, st)
        finally:
            torch.cuda.set_sync_debug_mode("default")


# ---- 6. counts and routing -------------------------------------------------------------------------------------------------------------
def test_bf16_step_counts_equal_the_fp32_forms_and_routing():
    B, O, H, W, hidden = STEP["B"], STEP["O"], STEP["H"], STEP["W"], STEP["hidden"]
    dec32 = step_decoder(31, hidden)
    dec16 = copy.deepcopy(dec32)
    dec16.compute_dtype = BF16
    valid = torch.ones(B, O, dtype=torch.long, device=DEV)
    frames = step_frames(32, 2, B, O, H, W, hidden)
    counts = {}
    with torch.no_grad():
        for name, dec in (("fp32", dec32), ("bf16", dec16)):
            step = RefineStep(dec)
            maps = lambda f: {"refine_input_feat": f[0] if name == "bf16" else tuple(x.float() for x in f[0])}
            f = frames[0]
            _, _, st = step(maps(f), f[1], f[2], f[3], f[4].clone(), valid, None)
            torch.cuda.synchronize()
            c0, l0 = dec.conv_calls, int(_lib.load().dmm_launch_count())
            f = frames[1]
            m = maps(f)
            step(m, f[1], f[2], f[3], f[4].clone(), valid, st)
            counts[name] = (dec.conv_calls - c0, int(_lib.load().dmm_launch_count()) - l0)
    record_achieved("decoder_bf16/launches/convs_per_frame", counts["bf16"][0])
    record_achieved("decoder_bf16/launches/kernels_per_frame", counts["bf16"][1])
    assert counts["bf16"] == counts["fp32"] == (4 + 4 + 1 + 4 * O - 1, 1 + O * (4 + 3) + 1 + 1), counts
    f = frames[0]
    ts16 = list(f[0]) + [f[1], f[2], f[3], f[4]]                          # the bf16 operand set: bf16 maps, fp32 planes
    with torch.no_grad():
        assert dec16.fused_ok(ts16) and not dec32.fused_ok(ts16)
        assert dec32.fused_ok([x.float() for x in ts16]) and dec16._route(ts16) == "fused"
        assert not dec16.fused_ok([x.half() for x in f[0]] + [f[1]])      # fp16 is not taken
    assert dec16._route(ts16) == dec32._route(ts16) == "stock"            # a gradient is required (the parameters'):
    dec16.fused_train = dec32.fused_train = True                          # compute_dtype is ignored, the routes are today's
    assert dec16._route(ts16) == dec32._route(ts16) == "stock"
    ts32 = [x.float() for x in ts16]
    assert dec16._route(ts32) == dec32._route(ts32) == "train"


# ---- 7. one FrameLoop run ----------------------------------------------------------------------------------------------------------------
def test_frame_loop_with_a_bf16_encoder_and_the_bf16_decoder():
    from dmm_net_amd.dmm_model import DMM_Model
    from dmm_net_amd.roi_features import FeatureExtractor
    from test_gpu_decoder import _ToyEncoder, _raw_proposals
    rng = np.random.default_rng(41)
    B, T, O, H, W, hidden = 2, 3, 3, 64, 96, 16
    cfgs = {"matching": {"algo": "relax"}, "relax_max_iter": 40, "relax_proj_iter": 5, "relax_learning_rate": 0.1,
            "score_weight": 0.3}
    frames = torch.randn(B, T, 3, H, W, device=DEV)
    props = [[_raw_proposals(rng, 20 + 3 * b + t, H, W) for t in range(T)] for b in range(B)]
    first = torch.zeros(B, O, H, W, device=DEV)
    for b, n in enumerate((3, 2)):
        for o in range(n):
            y0, x0 = int(rng.integers(0, H - 30)), int(rng.integers(0, W - 30))
            first[b, o, y0:y0 + 25, x0:x0 + 28] = 1.0
    first = first.view(B, O, H * W)
    dec = step_decoder(42, hidden)
    dec.compute_dtype = BF16
    toy = _ToyEncoder(hidden)

    def encoder(x):                                                       # a stub encoder handing out bf16 skip maps
        out = toy(x)
        out["refine_input_feat"] = tuple(f.to(BF16) for f in out["refine_input_feat"])
        return out

    class Recorder:
        def __init__(self):
            self.step, self.seen = RefineStep(dec), []

        def __call__(self, features, *rest):
            assert all(f.dtype == BF16 for f in features["refine_input_feat"])
            outs, hist_new, state = self.step(features, *rest)
            self.seen.append((outs.clone(), [h.dtype for hs in state.thid for h in hs]))
            return outs, hist_new, state

    rec = Recorder()
    c0 = dec.conv_calls
    lp = video.FrameLoop(encoder, DMM_Model(cfgs, is_test=1, feature_extractor=FeatureExtractor()), refine=rec,
                         nms_thresh=0.4, max_proposals=20)
    hist = lp.run(frames, first, props)
    assert dec.conv_calls > c0 and len(rec.seen) >= T - 1                 # the fused bf16 form ran in the loop
    for outs, dts in rec.seen:
        assert outs.dtype == torch.float32 and bool(torch.isfinite(outs).all())
        assert float(outs.min()) >= 0.0 and float(outs.max()) <= 1.0 and float(outs.max()) > 0.0
        assert dts and all(d == BF16 for d in dts)
    for h in hist:
        assert bool(torch.isfinite(h).all()) and float(h.min()) >= 0.0 and float(h.max()) <= 1.0
