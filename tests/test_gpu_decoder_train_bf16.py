"""The refine decoder's bf16 TRAINING form on the GPU (``RSISMask.train_dtype = torch.bfloat16`` with ``fused_train``;
include/dmm_match.h (12l)-(12o)).

The kernels: a 16-bit entry widens every 16-bit value on load, evaluates its fp32 sibling's expressions in the same order and
rounds every 16-bit output once, so ``entry_bf16(x) == entry_f32(x.float())`` -- 16-bit outputs after ``.to(bfloat16)``, fp32
outputs as they are -- BIT FOR BIT: no tolerance.  In every kernel case at least one 16-bit operand sits at a base that is only
2-byte aligned, and every entry runs between guard bands.

The module and the step: the yardstick is ``held16`` of test_gpu_decoder_bf16.py -- the stock torch decoder in bf16 under torch
autograd on the same (bf16-rounded) inputs, both held against an fp64 autograd evaluation: max|got - ref64| <= 2 * max|stock16 -
ref64| per tensor, no floor, no ulp slack.  Every achieved pair is recorded under ``decoder_train_bf16/``."""
import copy
import itertools

import pytest
import torch

from conftest import record_achieved
from dmm_net_amd import _lib, decoder as D
from dmm_net_amd.decoder import RSISMask, RefineTrainStep
from test_decoder_cpu import CASES, case_inputs, flat_outputs, load_decoder
from test_gpu_decoder_bf16 import BF16, DEV, odd, rounded_inputs, same, step_decoder
from test_gpu_guard_bands import run_row
from test_refine_train_cpu import clip, run_clip, step_call

pytestmark = pytest.mark.gpu


def held16(name, got, stock16, ref64):
    """The rule of test_gpu_decoder_bf16.py's ``held16``: max|got - ref64| <= 2 * max|stock16 - ref64|, no floor, no slack."""
    err = float((got.double() - ref64).abs().max())
    e_stock16 = float((stock16.double() - ref64).abs().max())
    print(f"{name}: err {err:.3e}  e_stock16 {e_stock16:.3e}  ratio {err / e_stock16 if e_stock16 else float('nan'):.3f}")
    record_achieved(f"decoder_train_bf16/{name}/err", err)
    record_achieved(f"decoder_train_bf16/{name}/e_stock16", e_stock16)
    assert err <= 2 * e_stock16, (name, err, e_stock16)


def same_as_fp32(got, want, low):
    """``got`` (the bf16 entry's output) against ``want`` (the fp32 entry's on the widened inputs): a 16-bit output equals the
    fp32 one rounded, an fp32 output equals it as it is; None where None."""
    if got is None or want is None:
        return got is None and want is None
    return got.dtype == (BF16 if low else torch.float32) and same(got, want.to(BF16) if low else want)


# ---- 1. each kernel against its fp32 sibling, bit for bit -----------------------------------------------------------------------
CELL = [(3, 6, 5, 7, 1, False), (1, 16, 24, 33, 2, True), (2, 32, 8, 14, 3, True), (1, 1, 3, 3, 1, False), (1, 4, 1, 1, 1, True),
        (2, 8, 1, 9, 2, False)]
UPSTREAM = ("hc", "h", "c")                                              # d_hidden + d_cell, d_hidden only, d_cell only
LOW_OUT = (True, False, False, False)                                    # d_pre is 16-bit; d_cell_prev, d_masks, d_w_mask fp32


def cell_inputs(shape, seed=2, gen=None):
    B, Hd, h, w, n_pre, with_cell = shape
    if gen is None:
        gen = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s: torch.randn(s, device=DEV, generator=gen)
    pre = [r(B, 4 * Hd, h, w).to(BF16) for _ in range(n_pre)]
    masks = torch.rand((B, 3, h, w), device=DEV, generator=gen)
    w_mask = r(4 * Hd, 9) * 0.3
    cell_prev = r(B, Hd, h, w) if with_cell else None
    return pre, masks, w_mask, cell_prev, r(B, Hd, h, w).to(BF16), r(B, Hd, h, w)


def upstream(which, d_hidden, d_cell):
    return (d_hidden if "h" in which else None), (d_cell if "c" in which else None)


def widened(pre, d_hidden):
    return [p.float() for p in pre], None if d_hidden is None else d_hidden.float()


@pytest.mark.parametrize("which", UPSTREAM)
@pytest.mark.parametrize("shape", CELL)
def test_clstm_gates_bwd_bf16_equals_fp32_on_widened_inputs(shape, which):
    pre, masks, w_mask, cell_prev, d_hidden, d_cell = cell_inputs(shape)
    dh, dc = upstream(which, d_hidden, d_cell)
    pre32, dh32 = widened(pre, dh)
    pre16, dh16 = [odd(p) for p in pre], None if dh is None else odd(dh)
    for need in itertools.product((False, True), repeat=3):               # every subset of the wanted outputs
        if need[0] and cell_prev is None:
            continue
        got = D.clstm_gates_bwd(pre16, masks, w_mask, cell_prev, dh16, dc, need=need)
        want = D.clstm_gates_bwd(pre32, masks, w_mask, cell_prev, dh32, dc, need=need)
        assert [g is not None for g in got[1:]] == list(need)
        for name, g, wnt, low in zip(("d_pre", "d_cell_prev", "d_masks", "d_w_mask"), got, want, LOW_OUT):
            assert same_as_fp32(g, wnt, low), (need, name)
        assert bool(torch.isfinite(want[0]).all()) and float(want[0].abs().max()) > 0


UPSAMPLE = [(2, 3, 1, 4, 7, 9), (2, 5, 3, 5, 6, 9), (1, 16, 24, 33, 48, 66)]


def upsample_inputs(shape, c0, gen=None):
    """d_dst: [B, C', H, W] with C' = C for c0 == 0, else C + 5 (the channel range lies inside a wider tensor)."""
    B, C, h, w, H, W = shape
    if gen is None:
        gen = torch.Generator(device=DEV).manual_seed(3)
    return torch.randn((B, C if c0 == 0 else C + 5, H, W), device=DEV, generator=gen).to(BF16)


@pytest.mark.parametrize("c0", [0, 2])
@pytest.mark.parametrize("shape", UPSAMPLE)
def test_upsample_bilinear_bwd_bf16_equals_fp32_on_widened_inputs(shape, c0):
    B, C, h, w, H, W = shape
    d_dst = upsample_inputs(shape, c0)
    got = D.upsample_bilinear_bwd(odd(d_dst), c0, C, h, w)
    want = D.upsample_bilinear_bwd(d_dst.float(), c0, C, h, w)
    assert tuple(got.shape) == (B, C, h, w) and same_as_fp32(got, want, True)
    assert float(want.abs().max()) > 0


FINISH = [(1, 2, 2, 2, 2, 5, 7), (2, 4, 3, 24, 34, 47, 66)]


def finish_inputs(shape, gen=None):
    B, O, n_obj, h, w, H, W = shape
    if gen is None:
        gen = torch.Generator(device=DEV).manual_seed(4)
    logits = (torch.randn((n_obj * B, 1, h, w), device=DEV, generator=gen) * 3).to(BF16)
    return logits, torch.randn((B, O, H, W), device=DEV, generator=gen)


def obj_view(logits, shape):
    """conv_out's output for all objects as the step hands it over: the strided [B, n_obj] view."""
    B, O, n_obj, h, w, H, W = shape
    return logits.view(n_obj, B, h, w).transpose(0, 1)


@pytest.mark.parametrize("shape", FINISH)
def test_refine_train_finish_bf16_equals_fp32_on_widened_inputs(shape):
    B, O, n_obj, h, w, H, W = shape
    logits, d_outs = finish_inputs(shape)
    lg16, lg32 = obj_view(odd(logits), shape), obj_view(logits.float(), shape)
    assert B == 1 or not lg16.is_contiguous()
    o16, o32 = D.refine_train_finish(lg16, O, H, W), D.refine_train_finish(lg32, O, H, W)
    assert same_as_fp32(o16, o32, False)                                  # the probabilities are fp32: the very bits
    assert n_obj == O or float(o16[:, n_obj:].abs().max()) == 0.0
    assert float(o16[:, :n_obj].min()) >= 0.0 and float(o16[:, :n_obj].max()) <= 1.0 and float(o16[:, :n_obj].max()) > 0.0
    g16, g32 = D.refine_train_finish_bwd(lg16, d_outs), D.refine_train_finish_bwd(lg32, d_outs)
    assert tuple(g16.shape) == (B, n_obj, h, w) and same_as_fp32(g16, g32, True)
    assert float(g32.abs().max()) > 0
    # under autograd: bf16 logits, fp32 probabilities, a bf16 gradient
    leaf = lg16.detach().clone().requires_grad_(True)
    o = D.refine_train_finish_fn(leaf, O, H, W)
    (g,) = torch.autograd.grad(o, leaf, d_outs)
    assert o.dtype == torch.float32 and same(o, o16) and g.dtype == BF16 and same(g, g16)


def test_upsample_bilinear_fn_keeps_the_dtype_of_its_input():
    shape = UPSAMPLE[1]
    B, C, h, w, H, W = shape
    gen = torch.Generator(device=DEV).manual_seed(5)
    src = torch.randn((B, C, h, w), device=DEV, generator=gen).to(BF16)
    d_dst = upsample_inputs(shape, 0, gen)
    leaf = odd(src).requires_grad_(True)
    up = D.upsample_bilinear_fn(leaf, (H, W))
    dst = torch.empty((B, C, H, W), dtype=BF16, device=DEV)
    D.upsample_bilinear_into(src, dst, 0, "write")
    (g,) = torch.autograd.grad(up, leaf, d_dst)
    assert up.dtype == BF16 and same(up, dst) and g.dtype == BF16 and same(g, D.upsample_bilinear_bwd(d_dst, 0, C, h, w))
    leaf32 = src.float().requires_grad_(True)                             # fp32 in: fp32 out, as before
    assert D.upsample_bilinear_fn(leaf32, (H, W)).dtype == torch.float32


# ---- 2. repeatability and batch independence -------------------------------------------------------------------------------------
def test_backward_entries_three_calls_are_bit_identical():
    for shape in CELL:
        pre, masks, w_mask, cell_prev, d_hidden, d_cell = cell_inputs(shape)
        need = (cell_prev is not None, True, True)
        runs = [D.clstm_gates_bwd([odd(p) for p in pre], masks, w_mask, cell_prev, d_hidden, d_cell, need=need) for _ in range(3)]
        for other in runs[1:]:
            assert all((a is None and b is None) or same(a, b) for a, b in zip(runs[0], other)), shape
    for shape in UPSAMPLE:
        d_dst = odd(upsample_inputs(shape, 2))
        runs = [D.upsample_bilinear_bwd(d_dst, 2, shape[1], shape[2], shape[3]) for _ in range(3)]
        assert same(runs[0], runs[1]) and same(runs[0], runs[2]), shape
    for shape in FINISH:
        logits, d_outs = finish_inputs(shape)
        lg = obj_view(odd(logits), shape)
        runs = [D.refine_train_finish_bwd(lg, d_outs) for _ in range(3)]
        assert same(runs[0], runs[1]) and same(runs[0], runs[2]), shape


def test_clstm_gates_bwd_bf16_image_0_does_not_depend_on_the_batch():
    """792 positions per image at 24 x 33: the workgroups of 256 positions straddle the images."""
    pre, masks, w_mask, cell_prev, d_hidden, d_cell = cell_inputs((3, 16, 24, 33, 3, True))
    whole = D.clstm_gates_bwd(pre, masks, w_mask, cell_prev, d_hidden, d_cell)
    one = D.clstm_gates_bwd([p[:1] for p in pre], masks[:1], w_mask, cell_prev[:1], d_hidden[:1], d_cell[:1])
    for name, a, b in zip(("d_pre", "d_cell_prev", "d_masks"), whole[:3], one[:3]):
        assert same(a[:1], b), name


# ---- 3. the new entries between guard bands ----------------------------------------------------------------------------------------
def wider(t, extra=3):
    """``t`` as the leading channels of a tensor with ``extra`` more: a batch stride larger than the sample's extent."""
    big = torch.zeros((t.shape[0], t.shape[1] + extra) + tuple(t.shape[2:]), dtype=t.dtype, device=t.device)
    big[:, :t.shape[1]] = t
    return big[:, :t.shape[1]]


@pytest.mark.parametrize("shape", [(3, 6, 5, 7, 1, False), (2, 8, 1, 9, 2, True)])
def test_clstm_gates_bwd_bf16_between_bands(shape):
    """Outputs and workspace (allocated by the launcher under the guard) between poisoned bands; inputs between NaN bands, the
    addends with a batch stride larger than their extent and NaN in the gaps."""
    B, Hd, h, w, n_pre, with_cell = shape
    gen = torch.Generator(device=DEV).manual_seed(2)
    pre, masks, w_mask, cell_prev, d_hidden, d_cell = cell_inputs(shape, gen=gen)
    pre = [wider(p) for p in pre]
    assert all(p.stride(0) > 4 * Hd * h * w for p in pre)

    def make(wr):
        opt = lambda t: None if t is None else wr(t)
        return (wr(masks), wr(w_mask), opt(cell_prev), wr(d_hidden), wr(d_cell)) + tuple(wr(p) for p in pre)

    def call(m, wm, cp, dh, dc, *pres):
        out = list(D.clstm_gates_bwd(list(pres), m, wm, cp, dh, dc, need=(with_cell, True, True)))
        out += list(D.clstm_gates_bwd(list(pres), m, wm, cp, dh, None, need=(False, False, False)))
        return [t for t in out if t is not None]
    A, _ = run_row(f"decoder_train_bf16/gates_bwd_{B}x{Hd}x{h}x{w}", make, call)
    assert not any(bool(torch.isnan(t.float()).any()) for t in A)


def test_upsample_bilinear_bwd_bf16_between_bands():
    shape = UPSAMPLE[0]
    B, C, h, w, H, W = shape
    gen = torch.Generator(device=DEV).manual_seed(3)
    d_dst = wider(upsample_inputs(shape, 2, gen))
    assert d_dst.stride(0) > (C + 5) * H * W

    def call(d):
        return [D.upsample_bilinear_bwd(d, c0, C, h, w) for c0 in (0, 2, 5)]      # the last slice included (c0 + C = C')
    A, _ = run_row(f"decoder_train_bf16/upsample_bwd_{h}x{w}_to_{H}x{W}", lambda wr: (wr(d_dst),), call)
    assert not any(bool(torch.isnan(t.float()).any()) for t in A)


def test_refine_train_finish_bf16_between_bands():
    shape = FINISH[0]
    B, O, n_obj, h, w, H, W = shape
    gen = torch.Generator(device=DEV).manual_seed(4)
    logits, d_outs = finish_inputs(shape, gen)
    # the [B, n_obj] view of a conv_out output with more rows than the step reads: batch and object strides beyond the extent
    big = torch.zeros((n_obj + 1, B + 1, h, w), dtype=BF16, device=DEV)
    big[:n_obj, :B] = logits.view(n_obj, B, h, w)
    lg = big[:n_obj, :B].transpose(0, 1)

    def call(l, d):
        return [D.refine_train_finish(l, O, H, W), D.refine_train_finish_bwd(l, d)]
    A, _ = run_row(f"decoder_train_bf16/train_finish_{h}x{w}_to_{H}x{W}", lambda wr: (wr(lg), wr(d_outs)), call)
    assert not any(bool(torch.isnan(t.float()).any()) for t in A)


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------
def test_launchers_refuse_mixed_dtypes_and_fp16():
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=DEV)
    pre16, pre32, masks, wm = z(1, 8, 3, 4, dt=BF16), z(1, 8, 3, 4), z(1, 3, 3, 4), z(8, 9)
    h16, h32, cell = z(1, 2, 3, 4, dt=BF16), z(1, 2, 3, 4), z(1, 2, 3, 4)
    for args in (([pre16, pre32], masks, wm, None, h16, cell), ([pre16], masks, wm, None, h32, cell),
                 ([pre32], masks, wm, None, h16, cell), ([pre16], masks.to(BF16), wm, None, h16, cell),
                 ([pre16], masks, wm.to(BF16), None, h16, cell), ([pre16], masks, wm, cell.to(BF16), h16, cell),
                 ([pre16], masks, wm, None, h16, cell.to(BF16)), ([pre16.half()], masks, wm, None, h16.half(), cell)):
        with pytest.raises(_lib.DmmError):
            D.clstm_gates_bwd(*args, need=(False, True, True))
    with pytest.raises(_lib.DmmError):
        D.upsample_bilinear_bwd(z(1, 2, 6, 8, dt=torch.float16), 0, 2, 3, 4)
    with pytest.raises(_lib.DmmError):
        D.refine_train_finish(z(1, 2, 3, 4, dt=torch.float16), 2, 6, 8)
    with pytest.raises(_lib.DmmError):
        D.refine_train_finish_bwd(z(1, 2, 3, 4, dt=torch.float16), z(1, 2, 6, 8))
    with pytest.raises(_lib.DmmError):
        D.refine_train_finish_bwd(z(1, 2, 3, 4, dt=BF16), z(1, 2, 6, 8, dt=BF16))
    # the fp32 and bf16 sets themselves are taken
    D.clstm_gates_bwd([pre16], masks, wm, None, h16, cell, need=(False, True, True))
    D.clstm_gates_bwd([pre32], masks, wm, None, h32, cell, need=(False, True, True))
    torch.cuda.synchronize()


# ---- 5. the cell under autograd ------------------------------------------------------------------------------------------------------
def test_clstm_gates_fn_under_autograd_on_bf16_addends():
    shape = (2, 8, 5, 7, 3, True)
    pre, masks, w_mask, cell_prev, d_hidden, d_cell = cell_inputs(shape)
    leaves = [p.clone().requires_grad_(True) for p in pre]
    masks_l, w_l, cell_l = (t.clone().requires_grad_(True) for t in (masks, w_mask, cell_prev))
    hidden, cell = D.clstm_gates_fn(leaves, masks_l, w_l, cell_l)
    assert hidden.dtype == BF16 and cell.dtype == torch.float32
    h0, c0 = torch.empty_like(hidden), torch.empty_like(cell)
    D.clstm_gates(pre, masks, w_mask, cell_prev, h0, c0)
    assert same(hidden, h0) and same(cell, c0)
    got = torch.autograd.grad([hidden, cell], leaves + [masks_l, w_l, cell_l], [d_hidden, d_cell])
    want = D.clstm_gates_bwd(pre, masks, w_mask, cell_prev, d_hidden, d_cell)
    assert [g.dtype for g in got] == [BF16] * 3 + [torch.float32] * 3
    for gr in got[:3]:                                                      # every addend: the same gradient
        assert same(gr, want[0])
    assert same(got[3], want[2]) and same(got[4], want[3]) and same(got[5], want[1]) and got[4].shape == w_mask.shape
    hidden, cell = D.clstm_gates_fn(leaves, masks_l, w_l, cell_l)          # only one upstream gradient
    only_h = torch.autograd.grad([hidden], [leaves[0], w_l], [d_hidden])
    want_h = D.clstm_gates_bwd(pre, masks, w_mask, cell_prev, d_hidden, None)
    assert same(only_h[0], want_h[0]) and same(only_h[1], want_h[3])


# ---- 6. RSISMask with fused_train and train_dtype = bf16 on the reference fixture ---------------------------------------------------
def run_module(dec, args, cots):
    """One call of ``dec`` on leaves made of ``args`` -> ({output: tensor}, {leaf or parameter: gradient}) of the cotangents
    ``cots`` (bf16-representable, so every form sees the same ones).  Leaves: the skip maps, the hiddens, the mask planes."""
    feats, masks, spatial, temporal = args
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    named = {f"skip{i}": leaf(t) for i, t in enumerate(feats)}
    named.update({f"mask{i}": leaf(t) for i, t in enumerate(masks)})
    if spatial is not None:
        named.update({f"sp{i}_h": leaf(st[0]) for i, st in enumerate(spatial)})
    if temporal is not None:
        named.update({f"tm{i}": leaf(t) for i, t in enumerate(temporal)})
    call = ([named[f"skip{i}"] for i in range(4)], [named[f"mask{i}"] for i in range(4)],
            None if spatial is None else [[named[f"sp{i}_h"], spatial[i][1]] for i in range(4)],
            None if temporal is None else [named[f"tm{i}"] for i in range(4)])
    out = flat_outputs(dec(*call))
    params = dict(dec.named_parameters())
    grads = torch.autograd.grad([out[k] for k in out], list(named.values()) + list(params.values()),
                                [cots[k].to(out[k].dtype) for k in out])
    return {k: v.detach() for k, v in out.items()}, dict(zip(list(named) + list(params), grads))


@pytest.mark.parametrize("mode", ["concat", "sum"])
@pytest.mark.parametrize("case", list(CASES))
def test_bf16_fused_train_against_the_reference_fixture(mode, case):
    dec, g = load_decoder(mode, DEV)
    dec16 = copy.deepcopy(dec).to(BF16)                                   # the yardstick: the stock torch decoder in bf16
    dec64 = copy.deepcopy(dec).double()
    dec.fused_train, dec.train_dtype = True, BF16
    low, all16, wide = rounded_inputs(case_inputs(g, mode, case, DEV))
    with torch.no_grad():
        shapes = flat_outputs(dec64.forward_stock(*wide))
    gen = torch.Generator(device=DEV).manual_seed(7)
    cots = {k: torch.randn(v.shape, device=DEV, generator=gen).to(BF16).double() for k, v in shapes.items()}
    assert dec._route(low[0] + low[1]) == "train"
    n0, l0 = dec.conv_calls, int(_lib.load().dmm_launch_count())
    got_o, got_g = run_module(dec, low, cots)
    assert dec.conv_calls > n0 and int(_lib.load().dmm_launch_count()) > l0                # the fused training form ran
    assert got_o["out_mask"].dtype == BF16
    assert all(got_o[f"h{i}"].dtype == BF16 and got_o[f"c{i}"].dtype == torch.float32 for i in range(4))
    n16 = dec16.conv_calls
    s_o, s_g = run_module(dec16, all16, cots)
    r_o, r_g = run_module(dec64, wide, cots)
    assert dec16.conv_calls == n16 and sorted(got_g) == sorted(r_g) == sorted(s_g)
    params = dict(dec.named_parameters())
    for k, v in got_g.items():
        want = torch.float32 if (k in params or k.startswith("mask")) else BF16
        assert v.dtype == want, (k, v.dtype)                              # the masters' gradients are fp32
    for k in got_o:
        held16(f"fixture/{mode}/{case}/out/{k}", got_o[k], s_o[k], r_o[k])
    for k in got_g:
        held16(f"fixture/{mode}/{case}/grad/{k}", got_g[k], s_g[k], r_g[k])


def test_bf16_train_form_names_a_wrong_operand_set_and_the_default_is_stock():
    dec, g = load_decoder("concat", DEV)
    args = case_inputs(g, "concat", "st", DEV)
    low, all16, _ = rounded_inputs(args)
    ts16 = low[0] + low[1]
    dec.fused_train = True
    assert dec.train_dtype == torch.float32 and dec._route(ts16) == "stock"       # the default: today's route
    assert dec._route(args[0] + args[1]) == "train"
    dec.train_dtype = BF16
    assert dec._route(ts16) == "train" and dec._route(args[0] + args[1]) == "train"
    assert dec._route([x.half() for x in low[0]] + low[1]) == "stock"             # fp16 is not taken
    with pytest.raises(_lib.DmmError, match="train_dtype = torch.bfloat16 takes bfloat16 skip maps"):
        dec(*args)                                                                # fp32 maps with bf16 set: named, not cast
    with pytest.raises(_lib.DmmError, match="float32 mask planes"):
        dec(*all16)
    with torch.no_grad():                                                         # without a gradient compute_dtype decides
        assert dec._route(ts16) == "stock" and dec._route(args[0] + args[1]) == "fused"
    dec.fused_train = False
    assert dec._route(ts16) == "stock"


# ---- 7. RefineTrainStep over two chained frames -----------------------------------------------------------------------------------------
B_, O_, H_, W_, HID = 2, 3, 47, 66, 16
VALID = [[1, 1, 1], [1, 0, 1]]                                            # 3 objects, one invalid (video, object) pair
_REFS = {}


def step_case(only_temporal):
    """The decoder, the frames (bf16-rounded skip maps, fp32 planes) and, computed once and shared, the same step on the bf16
    stock decoder and on the fp64 decoder."""
    if only_temporal not in _REFS:
        dec = step_decoder(81, HID)
        frames = clip(82, B_, O_, H_, W_, HID, 2, device=DEV)
        for fr in frames:
            fr["feats"] = [f.to(BF16) for f in fr["feats"]]
        valid = torch.tensor(VALID, device=DEV)
        sw = valid.float()
        dec16, dec64 = copy.deepcopy(dec).to(BF16), copy.deepcopy(dec).double()
        step16 = RefineTrainStep(dec16, only_temporal=only_temporal)
        stock16 = run_clip(step_call(step16, valid, sw), dec16, frames, valid, sw)
        frames64 = [{"feats": [t.double() for t in fr["feats"]], "y_mask": fr["y_mask"].double(),
                     "init_pred": fr["init_pred"].double()} for fr in frames]
        step64 = RefineTrainStep(dec64, only_temporal=only_temporal)
        ref64 = run_clip(step_call(step64, valid, sw), dec64, frames64, valid, sw)
        assert step16.last_route == step64.last_route == "stock"
        _REFS[only_temporal] = (dec, frames, valid, sw, stock16, ref64)
    return _REFS[only_temporal]


def run_bf16_step(dec, frames, valid, sw, only_temporal, off=None):
    d = copy.deepcopy(dec)
    d.fused_train, d.train_dtype = True, BF16
    step = RefineTrainStep(d, only_temporal=only_temporal)
    if off is not None:
        step.kernels[off] = False
    seen = []
    inner = step_call(step, valid, sw)

    def call(*a):
        res = inner(*a)
        seen.append((step.last_route, res[2].dtype, [h.dtype for hs in res[3] for h in hs]))
        return res
    got = run_clip(call, d, frames, valid, sw)
    assert len(seen) == 2
    for route, outs_dtype, thid_dtypes in seen:
        assert route == "fused" and outs_dtype == torch.float32 and len(thid_dtypes) == 3 * 4
        assert all(t == BF16 for t in thid_dtypes)                         # the temporal state is bf16
    return got, d


def hold_step(tag, got, stock16, ref64, n_params):
    held16(tag + "/loss", got[0], stock16[0], ref64[0])
    for f in range(2):
        assert got[1][f].dtype == torch.float32 and got[1][f].shape == (B_, O_, H_ * W_)
        held16(f"{tag}/f{f}/outs_pad", got[1][f], stock16[1][f], ref64[1][f])
    assert sorted(got[2]) == sorted(ref64[2]) == sorted(stock16[2]) and len(got[2]) == 2 * 5 + n_params
    for k in got[2]:
        held16(f"{tag}/grad/{k}", got[2][k], stock16[2][k], ref64[2][k])


@pytest.mark.parametrize("only_temporal", [False, True])
def test_step_bf16_against_the_bf16_stock_decoder_and_fp64(only_temporal):
    dec, frames, valid, sw, stock16, ref64 = step_case(only_temporal)
    got, d = run_bf16_step(dec, frames, valid, sw, only_temporal)
    params = dict(d.named_parameters())
    for k, v in got[2].items():
        want = torch.float32 if (k in params or k.endswith("init_pred")) else BF16
        assert v.dtype == want, (k, v.dtype)                              # fp32 masters, fp32 gradients
    hold_step("step" + ("_only_temporal" if only_temporal else ""), got, stock16, ref64, len(params))


@pytest.mark.parametrize("piece", ["pyramid", "upsample", "finish"])
def test_step_bf16_with_one_torch_twin(piece):
    dec, frames, valid, sw, stock16, ref64 = step_case(False)
    got, d = run_bf16_step(dec, frames, valid, sw, False, off=piece)
    hold_step(f"step_twin_{piece}", got, stock16, ref64, len(list(d.parameters())))


def test_step_bf16_rows_beyond_n_obj_are_zero_and_wrong_sets_are_named():
    dec = step_decoder(83, HID)
    dec.fused_train, dec.train_dtype = True, BF16
    O = O_ + 1
    fr = clip(84, B_, O, H_, W_, HID, 1, device=DEV)[0]
    valid = torch.tensor([v + [0] for v in VALID], device=DEV)
    feats16 = [f.to(BF16) for f in fr["feats"]]
    step = RefineTrainStep(dec)
    loss, _, outs, state = step(feats16, fr["y_mask"], fr["y_mask"], fr["init_pred"], fr["y_mask"], valid.float(), valid, None)
    assert step.last_route == "fused" and state.n_obj == 3 and loss.requires_grad and loss.dtype == torch.float32
    assert outs.dtype == torch.float32 and float(outs.detach()[:, 3:].abs().max()) == 0.0
    assert float(outs.detach()[:, :3].abs().max()) > 0.0 and all(h.dtype == BF16 for hs in state.thid for h in hs)
    with pytest.raises(_lib.DmmError, match="bfloat16 skip maps"):
        step(fr["feats"], fr["y_mask"], fr["y_mask"], fr["init_pred"], fr["y_mask"], valid.float(), valid, None)
    with pytest.raises(_lib.DmmError, match="float32 mask planes"):
        step(feats16, fr["y_mask"].to(BF16), fr["y_mask"], fr["init_pred"], fr["y_mask"], valid.float(), valid, None)
    dec.train_dtype = torch.float32                                       # the default: bf16 maps are not the fused form's
    assert dec._route(feats16 + [fr["y_mask"], fr["init_pred"]]) == "stock"


# ---- 8. counts -----------------------------------------------------------------------------------------------------------------------------
def test_bf16_step_issues_the_fp32_steps_convolutions_and_launches():
    dec = step_decoder(85, HID)
    dec.fused_train = True
    frames = clip(86, B_, O_, H_, W_, HID, 2, device=DEV)
    valid = torch.tensor(VALID, device=DEV)
    sw = valid.float()
    counts = {}
    for name, dt in (("fp32", torch.float32), ("bf16", BF16)):
        d = copy.deepcopy(dec)
        d.train_dtype = dt
        fs = [dict(fr, feats=[f.to(dt) for f in fr["feats"]]) for fr in frames]
        step = RefineTrainStep(d)
        torch.cuda.synchronize()
        c0, l0 = d.conv_calls, int(_lib.load().dmm_launch_count())
        run_clip(step_call(step, valid, sw), d, fs, valid, sw)             # two frames, forward and backward
        torch.cuda.synchronize()
        assert step.last_route == "fused"
        counts[name] = (d.conv_calls - c0, int(_lib.load().dmm_launch_count()) - l0)
    record_achieved("decoder_train_bf16/launches/convs_per_clip", counts["bf16"][0])
    record_achieved("decoder_train_bf16/launches/kernels_per_clip", counts["bf16"][1])
    assert counts["bf16"] == counts["fp32"] and counts["bf16"][0] > 0 and counts["bf16"][1] > 0, counts
