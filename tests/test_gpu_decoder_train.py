"""Training the refine decoder on its fused form, on the GPU: the cell's backward kernel (``dmm_clstm_gates_bwd_f32``) against
fp64 autograd of the cell's forward, its repeatability, batch independence and guard bands, ``clstm_gates_fn`` under
``torch.autograd.grad``, ``RSISMask`` with ``fused_train = True`` against the stock form and fp64 -- one call and the trainer's
object chain -- and the routes.

The tolerance is the rule of tests/test_gpu_decoder.py (``held``): err <= 2 * max(e_stock, floor) + 1 ulp of max|ref|, both
errors against the fp64 evaluation on the same device, e_stock = the fp32 torch-autograd evaluation of the same function,
floor = one fp32 ulp of max|ref|.  For the module, e_stock is the larger of the stock form's error and the error of the
``split_forward`` algebra (tests/test_decoder_cpu.py) under fp32 torch autograd: the fused form reorders fp32 sums by design,
and that restatement measures the reordering with none of the new code in it.  Every pair is recorded."""
import copy
import itertools

import pytest
import torch
import torch.nn.functional as F

import dmm_net_amd
from conftest import record_achieved
from dmm_net_amd import decoder as D
from dmm_net_amd.decoder import RSISMask, pyramid_sizes
from guarded import banded, guarded
from test_decoder_cpu import CASES, flat_outputs, make_args, split_forward
from test_gpu_decoder import DEV, gates_torch, held, ulp

pytestmark = pytest.mark.gpu

SHAPES = [(2, 32, 8, 14, 3, True), (3, 6, 5, 7, 1, False), (1, 16, 24, 33, 2, True), (1, 1, 3, 3, 1, False),
          (1, 4, 1, 1, 1, True), (2, 8, 1, 9, 2, False), (4, 16, 64, 112, 3, True)]
NAMES = ("d_pre", "d_cell_prev", "d_masks", "d_w_mask")


def tag_of(shape):
    B, Hd, h, w, n_pre, with_cell = shape
    return f"gates_bwd_{B}x{Hd}x{h}x{w}_{n_pre}{'c' if with_cell else ''}"


def cell_inputs(shape, seed=2):
    B, Hd, h, w, n_pre, with_cell = shape
    torch.manual_seed(seed)
    pre = [torch.randn(B, 4 * Hd, h, w, device=DEV) for _ in range(n_pre)]
    masks = torch.rand(B, 3, h, w, device=DEV)
    w_mask = torch.randn(4 * Hd, 9, device=DEV) * 0.3
    cell_prev = torch.randn(B, Hd, h, w, device=DEV) if with_cell else None
    d_hidden, d_cell = torch.randn(B, Hd, h, w, device=DEV), torch.randn(B, Hd, h, w, device=DEV)
    return pre, masks, w_mask, cell_prev, d_hidden, d_cell


def autograd_of_gates(pre, masks, w_mask, cell_prev, d_hidden, d_cell, dtype):
    """(d_pre, d_cell_prev or None, d_masks, d_w_mask) of ``gates_torch`` by torch autograd in ``dtype``."""
    leaf = lambda t: None if t is None else t.detach().to(dtype).requires_grad_(True)
    pre_l = [leaf(p) for p in pre]
    masks_l, w_l, cell_l = leaf(masks), leaf(w_mask), leaf(cell_prev)
    hidden, cell = gates_torch(pre_l, masks_l, w_l, cell_l)
    outs = [o for o, d in ((hidden, d_hidden), (cell, d_cell)) if d is not None]
    ups = [d.to(dtype) for d in (d_hidden, d_cell) if d is not None]
    leaves = [pre_l[0], masks_l, w_l] + ([cell_l] if cell_l is not None else [])
    g = torch.autograd.grad(outs, leaves, ups)                              # (every addend's gradient is that of the first)
    return g[0], (g[3] if cell_l is not None else None), g[1], g[2]


@pytest.mark.parametrize("shape", SHAPES, ids=tag_of)
def test_gates_bwd_kernel(shape):
    pre, masks, w_mask, cell_prev, d_hidden, d_cell = cell_inputs(shape)
    with_cell = cell_prev is not None
    full = None
    for label, dh, dc in (("hc", d_hidden, d_cell), ("h", d_hidden, None), ("c", None, d_cell)):
        got = D.clstm_gates_bwd(pre, masks, w_mask, cell_prev, dh, dc, need=(with_cell, True, True))
        stock = autograd_of_gates(pre, masks, w_mask, cell_prev, dh, dc, torch.float32)
        ref = autograd_of_gates(pre, masks, w_mask, cell_prev, dh, dc, torch.float64)
        assert (got[1] is None) == (not with_cell)
        for name, a, s, r in zip(NAMES, got, stock, ref):
            if a is not None:
                assert a.shape == r.shape and a.is_contiguous()
                held(f"{tag_of(shape)}/{label}/{name}", a, s, r, floor=ulp(r.abs().max()))
        if label == "hc":
            full = got
    # every subset of the wanted outputs: the same bits as in the full call, None for the rest
    for need in itertools.product((False, True), repeat=3):
        if need[0] and not with_cell:
            continue
        got = D.clstm_gates_bwd(pre, masks, w_mask, cell_prev, d_hidden, d_cell, need=need)
        assert torch.equal(got[0], full[0]), need
        for name, wanted, a, f in zip(NAMES[1:], need, got[1:], full[1:]):
            assert (a is not None) == wanted, (need, name)
            if wanted:
                assert torch.equal(a, f), (need, name)


@pytest.mark.parametrize("shape", SHAPES, ids=tag_of)
def test_gates_bwd_three_calls_are_bit_identical(shape):
    args = cell_inputs(shape)
    need = (args[3] is not None, True, True)
    runs = [D.clstm_gates_bwd(*args, need=need) for _ in range(3)]
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert (a is None and b is None) or torch.equal(a, b)


@pytest.mark.parametrize("shape", [(3, 6, 5, 7, 1, True), (3, 16, 24, 33, 3, True)], ids=tag_of)
def test_gates_bwd_image_0_does_not_depend_on_the_batch(shape):
    """792 positions per image at 24 x 33: the workgroups of 256 positions straddle the images."""
    pre, masks, w_mask, cell_prev, d_hidden, d_cell = cell_inputs(shape)
    whole = D.clstm_gates_bwd(pre, masks, w_mask, cell_prev, d_hidden, d_cell)
    one = D.clstm_gates_bwd([p[:1] for p in pre], masks[:1], w_mask, cell_prev[:1], d_hidden[:1], d_cell[:1])
    for name, a, b in zip(NAMES[:3], whole[:3], one[:3]):
        assert torch.equal(a[:1], b), name


@pytest.mark.parametrize("shape", [(2, 6, 5, 7, 3, True), (1, 16, 24, 33, 2, True), (2, 8, 1, 9, 1, False)], ids=tag_of)
def test_gates_bwd_stays_inside_its_buffers(shape):
    """Outputs and workspace between poisoned bands: no byte outside them changes.  Inputs between NaN bands, the addends with
    a batch stride larger than their extent and NaN in the gaps: no load outside them reaches an output."""
    B, Hd, h, w, n_pre, with_cell = shape
    pre, masks, w_mask, cell_prev, d_hidden, d_cell = cell_inputs(shape)
    plain = D.clstm_gates_bwd(pre, masks, w_mask, cell_prev, d_hidden, d_cell, need=(with_cell, True, True))
    wide = [torch.zeros(B, 4 * Hd + 3, h, w, device=DEV) for _ in pre]
    for wd, p in zip(wide, pre):
        wd[:, :4 * Hd] = p
    with guarded() as g:
        pre_b = [banded(wd[:, :4 * Hd]) for wd in wide]
        assert all(p.stride(0) > 4 * Hd * h * w for p in pre_b) and all(torch.equal(a, b) for a, b in zip(pre_b, pre))
        rest = [None if t is None else banded(t) for t in (masks, w_mask, cell_prev, d_hidden, d_cell)]
        got = D.clstm_gates_bwd(pre_b, *rest, need=(with_cell, True, True))
        torch.cuda.synchronize()
        assert g.check() == []
        assert g.outside([t for t in got if t is not None]) == []          # the outputs were allocated under the guard
    for name, a, b in zip(NAMES, got, plain):
        if a is not None:
            assert not bool(torch.isnan(a).any()), name
            assert torch.equal(a, b), name


# ---- the autograd function ------------------------------------------------------------------------------------------------
def test_clstm_gates_fn_under_autograd(monkeypatch):
    shape = (2, 8, 5, 7, 3, True)
    pre, masks, w_mask, cell_prev, d_hidden, d_cell = cell_inputs(shape)
    leaves = [p.clone().requires_grad_(True) for p in pre]
    masks_l, w_l, cell_l = (t.clone().requires_grad_(True) for t in (masks, w_mask, cell_prev))
    hidden, cell = D.clstm_gates_fn(leaves, masks_l, w_l, cell_l)
    h0, c0 = torch.empty_like(hidden), torch.empty_like(cell)
    D.clstm_gates(pre, masks, w_mask, cell_prev, h0, c0)
    assert torch.equal(hidden, h0) and torch.equal(cell, c0)
    got = torch.autograd.grad([hidden, cell], leaves + [masks_l, w_l, cell_l], [d_hidden, d_cell])
    want = D.clstm_gates_bwd(pre, masks, w_mask, cell_prev, d_hidden, d_cell)
    for gr in got[:3]:                                                      # every addend: the same gradient
        assert torch.equal(gr, want[0])
    assert torch.equal(got[3], want[2]) and torch.equal(got[4], want[3]) and torch.equal(got[5], want[1])
    assert got[4].shape == w_mask.shape
    # only one upstream gradient: the other is passed as null
    hidden, cell = D.clstm_gates_fn(leaves, masks_l, w_l, cell_l)
    only_h = torch.autograd.grad([hidden], [leaves[0], w_l], [d_hidden])
    want_h = D.clstm_gates_bwd(pre, masks, w_mask, cell_prev, d_hidden, None)
    assert torch.equal(only_h[0], want_h[0]) and torch.equal(only_h[1], want_h[3])
    # inputs without requires_grad get None, and the kernel is not asked for them
    asked = []
    real = D.clstm_gates_bwd
    monkeypatch.setattr(D, "clstm_gates_bwd", lambda *a, need: asked.append(tuple(need)) or real(*a, need=need))
    for want_m, want_w in ((False, True), (True, False), (False, False)):
        m = masks.clone().requires_grad_(want_m)
        wl = w_mask.clone().requires_grad_(want_w)
        p0 = pre[0].clone().requires_grad_(True)
        hidden, cell = D.clstm_gates_fn([p0, pre[1], None], m, wl, cell_prev)
        ((hidden * d_hidden).sum() + (cell * d_cell).sum()).backward()
        assert asked[-1] == (False, want_m, want_w)
        assert (m.grad is not None) == want_m and (wl.grad is not None) == want_w and p0.grad is not None


# ---- the module ------------------------------------------------------------------------------------------------------------
class Sliced:
    """``split_forward``'s view of a decoder with DIFFERENTIABLE weight slices (``RSISMask.weight_slices`` is a no-grad
    memo): the fused algebra in torch ops under autograd, with none of the training form's code in it."""

    def __init__(self, dec):
        self.dec, self.skip_dims_out, self.skip_mode, self.conv_out = dec, dec.skip_dims_out, dec.skip_mode, dec.conv_out

    def weight_slices(self):
        out = []
        for i, cell in enumerate(self.dec.clstm_list):
            Wt, Hd, cin = cell.Gates.weight, cell.hidden_size, cell.input_size
            x = Wt[:, :cin]
            d = {"m": Wt[:, cin:cin + 1].reshape(4 * Hd, 9), "hs": Wt[:, cin + 1:cin + 1 + Hd], "ht": Wt[:, cin + 1 + Hd:],
                 "bias": cell.Gates.bias, "up": None, "skip": None, "cat": None}
            if i == 0:
                d["skip"] = x
            else:
                cup = self.skip_dims_out[i - 1]
                d["up"] = x[:, :cup]
                if self.skip_mode == "concat":
                    d["skip"] = x[:, cup:]
                elif self.skip_mode == "sum":
                    d["skip"] = d["up"]
                d["cat"] = torch.cat([d["up"], d["hs"]], 1)
            out.append(d)
        return out


def held_all(name, got, stocks, ref64):
    """``held`` with e_stock = the largest error among ``stocks`` and the floor of one ulp of max|ref|."""
    worst = max(stocks, key=lambda s: float((s.double() - ref64).abs().max()))
    held(name, got, worst, ref64, floor=ulp(ref64.abs().max()))


def module_inputs(mode, seed, B=2, hidden=32, H=95, W=130):
    torch.manual_seed(seed)
    dec = RSISMask(make_args(mode, hidden=hidden)).eval().to(DEV)
    with torch.no_grad():
        dec.conv_out.weight.mul_(10)                                      # (default weights leave every logit within +-0.3)
    sizes = pyramid_sizes(H, W)
    ch = [hidden, hidden, hidden // 2, hidden // 4]
    feats = [torch.randn((B, c) + s, device=DEV) for c, s in zip(ch, sizes)]
    masks = [torch.rand((B, 3) + s, device=DEV) for s in sizes]
    spatial = [[0.5 * torch.randn((B, d) + s, device=DEV).tanh(), torch.randn((B, d) + s, device=DEV)]
               for d, s in zip(dec.skip_dims_out, sizes)]
    temporal = [0.5 * torch.randn((B, d) + s, device=DEV).tanh() for d, s in zip(dec.skip_dims_out, sizes)]
    return dec, feats, masks, spatial, temporal


def run_form(dec, form, dtype, feats, masks, spatial, temporal, weights):
    """One call of ``form`` ('train' | 'stock' | 'split') in ``dtype`` -> ({output: tensor}, {leaf or parameter: gradient})
    of the fixed linear functional sum_k <weights[k], output_k>."""
    d = copy.deepcopy(dec).to(dtype)
    d.fused_train = form == "train"
    leaf = lambda t: t.detach().to(dtype).requires_grad_(True)
    named = {f"skip{i}": leaf(t) for i, t in enumerate(feats)}
    named.update({f"mask{i}": leaf(t) for i, t in enumerate(masks)})
    if spatial is not None:
        named.update({f"sp{i}_{n}": leaf(t) for i, st in enumerate(spatial) for n, t in zip("hc", st)})
    if temporal is not None:
        named.update({f"tm{i}": leaf(t) for i, t in enumerate(temporal)})
    args = ([named[f"skip{i}"] for i in range(4)], [named[f"mask{i}"] for i in range(4)],
            None if spatial is None else [[named[f"sp{i}_h"], named[f"sp{i}_c"]] for i in range(4)],
            None if temporal is None else [named[f"tm{i}"] for i in range(4)])
    n0 = d.conv_calls
    if form == "split":
        out = flat_outputs(split_forward(Sliced(d), *args))
    else:
        out = flat_outputs(d(*args))
    assert (d.conv_calls > n0) == (form == "train")                        # the training form ran exactly where asked
    loss = sum((out[k] * weights[k].to(dtype)).sum() for k in out)
    params = dict(d.named_parameters())
    # (skip mode 'none' does not read the skip maps above level 0: their gradient is None in every form)
    grads = torch.autograd.grad(loss, list(named.values()) + list(params.values()), allow_unused=True)
    return {k: v.detach() for k, v in out.items()}, dict(zip(list(named) + list(params), grads))


@pytest.mark.parametrize("mode", ["concat", "sum", "mul", "none"])
def test_fused_train_against_stock_and_fp64(mode):
    dec, feats, masks, spatial, temporal = module_inputs(mode, seed=51)
    weights = None
    for case, (sp, tm) in CASES.items():
        s, t = (spatial if sp else None), (temporal if tm else None)
        if weights is None:
            with torch.no_grad():
                shapes = flat_outputs(dec.forward_stock(feats, masks, s, t))
            weights = {k: torch.randn(v.shape, device=DEV, dtype=torch.float64) for k, v in shapes.items()}
        ref_o, ref_g = run_form(dec, "stock", torch.float64, feats, masks, s, t, weights)
        got_o, got_g = run_form(dec, "train", torch.float32, feats, masks, s, t, weights)
        stocks = [run_form(dec, f, torch.float32, feats, masks, s, t, weights) for f in ("stock", "split")]
        assert sorted(got_g) == sorted(ref_g) and len(got_g) == len(stocks[0][1])
        for k in got_o:
            held_all(f"train/{mode}/{case}/out/{k}", got_o[k], [so[k] for so, _ in stocks], ref_o[k])
        for k in got_g:
            if ref_g[k] is None:
                assert got_g[k] is None and mode == "none" and k in ("skip1", "skip2", "skip3"), k
            else:
                held_all(f"train/{mode}/{case}/grad/{k}", got_g[k], [sg[k] for _, sg in stocks], ref_g[k])


# ---- the trainer's object chain ----------------------------------------------------------------------------------------------
def run_chain(dec, form, dtype, frames, H, W, weights):
    """trainer.py:248-276 over the objects of each frame: object t's spatial state is object t - 1's ``hidden``, the temporal
    hidden comes from the same object of the previous frame; ``out_mask`` is upsampled to the image, passed through a sigmoid
    and summed under fixed weights -> ({name: output}, {name: gradient})."""
    d = copy.deepcopy(dec).to(dtype)
    d.fused_train = form == "train"
    fwd = (lambda *a: split_forward(Sliced(d), *a)) if form == "split" else d
    leaf = lambda t: t.detach().to(dtype).requires_grad_(True)
    named, outs = {}, {}
    prev_thid, loss = None, 0
    for f, (feats, mask_lists) in enumerate(frames):
        fl = [leaf(t) for t in feats]
        named.update({f"f{f}/skip{i}": t for i, t in enumerate(fl)})
        hidden_spatial, thid = None, []
        for t, ml in enumerate(mask_lists):
            ml = [leaf(m) for m in ml]
            named.update({f"f{f}/o{t}/mask{i}": m for i, m in enumerate(ml)})
            out_mask, hidden = fwd(fl, ml, hidden_spatial, None if prev_thid is None else prev_thid[t])
            thid.append([hc[0] for hc in hidden])
            hidden_spatial = hidden
            prob = torch.sigmoid(F.interpolate(out_mask, (H, W)))
            outs[f"f{f}/o{t}/prob"] = prob.detach()
            loss = loss + (prob * weights[f][t].to(dtype)).sum()
        prev_thid = thid
    params = dict(d.named_parameters())
    grads = torch.autograd.grad(loss, list(named.values()) + list(params.values()))
    return outs, dict(zip(list(named) + list(params), grads))


def test_object_chain_against_stock_and_fp64_and_bit_identical_twice():
    """Three objects over two frames.  The library convolutions have to repeat as well for the second half: the project's
    deterministic mode and cudnn.deterministic for torch's own convolution calls (forward and backward)."""
    B, hidden, H, W, n_obj = 2, 32, 95, 130, 3
    torch.manual_seed(61)
    dec = RSISMask(make_args("concat", hidden=hidden)).eval().to(DEV)
    with torch.no_grad():
        dec.conv_out.weight.mul_(10)
    sizes = pyramid_sizes(H, W)
    ch = [hidden, hidden, hidden // 2, hidden // 4]
    frames = [([torch.randn((B, c) + s, device=DEV) for c, s in zip(ch, sizes)],
               [[torch.rand((B, 3) + s, device=DEV) for s in sizes] for _ in range(n_obj)]) for _ in range(2)]
    weights = [[torch.randn(B, 1, H, W, device=DEV, dtype=torch.float64) for _ in range(n_obj)] for _ in range(2)]
    with dmm_net_amd.deterministic(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        ref_o, ref_g = run_chain(dec, "stock", torch.float64, frames, H, W, weights)
        got_o, got_g = run_chain(dec, "train", torch.float32, frames, H, W, weights)
        again_o, again_g = run_chain(dec, "train", torch.float32, frames, H, W, weights)
        stocks = [run_chain(dec, f, torch.float32, frames, H, W, weights) for f in ("stock", "split")]
    for k in got_o:
        held_all(f"train/chain/out/{k}", got_o[k], [so[k] for so, _ in stocks], ref_o[k])
        assert torch.equal(got_o[k], again_o[k]), k
    assert sorted(got_g) == sorted(ref_g)
    for k in got_g:
        held_all(f"train/chain/grad/{k}", got_g[k], [sg[k] for _, sg in stocks], ref_g[k])
        assert torch.equal(got_g[k], again_g[k]), k


# ---- the routes --------------------------------------------------------------------------------------------------------------
def test_routes():
    dec, feats, masks, spatial, temporal = module_inputs("concat", seed=71)
    leaves = lambda: [f.clone().requires_grad_(True) for f in feats]
    # default: a gradient means the stock form (today's behaviour)
    assert dec.fused_train is False
    n0 = dec.conv_calls
    out, _ = dec(leaves(), masks, spatial, temporal)
    assert dec.conv_calls == n0 and out.requires_grad
    # fused_train: at most 3 convolutions per level + conv_out
    dec.fused_train = True
    for sp, tm, convs in ((None, None, 4 + 3 + 1), (spatial, None, 4 + 4 + 1), (None, temporal, 4 + 4 + 3 + 1),
                          (spatial, temporal, 3 * 4 + 1)):
        n0 = dec.conv_calls
        out, hidden_list = dec(leaves(), masks, sp, tm)
        assert dec.conv_calls - n0 == convs <= 3 * 4 + 1, (convs, dec.conv_calls - n0)
        assert out.requires_grad and all(h.requires_grad and c.requires_grad for h, c in hidden_list)
    # parameters alone requiring the gradient take it too
    n0 = dec.conv_calls
    out, _ = dec(feats, masks, spatial, temporal)
    assert dec.conv_calls - n0 == 13 and out.requires_grad
    # outside the envelope: the stock form, no convolution counted
    drop = RSISMask(make_args("concat", hidden=32, dropout=0.5)).to(DEV).train()
    one = RSISMask(make_args("concat", hidden=32, kernel_size=1)).to(DEV).eval()
    dbl = copy.deepcopy(dec).double()
    for d, to in ((drop, torch.float32), (one, torch.float32), (dbl, torch.float64)):
        d.fused_train = True
        n0 = d.conv_calls
        args = [[t.to(to) for t in feats], [t.to(to) for t in masks], [[t.to(to) for t in st] for st in spatial],
                [t.to(to) for t in temporal]]
        out, _ = d(*args)
        assert d.conv_calls == n0 and out.requires_grad
    drop.eval()                                                             # dropout inactive: inside the envelope again
    n0 = drop.conv_calls
    drop(feats, masks, spatial, temporal)
    assert drop.conv_calls - n0 == 13
    # eval() + no_grad is still the inference form, bit for bit what it is without fused_train
    plain = copy.deepcopy(dec)
    plain.fused_train = False
    with torch.no_grad():
        assert dec.fused_ok(feats + masks)
        a, b = flat_outputs(dec(feats, masks, spatial, temporal)), flat_outputs(plain(feats, masks, spatial, temporal))
    for k in a:
        assert torch.equal(a[k], b[k]) and not a[k].requires_grad
