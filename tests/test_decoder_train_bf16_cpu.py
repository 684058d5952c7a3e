"""The bf16 training form of the refine decoder without a GPU (dmm_net_amd/decoder.py, include/dmm_match.h (12l)-(12o)): the
``train_dtype`` switch, the routes it must leave alone (CPU tensors with every combination of the two switches), the torch
twins of the step's three pieces in bf16, the bf16 convolution on fp32 master weights (fp32 weight gradients, widened before
they are added), and the four 16-bit training entries: bound from the header, and answering the calls they refuse as their
fp32 siblings do, before any HIP call."""
import copy
import ctypes
import itertools
import os

import pytest
import torch
import torch.nn.functional as F

from dmm_net_amd import _lib, decoder as D
from dmm_net_amd.decoder import RSISMask, RefineTrainStep
from test_decoder_cpu import CASES, case_inputs, flat_outputs, load_decoder, make_args
from test_refine_train_cpu import clip

BF16 = torch.bfloat16
ENTRIES = ("dmm_clstm_gates_bwd_bf16", "dmm_upsample_bilinear_bwd_bf16", "dmm_refine_train_finish_bf16",
           "dmm_refine_train_finish_bwd_bf16")


def test_train_dtype_accepts_fp32_and_bf16_only():
    dec = RSISMask(make_args("concat"))
    assert dec.train_dtype == torch.float32                          # the default: nothing changes unless asked
    dec.train_dtype = BF16
    assert dec.train_dtype == BF16 and dec.compute_dtype == torch.float32        # a switch of its own
    for bad in (torch.float16, torch.float64, torch.int32, "bf16", None):
        with pytest.raises(ValueError, match="train_dtype"):
            dec.train_dtype = bad
    assert dec.train_dtype == BF16                                   # a refused value leaves the setting alone
    assert copy.deepcopy(dec).train_dtype == BF16
    dec.load_state_dict(copy.deepcopy(dec.state_dict()), strict=True)
    assert all(p.dtype == torch.float32 for p in dec.parameters())   # fp32 masters whatever the setting
    dec.train_dtype = torch.float32
    assert dec.train_dtype == torch.float32 and copy.deepcopy(dec).train_dtype == torch.float32


@pytest.mark.parametrize("fused_train,train_dtype", list(itertools.product((False, True), (torch.float32, BF16))))
def test_cpu_tensors_route_to_stock_with_every_combination_of_the_switches(fused_train, train_dtype):
    dec, g = load_decoder("concat")
    plain = copy.deepcopy(dec)
    dec.fused_train, dec.train_dtype = fused_train, train_dtype
    feats, masks, spatial, temporal = case_inputs(g, "concat", "st")
    x = [f.clone().requires_grad_(True) for f in feats]
    low = [f.to(BF16).requires_grad_(True) for f in feats]
    assert dec._route(x + masks) == "stock" and dec._route(feats + masks) == "stock" and dec._route(low + masks) == "stock"
    with torch.no_grad():
        assert dec._route(feats + masks) == "stock" and dec._route([f.to(BF16) for f in feats] + masks) == "stock"
    a, b = dec(x, masks, spatial, temporal), plain(x, masks, spatial, temporal)
    for k, v in flat_outputs(a).items():
        assert v.dtype == torch.float32 and torch.equal(v, flat_outputs(b)[k]), k
    assert a[0].requires_grad and dec.conv_calls == 0                # the fused forms never ran
    # the step too
    fr = clip(8, 1, 3, 29, 43, 32, 1)[0]
    valid = torch.tensor([[1, 1, 0]])
    step = RefineTrainStep(dec)
    out = step(fr["feats"], fr["y_mask"], fr["y_mask"], fr["init_pred"], fr["y_mask"], valid.float(), valid, None)
    assert step.last_route == "stock" and out[0].requires_grad and out[2].dtype == torch.float32


def test_the_torch_twins_run_in_bf16_with_the_dtypes_of_the_kernels():
    g = torch.Generator().manual_seed(3)
    B, O, n_obj, H, W = 2, 4, 3, 29, 43
    # the pyramid: mask planes are fp32 in every form, and so are its levels and the planes' gradients
    planes = [torch.rand(B, O, H * W, generator=g).requires_grad_(k != 1) for k in range(3)]
    pyr = D.mask_pyramid_torch(planes[0], planes[1], planes[2].view(B, O, H, W), n_obj, H, W)
    assert [tuple(p.shape) for p in pyr] == [(n_obj, B, 3, h, w) for h, w in D.pyramid_sizes(H, W)]
    assert all(p.dtype == torch.float32 for p in pyr)
    sum(p.sum() for p in pyr).backward()
    assert planes[0].grad.dtype == planes[2].grad.dtype == torch.float32
    # the upsample: bf16 in, bf16 out, bf16 gradient
    src = torch.randn(B, 5, 4, 6, generator=g).to(BF16).requires_grad_(True)
    up = D.upsample_bilinear_torch(src, (8, 11))
    assert up.dtype == BF16 and tuple(up.shape) == (B, 5, 8, 11)
    up.backward(torch.randn(up.shape, generator=g).to(BF16))
    assert src.grad.dtype == BF16 and bool(torch.isfinite(src.grad.float()).all())
    # the finish: bf16 logits, fp32 probabilities (the sigmoid of the WIDENED logit), bf16 gradient of the logits
    logits = (torch.randn(B, n_obj, 8, 12, generator=g) * 3).to(BF16).requires_grad_(True)
    outs = D.refine_train_finish_torch(logits, O, H, W)
    assert outs.dtype == torch.float32 and tuple(outs.shape) == (B, O, H, W) and float(outs.detach()[:, n_obj:].abs().max()) == 0.0
    want = torch.sigmoid(F.interpolate(logits.detach().float(), (H, W)))
    assert torch.equal(outs[:, :n_obj].detach(), want)
    outs.backward(torch.randn(outs.shape, generator=g))
    assert logits.grad.dtype == BF16
    # and on fp32 logits the twin is what it was
    lg32 = logits.detach().float()
    o32 = D.refine_train_finish_torch(lg32, O, H, W)
    assert o32.dtype == torch.float32 and torch.equal(o32[:, :n_obj], torch.sigmoid(F.interpolate(lg32, (H, W))))


@pytest.mark.parametrize("chunks", [1, 3])
def test_bf16_convolution_on_fp32_masters_hands_back_fp32_weight_gradients(chunks):
    """``_ConvStacked`` with bf16 ``x`` and fp32 ``weight`` / ``bias``: the forward is the bf16 convolution on the cast weights;
    the gradient of ``x`` is bf16, those of the masters fp32: the weight's equal to the fp32 sum, in group order, of the groups'
    widened bf16 gradients, the bias's to the fp32 sums of ``dy`` (which the library's bf16 bias gradient is a rounding of:
    2^-7 of the largest is several bf16 ulps of slack on values of mixed magnitude)."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(6, 4, 5, 7, generator=g).to(BF16).requires_grad_(True)
    w = torch.randn(2, 4, 3, 3, generator=g).requires_grad_(True)
    b = torch.randn(2, generator=g).requires_grad_(True)
    d = torch.randn(6, 2, 5, 7, generator=g).to(BF16)
    y = D._ConvStacked.apply(x, w, b, chunks, None)
    assert y.dtype == BF16 and torch.equal(y, F.conv2d(x, w.to(BF16), b.to(BF16), padding=1))
    gx, gw, gb = torch.autograd.grad(y, [x, w, b], d)
    assert gx.dtype == BF16 and gw.dtype == gb.dtype == torch.float32 and gw.shape == w.shape and gb.shape == b.shape
    want_w = want_b = None
    for xc, dc in zip(x.detach().chunk(chunks, 0), d.chunk(chunks, 0)):
        wl, bl = w.detach().to(BF16).requires_grad_(True), b.detach().to(BF16).requires_grad_(True)
        a, c = torch.autograd.grad(F.conv2d(xc, wl, bl, padding=1), [wl, bl], dc)
        want_w = a.float() if want_w is None else want_w + a.float()
        s = dc.sum((0, 2, 3), dtype=torch.float32)                       # the bias: an fp32 sum of the bf16 gradient
        assert float((s - c.float()).abs().max()) <= 2.0 ** -7 * float(s.abs().max())
        want_b = s if want_b is None else want_b + s
    assert torch.equal(gw, want_w) and torch.equal(gb, want_b)
    # a cast pair handed over is used as it is
    pair = (w.detach().to(BF16), b.detach().to(BF16))
    assert torch.equal(D._ConvStacked.apply(x, w, b, chunks, pair), y)


def test_conv_casts_a_slice_once_per_frame_and_sums_its_uses_in_fp32():
    torch.manual_seed(7)
    dec = RSISMask(make_args("concat", hidden=16)).eval()
    sl = dec.train_slices()
    assert all(d.low == {} for d in sl)
    assert all(d.low == {} for d in dec.weight_slices())             # (the no-grad cut never fills it)
    d = sl[0]
    xs = [torch.randn(1, 16, 4, 5).to(BF16) for _ in range(3)]
    n0 = dec.conv_calls
    ys = [dec._conv(x, d["ht"], None, d.low) for x in xs]
    assert dec.conv_calls - n0 == 3 and len(d.low) == 1 and all(y.dtype == BF16 for y in ys)
    (cast, none), = d.low.values()
    assert none is None and cast.dtype == BF16 and not cast.requires_grad and torch.equal(cast, d["ht"].detach().to(BF16))
    cot = [torch.randn(y.shape).to(BF16) for y in ys]
    (got,) = torch.autograd.grad(ys, [dec.clstm_list[0].Gates.weight], cot)
    assert got.dtype == torch.float32
    want = None
    for x, c in zip(xs, cot):
        wl = cast.clone().requires_grad_(True)
        (a,) = torch.autograd.grad(F.conv2d(x, wl, None, padding=1), [wl], c)
        want = a.float() if want is None else want + a.float()
    cin = dec.clstm_list[0].input_size
    assert torch.equal(got[:, cin + 1 + 16:], want) and float(got[:, :cin + 1 + 16].abs().max()) == 0.0
    # fp32 activations: the plain library call, no cast
    y32 = dec._conv(xs[0].float(), d["ht"], None, d.low)
    assert y32.dtype == torch.float32 and len(d.low) == 1


def test_check_names_the_setting():
    with pytest.raises(_lib.DmmError, match="train_dtype = torch.bfloat16 takes bfloat16 skip maps"):
        RSISMask._check_bf16_operands([torch.zeros(1)], [torch.zeros(1)], "train_dtype")
    with pytest.raises(_lib.DmmError, match="float32 mask planes"):
        RSISMask._check_bf16_operands([torch.zeros(1, dtype=BF16)], [torch.zeros(1, dtype=BF16)], "train_dtype")
    RSISMask._check_bf16_operands([torch.zeros(1, dtype=BF16)], [torch.zeros(1)], "train_dtype")


def test_launchers_refuse_cpu_tensors_before_any_call():
    z = lambda *s, dt=BF16: torch.zeros(s, dtype=dt)
    with pytest.raises(_lib.DmmError, match="MI355X"):
        D.clstm_gates_bwd([z(1, 8, 3, 4)], z(1, 3, 3, 4, dt=torch.float32), z(8, 9, dt=torch.float32), None, z(1, 2, 3, 4), None)
    with pytest.raises(_lib.DmmError, match="MI355X"):
        D.upsample_bilinear_bwd(z(1, 2, 6, 8), 0, 2, 3, 4)
    with pytest.raises(_lib.DmmError, match="MI355X"):
        D.refine_train_finish(z(1, 2, 3, 4), 2, 6, 8)
    with pytest.raises(_lib.DmmError, match="MI355X"):
        D.refine_train_finish_bwd(z(1, 2, 3, 4), z(1, 2, 6, 8, dt=torch.float32))


# ---- the entries ------------------------------------------------------------------------------------------------------------
def _lib_loaded():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_the_four_entries_have_prototypes_and_bindings_derived_from_them():
    with open(_lib.HEADER) as f:
        decls, _ = _lib.parse_header(f.read())
    L = _lib_loaded()
    for name in ENTRIES:
        assert name in decls and _lib.SYMBOLS.count(name) == 1, name
        fn, twin = getattr(L, name), getattr(L, name.replace("_bf16", "_f32"))
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == list(decls[name][1])
        assert fn.argtypes == twin.argtypes, name                     # void * where the sibling has float *: the same binding


P = lambda have=True: ctypes.c_void_p(8) if have else None


def _gates_bwd(L, sfx, *, pre0=True, masks=True, wm=True, cp=True, dh=True, dc=True, d_pre=True, d_cp=True, d_m=True, d_w=True,
               ws=True, ws_bytes=None, B=2, Hd=6, h=5, w=7, sb=None, sb_m=None):
    hw = h * w
    sb = 4 * Hd * hw if sb is None else sb
    if ws_bytes is None:
        ws_bytes = int(L.dmm_clstm_gates_bwd_workspace_bytes(B, Hd, h, w))
    return getattr(L, "dmm_clstm_gates_bwd_" + sfx)(P(pre0), P(), P(), sb, sb, sb, P(masks), 3 * hw if sb_m is None else sb_m, P(wm),
                                                    P(cp), B, Hd, h, w, P(dh), P(dc), P(d_pre), P(d_cp), P(d_m), P(d_w), P(ws),
                                                    ws_bytes, None)


def _up_bwd(L, sfx, *, B=2, C=3, H=6, W=10, Cd=5, c0=1, h=3, w=5, d_dst=True, d_src=True, sbd=None, sbs=None):
    return getattr(L, "dmm_upsample_bilinear_bwd_" + sfx)(P(d_dst), Cd * H * W if sbd is None else sbd, B, C, H, W, Cd, c0, P(d_src),
                                                          C * h * w if sbs is None else sbs, h, w, None)


def _fin(L, sfx, *, B=2, O=4, n_obj=3, h=8, w=12, H=15, W=23, logits=True, outs=True, sl=(288, 96)):
    return getattr(L, "dmm_refine_train_finish_" + sfx)(P(logits), sl[0], sl[1], h, w, B, O, n_obj, H, W, P(outs), None)


def _fin_bwd(L, sfx, *, B=2, O=4, n_obj=3, h=8, w=12, H=15, W=23, logits=True, d_outs=True, d_logits=True, sl=(288, 96), sd=None):
    sd = (n_obj * h * w, h * w) if sd is None else sd
    return getattr(L, "dmm_refine_train_finish_bwd_" + sfx)(P(logits), sl[0], sl[1], h, w, P(d_outs), B, O, n_obj, H, W, P(d_logits),
                                                            sd[0], sd[1], None)


BIG = dict(B=1 << 16, O=1 << 10, n_obj=1 << 10, h=1 << 10, w=1 << 10, H=1 << 10, W=1 << 10)
ROWS = {
    _gates_bwd: [dict(pre0=False), dict(masks=False), dict(wm=False), dict(d_pre=False), dict(dh=False, dc=False), dict(cp=False),
                 dict(B=-1), dict(Hd=0), dict(h=0), dict(w=-1), dict(sb=-1), dict(sb_m=3 * 35 - 1), dict(ws=False), dict(ws_bytes=8),
                 dict(B=0), dict(B=0, pre0=False, d_pre=False), dict(B=0, Hd=0), dict(Hd=4 * 65535 + 1),
                 dict(B=1 << 20, h=1 << 12, w=1 << 12)],
    _up_bwd: [dict(B=-1), dict(C=0), dict(H=0), dict(w=0), dict(Cd=0), dict(c0=-1), dict(c0=3), dict(d_dst=False), dict(d_src=False),
              dict(sbd=299), dict(sbs=44), dict(h=7), dict(w=11), dict(h=3, w=4, H=1, W=1), dict(B=0, h=7), dict(B=0),
              dict(B=0, d_dst=False, d_src=False),
              dict(B=1 << 20, C=1 << 10, h=1 << 10, w=1 << 10, H=1 << 10, W=1 << 10, Cd=1 << 10, c0=0, sbd=1 << 30, sbs=1 << 30)],
    _fin: [dict(B=-1), dict(O=-1), dict(n_obj=-1), dict(n_obj=5), dict(h=0), dict(W=0), dict(logits=False), dict(outs=False),
           dict(sl=(-1, 96)), dict(sl=(288, -1)), dict(B=0), dict(B=0, logits=False), dict(B=0, H=0), dict(O=0, n_obj=0), BIG],
    _fin_bwd: [dict(B=-1), dict(O=-1), dict(n_obj=-1), dict(n_obj=5), dict(h=0), dict(W=0), dict(logits=False), dict(d_outs=False),
               dict(d_logits=False), dict(sl=(-1, 96)), dict(sl=(288, -1)), dict(sd=(288, 95)), dict(sd=(-1, 96)), dict(B=0),
               dict(B=0, logits=False), dict(B=0, H=0), dict(n_obj=0, logits=False), BIG],
}


@pytest.mark.parametrize("fn", list(ROWS), ids=lambda f: f.__name__.strip("_"))
def test_bf16_training_entries_answer_as_their_fp32_siblings_without_gpu(fn):
    """Every row is answered before a launch (the pointers are the address 8, not memory), and the bf16 entry's answer is the
    fp32 entry's."""
    L = _lib_loaded()
    seen = set()
    for kw in ROWS[fn]:
        a, b = fn(L, "f32", **kw), fn(L, "bf16", **kw)
        nothing_to_do = kw.get("B") == 0 or kw.get("O") == 0 or kw.get("n_obj") == 0
        assert a in (_lib.DMM_ERR_BAD_ARG, _lib.DMM_ERR_UNSUPPORTED, _lib.DMM_ERR_WORKSPACE) or \
            (a == _lib.DMM_OK and nothing_to_do), (kw, a)
        assert b == a, (kw, a, b)
        seen.add(a)
    assert {_lib.DMM_OK, _lib.DMM_ERR_BAD_ARG, _lib.DMM_ERR_UNSUPPORTED} <= seen
    assert _gates_bwd(L, "bf16", ws_bytes=8) == _lib.DMM_ERR_WORKSPACE and _up_bwd(L, "bf16", h=7) == _lib.DMM_ERR_UNSUPPORTED
