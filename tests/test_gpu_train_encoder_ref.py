"""``TrainEncoder``'s autograd functions and segments against a float64 reference of the same operation on the same bf16
values.  The kernels are tested one by one elsewhere; here the compositions are: ``_conv``'s routes (``_Conv1x1Fn``,
``_Conv3x3Fn``, ``_DetConvFn``, the library and matrix-product fallbacks, with their subsamples, flipped data gradients and
bias sums), every body segment and every pyramid level's heads of ResNet-34 / 50 / 101, in the default and the deterministic
mode, and one whole deterministic step with the decoder's skips against the fp32 encoder.  Achieved errors are recorded
(``record_achieved``); the bounds sit at most 3x above what an MI355X reaches."""
import copy
import gc
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import dmm_net_amd
from dmm_net_amd import train_encoder as te_mod
from dmm_net_amd.encoder import BasicBlock, Bottleneck, FeatureEncoder
from dmm_net_amd.train_encoder import TrainEncoder, _conv, _det_scope
from test_gpu_train_encoder import _grads, _loss, _rel, _tame

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
ULP = 2.0 ** -8                          # bf16: 8 significant bits


@pytest.fixture(autouse=True)
def _release():
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _record(name, v):
    from conftest import record_achieved
    record_achieved(name, v)


def _modes(det):
    """The mode for an op called outside a TrainEncoder call, with the library flags the encoder's own calls run under."""
    class _Both:
        def __enter__(self):
            self.a, self.b = dmm_net_amd.deterministic(det), _det_scope(det)
            self.a.__enter__(), self.b.__enter__()

        def __exit__(self, *exc):
            self.b.__exit__(*exc)
            return self.a.__exit__(*exc)
    return _Both()


# ---- op level: _conv on every route ------------------------------------------------------------------------------------
# name: (ci, co, kernel, stride, padding, bias, (B, H, W)),
#       routes with (linear_1x1, own_wgrad) = (True, True), (False, True), (True, False) in the default mode
#       ("lib": F.conv2d, which the deterministic mode replaces by _DetConvFn; "linear": F.linear on the activation matrix)
OPS = {
    "1x1_s1": ((256, 64, 1, 1, 0, False, (2, 17, 23)), ("1x1", "lib", "linear")),
    "1x1_s2_even": ((256, 512, 1, 2, 0, False, (2, 16, 24)), ("1x1", "lib", "linear")),
    "1x1_s2_odd": ((256, 512, 1, 2, 0, False, (2, 17, 23)), ("1x1", "lib", "linear")),
    "3x3_s1_square": ((64, 64, 3, 1, 1, False, (2, 17, 23)), ("3x3", "3x3", "lib")),
    "3x3_s1_wide": ((64, 128, 3, 1, 1, False, (2, 17, 23)), ("3x3", "3x3", "lib")),
    "3x3_s2_odd": ((128, 128, 3, 2, 1, False, (2, 17, 23)), ("3x3", "3x3", "lib")),
    "3x3_bias64": ((512, 64, 3, 1, 1, True, (2, 9, 13)), ("3x3", "3x3", "lib")),         # bias: _channel_sums' kernel
    "3x3_bias192": ((192, 192, 3, 1, 1, True, (2, 9, 13)), ("3x3", "3x3", "lib")),       # 256 % 24 != 0: its torch sum
    "head_3x3_32out": ((256, 32, 3, 1, 1, True, (2, 17, 23)), ("lib", "lib", "lib")),    # prop2[0] / sk2 of ResNet-50
    "head_3x3_32in": ((32, 128, 3, 1, 1, True, (2, 17, 23)), ("lib", "lib", "lib")),     # prop2[3]
    "stem_7x7": ((3, 64, 7, 2, 3, False, (2, 67, 97)), ("lib", "lib", "lib")),
}
SWITCHES = {"fast": (True, True), "no_linear_1x1": (False, True), "no_own_wgrad": (True, False)}


def _route(y):
    """Which of _conv's routes produced y, from the autograd nodes behind it."""
    names, todo = set(), [y.grad_fn]
    while todo:
        n = todo.pop()
        if n is not None:
            names.add(type(n).__name__)
            todo += [m for m, _ in n.next_functions]
    for node, route in (("_Conv1x1FnBackward", "1x1"), ("_Conv3x3FnBackward", "3x3"), ("_DetConvFnBackward", "det"),
                        ("ConvolutionBackward0", "lib")):
        if node in names:
            return route
    return "linear"


def _elementwise(got, ref, pre=None):
    """max over elements of |got - ref| / (2^-8 |ref| + 1e-3 max|ref|): <= 1 is the bound of a bf16 result.  ``pre``: the
    convolution before its bias, which the libraries round to bf16 before they add the bias -- a second rounding, of |pre|."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    tol = ULP * ref.abs() + 1e-3 * float(ref.abs().max())
    if pre is not None:
        tol = tol + ULP * pre.detach().abs()
    return float(((got - ref).abs() / tol.clamp_min(1e-300)).max())


@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
@pytest.mark.parametrize("switch", list(SWITCHES))
@pytest.mark.parametrize("case", list(OPS))
def test_conv_routes_against_fp64(case, switch, det, monkeypatch):
    """``_conv(x, m, bf16, linear_1x1, own_wgrad)`` against fp64 ``F.conv2d`` autograd of the same bf16 x, dy and the
    bf16-rounded weight and bias: y, dx, dw, db.  bf16 results (y, dx, the libraries' and ``_DetConvFn``'s dw / db) within
    2^-8 |ref| + 1e-3 max|ref| elementwise; ``dmm_wgrad*``'s fp32 dw within 1e-4 max|ref|; ``_channel_sums``' bias as in
    ``test_bias_gradient_through_the_statistics_kernel``.  Each case must take the route it was built for."""
    (ci, co, k, stride, pad, bias, (B, H, W)), routes = OPS[case]
    linear_1x1, own_wgrad = SWITCHES[switch]
    want = routes[list(SWITCHES).index(switch)]
    want = "det" if (det and want == "lib") else want
    g = torch.Generator(device=DEV).manual_seed(sum(map(ord, case)))
    m = nn.Conv2d(ci, co, k, stride, pad, bias=bias).to(DEV)
    with torch.no_grad():
        m.weight.normal_(0.0, 1.0 / math.sqrt(ci * k * k), generator=g)
        if bias:
            m.bias.normal_(0.0, 0.5, generator=g)
    x = torch.randn((B, ci, H, W), generator=g, device=DEV).relu().bfloat16().contiguous(memory_format=CL)
    wgrads, sums = [], []
    real_wgrad, real_sums = te_mod._wgrad, te_mod._channel_sums
    monkeypatch.setattr(te_mod, "_wgrad", lambda rec: (wgrads.append(rec[0]), real_wgrad(rec))[1])
    monkeypatch.setattr(te_mod, "_channel_sums", lambda dy, det=False: (sums.append(det), real_sums(dy, det))[1])
    xg = x.clone().requires_grad_(True)
    with _modes(det):
        y = _conv(xg, m, torch.bfloat16, linear_1x1, own_wgrad)
    assert y.dtype == torch.bfloat16
    assert _route(y) == want, (_route(y), want)
    if want == "3x3":
        assert y.grad_fn.flipped == (stride == 1 and ci == co) and y.grad_fn.det == det
    dy = torch.randn(y.shape, generator=g, device=DEV).bfloat16().contiguous(memory_format=CL)
    y.backward(dy)
    torch.cuda.synchronize()
    own = want in ("1x1", "3x3")
    assert wgrads == ([want] if own else [])                      # dmm_wgrad* wrote the master's fp32 gradient
    assert sums == ([det] if (want == "3x3" and bias) else [])

    # fp64 reference on the host, from the same bf16 values
    x64 = x.double().cpu().requires_grad_(True)
    w64 = m.weight.detach().bfloat16().double().cpu().requires_grad_(True)
    b64 = m.bias.detach().bfloat16().double().cpu().requires_grad_(True) if bias else None
    ry = F.conv2d(x64, w64, b64, stride, pad)
    rgrads = torch.autograd.grad(ry, [x64, w64] + ([b64] if bias else []), dy.double().cpu())

    tag = f"train_encoder_ref/op/{case}/{switch}/{'det' if det else 'default'}"
    errs = {"y": _elementwise(y, ry, None if not bias else ry - b64.view(1, -1, 1, 1)), "dx": _elementwise(xg.grad, rgrads[0])}
    if own:                                                       # fp32 from dmm_wgrad*
        errs["dw_fp32"] = float((m.weight.grad.double().cpu() - rgrads[1]).abs().max()) / float(rgrads[1].abs().max())
    else:
        errs["dw"] = _elementwise(m.weight.grad, rgrads[1])
    if bias:
        rdb = rgrads[2]
        if want == "3x3":                                         # fp32 channel sums (kernel or torch), not rounded to bf16
            scale = 1e-4 * (1 + float(rdb.abs().max())) * math.sqrt(dy.numel() / co)
            errs["db_sums"] = float((m.bias.grad.double().cpu() - rdb).abs().max()) / scale
        else:
            errs["db"] = _elementwise(m.bias.grad, rdb)
    for k_, v in errs.items():
        _record(f"{tag}/{k_}", v)
    # MIOpen's default bf16 solvers (outside cudnn.deterministic) may round twice: up to 1.44x a single rounding's bound on
    # the 7x7 stem's forward and a 32-channel head's data gradient; under cudnn.deterministic they stay within one rounding
    lim = {"dw_fp32": 1e-4, "db_sums": 1.0, "db": 1.0}
    twice = not det and want in ("lib", "3x3")
    bad = {k_: v for k_, v in errs.items() if not (v <= lim.get(k_, 2.0 if twice else 1.0))}
    assert not bad, bad


# ---- segment level: every segment of the chain and the heads, fp64 reference of the encoder's own modules -------------
SEGMENTS = [("resnet50", (2, 128, 224)), ("resnet50", (2, 97, 161)), ("resnet34", (2, 112, 176)), ("resnet101", (2, 96, 160))]

# bounds by segment kind and quantity (relative L2 error, worst output channel, bias-before-BatchNorm), about 2.5x the largest
# value an MI355X reached over the four cases, both modes and default-vs-deterministic (all recorded: parity_achieved.jsonl,
# profiles/r08_train_encoder_ref_achieved.jsonl).  Outputs and running statistics sit near bf16 rounding.  Gradients do
# not, and cannot: the stem's max-pool and every ReLU pick their branch on bf16 values, and wherever two candidates lie
# within a rounding of each other, one bf16 evaluation routes the whole gradient element
# elsewhere.  The default and the deterministic step -- the same kernels but for their summation orders -- differ from each
# other as much as either differs from fp64 (stem dx 8 %, ResNet-101 layer3's eight-block runs 13-19 %).
BOUNDS = {
    "stem": {"out_rel": 0.01, "out_ch": 0.011, "dx_rel": 0.2, "dx_ch": 0.2, "grad_rel": 0.2, "grad_ch": 0.45,
             "stat_rel": 0.012, "stat_ch": 0.17},
    "body": {"out_rel": 0.02, "out_ch": 0.03, "dx_rel": 0.3, "dx_ch": 0.8, "grad_rel": 0.45, "grad_ch": 20.0,
             "stat_rel": 0.01, "stat_ch": 0.25},
    "heads": {"out_rel": 0.016, "out_ch": 0.025, "dx_rel": 0.1, "dx_ch": 0.15, "grad_rel": 0.16, "grad_ch": 6.0,
              "stat_rel": 0.008, "stat_ch": 0.075, "bias_abs": 0.8},
}


def _bf16_store(mod, inp, out):
    """Forward hook: the output as the bf16 step stores it (rounded to bf16), the gradient passed straight through."""
    return out + (out.bfloat16().double() - out).detach()


def _ref_copy(enc):
    """float64 host copy of the encoder whose convolution weights and biases went through bf16 (what the kernels read), and
    whose activations are rounded to bf16 where the bf16 step stores them: every convolution's output, every BatchNorm (+ ReLU)
    output, and a residual block's output after the add and ReLU (its last BatchNorm feeds the add unrounded, as in the fused
    kernel).  Arithmetic stays float64, so the reference's batch statistics and outputs are those of the activations the bf16
    step actually holds, and the bounds measure what the kernels add."""
    r = copy.deepcopy(enc).cpu().double().train()
    with torch.no_grad():
        for m in r.modules():
            if isinstance(m, nn.Conv2d):
                m.weight.copy_(m.weight.bfloat16().double())
                if m.bias is not None:
                    m.bias.copy_(m.bias.bfloat16().double())
    blocks = [m for m in r.modules() if isinstance(m, (Bottleneck, BasicBlock))]
    into_add = {id(b.bn3 if isinstance(b, Bottleneck) else b.bn2) for b in blocks}
    for m in r.modules():
        if isinstance(m, (nn.Conv2d, nn.BatchNorm2d, Bottleneck, BasicBlock)) and id(m) not in into_add:
            m.register_forward_hook(_bf16_store)
    return r


def _errs(got, ref, ch_dim):
    """(relative L2 error, worst output channel's relative L2 error).  A channel's error is taken relative to its own norm,
    but at least to a tenth of the channels' RMS norm (a channel that is nearly zero is judged against the typical one)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    d = got - ref
    rel = float(d.norm()) / max(float(ref.norm()), 1e-300)
    if ref.dim() == 0:
        return rel, rel
    C = ref.shape[ch_dim]
    dc = d.transpose(0, ch_dim).reshape(C, -1).norm(dim=1)
    rc = ref.transpose(0, ch_dim).reshape(C, -1).norm(dim=1)
    floor = max(0.1 * float(rc.square().mean().sqrt()), 1e-300)
    return rel, float((dc / rc.clamp_min(floor)).max())


class _Worst:
    """The largest error per quantity over the tensors of one segment (and which tensor it was)."""

    def __init__(self):
        self.v = {}

    def add(self, q, val, what):
        if q not in self.v or val > self.v[q][0] or math.isnan(val):
            self.v[q] = (val, what)

    def pair(self, q, rel_ch, what):
        self.add(f"{q}_rel", rel_ch[0], what)
        self.add(f"{q}_ch", rel_ch[1], what)


def _seg_names(te, name):
    """Names (in the wrapped encoder, and so in every copy of it) of the parameters and buffers of one segment."""
    enc = te.src
    mods = te._head_modules(int(name[5:])) if name.startswith("heads") else te._seg_modules()[name]
    pre = tuple(_mname(enc, m) for m in mods)
    return ([n for n, _ in enc.named_parameters() if n.startswith(pre)], [n for n, _ in enc.named_buffers() if n.startswith(pre)])


def _mname(root, mod):
    return next(n for n, m in root.named_modules() if m is mod) + "."


def _seg_run(te, name, x, cots, det):
    """One eager segment of ``te`` (body: ``_seg_body``; heads ``heads<k>``: ``_head_level(k)``) forward and backward, as an
    encoder call runs it.  -> (outputs, dx, {parameter: grad}, {buffer: (before, after)})"""
    enc = te.src
    params, bufs = _seg_names(te, name)
    before = {n: enc.get_buffer(n).clone() for n in bufs}
    enc.zero_grad(set_to_none=True)
    te._ticked.clear()
    xg = x.clone().requires_grad_(True)
    with _modes(det):
        outs = te._head_level(int(name[5:]), xg) if name.startswith("heads") else te._seg_body(name, xg)
        torch.autograd.backward(list(outs), list(cots))
    torch.cuda.synchronize()
    return ([o.detach() for o in outs], xg.grad, {n: enc.get_parameter(n).grad for n in params},
            {n: (before[n], enc.get_buffer(n).clone()) for n in bufs})


def _ref_run(ref, te, name, x, cot_gen):
    """The same segment with the encoder's own modules, float64, training mode, on the host; the cotangents are drawn for its
    outputs' shapes.  -> (the same tuple as ``_seg_run``, {bias before a BatchNorm: sum of |its incoming gradient|}, cots)"""
    body = ref.base
    params, bufs = _seg_names(te, name)
    ref.zero_grad(set_to_none=True)
    bias_in, hooks = {}, []
    if name.startswith("heads"):                  # every head convolution has a bias and feeds a BatchNorm
        k = int(name[5:])
        for conv in (getattr(ref, f"prop{k}")[0], getattr(ref, f"prop{k}")[3], getattr(ref, f"sk{k}")):
            def fwd(mod, inp, out, key=_mname(ref, conv) + "bias"):
                out.register_hook(lambda g_: bias_in.__setitem__(key, g_.abs().sum((0, 2, 3))))
            hooks.append(conv.register_forward_hook(fwd))
    before = {n: ref.get_buffer(n).clone() for n in bufs}
    xr = x.double().cpu().requires_grad_(True)
    if name == "stem":
        outs = (body.maxpool(F.relu(body.bn1(body.conv1(xr)))),)
    elif name.startswith("heads"):
        k = int(name[5:])
        outs = (getattr(ref, f"prop{k}")(xr), getattr(ref, f"bn{k}")(getattr(ref, f"sk{k}")(xr)))
    else:
        h = xr
        for blk in next(c[1] for c in te._chain if c[0] == name):
            h = ref.get_submodule(_mname(te.src, blk)[:-1])(h)
        outs = (h,)
    cots = cot_gen([tuple(o.shape) for o in outs])
    torch.autograd.backward(list(outs), [c.double().cpu() for c in cots])
    for h_ in hooks:
        h_.remove()
    got = ([o.detach() for o in outs], xr.grad, {n: ref.get_parameter(n).grad for n in params},
           {n: (before[n], ref.get_buffer(n).clone()) for n in bufs})
    return got, bias_in, cots


def _compare(got, want, biases, worst, tag):
    """Record the worst error per quantity of ``got`` against ``want`` (both as ``_seg_run`` returns them)."""
    outs, dx, grads, stats = got
    routs, rdx, rgrads, rstats = want
    assert len(outs) == len(routs)
    for i, (o, ro) in enumerate(zip(outs, routs)):
        assert tuple(o.shape) == tuple(ro.shape), (tag, i)
        worst.pair("out", _errs(o, ro, 1), f"out{i}")
    worst.pair("dx", _errs(dx, rdx, 1), "dx")
    assert grads.keys() == rgrads.keys() and len(grads) > 0
    for n, gp in grads.items():
        rg = rgrads[n]
        assert gp is not None and rg is not None, (tag, n)
        if n in biases:                           # zero up to rounding: against the sum of the |gradient| it sums
            err = float(((gp.double().cpu() - rg.double().cpu()).abs() / (ULP * biases[n]).clamp_min(1e-300)).max())
            worst.add("bias_abs", err, n)
        else:
            worst.pair("grad", _errs(gp, rg, 0), n)
    assert stats.keys() == rstats.keys() and len(stats) > 0
    for n, (b0, b1) in stats.items():
        r0, r1 = rstats[n]
        if n.endswith("num_batches_tracked"):
            assert int(b1) - int(b0) == int(r1) - int(r0), (tag, n, int(b1) - int(b0), int(r1) - int(r0))
        else:                                     # the update (momentum x (statistic - old)): the old value cancels
            worst.pair("stat", _errs(b1 - b0, r1.to(b1.device) - r0.to(b1.device), 0), n)


def _check(worst, tag, kind, failures):
    for q, (v, what) in sorted(worst.v.items()):
        _record(f"{tag}/{q}", v)
        if not (v <= BOUNDS[kind][q]):
            failures.append(f"{tag}/{q} = {v:.3g} ({what}) > {BOUNDS[kind][q]:.3g}")


@pytest.mark.parametrize("arch,size", SEGMENTS, ids=[f"{a}_{b}x{h}x{w}" for a, (b, h, w) in SEGMENTS])
def test_segments_against_fp64(arch, size):
    """Every segment of ``TrainEncoder.segments`` (``_seg_body`` of the chain, ``_head_level(k)`` with the skips) run eagerly
    in bf16, in the default and the deterministic mode, against the encoder's own modules in float64 on the host (a copy with
    bf16-rounded convolution weights): outputs, dx, every parameter gradient of the fp32 masters, every BatchNorm's running
    statistics update and ``num_batches_tracked``; default and deterministic results within the same bounds of each other."""
    torch.manual_seed(8)
    B, H, W = size
    enc = _tame(FeatureEncoder(arch).to(DEV).train())
    ref = _ref_copy(enc)
    tes = {det: TrainEncoder(copy.deepcopy(enc), graphs=False) for det in (False, True)}
    te = tes[False]
    assert te.skips_need_grad
    gen = torch.Generator().manual_seed(B * H * W)

    def cot_gen(shapes):                          # heads: (prop: fp32 NCHW, skip: bf16); body: one bf16 output
        return [torch.randn(sh, generator=gen).to(DEV) if len(shapes) == 2 and i == 0 else
                torch.randn(sh, generator=gen).bfloat16().to(DEV).contiguous(memory_format=CL) for i, sh in enumerate(shapes)]
    shape, taps, failures, seen = (B, 3, H, W), {}, [], []
    order = [(n, tap) for n, _, tap in te._chain] + [(f"heads{k}", None) for k in (2, 3, 4, 5)]
    for name, tap in order:
        seen.append(name if not name.startswith("heads") else "heads")
        if name.startswith("heads"):
            shape = taps[int(name[5:])]
        x = torch.randn(shape, generator=gen)
        x = (x if name == "stem" else x.relu()).bfloat16().to(DEV).contiguous(memory_format=CL)   # (the stem takes an image)
        want, biases, cots = _ref_run(ref, te, name, x, cot_gen)
        tag = f"train_encoder_ref/seg/{arch}_{B}x{H}x{W}/{name}"
        kind = "stem" if name == "stem" else ("heads" if name.startswith("heads") else "body")
        got = {}
        for det in (False, True):
            got[det] = _seg_run(tes[det], name, x, cots, det)
            worst = _Worst()
            _compare(got[det], want, biases, worst, tag)
            _check(worst, f"{tag}/{'det' if det else 'default'}", kind, failures)
        worst = _Worst()                          # default against deterministic: within the same bounds
        _compare(got[False], got[True], biases, worst, tag)
        _check(worst, f"{tag}/default_vs_det", kind, failures)
        if tap is not None:
            taps[tap + 2] = tuple(want[0][0].shape)
        if not name.startswith("heads"):
            shape = tuple(want[0][0].shape)
    assert tuple(dict.fromkeys(seen)) == te.segments
    assert not failures, failures


# ---- the whole encoder: a deterministic eager step with the decoder's skips --------------------------------------------
def test_deterministic_eager_step_with_skips_is_as_close_to_fp32_as_the_default_step(monkeypatch):
    """A ResNet-50 eager step in the deterministic mode with ``skips_need_grad=True`` and a loss on ``refine_input_feat`` too
    -- where the eager path adds each tap's body and head gradients in ``_TapSplit`` and runs the stem and the 32-channel
    heads through ``_DetConvFn`` -- against the fp32 ``FeatureEncoder``: as close as the default-mode eager step (x 1.15 +
    0.02), every gradient aligned (cosine >= 0.85)."""
    torch.manual_seed(12)
    ref = _tame(FeatureEncoder("resnet50").to(DEV).train())
    a, b = copy.deepcopy(ref), copy.deepcopy(ref)
    det_te, def_te = TrainEncoder(a, graphs=False), TrainEncoder(b, graphs=False)
    calls = {"_TapSplit": 0, "_DetConvFn": 0}
    for name in calls:
        base = getattr(te_mod, name)

        def apply(*args, base=base, name=name):
            calls[name] += 1
            return base.apply(*args)
        monkeypatch.setattr(te_mod, name, type(name, (), {"apply": staticmethod(apply)}))
    img = torch.randn(4, 3, 128, 224, device=DEV)
    for m in (ref, a, b):
        m.zero_grad(set_to_none=True)
    _loss(ref(img)).backward()
    with dmm_net_amd.deterministic():
        _loss(det_te(img)).backward()
    assert calls == {"_TapSplit": 3, "_DetConvFn": 4}, calls      # taps x2..x4; the stem, both of prop2, sk2
    with dmm_net_amd.deterministic(False):
        _loss(def_te(img)).backward()
    assert calls == {"_TapSplit": 3, "_DetConvFn": 4}, calls
    gd, ge, gr = _grads(a), _grads(b), _grads(ref)
    assert all((gd[k] is None) == (gr[k] is None) == (ge[k] is None) for k in gr)
    assert all(gd[k] is not None for k in gd if k.startswith(("sk", "bn", "prop")))
    bad = [k for k, v in gd.items() if v is not None and not bool(torch.isfinite(v).all())]
    assert not bad, bad[:4]
    e_det, e_def = _rel(gd, gr), _rel(ge, gr)
    ks = [k for k in gr if gr[k] is not None]
    dot = sum(float((gd[k] * gr[k]).sum()) for k in ks)
    cos = dot / math.sqrt(sum(float(gd[k].square().sum()) for k in ks) * sum(float(gr[k].square().sum()) for k in ks))
    _record("train_encoder_ref/step/det_vs_fp32", e_det)
    _record("train_encoder_ref/step/default_vs_fp32", e_def)
    _record("train_encoder_ref/step/det_cos_vs_fp32", cos)
    assert e_det <= 1.15 * e_def + 0.02, (e_det, e_def)
    assert cos >= 0.85, cos
