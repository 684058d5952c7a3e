"""``dmm_conv3x3_bf16`` on the GPU (include/dmm_match.h (10d), ``ops.conv3x3_bf16`` / ``ops.conv3x3_dgrad_bf16``): y and dx
against the float64 reference of tests/conv_ref.py, bit-identical repeats, guard bands round every buffer, independence of the
batch -- and the deterministic ``TrainEncoder`` step with ``set_deterministic_conv("own")``: bit-reproducible eagerly and in
graph replay, as close to the fp32 encoder as the ``"library"`` step, no MIOpen convolution behind an in-envelope 3x3."""
import copy
import gc
import math
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import dmm_net_amd
from conv_ref import CASES, CL, case_id, elementwise, flipped, inputs, out_hw, record, reference
from dmm_net_amd import _lib, ops
from dmm_net_amd import train_encoder as te_mod
from dmm_net_amd.train_encoder import TrainEncoder, _conv, _det_scope

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIAS = [False, True]


@pytest.fixture(autouse=True)
def _restore_and_release():
    yield
    dmm_net_amd.set_deterministic_conv("library")
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _dev(case, bias):
    x, w, b, dy = (t.to(DEV) for t in inputs(case))
    x, w, dy = x.contiguous(memory_format=CL), w.contiguous(memory_format=CL), dy.contiguous(memory_format=CL)
    return x, w, (b if bias else None), dy


def _tag(case, bias):
    return f"{case_id(case)}_{'bias' if bias else 'nobias'}"


# ---- the kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", BIAS, ids=["nobias", "bias"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_y_and_dx_against_fp64(case, bias):
    ci, co, stride, B, H, W = case
    x, w, b, dy = _dev(case, bias)
    y = ops.conv3x3_bf16(x, w, b, stride)
    dx = ops.conv3x3_dgrad_bf16(dy, flipped(w), (H, W), stride)
    torch.cuda.synchronize()
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (B, co) + out_hw(H, W, stride) and y.is_contiguous(memory_format=CL)
    assert dx.dtype == torch.bfloat16 and dx.shape == x.shape and dx.is_contiguous(memory_format=CL)
    ry, rdx = reference(case)
    if bias:
        ry = ry + b.double().cpu().view(1, -1, 1, 1)
    ey, edx = elementwise(y, ry), elementwise(dx, rdx)
    record(f"{_tag(case, bias)}/y", ey)
    record(f"{_tag(case, bias)}/dx", edx)
    print(f"conv3x3 {_tag(case, bias)}: y {ey:.3f} dx {edx:.3f}")
    assert ey <= 1.0 and edx <= 1.0, (ey, edx)


@pytest.mark.parametrize("bias", BIAS, ids=["nobias", "bias"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_three_calls_are_bit_identical(case, bias):
    ci, co, stride, B, H, W = case
    x, w, b, dy = _dev(case, bias)
    wt = flipped(w)
    ys = [ops.conv3x3_bf16(x, w, b, stride) for _ in range(3)]
    dxs = [ops.conv3x3_dgrad_bf16(dy, wt, (H, W), stride) for _ in range(3)]
    torch.cuda.synchronize()
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])
    assert torch.equal(dxs[0], dxs[1]) and torch.equal(dxs[0], dxs[2])


def _banded(n, dtype, fill, margin):
    """A tensor of n elements inside a larger allocation whose margins hold ``fill`` -> (whole, the inner view)."""
    whole = torch.full((n + 2 * margin,), fill, dtype=dtype, device=DEV)
    return whole, whole[margin:margin + n]


@pytest.mark.parametrize("bias", BIAS, ids=["nobias", "bias"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_guard_bands(case, bias):
    """x, w (and the bias) sit between NaNs, y and the workspace between sentinels: no NaN reaches y (a masked piece that was
    fetched from beyond the tensor instead of zeroed would show), y is what the plain call gives, the sentinels are intact."""
    ci, co, stride, B, H, W = case
    x, w, b, _ = _dev(case, bias)
    Ho, Wo = out_hw(H, W, stride)
    M = 4096                                              # elements: keeps every inner view 16-byte aligned
    nan = float("nan")
    xa, xv = _banded(x.numel(), torch.bfloat16, nan, M)
    wa, wv = _banded(w.numel(), torch.bfloat16, nan, M)
    xv.copy_(x.permute(0, 2, 3, 1).reshape(-1))
    wv.copy_(w.permute(0, 2, 3, 1).reshape(-1))
    xg = xv.view(B, H, W, ci).permute(0, 3, 1, 2)
    wg = wv.view(co, 3, 3, ci).permute(0, 3, 1, 2)
    assert xg.is_contiguous(memory_format=CL) and wg.is_contiguous(memory_format=CL)
    bg = None
    if bias:
        ba, bg = _banded(co, torch.bfloat16, nan, M)
        bg.copy_(b)
    SENT = -12345.0                                       # exact in bf16; no convolution of these inputs comes near it
    ya, yv = _banded(B * Ho * Wo * co, torch.bfloat16, SENT, M)
    yv.fill_(nan)                                         # (the interior must be overwritten whole)
    yg = yv.view(B, Ho, Wo, co).permute(0, 3, 1, 2)
    need = int(_lib.load().dmm_conv3x3_workspace_bytes(B, H, W, ci, co, stride))
    ws_all, ws = _banded(need, torch.uint8, 0xA5, 4 * M)
    got = ops.conv3x3_bf16(xg, wg, bg, stride, out=yg, workspace=ws if need else None)
    plain = ops.conv3x3_bf16(x, w, b, stride)
    torch.cuda.synchronize()
    assert got.data_ptr() == yg.data_ptr()
    assert not bool(torch.isnan(yv).any()), "a NaN from a margin (or an unwritten output) reached y"
    assert torch.equal(got, plain)
    assert bool((ya[:M] == SENT).all()) and bool((ya[-M:] == SENT).all()), "a store outside y"
    assert bool((ws_all[:4 * M] == 0xA5).all()) and bool((ws_all[4 * M + need:] == 0xA5).all()), "a store outside the workspace"
    assert bool(torch.isnan(xa[:M]).all()) and bool(torch.isnan(xa[-M:]).all()) and bool(torch.isnan(wa[:M]).all()) \
        and bool(torch.isnan(wa[-M:]).all())


@pytest.mark.parametrize("bias", BIAS, ids=["nobias", "bias"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_an_image_does_not_depend_on_its_batch(case, bias):
    """Image 0 of a B = 3 call equals the B = 1 call bit for bit: the summation order is a function of the problem's shape
    without the batch (the K splits among it)."""
    ci, co, stride, B, H, W = case
    x, w, b, dy = _dev(case, bias)
    g = torch.Generator(device=DEV).manual_seed(7)
    x3 = torch.cat([x[:1], torch.randn((2, ci, H, W), generator=g, device=DEV).bfloat16()], 0).contiguous(memory_format=CL)
    dy3 = torch.cat([dy[:1], torch.randn((2,) + tuple(dy.shape[1:]), generator=g, device=DEV).bfloat16()], 0).contiguous(memory_format=CL)
    x1, dy1 = x[:1].contiguous(memory_format=CL), dy[:1].contiguous(memory_format=CL)
    wt = flipped(w)
    y3, y1 = ops.conv3x3_bf16(x3, w, b, stride), ops.conv3x3_bf16(x1, w, b, stride)
    d3, d1 = ops.conv3x3_dgrad_bf16(dy3, wt, (H, W), stride), ops.conv3x3_dgrad_bf16(dy1, wt, (H, W), stride)
    torch.cuda.synchronize()
    assert torch.equal(y3[:1], y1) and torch.equal(d3[:1], d1)


def test_op_rejects_what_the_kernel_does_not_take():
    x = torch.zeros((1, 64, 4, 4), dtype=torch.bfloat16, device=DEV).contiguous(memory_format=CL)
    w = torch.zeros((64, 64, 3, 3), dtype=torch.bfloat16, device=DEV).contiguous(memory_format=CL)
    for args in ((x[:, :32], w[:, :32]), (x.float(), w), (x, w[:32]), (x, w, None, 3), (x, w, torch.zeros(64, device=DEV))):
        with pytest.raises(_lib.DmmError):
            ops.conv3x3_bf16(*args)
    with pytest.raises(_lib.DmmError):
        ops.conv3x3_bf16(x.cpu(), w.cpu())


# ---- _conv's route in the mode --------------------------------------------------------------------------------------------
def _modes(det, which):
    class _Both:
        def __enter__(self):
            dmm_net_amd.set_deterministic_conv(which)
            self.a, self.b = dmm_net_amd.deterministic(det), _det_scope(det)
            self.a.__enter__(), self.b.__enter__()

        def __exit__(self, *exc):
            self.b.__exit__(*exc)
            r = self.a.__exit__(*exc)
            dmm_net_amd.set_deterministic_conv("library")
            return r
    return _Both()


@pytest.mark.parametrize("ci,co,stride,bias", [(64, 64, 1, False), (64, 128, 1, True), (128, 128, 2, False), (128, 64, 2, True)])
def test_in_envelope_conv_under_own_launches_no_miopen_convolution(ci, co, stride, bias, monkeypatch):
    """``_conv`` of an in-envelope 3x3 convolution in the deterministic mode with "own": the autograd node is still
    ``_Conv3x3Fn``, neither its forward nor its backward reaches ``F.conv2d`` / ``aten.convolution_backward`` (both raise
    here), and y, dx, dw, db hold their bounds against fp64.  The setting alone, outside the mode, changes nothing."""
    from test_gpu_train_encoder_ref import _route
    B, H, W = 2, 17, 23
    g = torch.Generator(device=DEV).manual_seed(ci + co + stride)
    m = nn.Conv2d(ci, co, 3, stride, 1, bias=bias).to(DEV)
    with torch.no_grad():
        m.weight.normal_(0.0, 1.0 / math.sqrt(9 * ci), generator=g)
        if bias:
            m.bias.normal_(0.0, 0.5, generator=g)
    x = torch.randn((B, ci, H, W), generator=g, device=DEV).relu().bfloat16().contiguous(memory_format=CL)

    def boom(*a, **k):
        raise AssertionError("a library convolution was called")
    real_F = te_mod.F
    proxy = types.SimpleNamespace(**{k: getattr(real_F, k) for k in dir(real_F) if not k.startswith("__")})
    proxy.conv2d = boom
    xg = x.clone().requires_grad_(True)
    with monkeypatch.context() as mp:
        mp.setattr(te_mod, "F", proxy)
        with _modes(True, "own"):
            y = _conv(xg, m, torch.bfloat16)
        assert _route(y) == "3x3" and y.grad_fn.own and y.grad_fn.det and y.grad_fn.flipped
        dy = torch.randn(y.shape, generator=g, device=DEV).bfloat16().contiguous(memory_format=CL)
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
            y.backward(dy)
        torch.cuda.synchronize()
        names = {e.key for e in prof.key_averages()}
        assert not any("convolution" in n or "conv2d" in n for n in names), sorted(n for n in names if "conv" in n)
    x64 = x.double().cpu().requires_grad_(True)
    w64 = m.weight.detach().bfloat16().double().cpu().requires_grad_(True)
    b64 = m.bias.detach().bfloat16().double().cpu().requires_grad_(True) if bias else None
    ry = F.conv2d(x64, w64, b64, stride, 1)
    rg = torch.autograd.grad(ry, [x64, w64] + ([b64] if bias else []), dy.double().cpu())
    ey, edx = elementwise(y, ry), elementwise(xg.grad, rg[0])
    edw = float((m.weight.grad.double().cpu() - rg[1]).abs().max()) / float(rg[1].abs().max())
    record(f"route/{ci}_{co}_s{stride}/y", ey)
    record(f"route/{ci}_{co}_s{stride}/dx", edx)
    assert ey <= 1.0 and edx <= 1.0 and edw <= 1e-4, (ey, edx, edw)       # (dw: dmm_wgrad3x3's fp32 bound, as in the ref tests)
    if bias:
        scale = 1e-4 * (1 + float(rg[2].abs().max())) * math.sqrt(dy.numel() / co)
        assert float((m.bias.grad.double().cpu() - rg[2]).abs().max()) <= scale
    # outside the mode the setting does nothing: the library route, flag off
    with _modes(False, "own"):
        y2 = _conv(x.clone().requires_grad_(True), m, torch.bfloat16)
    assert _route(y2) == "3x3" and not y2.grad_fn.own
    # out of the envelope (32 output channels) the mode's stock route stays
    m32 = nn.Conv2d(ci, 32, 3, 1, 1).to(DEV)
    with _modes(True, "own"):
        assert _route(_conv(x.clone().requires_grad_(True), m32, torch.bfloat16)) == "det"


def test_det_conv_as_one_gemm_under_own_against_fp64():
    """``_DetConvFn`` with "own": the 7x7 stem and the 32-channel heads, forward and stride-1 data gradient as unfold + one
    GEMM, against fp64 (the bias is added to the rounded product: a second rounding, the ``pre`` term of the reference
    tests), three runs bit-identical."""
    g = torch.Generator(device=DEV).manual_seed(5)
    for ci, co, k, stride, pad, bias, shape in ((3, 64, 7, 2, 3, False, (2, 67, 97)), (256, 32, 3, 1, 1, True, (2, 17, 23)),
                                                (32, 128, 3, 1, 1, True, (2, 17, 23))):
        m = nn.Conv2d(ci, co, k, stride, pad, bias=bias).to(DEV)
        with torch.no_grad():
            m.weight.normal_(0.0, 1.0 / math.sqrt(ci * k * k), generator=g)
        x = torch.randn((shape[0], ci) + shape[1:], generator=g, device=DEV).bfloat16().contiguous(memory_format=CL)
        runs, dy = [], None
        for _ in range(3):
            xg = x.clone().requires_grad_(True)
            m.zero_grad(set_to_none=True)
            with _modes(True, "own"):
                y = _conv(xg, m, torch.bfloat16)
            assert type(y.grad_fn).__name__ == "_DetConvFnBackward"
            if dy is None:
                dy = torch.randn(y.shape, generator=g, device=DEV).bfloat16().contiguous(memory_format=CL)
            y.backward(dy)
            runs.append((y.detach(), xg.grad, m.weight.grad.clone()))
        torch.cuda.synchronize()
        for q in range(3):
            assert torch.equal(runs[0][q], runs[1][q]) and torch.equal(runs[0][q], runs[2][q]), (ci, co, q)
        x64 = x.double().cpu().requires_grad_(True)
        w64 = m.weight.detach().bfloat16().double().cpu()
        b64 = m.bias.detach().bfloat16().double().cpu() if bias else None
        pre = F.conv2d(x64, w64, None, stride, pad)
        ref = pre if b64 is None else pre + b64.view(1, -1, 1, 1)
        rdx, = torch.autograd.grad(ref, x64, dy.double().cpu())
        ref, pre = ref.detach(), pre.detach()
        got = runs[0][0].double().cpu()
        tol = 2.0 ** -8 * ref.abs() + 1e-3 * float(ref.abs().max()) + (2.0 ** -8 * pre.abs() if bias else 0.0)
        ey, edx = float(((got - ref).abs() / tol).max()), elementwise(runs[0][1], rdx)
        record(f"det_gemm/{ci}_{co}_k{k}/y", ey)
        record(f"det_gemm/{ci}_{co}_k{k}/dx", edx)
        assert ey <= 1.0 and edx <= 1.0, (ci, co, ey, edx)


# ---- the TrainEncoder step --------------------------------------------------------------------------------------------------
def test_train_encoder_bit_reproducible_eager_and_graph_with_own_conv():
    """``test_train_encoder_bit_reproducible_eager_and_graph``'s encoder and sizes with the mode's 3x3 convolutions on
    ``dmm_conv3x3_bf16``: two eager runs and a graph replay agree bit for bit in features, every ``p.grad`` and every buffer,
    over two steps (running statistics carry over; the second graphed step replays the first one's plan).  The setting is part
    of a plan's key: a graph captured under one setting never replays under the other."""
    from dmm_net_amd.encoder import FeatureEncoder
    from test_gpu_deterministic import _same, _step
    torch.manual_seed(31)
    ref = FeatureEncoder("resnet50").to(DEV).train()                     # untamed weights
    g = torch.Generator(device=DEV).manual_seed(3)
    imgs = [torch.randn((6, 3, 128, 224), generator=g, device=DEV) for _ in range(2)]
    with torch.no_grad():
        probe = ref(imgs[0])
    cot = [torch.randn(f.shape, generator=g, device=DEV) for f in list(probe["backbone_feature"]) + list(probe["refine_input_feat"])]
    del probe
    encs = [copy.deepcopy(ref) for _ in range(3)]
    e1, e2, g1 = TrainEncoder(encs[0], graphs=False), TrainEncoder(encs[1], graphs=False), TrainEncoder(encs[2])
    dmm_net_amd.set_deterministic_conv("own")
    with dmm_net_amd.deterministic():
        for img in imgs:
            r_e1, r_e2, r_g1 = _step(e1, encs[0], img, cot), _step(e2, encs[1], img, cot), _step(g1, encs[2], img, cot)
            _same(r_e1, r_e2)                                            # two eager runs
            _same(r_g1, r_e1)                                            # graph replay == eager
    assert [k[-2:] for k in g1._plans] == [(True, True)]                 # (own, deterministic)


def test_own_conv_step_is_as_close_to_fp32_as_the_library_step():
    """A ResNet-50 eager step in the deterministic mode under "own" and under "library" against the fp32 ``FeatureEncoder``
    (tamed weights, skips in the loss): features and gradients of "own" as close to fp32 as those of "library", by the
    margin ``test_deterministic_eager_step_with_skips_is_as_close_to_fp32_as_the_default_step`` allows between two modes
    (x 1.15 + 0.02 on ``_rel``), every gradient aligned (cosine >= 0.85) -- the bounds are that test's, not this code's."""
    from dmm_net_amd.encoder import FeatureEncoder
    from test_gpu_train_encoder import _grads, _loss, _rel, _tame
    torch.manual_seed(12)
    ref = _tame(FeatureEncoder("resnet50").to(DEV).train())
    a, b = copy.deepcopy(ref), copy.deepcopy(ref)
    own_te, lib_te = TrainEncoder(a, graphs=False), TrainEncoder(b, graphs=False)
    img = torch.randn(4, 3, 128, 224, device=DEV)
    for m in (ref, a, b):
        m.zero_grad(set_to_none=True)
    fr = ref(img)
    _loss(fr).backward()
    feats = {}
    for which, te in (("own", own_te), ("library", lib_te)):
        dmm_net_amd.set_deterministic_conv(which)
        with dmm_net_amd.deterministic():
            f = te(img)
            _loss(f).backward()
        feats[which] = [t.detach().float() for t in f["backbone_feature"] + f["refine_input_feat"]]
    dmm_net_amd.set_deterministic_conv("library")
    fref = {str(k): t.detach().float() for k, t in enumerate(fr["backbone_feature"] + fr["refine_input_feat"])}
    e_feat = {w: _rel({str(k): t for k, t in enumerate(feats[w])}, fref) for w in feats}
    go, gl, gr = _grads(a), _grads(b), _grads(ref)
    assert all((go[k] is None) == (gr[k] is None) == (gl[k] is None) for k in gr)
    bad = [k for k, v in go.items() if v is not None and not bool(torch.isfinite(v).all())]
    assert not bad, bad[:4]
    e_own, e_lib = _rel(go, gr), _rel(gl, gr)
    ks = [k for k in gr if gr[k] is not None]
    dot = sum(float((go[k] * gr[k]).sum()) for k in ks)
    cos = dot / math.sqrt(sum(float(go[k].square().sum()) for k in ks) * sum(float(gr[k].square().sum()) for k in ks))
    for name, v in (("grads_own_vs_fp32", e_own), ("grads_library_vs_fp32", e_lib), ("grads_own_vs_library", _rel(go, gl)),
                    ("features_own_vs_fp32", e_feat["own"]), ("features_library_vs_fp32", e_feat["library"]), ("cos_own_vs_fp32", cos)):
        record("step/" + name, v)
        print(f"conv3x3 step {name}: {v:.5f}")
    assert e_own <= 1.15 * e_lib + 0.02, (e_own, e_lib)
    assert e_feat["own"] <= 1.15 * e_feat["library"] + 0.02, e_feat
    assert cos >= 0.85, cos
