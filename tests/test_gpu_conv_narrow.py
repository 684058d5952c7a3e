"""``dmm_conv3x3_narrow_bf16`` / ``dmm_wgrad3x3_narrow_bf16`` on the GPU (include/dmm_match.h (10e), ``ops.conv3x3_narrow_bf16``,
``ops.conv3x3_narrow_dgrad_bf16``, ``ops.wgrad3x3_narrow_bf16``): y, dx and dw against the float64 reference of
tests/conv_narrow_ref.py, bit-identical repeats, guard bands round every buffer, independence of the batch -- and the
deterministic ``TrainEncoder`` step with ``set_deterministic_conv("own_all")``: the narrow heads off the unfold route,
bit-reproducible eagerly and in graph replay, as close to the fp32 encoder as the ``"library"`` step."""
import copy
import gc
import math
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import dmm_net_amd
from conv_narrow_ref import CASES, CL, DW_BOUND, case_id, dw_error, elementwise, flipped, inputs, record, reference
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


def _tag(case, bias=None):
    return "narrow/" + case_id(case) + ("" if bias is None else "_bias" if bias else "_nobias")


# ---- the kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", BIAS, ids=["nobias", "bias"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_y_and_dx_against_fp64(case, bias):
    ci, co, B, H, W = case
    x, w, b, dy = _dev(case, bias)
    y = ops.conv3x3_narrow_bf16(x, w, b)
    dx = ops.conv3x3_narrow_dgrad_bf16(dy, flipped(w))
    torch.cuda.synchronize()
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (B, co, H, W) and y.is_contiguous(memory_format=CL)
    assert dx.dtype == torch.bfloat16 and dx.shape == x.shape and dx.is_contiguous(memory_format=CL)
    ry, rdx, _ = reference(case)
    if bias:
        ry = ry + b.double().cpu().view(1, -1, 1, 1)
    ey, edx = elementwise(y, ry), elementwise(dx, rdx)
    record(f"{_tag(case, bias)}/y", ey)
    record(f"{_tag(case, bias)}/dx", edx)
    print(f"conv3x3 {_tag(case, bias)}: y {ey:.3f} dx {edx:.3f}")
    assert ey <= 1.0 and edx <= 1.0, (ey, edx)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_dw_against_fp64(case):
    ci, co, B, H, W = case
    x, _, _, dy = _dev(case, False)
    dw = ops.wgrad3x3_narrow_bf16(dy, x)
    torch.cuda.synchronize()
    assert dw.dtype == torch.float32 and tuple(dw.shape) == (co, ci, 3, 3) and dw.is_contiguous()
    e = dw_error(dw, reference(case)[2])
    record(f"{_tag(case)}/dw", e)
    print(f"conv3x3 {_tag(case)}: dw {e:.3e}")
    assert e <= DW_BOUND, e


@pytest.mark.parametrize("bias", BIAS, ids=["nobias", "bias"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_three_calls_are_bit_identical(case, bias):
    x, w, b, dy = _dev(case, bias)
    wt = flipped(w)
    ys = [ops.conv3x3_narrow_bf16(x, w, b) for _ in range(3)]
    dxs = [ops.conv3x3_narrow_dgrad_bf16(dy, wt) for _ in range(3)]
    dws = [ops.wgrad3x3_narrow_bf16(dy, x) for _ in range(3)]
    torch.cuda.synchronize()
    for runs in (ys, dxs, dws):
        assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


def _banded(n, dtype, fill, margin):
    """A tensor of n elements inside a larger allocation whose margins hold ``fill`` -> (whole, the inner view)."""
    whole = torch.full((n + 2 * margin,), fill, dtype=dtype, device=DEV)
    return whole, whole[margin:margin + n]


@pytest.mark.parametrize("bias", BIAS, ids=["nobias", "bias"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_guard_bands(case, bias):
    """x, w, dy (and the bias) sit between NaNs; y, dw and the weight gradient's workspace between sentinels, their interiors
    NaN: no NaN comes out (a masked piece fetched from beyond a tensor instead of zeroed, or an element left unwritten, would
    show), the results are what the plain calls give, every margin is intact."""
    ci, co, B, H, W = case
    x, w, b, dy = _dev(case, bias)
    M = 4096                                              # elements: keeps every inner view 16-byte aligned
    nan = float("nan")
    xa, xv = _banded(x.numel(), torch.bfloat16, nan, M)
    wa, wv = _banded(w.numel(), torch.bfloat16, nan, M)
    da, dv = _banded(dy.numel(), torch.bfloat16, nan, M)
    xv.copy_(x.permute(0, 2, 3, 1).reshape(-1))
    wv.copy_(w.permute(0, 2, 3, 1).reshape(-1))
    dv.copy_(dy.permute(0, 2, 3, 1).reshape(-1))
    xg = xv.view(B, H, W, ci).permute(0, 3, 1, 2)
    wg = wv.view(co, 3, 3, ci).permute(0, 3, 1, 2)
    dg = dv.view(B, H, W, co).permute(0, 3, 1, 2)
    assert xg.is_contiguous(memory_format=CL) and wg.is_contiguous(memory_format=CL) and dg.is_contiguous(memory_format=CL)
    nan_margins = [xa, wa, da]
    bg = None
    if bias:
        ba, bg = _banded(co, torch.bfloat16, nan, M)
        bg.copy_(b)
        nan_margins.append(ba)
    SENT = -12345.0                                       # exact in bf16 and fp32; no result of these inputs comes near it
    ya, yv = _banded(B * H * W * co, torch.bfloat16, SENT, M)
    yv.fill_(nan)                                         # (the interior must be overwritten whole)
    yg = yv.view(B, H, W, co).permute(0, 3, 1, 2)
    wga, wgv = _banded(co * ci * 9, torch.float32, SENT, M)
    wgv.fill_(nan)
    dwg = wgv.view(co, ci, 3, 3)
    need = int(_lib.load().dmm_wgrad3x3_narrow_workspace_bytes(B, H, W, ci, co))
    assert need > 0 and need % 4 == 0
    ws_all, ws = _banded(need // 4, torch.float32, SENT, M)
    ws.fill_(nan)
    got_y = ops.conv3x3_narrow_bf16(xg, wg, bg, out=yg)
    got_dw = ops.wgrad3x3_narrow_bf16(dg, xg, out=dwg, workspace=ws.view(torch.uint8))
    plain_y, plain_dw = ops.conv3x3_narrow_bf16(x, w, b), ops.wgrad3x3_narrow_bf16(dy, x)
    torch.cuda.synchronize()
    assert got_y.data_ptr() == yg.data_ptr() and got_dw.data_ptr() == dwg.data_ptr()
    assert not bool(torch.isnan(yv).any()), "a NaN from a margin (or an unwritten output) reached y"
    assert not bool(torch.isnan(wgv).any()), "a NaN from a margin (or an unwritten output, or an unwritten partial) reached dw"
    assert torch.equal(got_y, plain_y) and torch.equal(got_dw, plain_dw)
    for whole, what in ((ya, "y"), (wga, "dw"), (ws_all, "the workspace")):
        assert bool((whole[:M] == SENT).all()) and bool((whole[-M:] == SENT).all()), "a store outside " + what
    for whole in nan_margins:
        assert bool(torch.isnan(whole[:M]).all()) and bool(torch.isnan(whole[-M:]).all())


@pytest.mark.parametrize("bias", BIAS, ids=["nobias", "bias"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_an_image_does_not_depend_on_its_batch(case, bias):
    """Image 0 of a B = 3 call equals the B = 1 call bit for bit: the summation order is a function of (ci, co) alone."""
    ci, co, B, H, W = case
    x, w, b, dy = _dev(case, bias)
    g = torch.Generator(device=DEV).manual_seed(7)
    x3 = torch.cat([x[:1], torch.randn((2, ci, H, W), generator=g, device=DEV).bfloat16()], 0).contiguous(memory_format=CL)
    dy3 = torch.cat([dy[:1], torch.randn((2, co, H, W), generator=g, device=DEV).bfloat16()], 0).contiguous(memory_format=CL)
    x1, dy1 = x[:1].contiguous(memory_format=CL), dy[:1].contiguous(memory_format=CL)
    wt = flipped(w)
    y3, y1 = ops.conv3x3_narrow_bf16(x3, w, b), ops.conv3x3_narrow_bf16(x1, w, b)
    d3, d1 = ops.conv3x3_narrow_dgrad_bf16(dy3, wt), ops.conv3x3_narrow_dgrad_bf16(dy1, wt)
    torch.cuda.synchronize()
    assert torch.equal(y3[:1], y1) and torch.equal(d3[:1], d1)


def test_ops_reject_what_the_kernels_do_not_take():
    def z(*shape, dtype=torch.bfloat16):
        t = torch.zeros(shape, dtype=dtype, device=DEV)
        return t.contiguous(memory_format=CL) if t.dim() == 4 else t
    x, w = z(1, 32, 4, 4), z(32, 32, 3, 3)
    for args in ((z(1, 16, 4, 4), z(32, 16, 3, 3)), (z(1, 48, 4, 4), z(32, 48, 3, 3)), (x, z(16, 32, 3, 3)), (x, z(48, 32, 3, 3)),
                 (x.float(), w), (x, w.float()), (x, z(32, 64, 3, 3)), (x, z(32, 32, 1, 1)), (x, w, z(32, dtype=torch.float32)),
                 (x, w, z(64)), (x.cpu(), w.cpu())):
        with pytest.raises(_lib.DmmError):
            ops.conv3x3_narrow_bf16(*args)
    for args in ((z(1, 16, 4, 4), w), (z(1, 48, 4, 4), z(32, 48, 3, 3)), (x.float(), w), (x.cpu(), w.cpu())):
        with pytest.raises(_lib.DmmError):
            ops.conv3x3_narrow_dgrad_bf16(*args)
    dy = z(1, 32, 4, 4)
    for args in ((z(1, 16, 4, 4), x), (dy, z(1, 48, 4, 4)), (dy.float(), x), (dy, x.float()), (z(2, 32, 4, 4), x), (z(1, 32, 4, 5), x),
                 (dy.cpu(), x.cpu())):
        with pytest.raises(_lib.DmmError):
            ops.wgrad3x3_narrow_bf16(*args)
    with pytest.raises(_lib.DmmError):
        ops.wgrad3x3_narrow_bf16(dy, x, out=torch.zeros((32, 32, 3, 3), dtype=torch.bfloat16, device=DEV))


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


def _node(y):
    return type(y.grad_fn).__name__


@pytest.mark.parametrize("ci,co", [(256, 32), (32, 128)])
def test_narrow_conv_under_own_all_leaves_the_library_and_the_unfold_route(ci, co, monkeypatch):
    """``_conv`` of a narrow head convolution in the deterministic mode with "own_all": the autograd node is ``_ConvNarrowFn``,
    neither its forward nor its backward reaches ``F.conv2d`` / ``F.unfold`` (both raise here) or an aten convolution / im2col,
    and y, dx, dw, db hold their bounds against fp64.  Under "own" the same call is the ``_DetConvFn`` route as before; outside
    the mode the setting changes nothing; a 16-channel output stays on ``_DetConvFn``."""
    from test_gpu_train_encoder_ref import _route
    B, H, W = 2, 17, 23
    g = torch.Generator(device=DEV).manual_seed(ci + co)
    m = nn.Conv2d(ci, co, 3, 1, 1, bias=True).to(DEV)
    with torch.no_grad():
        m.weight.normal_(0.0, 1.0 / math.sqrt(9 * ci), generator=g)
        m.bias.normal_(0.0, 0.5, generator=g)
    x = torch.randn((B, ci, H, W), generator=g, device=DEV).relu().bfloat16().contiguous(memory_format=CL)

    def boom(*a, **k):
        raise AssertionError("a library convolution or an unfold was called")
    real_F = te_mod.F
    proxy = types.SimpleNamespace(**{k: getattr(real_F, k) for k in dir(real_F) if not k.startswith("__")})
    proxy.conv2d = boom
    proxy.unfold = boom
    xg = x.clone().requires_grad_(True)
    with monkeypatch.context() as mp:
        mp.setattr(te_mod, "F", proxy)
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof_f:
            with _modes(True, "own_all"):
                y = _conv(xg, m, torch.bfloat16)
        assert _node(y) == "_ConvNarrowFnBackward" and y.grad_fn.det and y.grad_fn.flipped
        dy = torch.randn(y.shape, generator=g, device=DEV).bfloat16().contiguous(memory_format=CL)
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof_b:
            y.backward(dy)
        torch.cuda.synchronize()
        names = {e.key for e in prof_f.key_averages()} | {e.key for e in prof_b.key_averages()}
        bad = sorted(n for n in names if "convolution" in n or "conv2d" in n or "im2col" in n or "unfold" in n)
        assert not bad, bad
    x64 = x.double().cpu().requires_grad_(True)
    w64 = m.weight.detach().bfloat16().double().cpu().requires_grad_(True)
    b64 = m.bias.detach().bfloat16().double().cpu().requires_grad_(True)
    ry = F.conv2d(x64, w64, b64, 1, 1)
    rg = torch.autograd.grad(ry, [x64, w64, b64], dy.double().cpu())
    ey, edx, edw = elementwise(y, ry), elementwise(xg.grad, rg[0]), dw_error(m.weight.grad, rg[1])
    record(f"narrow/route/{ci}_{co}/y", ey)
    record(f"narrow/route/{ci}_{co}/dx", edx)
    record(f"narrow/route/{ci}_{co}/dw", edw)
    print(f"conv3x3 narrow route {ci}_{co}: y {ey:.3f} dx {edx:.3f} dw {edw:.3e}")
    assert m.weight.grad.dtype == torch.float32 and m.weight.grad.shape == m.weight.shape
    assert ey <= 1.0 and edx <= 1.0 and edw <= DW_BOUND, (ey, edx, edw)
    scale = 1e-4 * (1 + float(rg[2].abs().max())) * math.sqrt(dy.numel() / co)       # (the existing route test's db bound)
    assert float((m.bias.grad.double().cpu() - rg[2]).abs().max()) <= scale
    # under "own" the same call is the unfold + GEMM route, as before
    with _modes(True, "own"):
        y1 = _conv(x.clone().requires_grad_(True), m, torch.bfloat16)
    assert _route(y1) == "det" and _node(y1) == "_DetConvFnBackward"
    # outside the mode the setting does nothing: the stock node
    with _modes(False, "own_all"):
        y2 = _conv(x.clone().requires_grad_(True), m, torch.bfloat16)
    assert _route(y2) == "lib"
    # a multiple of 16 only stays on the mode's stock route
    m16 = nn.Conv2d(ci, 16, 3, 1, 1).to(DEV)
    with _modes(True, "own_all"):
        assert _route(_conv(x.clone().requires_grad_(True), m16, torch.bfloat16)) == "det"


# ---- the TrainEncoder step --------------------------------------------------------------------------------------------------
def test_train_encoder_bit_reproducible_eager_and_graph_with_own_all():
    """``test_train_encoder_bit_reproducible_eager_and_graph_with_own_conv``'s encoder, sizes and helpers under "own_all": two
    eager runs and a graph replay agree bit for bit in features, every ``p.grad`` and every buffer, over two steps.  The
    setting is part of a plan's key: a forward under "own" afterwards captures a second plan instead of replaying the first."""
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
    dmm_net_amd.set_deterministic_conv("own_all")
    with dmm_net_amd.deterministic():
        for img in imgs:
            r_e1, r_e2, r_g1 = _step(e1, encs[0], img, cot), _step(e2, encs[1], img, cot), _step(g1, encs[2], img, cot)
            _same(r_e1, r_e2)                                            # two eager runs
            _same(r_g1, r_e1)                                            # graph replay == eager
    assert len(g1._plans) == 1 and [len(v) for v in g1._plans.values()] == [1]
    (k_all,) = g1._plans
    assert "own_all" in k_all and k_all[-2:] == (True, True)
    dmm_net_amd.set_deterministic_conv("own")
    with dmm_net_amd.deterministic():
        _step(g1, encs[2], imgs[0], cot)
    assert len(g1._plans) == 2 and [len(v) for v in g1._plans.values()] == [1, 1]
    k_own = next(k for k in g1._plans if k != k_all)
    assert "own" in k_own and "own_all" not in k_own and k_own[-2:] == (True, True)


def _im2col_calls(te, img, which):
    from test_gpu_train_encoder import _loss
    dmm_net_amd.set_deterministic_conv(which)
    te.src.zero_grad(set_to_none=True)
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        with dmm_net_amd.deterministic():
            _loss(te(img)).backward()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.key == "aten::im2col")


def test_the_heads_left_the_unfold_route():
    """One eager ResNet-50 step of 4 x 3 x 128 x 224 in the mode: under "own_all" the only ``aten::im2col`` calls left are the
    7x7 stem's (its forward and its weight gradient; the image needs no gradient); under "own" the narrow heads add theirs."""
    from dmm_net_amd.encoder import FeatureEncoder
    from test_gpu_train_encoder import _tame
    torch.manual_seed(12)
    enc = _tame(FeatureEncoder("resnet50").to(DEV).train())
    te = TrainEncoder(enc, graphs=False)
    img = torch.randn(4, 3, 128, 224, device=DEV)
    n_all, n_own = _im2col_calls(te, img, "own_all"), _im2col_calls(te, img, "own")
    print(f"conv3x3 narrow: aten::im2col calls per step: own_all {n_all}, own {n_own}")
    assert n_all == 2, n_all
    assert n_own > n_all, (n_own, n_all)


def test_own_all_step_is_as_close_to_fp32_as_the_library_step():
    """``test_own_conv_step_is_as_close_to_fp32_as_the_library_step`` with "own_all" in place of "own": features and gradients
    as close to the fp32 ``FeatureEncoder`` as those of "library" by that test's margins (x 1.15 + 0.02 on ``_rel``), every
    gradient aligned (cosine >= 0.85) -- the bounds are that test's, not this code's."""
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
    for which, te in (("own_all", own_te), ("library", lib_te)):
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
    for name, v in (("grads_own_all_vs_fp32", e_own), ("grads_library_vs_fp32", e_lib), ("grads_own_all_vs_library", _rel(go, gl)),
                    ("features_own_all_vs_fp32", e_feat["own_all"]), ("features_library_vs_fp32", e_feat["library"]),
                    ("cos_own_all_vs_fp32", cos)):
        record("narrow/step/" + name, v)
        print(f"conv3x3 narrow step {name}: {v:.5f}")
    assert e_own <= 1.15 * e_lib + 0.02, (e_own, e_lib)
    assert e_feat["own_all"] <= 1.15 * e_feat["library"] + 0.02, e_feat
    assert cos >= 0.85, cos
