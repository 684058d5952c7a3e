"""``dmm_conv7x7s2_stem_bf16`` / ``dmm_wgrad7x7s2_stem_bf16`` on the GPU (include/dmm_match.h (10f), ``ops.conv7x7s2_stem_bf16``,
``ops.wgrad7x7s2_stem_bf16``): y and dw against the float64 reference of tests/conv_stem_ref.py, bit-identical repeats, guard
bands round every buffer (x also at a 2-byte-odd offset), independence of the batch -- and the deterministic ``TrainEncoder``
step with ``set_deterministic_conv("own_stem")``: the stem off the unfold route with an fp32 weight gradient, no ``im2col``
left in the step, bit-reproducible eagerly and in graph replay, as close to the fp32 encoder as the ``"library"`` step."""
import copy
import gc
import math
import types

import pytest
import torch
import torch.nn as nn

import dmm_net_amd
from conv_stem_ref import CASES, CL, DW_BOUND, case_id, dw_error, elementwise, inputs, out_hw, record, reference
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
    return "stem/" + case_id(case) + ("" if bias is None else "_bias" if bias else "_nobias")


# ---- the kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", BIAS, ids=["nobias", "bias"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_y_against_fp64(case, bias):
    B, H, W = case
    x, w, b, _ = _dev(case, bias)
    y = ops.conv7x7s2_stem_bf16(x, w, b)
    torch.cuda.synchronize()
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (B, 64) + out_hw(H, W) and y.is_contiguous(memory_format=CL)
    ry = reference(case)[0]
    if bias:
        ry = ry + b.double().cpu().view(1, -1, 1, 1)
    ey = elementwise(y, ry)
    record(f"{_tag(case, bias)}/y", ey)
    print(f"conv7x7 {_tag(case, bias)}: y {ey:.3f}")
    assert ey <= 1.0, ey


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_dw_against_fp64(case):
    x, _, _, dy = _dev(case, False)
    dw = ops.wgrad7x7s2_stem_bf16(dy, x)
    torch.cuda.synchronize()
    assert dw.dtype == torch.float32 and tuple(dw.shape) == (64, 3, 7, 7) and dw.is_contiguous()
    e = dw_error(dw, reference(case)[1])
    record(f"{_tag(case)}/dw", e)
    print(f"conv7x7 {_tag(case)}: dw {e:.3e}")
    assert e <= DW_BOUND, e


@pytest.mark.parametrize("bias", BIAS, ids=["nobias", "bias"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_three_calls_are_bit_identical(case, bias):
    x, w, b, dy = _dev(case, bias)
    ys = [ops.conv7x7s2_stem_bf16(x, w, b) for _ in range(3)]
    dws = [ops.wgrad7x7s2_stem_bf16(dy, x) for _ in range(3)]
    torch.cuda.synchronize()
    for runs in (ys, dws):
        assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


def _banded(n, dtype, fill, margin, shift=0):
    """A tensor of n elements inside a larger allocation whose margins hold ``fill``, ``shift`` elements off the margin's end
    -> (whole, the inner view)."""
    whole = torch.full((n + 2 * margin,), fill, dtype=dtype, device=DEV)
    return whole, whole[margin + shift:margin + shift + n]


@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "x_odd"])
@pytest.mark.parametrize("bias", BIAS, ids=["nobias", "bias"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_guard_bands(case, bias, odd):
    """x, w, dy (and the bias) sit between NaNs; y, dw and the weight gradient's workspace between sentinels, their interiors
    NaN: no NaN comes out (a value fetched from beyond a tensor or from a zero-weighted K lane instead of zeroed, or an element
    left unwritten, would show), the results are what the plain calls give, every margin is intact.  ``odd``: x starts one
    element into its allocation -- a base that is 2-byte but not 4-byte aligned."""
    B, H, W = case
    Ho, Wo = out_hw(H, W)
    x, w, b, dy = _dev(case, bias)
    M = 4096                                              # elements: keeps every inner view but the shifted x 16-byte aligned
    nan = float("nan")
    xa, xv = _banded(x.numel(), torch.bfloat16, nan, M, 1 if odd else 0)
    wa, wv = _banded(w.numel(), torch.bfloat16, nan, M)
    da, dv = _banded(dy.numel(), torch.bfloat16, nan, M)
    xv.copy_(x.permute(0, 2, 3, 1).reshape(-1))
    wv.copy_(w.permute(0, 2, 3, 1).reshape(-1))
    dv.copy_(dy.permute(0, 2, 3, 1).reshape(-1))
    xg = xv.view(B, H, W, 3).permute(0, 3, 1, 2)
    wg = wv.view(64, 7, 7, 3).permute(0, 3, 1, 2)
    dg = dv.view(B, Ho, Wo, 64).permute(0, 3, 1, 2)
    assert xg.is_contiguous(memory_format=CL) and wg.is_contiguous(memory_format=CL) and dg.is_contiguous(memory_format=CL)
    assert xg.data_ptr() % 4 == (2 if odd else 0)
    nan_margins = [(xa, M + (1 if odd else 0), M - (1 if odd else 0)), (wa, M, M), (da, M, M)]
    bg = None
    if bias:
        ba, bg = _banded(64, torch.bfloat16, nan, M)
        bg.copy_(b)
        nan_margins.append((ba, M, M))
    SENT = -12345.0                                       # exact in bf16 and fp32; no result of these inputs comes near it
    ya, yv = _banded(B * Ho * Wo * 64, torch.bfloat16, SENT, M)
    yv.fill_(nan)                                         # (the interior must be overwritten whole)
    yg = yv.view(B, Ho, Wo, 64).permute(0, 3, 1, 2)
    wga, wgv = _banded(64 * 147, torch.float32, SENT, M)
    wgv.fill_(nan)
    dwg = wgv.view(64, 3, 7, 7)
    need = int(_lib.load().dmm_wgrad7x7s2_stem_workspace_bytes(B, H, W))
    assert need > 0 and need % 4 == 0
    ws_all, ws = _banded(need // 4, torch.float32, SENT, M)
    ws.fill_(nan)
    got_y = ops.conv7x7s2_stem_bf16(xg, wg, bg, out=yg)
    got_dw = ops.wgrad7x7s2_stem_bf16(dg, xg, out=dwg, workspace=ws.view(torch.uint8))
    plain_y, plain_dw = ops.conv7x7s2_stem_bf16(x, w, b), ops.wgrad7x7s2_stem_bf16(dy, x)
    torch.cuda.synchronize()
    assert got_y.data_ptr() == yg.data_ptr() and got_dw.data_ptr() == dwg.data_ptr()
    assert not bool(torch.isnan(yv).any()), "a NaN from a margin (or an unwritten output) reached y"
    assert not bool(torch.isnan(wgv).any()), "a NaN from a margin (or an unwritten output, or an unwritten partial) reached dw"
    assert torch.equal(got_y, plain_y) and torch.equal(got_dw, plain_dw)
    for whole, what in ((ya, "y"), (wga, "dw"), (ws_all, "the workspace")):
        assert bool((whole[:M] == SENT).all()) and bool((whole[-M:] == SENT).all()), "a store outside " + what
    for whole, head, tail in nan_margins:
        assert bool(torch.isnan(whole[:head]).all()) and bool(torch.isnan(whole[-tail:]).all())


@pytest.mark.parametrize("bias", BIAS, ids=["nobias", "bias"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_an_image_does_not_depend_on_its_batch(case, bias):
    """Image 0 of a B = 3 call equals the B = 1 call bit for bit: the summation order is a function of nothing but a term's
    position in the reduction."""
    B, H, W = case
    x, w, b, _ = _dev(case, bias)
    g = torch.Generator(device=DEV).manual_seed(7)
    x3 = torch.cat([x[:1], torch.randn((2, 3, H, W), generator=g, device=DEV).bfloat16()], 0).contiguous(memory_format=CL)
    x1 = x[:1].contiguous(memory_format=CL)
    y3, y1 = ops.conv7x7s2_stem_bf16(x3, w, b), ops.conv7x7s2_stem_bf16(x1, w, b)
    torch.cuda.synchronize()
    assert torch.equal(y3[:1], y1)


def test_ops_reject_what_the_kernels_do_not_take():
    def z(*shape, dtype=torch.bfloat16):
        t = torch.zeros(shape, dtype=dtype, device=DEV)
        return t.contiguous(memory_format=CL) if t.dim() == 4 else t
    x, w = z(1, 3, 8, 8), z(64, 3, 7, 7)
    for args in ((z(1, 4, 8, 8), z(64, 4, 7, 7)), (z(1, 4, 8, 8), w), (x.float(), w), (x, w.float()), (x, z(32, 3, 7, 7)),
                 (x, z(64, 3, 3, 3)), (x, z(64, 3, 7, 5)), (x, w, z(64, dtype=torch.float32)), (x, w, z(32)), (x[0], w),
                 (x.cpu(), w.cpu())):
        with pytest.raises(_lib.DmmError):
            ops.conv7x7s2_stem_bf16(*args)
    with pytest.raises(_lib.DmmError):
        ops.conv7x7s2_stem_bf16(x, w, out=z(1, 64, 4, 4, dtype=torch.float32))
    dy = z(1, 64, 4, 4)
    for args in ((dy, z(1, 4, 8, 8)), (dy.float(), x), (dy, x.float()), (z(2, 64, 4, 4), x), (z(1, 64, 4, 5), x), (z(1, 64, 8, 8), x),
                 (z(1, 32, 4, 4), x), (dy.cpu(), x.cpu())):
        with pytest.raises(_lib.DmmError):
            ops.wgrad7x7s2_stem_bf16(*args)
    with pytest.raises(_lib.DmmError):
        ops.wgrad7x7s2_stem_bf16(dy, x, out=torch.zeros((64, 3, 7, 7), dtype=torch.bfloat16, device=DEV))


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


ROUTE_CASE = (2, 17, 23)


def _stem_module(bias):
    """The stem module with the route case's weight as its fp32 master (bf16 values, so the reference sees the same numbers)."""
    _, w, b, _ = inputs(ROUTE_CASE)
    m = nn.Conv2d(3, 64, 7, 2, 3, bias=bias).to(DEV)
    with torch.no_grad():
        m.weight.copy_(w.float())
        if bias:
            m.bias.copy_(b.float())
    return m


@pytest.mark.parametrize("bias", BIAS, ids=["nobias", "bias"])
def test_stem_under_own_stem_leaves_the_library_and_the_unfold_route(bias, monkeypatch):
    """``_conv`` of the stem in the deterministic mode with "own_stem": the autograd node is ``_ConvStemFn``, neither its
    forward nor its backward reaches ``F.conv2d`` / ``F.unfold`` (both raise here) or an aten convolution / im2col, y and dw
    hold their bounds against fp64 and the master's gradient is fp32 in its own layout.  Under "own_all" the same call is the
    ``_DetConvFn`` route as before; outside the mode the setting changes nothing; an input that requires a gradient stays on
    ``_DetConvFn``."""
    from test_gpu_train_encoder_ref import _route
    x, _, b, dy = _dev(ROUTE_CASE, bias)
    m = _stem_module(bias)

    def boom(*a, **k):
        raise AssertionError("a library convolution or an unfold was called")
    real_F = te_mod.F
    proxy = types.SimpleNamespace(**{k: getattr(real_F, k) for k in dir(real_F) if not k.startswith("__")})
    proxy.conv2d = boom
    proxy.unfold = boom
    with monkeypatch.context() as mp:
        mp.setattr(te_mod, "F", proxy)
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof_f:
            with _modes(True, "own_stem"):
                y = _conv(x, m, torch.bfloat16)
        assert _node(y) == "_ConvStemFnBackward" and y.grad_fn.det
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof_b:
            y.backward(dy)
        torch.cuda.synchronize()
        names = {e.key for e in prof_f.key_averages()} | {e.key for e in prof_b.key_averages()}
        bad = sorted(n for n in names if "convolution" in n or "conv2d" in n or "im2col" in n or "unfold" in n)
        assert not bad, bad
    ry, rdw = reference(ROUTE_CASE)
    if bias:
        ry = ry + b.double().cpu().view(1, -1, 1, 1)
    ey, edw = elementwise(y, ry), dw_error(m.weight.grad, rdw)
    record(f"stem/route/{'bias' if bias else 'nobias'}/y", ey)
    record(f"stem/route/{'bias' if bias else 'nobias'}/dw", edw)
    print(f"conv7x7 stem route bias={bias}: y {ey:.3f} dw {edw:.3e}")
    assert m.weight.grad.dtype == torch.float32 and m.weight.grad.shape == m.weight.shape and m.weight.grad.is_contiguous()
    assert ey <= 1.0 and edw <= DW_BOUND, (ey, edw)
    if bias:
        rdb = dy.double().cpu().sum((0, 2, 3))
        scale = 1e-4 * (1 + float(rdb.abs().max())) * math.sqrt(dy.numel() / 64)          # (the narrow route test's db bound)
        assert m.bias.grad.dtype == torch.float32 and float((m.bias.grad.double().cpu() - rdb).abs().max()) <= scale
    # under "own_all" the same call is the unfold + GEMM route, as before
    with _modes(True, "own_all"):
        y1 = _conv(x, m, torch.bfloat16)
    assert _route(y1) == "det" and _node(y1) == "_DetConvFnBackward"
    # outside the mode the setting does nothing: the stock node
    with _modes(False, "own_stem"):
        y2 = _conv(x, m, torch.bfloat16)
    assert _route(y2) == "lib"
    # an image that requires a gradient stays on the mode's stock route (the own kernels have no data gradient)
    with _modes(True, "own_stem"):
        y3 = _conv(x.clone().requires_grad_(True), m, torch.bfloat16)
    assert _route(y3) == "det" and _node(y3) == "_DetConvFnBackward"


def test_the_unfold_route_misses_the_weight_gradient_bound_the_own_kernel_holds():
    """The fidelity claim: on case (2, 17, 23) the present route's dw (unfold + ONE bf16 GEMM, widened to fp32 by autograd) is
    off by more than ``DW_BOUND`` of max|dw|, the own kernel's (fp32 from the kernel) holds it."""
    x, _, _, dy = _dev(ROUTE_CASE, False)
    rdw = reference(ROUTE_CASE)[1]
    errs = {}
    for which in ("own_all", "own_stem"):
        m = _stem_module(False)
        with _modes(True, which):
            y = _conv(x, m, torch.bfloat16)
        y.backward(dy)
        torch.cuda.synchronize()
        assert m.weight.grad.dtype == torch.float32
        errs[which] = dw_error(m.weight.grad, rdw)
        record(f"stem/fidelity/dw_{which}", errs[which])
    print(f"conv7x7 stem dw error: unfold + GEMM (own_all) {errs['own_all']:.3e}, own kernel (own_stem) {errs['own_stem']:.3e}")
    assert errs["own_all"] > DW_BOUND, errs
    assert errs["own_stem"] <= DW_BOUND, errs


# ---- the TrainEncoder step --------------------------------------------------------------------------------------------------
def test_train_encoder_bit_reproducible_eager_and_graph_with_own_stem():
    """``test_train_encoder_bit_reproducible_eager_and_graph_with_own_all``'s encoder, sizes and helpers under "own_stem": two
    eager runs and a graph replay agree bit for bit in features, every ``p.grad`` and every buffer, over two steps.  The
    setting is part of a plan's key: a forward under "own_all" afterwards captures a second plan instead of replaying the first."""
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
    dmm_net_amd.set_deterministic_conv("own_stem")
    with dmm_net_amd.deterministic():
        for img in imgs:
            r_e1, r_e2, r_g1 = _step(e1, encs[0], img, cot), _step(e2, encs[1], img, cot), _step(g1, encs[2], img, cot)
            _same(r_e1, r_e2)                                            # two eager runs
            _same(r_g1, r_e1)                                            # graph replay == eager
    assert encs[2].base.conv1.weight.grad.dtype == torch.float32
    assert len(g1._plans) == 1 and [len(v) for v in g1._plans.values()] == [1]
    (k_stem,) = g1._plans
    assert "own_stem" in k_stem and k_stem[-2:] == (True, True)
    dmm_net_amd.set_deterministic_conv("own_all")
    with dmm_net_amd.deterministic():
        _step(g1, encs[2], imgs[0], cot)
    assert len(g1._plans) == 2 and [len(v) for v in g1._plans.values()] == [1, 1]
    k_all = next(k for k in g1._plans if k != k_stem)
    assert "own_all" in k_all and "own_stem" not in k_all and k_all[-2:] == (True, True)
    # the weight tables of one setting are not handed to the other: every memo key carries the setting it was made under
    keys = list(g1._wprep)
    assert keys and all(k[-3:] in ((True, True, True), (True, True, False)) for k in keys)
    assert {k[-1] for k in keys} == {True, False}


def test_the_stem_left_the_unfold_route():
    """One eager ResNet-50 step of 4 x 3 x 128 x 224 in the mode: under "own_stem" no ``aten::im2col`` call is left; under
    "own_all" the 7x7 stem's two remain (its forward and its weight gradient)."""
    from dmm_net_amd.encoder import FeatureEncoder
    from test_gpu_conv_narrow import _im2col_calls
    from test_gpu_train_encoder import _tame
    torch.manual_seed(12)
    enc = _tame(FeatureEncoder("resnet50").to(DEV).train())
    te = TrainEncoder(enc, graphs=False)
    img = torch.randn(4, 3, 128, 224, device=DEV)
    n_stem, n_all = _im2col_calls(te, img, "own_stem"), _im2col_calls(te, img, "own_all")
    print(f"conv7x7 stem: aten::im2col calls per step: own_stem {n_stem}, own_all {n_all}")
    assert n_stem == 0, n_stem
    assert n_all == 2, n_all


def test_own_stem_step_is_as_close_to_fp32_as_the_library_step():
    """``test_own_all_step_is_as_close_to_fp32_as_the_library_step`` with "own_stem" in place of "own_all": features and
    gradients as close to the fp32 ``FeatureEncoder`` as those of "library" by that test's margins (x 1.15 + 0.02 on ``_rel``),
    every gradient aligned (cosine >= 0.85) -- the bounds are that test's, not this code's."""
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
    for which, te in (("own_stem", own_te), ("library", lib_te)):
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
    for name, v in (("grads_own_stem_vs_fp32", e_own), ("grads_library_vs_fp32", e_lib), ("grads_own_stem_vs_library", _rel(go, gl)),
                    ("features_own_stem_vs_fp32", e_feat["own_stem"]), ("features_library_vs_fp32", e_feat["library"]),
                    ("cos_own_stem_vs_fp32", cos)):
        record("stem/step/" + name, v)
        print(f"conv7x7 stem step {name}: {v:.5f}")
    assert e_own <= 1.15 * e_lib + 0.02, (e_own, e_lib)
    assert e_feat["own_stem"] <= 1.15 * e_feat["library"] + 0.02, e_feat
    assert cos >= 0.85, cos
