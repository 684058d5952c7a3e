"""The inference encoder's GEMM and patch paths against the float64 reference of tests/fast_enc_ref.py:
(a) ``dmm_conv1x1_bf16`` through the C entry -- every (rows, cin, cout) case in all four (relu, residual) forms, elementwise
    against ``bound_conv1x1`` (derived, no measured number; no element left out), and the states a process can put its plan
    cache in: new pointers for a cached shape, alternating forms, a workspace and then none, another stream, a shape first
    seen inside a capture, the tuning loop;
(b) ``dmm_im2col3x3_bf16`` bit for bit against ``im2col3x3_ref`` and ``FastEncoder._conv3x3_patches`` against float64 conv2d;
(c) ``FastEncoder._conv1x1``'s routes, each identified by the entries it calls;
(d) the pieces of the network, each fed the device's own previous output, against ``rounding_model`` -- with the eager bf16
    copy of the same piece as the yardstick (``FastEncoder`` may be at most 2x as far from the reference).
Achieved ratios go to ``record_achieved`` ("fast_enc_ref/..."); profiles/fast_encoder_ref_achieved.jsonl keeps a run's."""
import copy
import functools
import hashlib

import pytest
import torch
import torch.nn as nn

import fast_enc_ref as fr
from fast_enc_ref import BF16, CONV_CASES, FORMS, IM2COL_SHAPES, PIECES, ULP
from dmm_net_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WS_BYTES = 32 << 20
TWO_CHANNEL = {(130, 64, 2), (130, 2, 64)}          # the only cases where DMM_ERR_UNSUPPORTED is a legal answer
_ids = lambda c: "x".join(map(str, c))
_form = lambda f: ("relu" if f[0] else "lin") + ("+res" if f[1] else "")


def _record(name, v):
    from conftest import record_achieved
    record_achieved("fast_enc_ref/" + name, v)


@functools.lru_cache(maxsize=None)
def _ws():
    return torch.empty((WS_BYTES,), dtype=torch.uint8, device=DEV)


def _nan_like(shape):
    """A bf16 buffer of NaN bit patterns: an element the launch does not write is seen."""
    return torch.full(shape, 0xFFFF - 65536, dtype=torch.int16, device=DEV).view(BF16)


def _to_dev(d):
    """Fresh device buffers of a host input dict (a different allocation on every call)."""
    return {k: v.to(DEV).contiguous() for k, v in d.items()}


def _gemm(dv, relu, residual, ws=True, stream=None, allow=()):
    """``dmm_conv1x1_bf16`` on device buffers dv -> (status, y)."""
    rows, cin = dv["x"].shape
    cout = dv["w"].shape[1]
    y = _nan_like((rows, cout))
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    rc = _lib.call("dmm_conv1x1_bf16", DEV, dv["x"].data_ptr(), dv["w"].data_ptr(), dv["bias"].data_ptr(),
                   dv["res"].data_ptr() if residual else None, rows, cin, cout, int(relu), y.data_ptr(),
                   _ws().data_ptr() if ws else None, WS_BYTES if ws else 0, s, allow=allow)
    return rc, y


def _ratio(got, d, relu, residual, extra=None):
    """max over ALL elements of |got - ref| / bound_conv1x1 (a NaN -- an unwritten element -- gives inf)."""
    ref, S = fr.conv1x1_64(d["x"], d["w"], d["bias"], d["res"] if residual else None, relu)
    bound = fr.bound_conv1x1(ref, S, d["x"].shape[1])
    if extra is not None:
        bound = bound + extra
    got = got.detach().double().cpu().reshape(ref.shape)
    r = (got - ref).abs() / bound
    return float(torch.nan_to_num(r, nan=float("inf")).max())


def _pre_abs(d):
    """ULP |x w|: the extra store of a route that rounds the product to bf16 before the epilogue kernel adds the bias."""
    return ULP * (d["x"].double() @ d["w"].double()).abs()


@functools.lru_cache(maxsize=None)
def _fast_host():
    from dmm_net_amd.encoder import FastEncoder, FeatureEncoder
    return FastEncoder(FeatureEncoder("resnet34", hidden_size=16).to(DEV).eval())


def _fast_with(conv):
    """The shared small ``FastEncoder`` with ``conv`` (on the device) prepared as one of its convolutions."""
    fast = _fast_host()
    fast.src.add_module("extra", conv)
    fast._prepare()
    return fast


def _conv1x1_module(d, stride=1):
    """A 1x1 ``nn.Conv2d`` that holds a case's bf16 weight values (exact in fp32) and fp32 bias."""
    cin, cout = d["w"].shape
    m = nn.Conv2d(cin, cout, 1, stride)
    with torch.no_grad():
        m.weight.copy_(d["w"].float().t().reshape(cout, cin, 1, 1))
        m.bias.copy_(d["bias"])
    return m.to(DEV)


def _cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def _rows_as_map(t):
    """[rows, C] -> channels-last [1, C, rows, 1] on the device (the same memory)."""
    return _cl(t.t().reshape(1, t.shape[1], t.shape[0], 1))


@pytest.fixture
def calls(monkeypatch):
    """Names of the library entries called, in order."""
    seen, real = [], _lib.call

    def spy(name, *a, **kw):
        seen.append(name)
        return real(name, *a, **kw)
    monkeypatch.setattr(_lib, "call", spy)
    return seen


# ---- (a) dmm_conv1x1_bf16 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS, ids=_form)
@pytest.mark.parametrize("case", CONV_CASES, ids=_ids)
def test_conv1x1_entry_against_fp64(case, form):
    relu, residual = form
    d = fr.conv_inputs(*case)
    dv = _to_dev(d)
    rc, y = _gemm(dv, relu, residual, allow=(_lib.DMM_ERR_UNSUPPORTED,))
    name = f"conv1x1/{_ids(case)}/{_form(form)}"
    if rc == _lib.DMM_ERR_UNSUPPORTED:
        assert case in TWO_CHANNEL, case
        # the caller's fallback must still give the result: torch.mm (one store) + dmm_bias_act_bf16 (the second)
        fast = _fast_with(_conv1x1_module(d))
        y = fast._conv1x1(_rows_as_map(d["x"]), fast.src.extra, relu, _rows_as_map(d["res"]) if residual else None)
        r = _ratio(y.permute(0, 2, 3, 1), d, relu, residual, extra=_pre_abs(d))
        name += "/fallback"
    else:
        r = _ratio(y, d, relu, residual)
    print(name, r)
    _record(name, r)
    assert r <= 1.0, (name, r)


def test_cached_shape_follows_new_pointers():
    """The plan (and its descriptor's bias pointer) is cached per shape: a second and third call with OTHER x, w, bias, residual
    and y buffers must compute from those."""
    case, worst = (65, 576, 64), 0.0
    for tag in (0, 1, 0, 2):
        d = fr.conv_inputs(*case, tag)
        rc, y = _gemm(_to_dev(d), True, True)
        worst = max(worst, _ratio(y, d, True, True))
    _record("conv1x1/new_pointers", worst)
    assert worst <= 1.0, worst


def test_forms_alternate_without_interfering():
    """Four plans of one shape (relu x residual), called in turn and again in reverse with other buffers."""
    case, worst = (257, 24, 256), 0.0
    for tag, forms in ((0, FORMS), (1, FORMS[::-1]), (2, FORMS)):
        d = fr.conv_inputs(*case, tag)
        dv = _to_dev(d)
        for relu, residual in forms:
            rc, y = _gemm(dv, relu, residual)
            worst = max(worst, _ratio(y, d, relu, residual))
    _record("conv1x1/forms_alternate", worst)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("case", [(782, 1024, 256), (65, 576, 64), (48, 4608, 128)], ids=_ids)
def test_workspace_then_none(case):
    """A shape first called with the 32 MB workspace and then with workspace = NULL, 0: DMM_OK within the bound or
    DMM_ERR_UNSUPPORTED, never DMM_ERR_WORKSPACE ("kernels that need one are then not considered"); and the caller with a
    workspace is still served afterwards."""
    d = fr.conv_inputs(*case)
    dv = _to_dev(d)
    for relu, residual in ((True, True), (False, False)):
        rc, y = _gemm(dv, relu, residual)
        assert _ratio(y, d, relu, residual) <= 1.0
        rc, y = _gemm(dv, relu, residual, ws=False, allow=(_lib.DMM_ERR_UNSUPPORTED, _lib.DMM_ERR_WORKSPACE))
        assert rc in (_lib.DMM_OK, _lib.DMM_ERR_UNSUPPORTED), rc
        if rc == _lib.DMM_OK:
            r = _ratio(y, d, relu, residual)
            _record(f"conv1x1/no_workspace/{_ids(case)}/{_form((relu, residual))}", r)
            assert r <= 1.0, r
        rc, y = _gemm(dv, relu, residual)
        assert _ratio(y, d, relu, residual) <= 1.0


def test_launch_on_another_stream():
    case = (782, 256, 64)
    d = fr.conv_inputs(*case, 1)
    dv = _to_dev(d)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rc, y = _gemm(dv, True, True, stream=side.cuda_stream)
    side.synchronize()
    r = _ratio(y, d, True, True)
    _record("conv1x1/side_stream", r)
    assert r <= 1.0, r


def test_shape_first_seen_inside_a_capture():
    """A shape no other test uses, first called during ``torch.cuda.graph`` capture (one stream, no fork), then replayed twice
    with refreshed inputs."""
    case = (131, 96, 48)
    _gemm(_to_dev(fr.conv_inputs(7, 8, 40)), False, False)      # (the library handle exists before the capture begins)
    static = _to_dev(fr.conv_inputs(*case, 0))
    _ws()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        rc, y = _gemm(static, True, True)
    assert rc == _lib.DMM_OK
    worst = 0.0
    for tag in (1, 2):
        d = fr.conv_inputs(*case, tag)
        for k, v in d.items():
            static[k].copy_(v.to(DEV))
        y.view(torch.int16).fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        worst = max(worst, _ratio(y, d, True, True))
    _record("conv1x1/captured", worst)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("residual", [False, True], ids=["nores", "res"])
def test_tuning_loop_leaves_the_product_alone(residual):
    """DMM_OPT_GEMM_TUNE = 8 on shapes new to the process (a plan is tuned only when it is built): the tuning call launches
    every candidate nine times into y -- its result must be the product (no accumulation across runs), and so must the next
    call's (the kept algorithm)."""
    case = (391, 256, 64) if residual else (391, 576, 128)
    old = _lib.get_option("GEMM_TUNE")
    _lib.set_option("GEMM_TUNE", 8)
    try:
        d = fr.conv_inputs(*case)
        rc, y = _gemm(_to_dev(d), True, residual)
        torch.cuda.synchronize()
        r0 = _ratio(y, d, True, residual)
        d1 = fr.conv_inputs(*case, 1)
        rc, y1 = _gemm(_to_dev(d1), True, residual)
        r1 = _ratio(y1, d1, True, residual)
    finally:
        _lib.set_option("GEMM_TUNE", old)
    _record(f"conv1x1/tuned/{_ids(case)}/first", r0)
    _record(f"conv1x1/tuned/{_ids(case)}/next", r1)
    assert r0 <= 1.0 and r1 <= 1.0, (r0, r1)


# ---- (b) dmm_im2col3x3_bf16 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", IM2COL_SHAPES, ids=_ids)
def test_im2col_is_bit_exact(shape, stride):
    B, C, H, W = shape
    x = fr.patch_inputs(*shape)["x"]
    want = fr.im2col3x3_ref(x, stride)
    xd = _cl(x)
    cols = _nan_like(tuple(want.shape))
    _lib.call("dmm_im2col3x3_bf16", DEV, xd.data_ptr(), B, H, W, C, stride, cols.data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    assert torch.equal(cols.cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("residual", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", [(1, 72, 2, 3), (3, 64, 13, 18)], ids=_ids)
def test_conv3x3_patches_against_fp64(shape, stride, residual):
    """Patch matrix + ONE GEMM with the tail in its epilogue, against float64 conv2d of the same bf16 values: the bound of a
    product of 9 C terms."""
    B, C, H, W = shape
    d = fr.patch_inputs(*shape)
    cout = d["w"].shape[0]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    res = fr.patch_residual(B, cout, Ho, Wo) if residual else None
    conv = nn.Conv2d(C, cout, 3, stride, 1)
    with torch.no_grad():
        conv.weight.copy_(d["w"].float())
        conv.bias.copy_(d["bias"])
    fast = _fast_with(conv.to(DEV))
    y = fast._conv3x3_patches(_cl(d["x"]), fast.src.extra, True, None if res is None else _cl(res))
    assert y is not None and y.shape == (B, cout, Ho, Wo) and y.is_contiguous(memory_format=torch.channels_last)
    ref, S = fr.conv3x3_64(d["x"], d["w"], d["bias"], res, True, stride)
    r = float(torch.nan_to_num((y.double().cpu() - ref).abs() / fr.bound_conv1x1(ref, S, 9 * C), nan=float("inf")).max())
    _record(f"conv3x3_patches/{_ids(shape)}/s{stride}/{'res' if residual else 'nores'}", r)
    assert r <= 1.0, r


# ---- (c) FastEncoder._conv1x1's routes ---------------------------------------------------------------------------------
def _route(name, relu, residual, fused, calls, monkeypatch, channels_last=True, twice=None):
    B, cin, cout, H, W, s = fr.ROUTE_SHAPES[name]
    x, d = fr.route_inputs(name)
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    fast = _fast_with(_conv1x1_module(d, s))
    monkeypatch.setattr(fast, "fused_gemm", fused, raising=False)
    xd = _cl(x) if channels_last else x.to(DEV).contiguous()
    assert xd.is_contiguous(memory_format=torch.channels_last) == channels_last
    res = _cl(d["res"].view(B, Ho, Wo, cout).permute(0, 3, 1, 2)) if residual else None
    del calls[:]
    y = fast._conv1x1(xd, fast.src.extra, relu, res)
    assert y.shape == (B, cout, Ho, Wo)
    twice = (not fused) if twice is None else twice           # the product stored before the epilogue kernel adds the bias
    r = _ratio(y.permute(0, 2, 3, 1), d, relu, residual, extra=_pre_abs(d) if twice else None)
    return r, list(calls)


FUSED_ROUTES = [
    ("s1", True, (True, False), ["dmm_conv1x1_bf16"]),
    ("s1", True, (True, True), ["dmm_conv1x1_bf16"]),
    ("s1", True, (False, True), ["dmm_conv1x1_bf16"]),
    ("s2_even", True, (False, False), ["dmm_subsample2_bf16", "dmm_conv1x1_bf16"]),
    ("s2_odd", True, (False, False), ["dmm_subsample2_bf16", "dmm_conv1x1_bf16"]),
    ("s2_odd", True, (True, True), ["dmm_subsample2_bf16", "dmm_conv1x1_bf16"]),
    ("s2_odd", False, (False, False), ["dmm_conv1x1_bf16"]),              # the slicing branch
    ("s2_even", False, (True, True), ["dmm_conv1x1_bf16"]),
]


@pytest.mark.parametrize("name,channels_last,form,want", FUSED_ROUTES,
                         ids=[f"{n}-{'cl' if c else 'nchw'}-{_form(f)}" for n, c, f, _ in FUSED_ROUTES])
def test_conv1x1_fused_routes(name, channels_last, form, want, calls, monkeypatch):
    r, seen = _route(name, form[0], form[1], True, calls, monkeypatch, channels_last)
    assert seen == want, seen
    _record(f"route/{name}/{'cl' if channels_last else 'nchw'}/{_form(form)}", r)
    assert r <= 1.0, r


@pytest.mark.parametrize("form", FORMS, ids=_form)
@pytest.mark.parametrize("name", ["s1", "s2_odd"])
def test_conv1x1_unfused_route(name, form, calls, monkeypatch):
    """``fused_gemm = False``: torch.mm stores the product, ``dmm_bias_act_bf16`` adds the fp32 bias (+ residual) (+ ReLU) and
    stores again -- the bound gains ULP |x w| for the first store."""
    r, seen = _route(name, form[0], form[1], False, calls, monkeypatch)
    assert seen == (["dmm_subsample2_bf16"] if name != "s1" else []) + ["dmm_bias_act_bf16"], seen
    _record(f"route/{name}/unfused/{_form(form)}", r)
    assert r <= 1.0, r


@pytest.mark.parametrize("form", FORMS, ids=_form)
def test_conv1x1_unsupported_answer_takes_the_fallback(form, monkeypatch):
    """``DMM_ERR_UNSUPPORTED`` from the entry (answered here in its place: the library takes every shape of this file) is
    allowed by the caller and leads to torch.mm + ``dmm_bias_act_bf16`` with the fp32 bias, not to an error."""
    seen, real = [], _lib.call

    def answer(name, *a, **kw):
        seen.append(name)
        if name == "dmm_conv1x1_bf16":
            assert _lib.DMM_ERR_UNSUPPORTED in kw.get("allow", ())
            return _lib.DMM_ERR_UNSUPPORTED
        return real(name, *a, **kw)
    monkeypatch.setattr(_lib, "call", answer)
    r, names = _route("s2_odd", form[0], form[1], True, seen, monkeypatch, twice=True)
    assert names == ["dmm_subsample2_bf16", "dmm_conv1x1_bf16", "dmm_bias_act_bf16"], names
    _record(f"route/s2_odd/unsupported/{_form(form)}", r)
    assert r <= 1.0, r


@pytest.mark.parametrize("fused", [True, False], ids=["shipped", "unfused"])
def test_two_channel_heads(fused, calls, monkeypatch):
    """``hidden_size = 8`` with 1x1 heads: ``sk2``, ``prop2[0]`` (64 -> 2) and ``prop2[3]`` (2 -> 8) with real biases; whatever
    the library answers for two channels, the result is the convolution (through the scalar ``dmm_bias_act_bf16`` kernel where
    the product was stored first)."""
    from dmm_net_amd.encoder import FastEncoder
    fast = FastEncoder(fr.make_encoder("resnet34", hidden_size=8, kernel_size=1).to(DEV))
    monkeypatch.setattr(fast, "fused_gemm", fused, raising=False)
    B, H, W = 2, 9, 11
    for tag, conv, relu in (("sk2", fast.src.sk2, False), ("prop2.0", fast.src.prop2[0], True), ("prop2.3", fast.src.prop2[3], False)):
        cout, cin = conv.weight.shape[:2]
        assert min(cin, cout) == 2 and float(conv.bias.detach().abs().min()) > 0
        gen = torch.Generator().manual_seed(cin * 100 + cout)
        x = torch.randn((B * H * W, cin), generator=gen, dtype=torch.float64).clamp_min(0.0).to(BF16)
        d = {"x": x, "w": conv.weight.detach().cpu().view(cout, cin).t().to(BF16), "bias": conv.bias.detach().cpu().float(),
             "res": None}
        del calls[:]
        y = fast._conv(_cl(x.view(B, H, W, cin).permute(0, 3, 1, 2)), conv, relu)
        stored_twice = "dmm_bias_act_bf16" in calls
        assert stored_twice or (fused and calls == ["dmm_conv1x1_bf16"]), calls
        r = _ratio(y.permute(0, 2, 3, 1), d, relu, False, extra=_pre_abs(d) if stored_twice else None)
        _record(f"heads2/{tag}/{'shipped' if fused else 'unfused'}", r)
        assert r <= 1.0, (tag, r, calls)


# ---- (d) pieces of the network, teacher-forced -------------------------------------------------------------------------
FRAMES = [(2, 67, 97), (1, 64, 96)]
CONFIGS = ("shipped", "unfused", "patches")
_REF = {}


@functools.lru_cache(maxsize=None)
def _nets(arch):
    from dmm_net_amd.encoder import FastEncoder, fold_batchnorm
    folded = fold_batchnorm(fr.make_encoder(arch, hidden_size=64))
    dev = copy.deepcopy(folded).to(DEV)
    return folded, dev, FastEncoder(dev)


def _reference(arch, piece, x, patches):
    """``rounding_model`` of one piece on the host copy of the device's input, computed once per distinct input."""
    xh = x.detach().cpu()
    key = (arch, piece, patches, tuple(xh.shape), hashlib.sha1(xh.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest())
    if key not in _REF:
        _REF[key] = fr.rounding_model(_nets(arch)[0], piece, xh, patches=patches)
    return _REF[key]


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("frame", FRAMES, ids=_ids)
@pytest.mark.parametrize("arch", ["resnet50", "resnet34"])
def test_pieces_against_the_rounding_model(arch, frame, config, monkeypatch):
    """Each piece on the device's own previous bf16 output (the chain is never longer than one piece) against the float64
    rounding model of that piece; the yardstick is the eager bf16 channels-last copy of the same folded piece on the same input,
    which rounds at least as often.  ``FastEncoder`` may be at most 2x as far from the reference, in both metrics.  The model
    stores where the configuration stores: on the forced patch route a 3x3 convolution is ONE GEMM and rounds once."""
    folded, dev, fast = _nets(arch)
    if config == "unfused":
        monkeypatch.setattr(fast, "fused_gemm", False, raising=False)
    if config == "patches":
        monkeypatch.setattr(fast, "_use_patches", lambda x, conv, relu, residual: fast._p[id(conv)][2] is not None)
    B, H, W = frame
    img = torch.randn((B, 3, H, W), generator=torch.Generator().manual_seed(H * 1000 + W)).to(BF16).float().to(DEV)
    outs, failed = {}, []
    with torch.no_grad():
        for p in PIECES:
            src = fr.piece_input_of(p)
            x = img if src is None else outs[src]
            if p == "stem":
                y = fast._stem(x)
            elif p.startswith("layer"):
                y = fast._level(int(p[5:]) - 1, x)
            elif p.startswith("prop"):
                y = fast._prop(int(p[4:]), x)
            else:
                y = fast._skip(int(p[2:]), x)
            outs[p] = y
            eager = copy.deepcopy(fr.piece_module(dev, p)).to(BF16)
            y16 = eager(x.to(BF16).contiguous(memory_format=torch.channels_last))
            ref = _reference(arch, p, x, config == "patches")
            e_fast, e_yard = fr.piece_errors(y, ref), fr.piece_errors(y16, ref)
            tag = f"piece/{arch}/{_ids(frame)}/{config}/{p}"
            print(tag, e_fast, e_yard)
            for m, a, b in zip(("rel_l2", "worst_channel"), e_fast, e_yard):
                _record(f"{tag}/{m}/fast", a)
                _record(f"{tag}/{m}/eager_bf16", b)
                if not a <= 2.0 * b:
                    failed.append((p, m, a, b))
    assert not failed, failed
