"""Guards of the inference encoder's float64 reference (tests/fast_enc_ref.py) -- no GPU.

The reference, its bound and its cases are what ``tests/test_gpu_fast_encoder_ref.py`` holds the device to, so they are held
here: the bound to an fp32 emulation of the contract (it must pass) and to every listed mutant (each must fail, or the bound
is too loose to matter); the cases to the condition that makes the ReLU's position observable; the patch reference to a literal
loop; the rounding model to the folded network and to piece-level mutants."""
import copy
import functools

import pytest
import torch

import fast_enc_ref as fr
from fast_enc_ref import CONV_CASES, FORMS, IM2COL_SHAPES, MUTANTS, PIECES

_ids = lambda c: "x".join(map(str, c))


@pytest.mark.parametrize("case", CONV_CASES, ids=_ids)
def test_every_residual_relu_case_shows_both_sign_flips(case):
    """>= 10 % of the elements with pre < 0 < pre + res and >= 10 % with pre > 0 > pre + res, from the reference alone (every
    draw the GPU tests use: tags 0..2)."""
    for tag in (0, 1, 2):
        d = fr.conv_inputs(*case, tag)
        up, down = fr.flip_shares(d["x"], d["w"], d["bias"], d["res"])
        assert up >= fr.MIN_FLIP_SHARE and down >= fr.MIN_FLIP_SHARE, (case, tag, up, down)
        assert d["x"].dtype == d["w"].dtype == d["res"].dtype == torch.bfloat16 and d["bias"].dtype == torch.float32
        assert float(d["x"].min()) == 0.0                                   # (activations are relu(N(0, 1)))


@pytest.mark.parametrize("relu,residual", FORMS)
@pytest.mark.parametrize("case", CONV_CASES, ids=_ids)
def test_fp32_emulation_is_within_the_bound_and_every_mutant_is_not(case, relu, residual):
    d = fr.conv_inputs(*case)
    res = d["res"] if residual else None
    ref, S = fr.conv1x1_64(d["x"], d["w"], d["bias"], res, relu)
    bound = fr.bound_conv1x1(ref, S, case[1])
    got = fr.emulate_conv1x1(d["x"], d["w"], d["bias"], res, relu)
    assert bool(((got.double() - ref).abs() <= bound).all()), float(((got.double() - ref).abs() / bound).max())
    applied = []
    for m in MUTANTS:
        bad = fr.emulate_conv1x1(d["x"], d["w"], d["bias"], res, relu, mutant=m)
        if bad is None:
            continue
        applied.append(m)
        assert bool(((bad.double() - ref).abs() > bound).any()), (m, case, relu, residual)
    want = {"bias_rolled", "bias_by_row", "truncate", "bias_bf16"}
    want |= {"res_dropped", "res_twice"} if residual else set()
    want |= {"relu_before_res"} if (relu and residual) else set()
    want |= {"w_untransposed"} if case[1] == case[2] else set()
    assert set(applied) == want


def test_the_mutant_list_is_the_issues():
    """The seven of the issue, and the one the route tests found in ``FastEncoder._conv1x1``'s fallback (a bf16 bias)."""
    assert set(MUTANTS) == {"bias_rolled", "bias_by_row", "relu_before_res", "res_dropped", "res_twice", "truncate",
                            "w_untransposed", "bias_bf16"}
    assert any(c[1] == c[2] for c in CONV_CASES)                            # (the untransposed weight applies somewhere)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", IM2COL_SHAPES, ids=_ids)
def test_im2col_reference_is_the_literal_definition(shape, stride):
    """cols[(b, ho, wo), (kh, kw, c)] = x[b, s ho + kh - 1, s wo + kw - 1, c], zero outside: three loops over (b, ho, wo) x taps."""
    B, C, H, W = shape
    x = fr.patch_inputs(*shape)["x"]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    want = torch.zeros((B, Ho, Wo, 3, 3, C), dtype=x.dtype)
    for ho in range(Ho):
        for wo in range(Wo):
            for tap in range(9):
                hi, wi = stride * ho + tap // 3 - 1, stride * wo + tap % 3 - 1
                if 0 <= hi < H and 0 <= wi < W:
                    want[:, ho, wo, tap // 3, tap % 3] = x[:, :, hi, wi]
    got = fr.im2col3x3_ref(x, stride)
    assert got.dtype == x.dtype and torch.equal(got, want.reshape(B * Ho * Wo, 9 * C))
    assert bool((x != 0).all())                                             # (so every zero of the matrix is a border)
    # and the matrix times the (kh, kw, c)-ordered weight is the convolution
    d = fr.patch_inputs(*shape)
    wcol = d["w"].permute(2, 3, 1, 0).reshape(9 * C, -1)
    ref, S = fr.conv3x3_64(x, d["w"], d["bias"], None, False, stride)
    y = (got.double() @ wcol.double() + d["bias"].double()).view(B, Ho, Wo, -1).permute(0, 3, 1, 2)
    assert bool(((y - ref).abs() <= 1e-12 * S).all())


@pytest.mark.parametrize("name", list(fr.ROUTE_SHAPES))
def test_route_cases_show_both_sign_flips_and_keep_their_rows(name):
    B, cin, cout, H, W, s = fr.ROUTE_SHAPES[name]
    x, d = fr.route_inputs(name)
    assert min(fr.flip_shares(d["x"], d["w"], d["bias"], d["res"])) >= fr.MIN_FLIP_SHARE
    kept = x[:, :, ::s, ::s].permute(0, 2, 3, 1).reshape(-1, cin)
    assert torch.equal(kept, d["x"]) and (s == 1 or float(x[:, :, 1::2].min()) >= 3.0)


# ---- the rounding model ------------------------------------------------------------------------------------------------
FRAME = (1, 3, 33, 47)


@functools.lru_cache(maxsize=None)
def _folded(arch):
    from dmm_net_amd.encoder import fold_batchnorm
    return fold_batchnorm(fr.make_encoder(arch, hidden_size=64))


@functools.lru_cache(maxsize=None)
def _chain(arch, rounding):
    """Every piece's float64 output, each piece fed the previous piece's output of the same model."""
    folded = _folded(arch)
    img = torch.randn(FRAME, generator=torch.Generator().manual_seed(3))
    out = {}
    for p in PIECES:
        src = fr.piece_input_of(p)
        out[p] = fr.rounding_model(folded, p, img if src is None else out[src], rounding=rounding)
    return img, out


@pytest.mark.parametrize("arch", ["resnet34", "resnet50"])
def test_rounding_model_without_rounding_is_the_folded_network(arch):
    """Piece by piece against the float64 copy of ``fold_batchnorm(encoder)``'s own modules: 1e-10 relative."""
    folded = _folded(arch)
    img, out = _chain(arch, False)
    f64 = copy.deepcopy(folded).double()
    for p in PIECES:
        src = fr.piece_input_of(p)
        x = (img if src is None else out[src]).double()
        with torch.no_grad():
            want = fr.piece_module(f64, p)(x)
        assert want.shape == out[p].shape
        err = float((out[p] - want).abs().max()) / float(want.abs().max())
        assert err <= 1e-10, (p, err)
    # and the pieces chain to the whole forward
    with torch.no_grad():
        whole = f64(img.double())
    for k, t in zip((2, 3, 4, 5), whole["backbone_feature"]):
        assert float((out[f"prop{k}"] - t).abs().max()) <= 1e-9 * float(t.abs().max())
    for k, t in zip((5, 4, 3, 2), whole["refine_input_feat"]):
        assert float((out[f"sk{k}"] - t).abs().max()) <= 1e-9 * float(t.abs().max())


def test_rounding_model_stores_where_the_route_stores():
    """One 3x3 convolution (``sk5``): two stores on the library route (the convolution, then bias), one on the patch route."""
    import torch.nn.functional as F
    folded = _folded("resnet34")
    x = torch.randn((1, 512, 3, 4), generator=torch.Generator().manual_seed(5)).bfloat16()
    conv = F.conv2d(x.double(), folded.sk5.weight.detach().bfloat16().double(), None, 1, 1)
    b = folded.sk5.bias.detach().double().view(1, -1, 1, 1)
    two = fr.rounding_model(folded, "sk5", x)
    one = fr.rounding_model(folded, "sk5", x, patches=True)
    assert torch.equal(two, (conv.bfloat16().double() + b).bfloat16().double())
    assert torch.equal(one, (conv + b).bfloat16().double()) and not torch.equal(one, two)
    assert torch.equal(fr.rounding_model(folded, "sk5", x, rounding=False, patches=True),
                       fr.rounding_model(folded, "sk5", x, rounding=False))


def _applies(mutant, piece):
    if mutant == "sk_prop_swapped":
        return piece.startswith(("sk", "prop"))
    return piece.startswith("layer")


@pytest.mark.parametrize("arch", ["resnet34", "resnet50"])
def test_piece_comparison_flags_piece_level_mutants(arch):
    """The whole-piece comparison of the GPU test (both metrics of ``piece_errors`` against the rounding model): a mutant is
    flagged when its error exceeds twice that of an fp32-arithmetic evaluation of the same piece with the same roundings."""
    folded = _folded(arch)
    img, out = _chain(arch, True)
    seen = set()
    for p in PIECES:
        src = fr.piece_input_of(p)
        x = img if src is None else out[src]
        good = fr.piece_errors(fr.rounding_model(folded, p, x, arith=torch.float32), out[p])
        for m in fr.PIECE_MUTANTS:
            if not _applies(m, p):
                continue
            bad = fr.piece_errors(fr.rounding_model(folded, p, x, arith=torch.float32, mutant=m), out[p])
            assert bad[0] > 2.0 * good[0] and bad[1] > 2.0 * good[1], (p, m, bad, good)
            seen.add(m)
    assert seen == set(fr.PIECE_MUTANTS)
