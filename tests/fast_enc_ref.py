"""float64 reference of the inference encoder's GEMM and patch paths (``dmm_conv1x1_bf16`` in ``csrc/dmm_gemm.hip``,
``dmm_im2col3x3_bf16`` in ``csrc/dmm_encoder_ops.hip``, ``encoder.FastEncoder``), the derived error bound, the shared case
lists, the seeded input builders and the mutants -- TEST INFRASTRUCTURE ONLY (no test functions here).

Plain torch float64 on the host, from the same bf16 / fp32 values the device reads.  ``tests/test_fast_enc_ref_cpu.py`` holds
all of it (the bound against an fp32 emulation of the contract, every mutant against the bound, the patch reference against
a literal loop, the rounding model against the folded network); ``tests/test_gpu_fast_encoder_ref.py`` holds the device to it.
"""
import functools
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from bn_ref import U, ULP, gamma  # noqa: F401  (U, ULP re-exported: one definition of the units for all reference files)

BF16 = torch.bfloat16


# ---- dmm_conv1x1_bf16 -------------------------------------------------------------------------------------------------
def conv1x1_64(x, w, bias, res, relu):
    """x [rows, cin] bf16, w [cin, cout] bf16, bias [cout] fp32, res [rows, cout] bf16 or None ->
    (relu?(x w + bias (+ res)) in float64, the magnitude S = |x| |w| + |bias| (+ |res|) that entered it)."""
    xd, wd, bd = x.double(), w.double(), bias.double()
    ref, S = xd @ wd + bd, xd.abs() @ wd.abs() + bd.abs()
    if res is not None:
        ref, S = ref + res.double(), S + res.double().abs()
    return (ref.clamp_min(0.0) if relu else ref), S


def bound_conv1x1(ref, S, cin):
    """Elementwise bound of |device - ref| for  y = bf16( relu?( alpha (x . w) + beta res + bias ) ).

    The contract (header of dmm_gemm.hip, include/dmm_match.h 9b): a product of two bf16 values is exact in fp32 (8 + 8
    significant bits), the sum is kept in fp32, the bias is fp32, and the result is rounded to bf16 once.  Roundings on the
    path of one term into the fp32 value v before the store, whatever the order of the summation (a tree over cin leaves
    -- split-K included: its partial sums are added in fp32 -- puts at most cin - 1 additions above any leaf):
        cin - 1   additions of the products
        1 + 1     the alpha and beta multiplications (exact for alpha = beta = 1, counted as the issue counts them)
        1         the C (residual) add
        1         the bias add
    cin + 3 <= cin + 4, so |v - ref| <= gamma(cin + 4) S with S the sum of the magnitudes of all terms (Higham, Accuracy
    and Stability, 4.2); max(., 0) is 1-Lipschitz, so the ReLU changes nothing.  The store rounds v to nearest-even:
    |bf16(v) - v| <= ULP |v| <= ULP |ref| + ULP |v - ref|.  The last, second-order term is ULP (cin + 1) u S for the roundings
    that can actually happen; it fits under the spare three roundings of gamma(cin + 4) for cin <= 766 and is 0.4 % of the
    first-order term beyond (cin = 1024: 2.4e-7 S against 6.1e-5 S) -- the formula is the issue's, with no measured number."""
    return ULP * ref.abs() + gamma(cin + 4) * S


def emulate_conv1x1(x, w, bias, res, relu, mutant=None):
    """The contract in fp32 on the host: (x.float() @ w.float() + bias (+ res.float())), ReLU, one bf16 store.  ``mutant``: one of
    MUTANTS, a defect applied to the RESULT's arithmetic (never to a kernel); None where the mutant does not apply."""
    rows, cout = x.shape[0], w.shape[1]
    b = bias.float()
    if mutant == "w_untransposed":
        if w.shape[0] != w.shape[1]:
            return None
        w = w.t()
    if mutant in ("relu_before_res", "res_dropped", "res_twice") and res is None:
        return None
    if mutant == "relu_before_res" and not relu:
        return None
    v = x.float() @ w.float()
    if mutant == "bias_rolled":
        v = v + b.roll(1)
    elif mutant == "bias_by_row":                       # the bias along the other axis of the transposed problem
        v = v + b[torch.arange(rows) % cout][:, None]
    elif mutant == "bias_bf16":                         # the bias through bf16 (what a bf16 addmm does to it)
        v = v + b.bfloat16().float()
    else:
        v = v + b
    if mutant == "relu_before_res":
        v = v.clamp_min(0.0) + res.float()
    else:
        if res is not None and mutant != "res_dropped":
            v = v + res.float() * (2.0 if mutant == "res_twice" else 1.0)
        if relu:
            v = v.clamp_min(0.0)
    if mutant == "truncate":
        return (v.view(torch.int32) & -65536).view(torch.float32).bfloat16()
    return v.bfloat16()


MUTANTS = ("bias_rolled", "bias_by_row", "relu_before_res", "res_dropped", "res_twice", "truncate", "w_untransposed",
           "bias_bf16")

# (rows, cin, cout): rows != cout in all but the first, so a transposed bias cannot hide
CONV_CASES = [(1, 64, 64), (7, 8, 40), (63, 72, 8), (65, 576, 64), (257, 24, 256), (782, 256, 64), (782, 1024, 256),
              (130, 64, 2), (130, 2, 64)]
FORMS = [(False, False), (False, True), (True, False), (True, True)]          # (relu, residual)
MIN_FLIP_SHARE = 0.10


def flip_shares(x, w, bias, res):
    """(share of elements with pre < 0 < pre + res, share with pre > 0 > pre + res), pre = x w + bias in float64: where the
    position of the ReLU relative to the residual add decides the result."""
    pre = x.double() @ w.double() + bias.double()
    post = pre + res.double()
    return float(((pre < 0) & (post > 0)).double().mean()), float(((pre > 0) & (post < 0)).double().mean())


def _draw(rows, cin, cout, seed):
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=gen, dtype=torch.float64)
    x = rn(rows, cin).clamp_min(0.0).to(BF16)                                # activations: relu(N(0, 1))
    w = (rn(cin, cout) / math.sqrt(cin)).to(BF16)                            # weights: N(0, 1 / (cin k k)), k = 1
    bias = (math.sqrt(0.5) * rn(cout)).float()                               # bias: N(0, 0.5), fp32
    res = rn(rows, cout).to(BF16)                                            # residual: N(0, 1)
    return {"x": x, "w": w, "bias": bias, "res": res}


@functools.lru_cache(maxsize=None)
def conv_inputs(rows, cin, cout, tag=0):
    """Seeded host inputs of one (rows, cin, cout) case, never modified.  ``tag`` gives further independent draws of the same
    shape.  The seed is advanced until the REFERENCE shows both sign-flip shares >= MIN_FLIP_SHARE (12.5 % each in
    expectation: a small case can fall short by chance), so that the ReLU's position is observable in every case."""
    seed = (rows * 1_000_003 + cin * 1009 + cout) * 16 + tag * 7919
    for step in range(64):
        d = _draw(rows, cin, cout, seed + step * 104729)
        if min(flip_shares(d["x"], d["w"], d["bias"], d["res"])) >= MIN_FLIP_SHARE:
            return d
    raise AssertionError((rows, cin, cout, tag))


# FastEncoder._conv1x1's routes: (B, cin, cout, H, W, stride); weights, bias, residual and the rows the product sees are
# conv_inputs(B Ho Wo, cin, cout, ROUTE_TAG), the positions a stride skips hold other values
ROUTE_SHAPES = {"s1": (2, 64, 40, 9, 11, 1), "s2_even": (2, 64, 40, 16, 24, 2), "s2_odd": (2, 64, 40, 17, 23, 2)}
ROUTE_TAG = 3


@functools.lru_cache(maxsize=None)
def route_inputs(name):
    """-> x [B, cin, H, W] bf16 (NCHW-contiguous host tensor), and the conv_inputs dict of the rows a stride keeps."""
    B, cin, cout, H, W, s = ROUTE_SHAPES[name]
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    d = conv_inputs(B * Ho * Wo, cin, cout, ROUTE_TAG)
    gen = torch.Generator().manual_seed(H * 131 + W)
    x = (torch.randn((B, cin, H, W), generator=gen, dtype=torch.float64).clamp_min(0.0) + 3.0).to(BF16)
    x[:, :, ::s, ::s] = d["x"].view(B, Ho, Wo, cin).permute(0, 3, 1, 2)
    return x, d


# ---- dmm_im2col3x3_bf16 ------------------------------------------------------------------------------------------------
IM2COL_SHAPES = [(1, 8, 1, 1), (2, 8, 1, 7), (2, 16, 6, 1), (1, 72, 2, 3), (3, 64, 13, 18), (2, 24, 8, 8), (2, 24, 7, 9)]


def im2col3x3_ref(x, stride):
    """x [B, C, H, W] -> the patch matrix [B Ho Wo, 9 C] of a 3x3 / padding 1 convolution, columns ordered (kh, kw, c), zero
    outside the image (values copied, so the comparison is exact)."""
    B, C, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    ref = F.unfold(x.float(), 3, padding=1, stride=stride)                   # [B, C * 9, L], (c, kh, kw) order
    return ref.view(B, C, 9, Ho * Wo).permute(0, 3, 2, 1).reshape(B * Ho * Wo, 9 * C).to(x.dtype)


@functools.lru_cache(maxsize=None)
def patch_inputs(B, C, H, W, cout=40):
    """Seeded host inputs of a 3x3 convolution case: x [B, C, H, W] bf16 (no value zero, so a missing tap shows), the weight
    [cout, C, 3, 3] bf16 and fp32 bias; residuals are drawn by the caller's stride (``patch_residual``)."""
    gen = torch.Generator().manual_seed(B * 1_000_003 + C * 10007 + H * 101 + W)
    x = torch.randn((B, C, H, W), generator=gen, dtype=torch.float64).clamp_min(0.0) + 2.0 ** -6
    w = torch.randn((cout, C, 3, 3), generator=gen, dtype=torch.float64) / math.sqrt(9 * C)
    bias = math.sqrt(0.5) * torch.randn(cout, generator=gen, dtype=torch.float64)
    return {"x": x.to(BF16), "w": w.to(BF16), "bias": bias.float()}


def patch_residual(B, cout, Ho, Wo):
    gen = torch.Generator().manual_seed(B * 31 + cout * 17 + Ho * 7 + Wo)
    return torch.randn((B, cout, Ho, Wo), generator=gen, dtype=torch.float64).to(BF16)


def conv3x3_64(x, w, bias, res, relu, stride):
    """float64 ``F.conv2d`` of the bf16 values (+ bias (+ res)) (ReLU) and its magnitude S, both [B, cout, Ho, Wo]."""
    xd, wd, bd = x.double(), w.double(), bias.double()
    ref = F.conv2d(xd, wd, bd, stride, 1)
    S = F.conv2d(xd.abs(), wd.abs(), bd.abs(), stride, 1)
    if res is not None:
        ref, S = ref + res.double(), S + res.double().abs()
    return (ref.clamp_min(0.0) if relu else ref), S


# ---- pieces of the BatchNorm-folded network ----------------------------------------------------------------------------
PIECES = ("stem", "layer1", "layer2", "layer3", "layer4", "prop2", "prop3", "prop4", "prop5", "sk2", "sk3", "sk4", "sk5")
PIECE_MUTANTS = ("relu2_missing", "res_dropped", "sk_prop_swapped")


def piece_module(folded, piece):
    """The folded encoder's own module of one piece (what the eager yardstick runs)."""
    body = folded.base
    if piece == "stem":
        return nn.Sequential(body.conv1, body.bn1, body.relu, body.maxpool)
    if piece.startswith("layer"):
        return getattr(body, piece)
    if piece.startswith("prop"):
        return getattr(folded, piece)
    return nn.Sequential(getattr(folded, piece), getattr(folded, "bn" + piece[2:]))


def piece_input_of(piece):
    """The piece whose output a piece reads (None: the image)."""
    if piece == "stem":
        return None
    if piece.startswith("layer"):
        return "stem" if piece == "layer1" else "layer%d" % (int(piece[5:]) - 1)
    return "layer%d" % (int(piece[-1]) - 1)


def _patch_form(m):
    """The 3x3 convolutions ``FastEncoder`` can run as patch matrix + ONE GEMM (its ``_patch_ok``, from the module's own fields)."""
    return (m.kernel_size == (3, 3) and m.padding == (1, 1) and m.dilation == (1, 1) and m.groups == 1
            and m.stride in ((1, 1), (2, 2)) and m.in_channels % 8 == 0)


def rounding_model(folded, piece, x, rounding=True, arith=torch.float64, mutant=None, patches=False):
    """One piece of a BatchNorm-folded ``FeatureEncoder`` on the input x [B, C, H, W], evaluated in ``arith`` (float64: the
    reference; float32: an emulation of correct fp32 arithmetic), walked from the encoder's own modules -- the block
    definitions of the torchvision bodies and ``_prop_head`` -- and not from ``FastEncoder``.

    ``rounding``: weights go through bf16, biases stay fp32, and an activation is rounded to bf16 exactly where ``FastEncoder``
    stores it: once after a 1x1 convolution's whole tail (bias (+ residual) (+ ReLU) ride in the GEMM's epilogue); for a k x k
    convolution once after the convolution before its bias (the library's store) and once after bias (+ residual) (+ ReLU); for
    the stem after the convolution and after bias + ReLU + max-pool (rounding is monotone: it commutes with the maximum).
    ``patches``: the model of the forced patch route -- a 3x3 convolution that has a patch form is a GEMM there and stores once,
    like a 1x1.  Switched off, nothing is rounded: the piece of ``fold_batchnorm(encoder)`` itself.  ``mutant``: one of
    PIECE_MUTANTS."""
    from dmm_net_amd.encoder import Bottleneck

    def rnd(t):
        return t.to(BF16).to(arith) if rounding else t

    def conv(t, m, relu, res=None, pool=None):
        assert isinstance(m, nn.Conv2d) and m.bias is not None and m.groups == 1, m
        w = m.weight.detach().cpu()
        w = (w.to(BF16) if rounding else w).to(arith)
        b = m.bias.detach().cpu().float().to(arith).view(1, -1, 1, 1)
        y = F.conv2d(t, w, None, m.stride, m.padding, m.dilation)
        if m.kernel_size != (1, 1) and not (patches and _patch_form(m)):
            y = rnd(y)
        y = y + b
        if res is not None:
            y = y + res
        if relu:
            y = y.clamp_min(0.0)
        if pool is not None:
            y = pool(y)
        return rnd(y)

    def block(t, blk):
        idt = t if blk.downsample is None else conv(t, blk.downsample[0], False)
        if mutant == "res_dropped":
            idt = None
        if isinstance(blk, Bottleneck):
            out = conv(t, blk.conv1, True)
            out = conv(out, blk.conv2, mutant != "relu2_missing")
            return conv(out, blk.conv3, True, idt)
        out = conv(t, blk.conv1, True)
        return conv(out, blk.conv2, mutant != "relu2_missing", idt)

    x = x.detach().cpu().to(arith)
    with torch.no_grad():
        if piece == "stem":
            body = folded.base
            return conv(rnd(x), body.conv1, True, pool=body.maxpool)
        if piece.startswith("layer"):
            for blk in getattr(folded.base, piece):
                x = block(x, blk)
            return x
        k = piece[-1]
        sk, head = getattr(folded, "sk" + k), getattr(folded, "prop" + k)
        first = head[0]
        if mutant == "sk_prop_swapped":
            assert sk.weight.shape == first.weight.shape
            sk, first = first, sk
        if piece.startswith("sk"):
            return conv(x, sk, False)
        return conv(conv(x, first, True), head[3], False)


def piece_errors(got, ref):
    """(relative L2 of the whole tensor, the worst channel's L2 error / (the tensor's RMS sqrt(elements per channel)))."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = got - ref
    rel = float(err.norm() / ref.norm())
    per_c = err.pow(2).sum((0, 2, 3)).sqrt()
    n_c = ref.numel() // ref.shape[1]
    rms = float(ref.pow(2).mean().sqrt())
    return rel, float(per_c.max()) / (rms * math.sqrt(n_c))


def make_encoder(arch, hidden_size=64, kernel_size=3, seed=7):
    """A host ``FeatureEncoder`` in eval mode with BatchNorm running statistics randomised as the existing encoder tests do."""
    from dmm_net_amd.encoder import FeatureEncoder
    torch.manual_seed(seed)
    enc = FeatureEncoder(arch, hidden_size=hidden_size, kernel_size=kernel_size)
    gen = torch.Generator().manual_seed(seed + 1)
    for m in enc.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.2, generator=gen)
            m.running_var.uniform_(0.5, 1.5, generator=gen)
    return enc.eval()

