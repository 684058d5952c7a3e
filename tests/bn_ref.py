"""float64 reference of the training encoder's BatchNorm kernels (``dmm_bn_*`` in ``csrc/dmm_encoder_train.hip``), the derived
error bounds, the shared case list and the seeded input builders -- TEST INFRASTRUCTURE ONLY (no test functions here).

Plain torch float64 on the host, from the same bf16 / fp32 values the kernels read.  Everything is 3-D: an activation is
``[G, n, C]`` (G statistics groups of n consecutive rows of a channels-last tensor viewed ``[rows, C]``), a statistic ``[G, C]``.

The reference DECIDES NOTHING in the backward: the ReLU gate is an input (the device's own ``y > 0`` in the GPU tests), so a
float64 run can never take another branch than the bf16 forward did, and no element is ever left out of a comparison.  The
forward's own ``max(v, 0)`` is 1-Lipschitz, so there the reference clamps for itself and the bounds still stand.

Bounds.  u = 2^-24 (one fp32 rounding), ULP = 2^-8 (one bf16 rounding), gamma(k) = k u / (1 - k u) (k roundings, Higham).
Each ``bound_*`` is gamma(k) x (the magnitudes that enter the fp32 path) (+ ULP |ref| for a bf16 store); k is counted from
the kernel source (compiled with -ffp-contract=off: every operation written there rounds once, an fma once) and written
beside the formula.  ``tests/test_bn_ref_cpu.py`` holds them against an fp32 emulation of the kernels' arithmetic.
"""
import collections
import functools
import math

import torch

U = 2.0 ** -24
ULP = 2.0 ** -8
EPS = 1e-5


def gamma(k):
    return k * U / (1.0 - k * U)


def f32(v):
    """The fp32 value of a Python scalar (what a ``float`` kernel argument holds), as a Python float."""
    return float(torch.tensor(v, dtype=torch.float32))


# ---- the reference --------------------------------------------------------------------------------------------------
def stats64(x):
    """x [G, n, C] -> S = sum x, Q = sum x^2, each [G, C]."""
    x = x.double()
    return x.sum(1), (x * x).sum(1)


def moments64(S, Q, n, eps):
    """-> mean, biased var (clamped at 0, as the kernel clamps), invstd; each [G, C]."""
    mean = S.double() / n
    var = (Q.double() / n - mean * mean).clamp_min(0.0)
    return mean, var, 1.0 / torch.sqrt(var + eps)


def normalize64(x, res, mean, invstd, w, b, relu):
    """The unrounded y from GIVEN statistics: (x - mean) invstd w + b (+ res), then max(., 0)."""
    y = (x.double() - mean.double()[:, None]) * (invstd.double() * w.double())[:, None] + b.double()
    if res is not None:
        y = y + res.double()
    return y.clamp_min(0.0) if relu else y


def apply64(x, res, S, Q, w, b, eps, relu):
    """-> mean, biased var, invstd [G, C] and the unrounded y [G, n, C], from the sums S, Q."""
    mean, var, invstd = moments64(S, Q, x.shape[1], eps)
    return mean, var, invstd, normalize64(x, res, mean, invstd, w, b, relu)


def running64(S, Q, n, rm, rv, momentum):
    """The running buffers after G updates in group order; the unbiased factor only where n > 1."""
    mean, var, _ = moments64(S, Q, n, 0.0)
    rm, rv = rm.double().clone(), rv.double().clone()
    for g in range(S.shape[0]):
        unb = var[g] * (n / (n - 1.0)) if n > 1 else var[g]
        rm = rm + momentum * (mean[g] - rm)
        rv = rv + momentum * (unb - rv)
    return rm, rv


def cotangent64(dy, dy2, gate):
    g = dy.double() if dy2 is None else dy.double() + dy2.double()
    return g if gate is None else g * gate.double()


def reduce64(dy, dy2, x, gate, mean, invstd):
    """-> sum g, sum g xhat per group [G, C]; g = (dy + dy2) gate (gate None: no ReLU)."""
    g = cotangent64(dy, dy2, gate)
    xhat = (x.double() - mean.double()[:, None]) * invstd.double()[:, None]
    return g.sum(1), (g * xhat).sum(1)


def dx_terms64(dy, dy2, x, gate, mean, invstd, w, sg, sgx):
    """The three terms of dx = a g - a mean(g) - a xhat mean(g xhat), a = w invstd; each [G, n, C]."""
    n = x.shape[1]
    g = cotangent64(dy, dy2, gate)
    a = (w.double() * invstd.double())[:, None]
    xhat = (x.double() - mean.double()[:, None]) * invstd.double()[:, None]
    return a * g, (a * (sg.double() / n)[:, None]).expand_as(g), a * xhat * (sgx.double() / n)[:, None]


def dx64(dy, dy2, x, gate, mean, invstd, w, sg, sgx):
    t0, t1, t2 = dx_terms64(dy, dy2, x, gate, mean, invstd, w, sg, sgx)
    return t0 - t1 - t2


def dres64(dy, dy2, gate):
    """The residual branch's gradient: g rounded to bf16 ONCE (fp32 sum of the two bf16 cotangents, then the store)."""
    g = dy.float() if dy2 is None else dy.float() + dy2.float()
    g = g.bfloat16()
    return g if gate is None else torch.where(gate, g, torch.zeros_like(g))


def layer64(x, res, w, b, rm, rv, momentum, eps, relu, dy, dy2=None, gate=None):
    """The composition with statistics from x: what ``F.batch_norm(training=True)`` (+ residual) (+ ReLU) computes per group
    and its gradients, with the GIVEN gate (None with relu: the reference's own y > 0).  dweight / dbias: the groups' sums
    added in group order."""
    n = x.shape[1]
    S, Q = stats64(x)
    mean, var, invstd, y = apply64(x, res, S, Q, w, b, eps, relu)
    if relu and gate is None:
        gate = y > 0
    if not relu:
        gate = None
    sg, sgx = reduce64(dy, dy2, x, gate, mean, invstd)
    nrm, nrv = running64(S, Q, n, rm, rv, momentum)
    return {"y": y, "dx": dx64(dy, dy2, x, gate, mean, invstd, w, sg, sgx), "dres": dres64(dy, dy2, gate),
            "dweight": sgx.sum(0), "dbias": sg.sum(0), "running_mean": nrm, "running_var": nrv,
            "mean": mean, "var": var, "invstd": invstd, "S": S, "Q": Q, "sg": sg, "sgx": sgx}


# ---- derived bounds (all elementwise; shapes as the quantity they bound) ----------------------------------------------
def bound_S(x):
    # n terms in any order: at most n - 1 additions on a term's path (the accumulators and the zeroed buffer start at 0)
    n = x.shape[1]
    return gamma(max(n - 1, 0)) * x.double().abs().sum(1)


def bound_Q(x):
    # x^2 of a bf16 value is exact in fp32; the fma that enters it rounds once, then at most n - 1 additions: n
    n = x.shape[1]
    return gamma(n) * (x.double() ** 2).sum(1)


def sqrt_unit_S(x):
    """u sqrt(n) sqrt(sum x^2): the unit of the measured statistics bounds (a random walk of n roundings)."""
    n = x.shape[1]
    return U * math.sqrt(n) * (x.double() ** 2).sum(1).sqrt()


def sqrt_unit_Q(x):
    n = x.shape[1]
    return U * math.sqrt(n) * (x.double() ** 4).sum(1).sqrt()


def bound_mean(S, n):
    # inv_n = fl(1 / n), mean = fl(S inv_n): 2
    return gamma(0 if n & (n - 1) == 0 else 2) * (S.double() / n).abs()      # (n a power of two: both are exact)


def var_err(S, Q, n):
    # q inv_n: inv_n (1) + the product (1); mean^2: 2 roundings in each factor (4); the fma's own rounding (1) on the
    # result, which is below Q/n + mean^2: at most 5 on either magnitude (the clamp at 0 is 1-Lipschitz)
    # n a power of two (n = 1 and 2 among them): inv_n, q inv_n and mean are exact, the fma rounds the difference itself once
    mean = S.double() / n
    if n & (n - 1) == 0:
        return gamma(1) * (Q.double() / n - mean * mean).abs()
    return gamma(5) * (Q.double() / n + mean * mean)


def bound_invstd_rel(S, Q, n, eps):
    """|invstd / invstd64 - 1|: fl(var + eps) (half a rounding after the root), sqrtf, the division (both correctly
    rounded): 2.5 <= 3; the variance's error r relative to var64 + eps goes through 1 / sqrt: 1 / sqrt(1 - r) - 1."""
    _, var, _ = moments64(S, Q, n, eps)
    r = var_err(S, Q, n) / (var + eps)
    assert float(r.max()) < 0.5, float(r.max())               # (beyond that the case says nothing about the kernel)
    return gamma(3) + (1.0 / torch.sqrt(1.0 - r) - 1.0) * (1.0 + gamma(3))


def bound_y(x, res, mean, invstd, w, b, y64):
    # scale = fl(w invstd) (1, on x scale and on mean scale), shift = fma (1), v = fma (1), v + res (1): 4 with a residual,
    # 3 without; then the bf16 store of the fp32 value
    scale = (w.double() * invstd.double())[:, None]
    mag = (x.double() * scale).abs() + (mean.double()[:, None] * scale).abs() + b.double().abs()
    k = 3
    if res is not None:
        mag, k = mag + res.double().abs(), 4
    return ULP * y64.abs() + (1.0 + ULP) * gamma(k) * mag


def bound_running(S, Q, n, rm, rv, momentum):
    """-> (bound of running_mean, bound of running_var) after G updates.  Per update: mean (2) + the difference (1) + the
    fma (1) = 4 on |mean| + |rm|; unb = var fl(n / (n - 1)) (2) + the difference (1) + the fma (1) = 4 on |unb| + |rv|,
    plus momentum x the variance's own error x n / (n - 1).  An earlier update's error only shrinks ((1 - momentum) <= 1)."""
    G = S.shape[0]
    mean, var, _ = moments64(S, Q, n, 0.0)
    f = n / (n - 1.0) if n > 1 else 1.0
    unb = var * f
    bm, bv = torch.zeros_like(rm, dtype=torch.float64), torch.zeros_like(rv, dtype=torch.float64)
    crm, crv = rm.double().clone(), rv.double().clone()
    for g in range(G):
        bm = bm + gamma(4) * (mean[g].abs() + crm.abs())
        bv = bv + gamma(4) * (unb[g].abs() + crv.abs()) + momentum * f * var_err(S[g:g + 1], Q[g:g + 1], n)[0]
        crm = crm + momentum * (mean[g] - crm)
        crv = crv + momentum * (unb[g] - crv)
    return bm, bv


def bound_sums(dy, dy2, x, gate, mean, invstd):
    """-> (bound of sum g, bound of sum g xhat).  g = fl(dy + dy2) (1); at most n - 1 additions: n.  xhat = fl(fl(x - mean)
    invstd) (2), the fma that enters the product (1), at most n - 1 additions, g (1): n + 3."""
    n = x.shape[1]
    g = cotangent64(dy, dy2, gate)
    xhat = (x.double() - mean.double()[:, None]) * invstd.double()[:, None]
    return gamma(n) * g.abs().sum(1), gamma(n + 3) * (g * xhat).abs().sum(1)


def sqrt_units_sums(dy, dy2, x, gate, mean, invstd):
    n = x.shape[1]
    g = cotangent64(dy, dy2, gate)
    xhat = (x.double() - mean.double()[:, None]) * invstd.double()[:, None]
    return U * math.sqrt(n) * (g ** 2).sum(1).sqrt(), U * math.sqrt(n) * ((g * xhat) ** 2).sum(1).sqrt()


def bound_dx(dy, dy2, x, gate, mean, invstd, w, sg, sgx):
    # a = fl(w invstd) (1); g = fl(dy + dy2) (1); mg = fl(sg fl(1 / n)) (2), mgx likewise (2); xhat (2); g - mg (1);
    # xhat mgx (1); the difference (1); a (...) (1).  The longest path, a xhat mgx: 1 + 2 + 2 + 1 + 1 + 1 = 8
    t0, t1, t2 = dx_terms64(dy, dy2, x, gate, mean, invstd, w, sg, sgx)
    return ULP * (t0 - t1 - t2).abs() + (1.0 + ULP) * gamma(8) * (t0.abs() + t1.abs() + t2.abs())


def bound_param_grads_det(folded):
    """dweight / dbias of the deterministic form: the G folded group totals [G, C] added in order: at most G - 1 additions
    (the issue's G kept: it is the larger)."""
    G = folded.shape[0]
    return gamma(G) * folded.double().abs().sum(0)


# ---- cases -----------------------------------------------------------------------------------------------------------
# name: C channels, `groups` statistics groups of n rows each; the activation is [B, C, H, W] channels-last with B a multiple
# of groups and B H W = groups n.  offset: |mean| / std rises across the channels to this value (0: x = 1.7 randn + 0.4).
Case = collections.namedtuple("Case", "name C groups n B H W offset momentum")


def _hw(n):
    h = max(d for d in range(1, int(math.isqrt(n)) + 1) if n % d == 0)
    return h, n // h


def _case(C, groups, n, offset=0, momentum=0.1, b=1):
    assert n % b == 0
    h, w = _hw(n // b)
    tag = f"c{C}_g{groups}_n{n}" + (f"_off{offset}" if offset else "")
    return Case(tag, C, groups, n, groups * b, h, w, offset, momentum)


def rows_per_pass(C):
    """(rows one pass of a reduction workgroup covers, rows one pass of an elementwise workgroup covers)."""
    c8 = C // 8
    return 256 // min(c8, 32), 256 // c8


CHANNELS = (8, 16, 32, 256, 512, 2048)
BIG = {8: 2115, 16: 2115, 32: 2115, 256: 2115, 512: 1155, 2048: 1155}      # 5 9 47 / 3 5 7 11: a multiple of nothing


def _cases():
    out = []
    for i, C in enumerate(CHANNELS):
        s, e = rows_per_pass(C)
        # 1: the rows > 1 branch; 2, 7: below one pass; around the eight-deep load pipeline; the four-deep mode-1 reduce; a
        # one-row range for the second elementwise workgroup; several row groups
        for j, n in enumerate(dict.fromkeys((1, 2, 7, 8 * s - 1, 8 * s + 1, 4 * s + 1, 2 * e + 1, BIG[C]))):
            out.append(_case(C, 1, n, momentum=0.5 if (i + j) % 3 == 0 else 0.1))
    out += [_case(16, 2, 257), _case(256, 2, 66, b=2), _case(32, 2, 2115, offset=8, momentum=0.5),
            _case(8, 3, 1025), _case(512, 3, 33, momentum=0.5), _case(2048, 3, 9),
            _case(32, 64, 1), _case(32, 64, 9, momentum=0.5), _case(256, 64, 1), _case(2048, 64, 9), _case(8, 64, 9)]
    out += [_case(16, 1, 2115, offset=8), _case(256, 1, 2115, offset=8), _case(2048, 1, 63, offset=8),
            _case(512, 3, 65, offset=8), _case(256, 1, 2115, offset=32), _case(8, 1, 2049, offset=32, momentum=0.5)]
    assert len({c.name for c in out}) == len(out)
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
# the composition (_BNActFn): every width class and kernel path once, with groups 1, 3 and 64
LAYER_CASES = ["c8_g1_n1025", "c32_g1_n513", "c256_g1_n65", "c512_g3_n33", "c2048_g1_n65", "c32_g64_n9",
               "c256_g2_n66", "c16_g1_n2115_off8", "c8_g64_n9"]
assert all(n in BY_NAME for n in LAYER_CASES), [n for n in LAYER_CASES if n not in BY_NAME]
# beside the list (8 MB a tensor): the only shape here whose statistics grid is cut by its cap / groups clamp -- 11 row groups
# of 64 rows wanted, 32 / 3 = 10 allowed
CLAMP_CASE = _case(2048, 3, 641)
BY_NAME[CLAMP_CASE.name] = CLAMP_CASE

CONST_VALUE = 0.125      # the constant channel: float64 variance exactly 0; 5 u 2 c^2 / eps = 1e-3, r of bound_invstd_rel


def special_channels(C):
    """(the constant channel, the channel with a negative weight, the channel with a zero weight)."""
    return C - 3, 1, C - 2


@functools.lru_cache(maxsize=None)
def inputs(name):
    """Seeded host inputs of one case, never modified: x, res, dy, dy2 [G, n, C] bf16; w, b, rm, rv [C] fp32."""
    c = BY_NAME[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 7919 + c.C)
    G, n, C = c.groups, c.n, c.C
    const, neg, zero = special_channels(C)

    def unit(lo, hi, shape):                                  # magnitudes in [lo, hi] with either sign
        v = lo + (hi - lo) * torch.rand(shape, generator=gen, dtype=torch.float64)
        return v * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)
    z = torch.randn((G, n, C), generator=gen, dtype=torch.float64)
    if c.offset:
        ratio = torch.linspace(0.0, float(c.offset), C, dtype=torch.float64)
        x = 1.7 * (z + ratio * (torch.randint(0, 2, (C,), generator=gen) * 2 - 1))
    else:
        x = 1.7 * z + 0.4
    x[:, :, const] = CONST_VALUE
    x = x.bfloat16()
    w = (0.5 + torch.rand(C, generator=gen, dtype=torch.float64)).float()
    w[neg], w[zero] = -w[neg], 0.0
    b = (0.3 * torch.randn(C, generator=gen, dtype=torch.float64)).float()
    b[zero] = 0.0                                             # w = b = 0: x scale + shift == 0 on every row, the gate's own edge
    res = torch.randn((G, n, C), generator=gen, dtype=torch.float64).bfloat16()
    rm = (0.3 * torch.randn(C, generator=gen, dtype=torch.float64)).float()
    rv = (0.5 + torch.rand(C, generator=gen, dtype=torch.float64)).float()
    S, Q = stats64(x)
    mean, _, invstd = moments64(S, Q, n, EPS)
    xhat = (x.double() - mean[:, None]) * invstd[:, None]
    xhat[:, :, const] = 0.0                                   # (exactly: the channel is constant)
    # dy, dy2 = bf16(randn + alpha_c + beta_c xhat), |alpha|, |beta| in [0.5, 1.5].  The signs are drawn once per channel, alpha's
    # at random and beta's so that the ReLU's gate (which favours xhat of w's sign) adds to mean(g) instead of cancelling it: the
    # narrow cases have six live channels, and every one of them has to carry both correction terms of dx
    sa = torch.randint(0, 2, (C,), generator=gen) * 2 - 1
    sb = sa * torch.where(w < 0, -1, 1)
    cots = []
    for _ in range(2):
        alpha, beta = unit(0.5, 1.5, (C,)).abs() * sa, unit(0.5, 1.5, (C,)).abs() * sb
        cots.append((torch.randn((G, n, C), generator=gen, dtype=torch.float64) + alpha + beta * xhat).bfloat16())
    return {"x": x, "res": res, "dy": cots[0], "dy2": cots[1], "w": w, "b": b, "rm": rm, "rv": rv}
