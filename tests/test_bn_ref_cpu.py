"""Guards of the BatchNorm kernels' float64 reference (tests/bn_ref.py) -- no GPU.

The reference is what ``tests/test_gpu_bn_ref.py`` holds the kernels to, so it is itself held here: to torch's float64 autograd
through ``F.batch_norm``; to the condition that makes the cases worth running (both correction terms of dx carry weight in
every one of them); and its derived bounds to an fp32 emulation of the kernels' arithmetic, operation by operation."""
import pytest
import torch
import torch.nn.functional as F

import bn_ref
from bn_ref import EPS, CASES, inputs

SMALL = [c.name for c in CASES if c.groups * c.n * c.C <= 600_000]
assert {c.C for c in CASES if c.name in SMALL} == set(bn_ref.CHANNELS) and {1, 2, 3, 64} == {c.groups for c in CASES if c.name in SMALL}


def _off_the_kink(c, d, has_res):
    """x moved (for this check only) until no pre-activation lies within 1e-9 of the ReLU's kink without being on it, where
    float64 rounding could put the two sides on different branches.  Exactly 0 stays (the w = b = 0 channel): there autograd's
    subgradient and the gate y > 0 are both 0."""
    x = d["x"].double().clone()
    for _ in range(4):
        S, Q = bn_ref.stats64(x)
        pre = bn_ref.apply64(x, d["res"] if has_res else None, S, Q, d["w"], d["b"], EPS, False)[3]
        near = (pre.abs() < 1e-9) & (pre != 0)
        if not bool(near.any()):
            return x
        x = x + 0.5 * near
    raise AssertionError(c.name)


@pytest.mark.parametrize("relu,has_res", [(True, False), (True, True), (False, False), (False, True)])
@pytest.mark.parametrize("name", SMALL)
def test_reference_equals_float64_autograd(name, relu, has_res):
    """``layer64`` == float64 autograd through ``F.batch_norm(training=True)`` (+ residual) (+ ReLU), chunk by chunk for
    groups > 1: y, dx, dres, dweight, dbias and both running buffers within 1e-10 of each tensor's largest entry."""
    c, d = bn_ref.BY_NAME[name], inputs(name)
    mom = bn_ref.f32(c.momentum)
    x = _off_the_kink(c, d, has_res)
    res = d["res"] if has_res else None
    got = bn_ref.layer64(x, res, d["w"], d["b"], d["rm"], d["rv"], mom, EPS, relu, d["dy"], d["dy2"])

    xg = x.clone().requires_grad_(True)
    rg = res.double().requires_grad_(True) if has_res else None
    wg, bg = d["w"].double().requires_grad_(True), d["b"].double().requires_grad_(True)
    rm, rv = d["rm"].double().clone(), d["rv"].double().clone()
    ys = []
    for g in range(c.groups):
        if c.n > 1:
            y = F.batch_norm(xg[g], rm, rv, wg, bg, True, mom, EPS)
        else:                                                 # (torch refuses one value per channel: the same expression by hand)
            mu, var = xg[g].mean(0), xg[g].var(0, unbiased=False)
            y = (xg[g] - mu) / torch.sqrt(var + EPS) * wg + bg
            rm, rv = rm + mom * (mu.detach() - rm), rv + mom * (var.detach() - rv)
        y = y + rg[g] if has_res else y
        ys.append(F.relu(y) if relu else y)
    y = torch.stack(ys)
    cot = d["dy"].double() + d["dy2"].double()
    grads = torch.autograd.grad(y, [xg, wg, bg] + ([rg] if has_res else []), cot)
    want = {"y": y.detach(), "dx": grads[0], "dweight": grads[1], "dbias": grads[2], "running_mean": rm, "running_var": rv}
    for k, ref in want.items():
        err = float((got[k] - ref).abs().max())
        assert err <= 1e-10 * max(float(ref.abs().max()), 1e-300), (k, err)
    if has_res:                                               # the same gradient, stored in bf16 (one rounding of the fp32 sum)
        assert torch.equal(got["dres"], grads[3].float().bfloat16())


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_every_term_of_dx_carries_weight(name):
    """With a = w invstd: max |a mean(g)| and max |a xhat mean(g xhat)| are both >= 0.1 max |dx| in every committed case, with
    and without the ReLU and the second cotangent -- a kernel that dropped or mis-scaled either term is off by a tenth of the
    largest gradient at least.  Exempt: the channel the case makes constant on purpose (n = 1: every channel is, dx = 0)."""
    c, d = bn_ref.BY_NAME[name], inputs(name)
    keep = torch.ones(c.C, dtype=torch.bool)
    keep[bn_ref.special_channels(c.C)[0]] = False
    for relu in (False, True):
        for dy2 in (None, d["dy2"]):
            r = bn_ref.layer64(d["x"], None, d["w"], d["b"], d["rm"], d["rv"], 0.1, EPS, relu, d["dy"], dy2)
            gate = (r["y"] > 0) if relu else None
            _, t1, t2 = bn_ref.dx_terms64(d["dy"], dy2, d["x"], gate, r["mean"], r["invstd"], d["w"], r["sg"], r["sgx"])
            top = float(r["dx"][..., keep].abs().max())
            if c.n == 1:
                assert top <= 1e-12
                continue
            assert float(t1[..., keep].abs().max()) >= 0.1 * top and float(t2[..., keep].abs().max()) >= 0.1 * top, (
                relu, dy2 is not None, float(t1[..., keep].abs().max()), float(t2[..., keep].abs().max()), top)


def _fma32(a, b, c):
    """fl32(a b + c) of fp32 tensors: the product of two fp32 values is exact in float64."""
    return (a.double() * b.double() + c.double()).float()


def _under(err, bound, what):
    bad = err > bound
    assert not bool(bad.any()), (what, float(err[bad].max()), float((err / bound.clamp_min(1e-300)).max()))


@pytest.mark.parametrize("name", SMALL)
def test_bounds_hold_for_an_fp32_emulation_of_the_kernels(name):
    """The kernels' arithmetic redone in fp32 on the host, one rounding per operation as the source has them (an fma through
    float64), each stage fed what the stage before produced in fp32 -- the reference is fed its own fp32-rounded statistics.
    Every error against the float64 reference of the same inputs stays under the derived bound the GPU test asserts."""
    c, d = bn_ref.BY_NAME[name], inputs(name)
    n, G = c.n, c.groups
    x, res, dy, dy2, w, b = (d[k] for k in ("x", "res", "dy", "dy2", "w", "b"))
    eps, mom = torch.tensor(EPS, dtype=torch.float32), torch.tensor(c.momentum, dtype=torch.float32)
    xf = x.float()
    S, Q = xf.sum(1), (xf * xf).sum(1)
    S64, Q64 = bn_ref.stats64(x)
    _under((S - S64).abs(), bn_ref.bound_S(x), "S")
    _under((Q - Q64).abs(), bn_ref.bound_Q(x), "Q")

    inv_n = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)
    mean = S * inv_n
    var = _fma32(-mean, mean, Q * inv_n).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    m64, v64, i64 = bn_ref.moments64(S, Q, n, float(eps))
    _under((mean - m64).abs(), bn_ref.bound_mean(S, n), "mean")
    _under((var - v64).abs(), bn_ref.var_err(S, Q, n), "var")
    _under((invstd / i64 - 1.0).abs(), bn_ref.bound_invstd_rel(S, Q, n, float(eps)), "invstd")

    rm, rv = d["rm"].clone(), d["rv"].clone()
    nf = torch.tensor(float(n), dtype=torch.float32)
    for g in range(G):
        unb = var[g] * (nf / (nf - 1.0)) if n > 1 else var[g]
        rm = _fma32(mom, mean[g] - rm, rm)
        rv = _fma32(mom, unb - rv, rv)
    rm64, rv64 = bn_ref.running64(S, Q, n, d["rm"], d["rv"], float(mom))
    bm, bv = bn_ref.bound_running(S, Q, n, d["rm"], d["rv"], float(mom))
    _under((rm - rm64).abs(), bm, "running_mean")
    _under((rv - rv64).abs(), bv, "running_var")

    scale = w * invstd
    shift = _fma32(-mean, scale, b.expand_as(mean))
    for relu, r in ((True, res), (True, None), (False, res)):
        v = _fma32(xf, scale[:, None].expand_as(xf), shift[:, None].expand_as(xf))
        v = v + r.float() if r is not None else v
        y = (v.clamp_min(0.0) if relu else v).bfloat16()
        y64 = bn_ref.normalize64(x, r, mean, invstd, w, b, relu)
        _under((y.double() - y64).abs(), bn_ref.bound_y(x, r, mean, invstd, w, b, y64), ("y", relu, r is not None))
        gate = (y > 0) if relu else None
        for d2 in (None, dy2):
            g = dy.float() if d2 is None else dy.float() + d2.float()
            g = g if gate is None else torch.where(gate, g, torch.zeros_like(g))
            xhat = (xf - mean[:, None]) * invstd[:, None]
            sg, sgx = g.sum(1), (g.double() * xhat.double()).float().sum(1)
            sg64, sgx64 = bn_ref.reduce64(dy, d2, x, gate, mean, invstd)
            bg, bgx = bn_ref.bound_sums(dy, d2, x, gate, mean, invstd)
            # (the products rounded before the sum instead of inside the fma: one rounding more than the kernel's n + 3)
            _under((sg - sg64).abs(), bg, "sg")
            _under((sgx - sgx64).abs(), bgx + bn_ref.gamma(1) * (g.double() * xhat.double()).abs().sum(1), "sgx")
            a, mg, mgx = w * invstd, sg * inv_n, sgx * inv_n
            dx = (a[:, None] * ((g - mg[:, None]) - xhat * mgx[:, None])).bfloat16()
            dx64 = bn_ref.dx64(dy, d2, x, gate, mean, invstd, w, sg, sgx)
            _under((dx.double() - dx64).abs(), bn_ref.bound_dx(dy, d2, x, gate, mean, invstd, w, sg, sgx), "dx")
