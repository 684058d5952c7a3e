"""``dmm_encoder_train.hip``'s BatchNorm kernels against the float64 reference of tests/bn_ref.py: kernel by kernel through the
C entries, each judged against float64 OF THE INPUTS THAT KERNEL RECEIVED (the device's sums for ``bn_apply``, the device's saved
statistics and y for the backward, the device's sums for ``bn_bwd_dx``) -- where a bound is exceeded, the kernel named is the
one at fault --, then the composition ``_BNActFn`` against ``layer64``.  The ReLU gate of every backward reference is the
device's own ``y > 0``; no element is left out anywhere.  Elementwise bounds are derived (bn_ref.bound_*: the rounding counts
are beside the formulas); the sqrt(n)-unit bounds of the sums and the composition's bounds are 3x what an MI355X reached
(``ACHIEVED``, from profiles/bn_ref_achieved.jsonl)."""
import functools
import types

import pytest
import torch

import bn_ref
from bn_ref import CASES, EPS, LAYER_CASES, ULP, f32, inputs
from dmm_net_amd import _lib
from dmm_net_amd import train_encoder as te_mod
from dmm_net_amd.train_encoder import _BNActFn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = [c.name for c in CASES]
# Worst achieved over the case list on an MI355X (profiles/bn_ref_achieved.jsonl, the "bn_ref/worst/..." records); every
# assertion below is against 3x these.  sums: |error| in units of u sqrt(n) sqrt(sum of the squared terms), per channel and
# group.  layer: bf16 outputs in units of 2^-8 |ref| + 1e-5 max|ref of the channel|, fp32 outputs relative to max|ref|.
ACHIEVED = {
    "stats/S": 2.46, "stats/Q": 10.4, "stats_det/S": 1.41, "stats_det/Q": 10.4,
    "reduce/sg": 3.11, "reduce/sgx": 4.41, "reduce_det/sg": 3.01, "reduce_det/sgx": 4.41,
    "layer/y": 0.99, "layer/dx": 0.992, "layer/dweight": 6.1e-6, "layer/dbias": 1.1e-7,
    "layer/running_mean": 7.4e-8, "layer/running_var": 2.3e-6,
}
# the composition's bounds may not exceed what test_bn_kernels_against_torch_fp32 allows: y 2^-8 |ref| + 1e-3 max|ref| (in
# this unit: 1.25 at the largest entry), dx 2e-2 of max|dx| (5.1), dweight / dbias 5e-3, running_mean 1e-4, running_var 1e-3
EXISTING = {"layer/y": 1.25, "layer/dx": 5.1, "layer/dweight": 5e-3, "layer/dbias": 5e-3, "layer/running_mean": 1e-4,
            "layer/running_var": 1e-3}


assert all(ACHIEVED[k] <= v for k, v in EXISTING.items())      # (otherwise: a finding to report, not a bound to loosen)


def _limit(key):
    """3x the achieved value, and never more than the existing test allows."""
    return min(3.0 * ACHIEVED[key], EXISTING.get(key, float("inf")))


def _record(name, v):
    from conftest import record_achieved
    record_achieved("bn_ref/" + name, v)


_WORST = {}


def _worst(key, v):
    """Record the running worst of one ACHIEVED quantity (the last record of a key in a run is the worst over its cases)."""
    if v > _WORST.get(key, -1.0):
        _WORST[key] = v
        _record("worst/" + key, v)


def _s():
    return torch.cuda.current_stream().cuda_stream


def _h(t, c=None):
    """Device tensor -> host; an activation [R, C] as [G, n, C]."""
    t = t.detach().cpu()
    return t if c is None else t.reshape(c.groups, c.n, c.C)


@functools.lru_cache(maxsize=None)
def _dev(name):
    """The case's inputs on the device, never modified: activations as [R, C] bf16 (a channels-last tensor viewed 2-D)."""
    c = bn_ref.BY_NAME[name]
    return {k: (v.reshape(-1, c.C) if v.dim() == 3 else v).to(DEV).contiguous() for k, v in inputs(name).items()}


def _ws(c):
    """A slab workspace of exactly the size the library asks for, filled with NaN patterns: the launch writes all it reads."""
    nb = int(_lib.load().dmm_bn_det_workspace_bytes(c.groups * c.n, c.C, c.groups))
    assert nb == c.groups * _parts(c) * 2 * c.C * 4 and nb > 0, nb
    return torch.full((nb,), 0xFF, dtype=torch.uint8, device=DEV), nb


def _parts(c):
    """Row groups of the statistics grid (bn_stat_grid): ceil(n / (8 rows-per-pass)), at most min(65536 / C, 256) / groups."""
    s = bn_ref.rows_per_pass(c.C)[0]
    cap = max(min(65536 // c.C, 256) // c.groups, 1)
    return max(min(-(-c.n // (8 * s)), cap), 1)


def _fold(c, ws, nb):
    out = torch.empty((c.groups, 2, c.C), device=DEV)
    _lib.call("dmm_bn_fold_det", DEV, ws.data_ptr(), nb, c.groups * c.n, c.C, c.groups, out.data_ptr(), _s())
    return out


def _p(t):
    return None if t is None else t.data_ptr()


def _stats(c, dv, det):
    """-> (what bn_apply is handed: the [G, 2, C] sums or the slab, its byte count, the [G, 2, C] totals)."""
    R = c.groups * c.n
    if det:
        ws, nb = _ws(c)
        _lib.call("dmm_bn_stats_det_grouped_bf16", DEV, dv["x"].data_ptr(), R, c.C, c.groups, ws.data_ptr(), nb, _s())
        return ws, nb, _fold(c, ws, nb)
    st = torch.zeros((c.groups, 2, c.C), device=DEV)
    _lib.call("dmm_bn_stats_grouped_bf16", DEV, dv["x"].data_ptr(), R, c.C, c.groups, st.data_ptr(), _s())
    return st, 0, st


def _apply(c, dv, det, stats, nb, relu, res, running=True):
    R = c.groups * c.n
    o = types.SimpleNamespace(y=torch.empty((R, c.C), dtype=torch.bfloat16, device=DEV),
                              saved=torch.empty((c.groups, 2, c.C), device=DEV),
                              rm=dv["rm"].clone() if running else None, rv=dv["rv"].clone() if running else None)
    tail = (dv["w"].data_ptr(), dv["b"].data_ptr(), _p(o.rm), _p(o.rv), c.momentum, EPS, int(relu), o.y.data_ptr(),
            o.saved.data_ptr(), _s())
    if det:
        _lib.call("dmm_bn_apply_det_grouped_bf16", DEV, dv["x"].data_ptr(), _p(res), R, c.C, c.groups, stats.data_ptr(), nb, *tail)
    else:
        _lib.call("dmm_bn_apply_grouped_bf16", DEV, dv["x"].data_ptr(), _p(res), R, c.C, c.groups, stats.data_ptr(), *tail)
    return o


def _forward(c, dv, relu, res):
    st, nb, _ = _stats(c, dv, False)
    return _apply(c, dv, False, st, nb, relu, res, running=False)


def _reduce(c, dv, det, mode, dy2, fwd):
    """-> (what bn_bwd_dx is handed, its byte count, the [G, 2, C] totals).  Mode 2 is handed no y: it recomputes the gate."""
    R = c.groups * c.n
    head = (dv["dy"].data_ptr(), _p(dy2), dv["x"].data_ptr(), fwd.y.data_ptr() if mode == 1 else None, R, c.C, c.groups,
            fwd.saved.data_ptr(), dv["w"].data_ptr(), dv["b"].data_ptr(), mode)
    if det:
        ws, nb = _ws(c)
        _lib.call("dmm_bn_bwd_reduce_det_grouped_bf16", DEV, *head, ws.data_ptr(), nb, _s())
        return ws, nb, _fold(c, ws, nb)
    sums = torch.zeros((c.groups, 2, c.C), device=DEV)
    _lib.call("dmm_bn_bwd_reduce_grouped_bf16", DEV, *head, sums.data_ptr(), _s())
    return sums, 0, sums


def _dx(c, dv, det, mode, dy2, fwd, sums, nb, dres=True, allow=()):
    R = c.groups * c.n
    o = types.SimpleNamespace(dx=torch.empty((R, c.C), dtype=torch.bfloat16, device=DEV),
                              dres=torch.empty((R, c.C), dtype=torch.bfloat16, device=DEV) if dres else None,
                              dw=torch.empty(c.C, device=DEV), db=torch.empty(c.C, device=DEV))
    head = (dv["dy"].data_ptr(), _p(dy2), dv["x"].data_ptr(), fwd.y.data_ptr() if mode == 1 else None, R, c.C, c.groups,
            fwd.saved.data_ptr(), dv["w"].data_ptr(), dv["b"].data_ptr())
    tail = (mode, o.dx.data_ptr(), _p(o.dres), o.dw.data_ptr(), o.db.data_ptr(), _s())
    if det:
        o.rc = _lib.call("dmm_bn_bwd_dx_det_grouped_bf16", DEV, *head, sums.data_ptr(), nb, *tail, allow=allow)
    else:
        o.rc = _lib.call("dmm_bn_bwd_dx_grouped_bf16", DEV, *head, sums.data_ptr(), *tail, allow=allow)
    return o


def _chk(fails, what, err, bound):
    """|error| <= bound on EVERY element; otherwise note the worst excess."""
    over = err > bound
    if bool(over.any()) or not bool(torch.isfinite(err).all()):
        ratio = err / bound.clamp_min(1e-300)
        fails.append(f"{what}: |err| up to {float(err.max()):.3g}, {float(ratio.max()):.3g} x its bound "
                     f"({int(over.sum())} of {over.numel()} elements over)")


def _in_units(err, unit):
    """max of err / unit; where the unit is 0 (n = 1, an all-zero column) the error must be 0 too."""
    assert bool((err[unit == 0] == 0).all())
    return float((err / unit.clamp_min(1e-300))[unit > 0].max()) if bool((unit > 0).any()) else 0.0


# (mode, relu, residual of the forward it belongs to): 0 no ReLU, 1 residual + ReLU (the gate from y), 2 ReLU alone (recomputed)
MODES = ((0, False, False), (1, True, True), (2, True, False))


# ---- statistics ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_bn_stats_against_fp64(name):
    """``bn_stats``, the atomic form and the deterministic form + ``bn_fold``: S and Q within the worst case of any order of
    n fp32 additions, and within 3x the achieved error in units of u sqrt(n) sqrt(sum x^2) (Q: sum x^4); the deterministic
    form bit-identical over three calls."""
    c, dv, x = bn_ref.BY_NAME[name], _dev(name), inputs(name)["x"]
    S64, Q64 = bn_ref.stats64(x)
    fails = []
    for det in (False, True):
        tot = _stats(c, dv, det)[2]
        if det:
            for _ in range(2):
                assert torch.equal(_stats(c, dv, True)[2], tot), "bn_stats (deterministic) differs between calls"
        tot = _h(tot).double()
        form = "stats_det" if det else "stats"
        for k, ref, bound, unit in ((0, S64, bn_ref.bound_S(x), bn_ref.sqrt_unit_S(x)),
                                    (1, Q64, bn_ref.bound_Q(x), bn_ref.sqrt_unit_Q(x))):
            err, key = (tot[:, k] - ref).abs(), f"{form}/{'SQ'[k]}"
            _chk(fails, f"bn_stats {key}", err, bound)
            got = _in_units(err, unit)
            _record(f"{key}/{name}", got)
            _worst(key, got)
            if not got <= _limit(key):
                fails.append(f"bn_stats {key}: {got:.3g} u sqrt(n) units > {_limit(key):.3g}")
    assert not fails, fails


# ---- forward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_bn_apply_against_fp64_of_the_device_sums(name):
    """``bn_apply`` in both forms: ``saved`` (mean, invstd) and the running statistics after G updates against float64 of
    the DEVICE's S, Q; y for relu x residual against float64 of the device's ``saved``, on every element; null running
    pointers change no bit of ``saved`` and y."""
    c, dv, h = bn_ref.BY_NAME[name], _dev(name), inputs(name)
    n, mom, eps = c.n, f32(c.momentum), f32(EPS)
    const = bn_ref.special_channels(c.C)[0]
    fails = []
    for det in (False, True):
        form = "det" if det else "atomic"
        st, nb, tot = _stats(c, dv, det)
        S, Q = _h(tot)[:, 0].double(), _h(tot)[:, 1].double()
        for relu in (False, True):
            for res in (None, dv["res"]):
                o = _apply(c, dv, det, st, nb, relu, res)
                tag = f"bn_apply[{form}, relu={int(relu)}, res={int(res is not None)}]"
                mean, invstd = _h(o.saved)[:, 0], _h(o.saved)[:, 1]
                m64, _, i64 = bn_ref.moments64(S, Q, n, eps)
                _chk(fails, f"{tag} saved mean", (mean - m64).abs(), bn_ref.bound_mean(S, n))
                rel = (invstd / i64 - 1.0).abs()
                _chk(fails, f"{tag} saved invstd", rel, bn_ref.bound_invstd_rel(S, Q, n, eps))
                y64 = bn_ref.normalize64(h["x"], None if res is None else h["res"], mean, invstd, h["w"], h["b"], relu)
                _chk(fails, f"{tag} y", (_h(o.y, c).double() - y64).abs(),
                     bn_ref.bound_y(h["x"], None if res is None else h["res"], mean, invstd, h["w"], h["b"], y64))
                rm64, rv64 = bn_ref.running64(S, Q, n, h["rm"], h["rv"], mom)
                bm, bv = bn_ref.bound_running(S, Q, n, h["rm"], h["rv"], mom)
                _chk(fails, f"{tag} running_mean", (_h(o.rm) - rm64).abs(), bm)
                _chk(fails, f"{tag} running_var", (_h(o.rv) - rv64).abs(), bv)
                if relu and res is not None:
                    keep = torch.arange(c.C) != const
                    _record(f"invstd_rel/{form}/{name}", float(rel[:, keep].max()))
                    q = _apply(c, dv, det, st, nb, relu, res, running=False)
                    if not (torch.equal(q.saved, o.saved) and torch.equal(q.y, o.y)):
                        fails.append(f"{tag}: null running pointers change saved / y")
    assert not fails, fails


# ---- backward --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_bn_bwd_reduce_against_fp64_of_the_device_forward(name):
    """``bn_bwd_reduce`` in modes 0, 1, 2, with and without dy2, both forms, given the device's ``saved`` (and y): sum g and
    sum g xhat with g = (dy + dy2) [y > 0] of the DEVICE's y -- a mode-2 gate that disagrees with it anywhere is a whole
    gradient element.  Worst-case bounds, and 3x the achieved error in sqrt(n) units."""
    c, dv, h = bn_ref.BY_NAME[name], _dev(name), inputs(name)
    fails = []
    for mode, relu, has_res in MODES:
        fwd = _forward(c, dv, relu, dv["res"] if has_res else None)
        gate = (_h(fwd.y, c) > 0) if relu else None
        mean, invstd = _h(fwd.saved)[:, 0], _h(fwd.saved)[:, 1]
        for dy2 in (None, "dy2"):
            d2 = None if dy2 is None else h["dy2"]
            ref = bn_ref.reduce64(h["dy"], d2, h["x"], gate, mean, invstd)
            bounds = bn_ref.bound_sums(h["dy"], d2, h["x"], gate, mean, invstd)
            units = bn_ref.sqrt_units_sums(h["dy"], d2, h["x"], gate, mean, invstd)
            for det in (False, True):
                tot = _h(_reduce(c, dv, det, mode, None if dy2 is None else dv["dy2"], fwd)[2]).double()
                form = "reduce_det" if det else "reduce"
                for k in (0, 1):
                    key = f"{form}/{('sg', 'sgx')[k]}"
                    tag = f"bn_bwd_reduce[{key}, mode={mode}, dy2={int(dy2 is not None)}]"
                    err = (tot[:, k] - ref[k]).abs()
                    _chk(fails, tag, err, bounds[k])
                    got = _in_units(err, units[k]) if not bool((err > bounds[k]).any()) else float("nan")
                    if got == got:
                        _record(f"{key}/{name}/mode{mode}_dy2{int(dy2 is not None)}", got)
                        _worst(key, got)
                        if not got <= _limit(key):
                            fails.append(f"{tag}: {got:.3g} u sqrt(n) units > {_limit(key):.3g}")
    assert not fails, fails


@pytest.mark.parametrize("name", NAMES)
def test_bn_bwd_dx_against_fp64_of_the_device_sums(name):
    """``bn_bwd_dx`` in modes 0, 1, 2, with and without dy2, both forms, given the device's ``saved`` and sums: dx on every
    element; dres bit-equal to torch's bf16(dy + dy2) under the device's gate; dweight / dbias bit-equal to the fp32 sum of
    the groups' sums in group order (atomic form), within G u sum|group sums| of the folded totals' float64 sum (deterministic
    form); without dres the same dx bits."""
    c, dv, h = bn_ref.BY_NAME[name], _dev(name), inputs(name)
    fails = []
    for mode, relu, has_res in MODES:
        fwd = _forward(c, dv, relu, dv["res"] if has_res else None)
        gate_d = (fwd.y > 0) if relu else None
        gate = _h(gate_d, c) if relu else None
        mean, invstd = _h(fwd.saved)[:, 0], _h(fwd.saved)[:, 1]
        for dy2 in (None, "dy2"):
            d2, d2d = (None, None) if dy2 is None else (h["dy2"], dv["dy2"])
            want_dres = bn_ref.dres64(dv["dy"], d2d, gate_d)
            for det in (False, True):
                tag = f"bn_bwd_dx[{'det' if det else 'atomic'}, mode={mode}, dy2={int(dy2 is not None)}]"
                sums, nb, tot = _reduce(c, dv, det, mode, d2d, fwd)
                o = _dx(c, dv, det, mode, d2d, fwd, sums, nb, dres=mode != 2)
                sg, sgx = _h(tot)[:, 0], _h(tot)[:, 1]
                args = (h["dy"], d2, h["x"], gate, mean, invstd, h["w"], sg, sgx)
                _chk(fails, f"{tag} dx", (_h(o.dx, c).double() - bn_ref.dx64(*args)).abs(), bn_ref.bound_dx(*args))
                if mode != 2:
                    if not torch.equal(o.dres, want_dres):
                        fails.append(f"{tag} dres: {int((o.dres != want_dres).sum())} elements differ from bf16(dy + dy2) [y > 0]")
                    q = _dx(c, dv, det, mode, d2d, fwd, sums, nb, dres=False)
                    if not torch.equal(q.dx, o.dx):
                        fails.append(f"{tag}: dx differs without dres")
                if det:
                    bound = bn_ref.bound_param_grads_det(_h(tot)[:, 1]), bn_ref.bound_param_grads_det(_h(tot)[:, 0])
                    _chk(fails, f"{tag} dweight", (_h(o.dw).double() - sgx.double().sum(0)).abs(), bound[0])
                    _chk(fails, f"{tag} dbias", (_h(o.db).double() - sg.double().sum(0)).abs(), bound[1])
                else:
                    acc = torch.zeros((2, c.C), device=DEV)
                    for g in range(c.groups):
                        acc = acc + tot[g]
                    if not (torch.equal(o.db, acc[0]) and torch.equal(o.dw, acc[1])):
                        fails.append(f"{tag}: dweight / dbias are not the fp32 sum of the groups' sums in group order")
    assert not fails, fails


# ---- the composition -------------------------------------------------------------------------------------------------
def _bf16_units(got, ref):
    """max |got - ref| / (2^-8 |ref| + 1e-5 max|ref of the channel|): test_gpu_train_encoder_ref's ``_elementwise`` with its
    floor of 1e-3 lowered to 1e-5 (what the statistics' own fp32 error needs) and taken per channel (the constant channel's
    invstd of 316 does not lend its magnitude to the others)."""
    tol = ULP * ref.abs() + 1e-5 * ref.abs().amax((0, 1))
    return float(((got.double() - ref).abs() / tol.clamp_min(1e-300)).max())


@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
@pytest.mark.parametrize("name", LAYER_CASES)
def test_bn_layer_against_fp64(name, det):
    """``_BNActFn`` against ``layer64`` (statistics from x in float64, the gate the device's y > 0): y, dx, dres, dweight, dbias
    and both running buffers for relu x residual x fork (none; both gradients; only the alias used)."""
    c, dv, h = bn_ref.BY_NAME[name], _dev(name), inputs(name)
    mom = f32(c.momentum)

    def nchw(t):                                              # the [R, C] buffer as the channels-last [B, C, H, W] it is
        return t.view(c.B, c.H, c.W, c.C).permute(0, 3, 1, 2)
    fails = []
    for relu in (False, True):
        for has_res in (False, True):
            for fork in ("none", "both", "alias"):
                xg = nchw(dv["x"]).clone(memory_format=torch.channels_last).requires_grad_(True)
                rg = nchw(dv["res"]).clone(memory_format=torch.channels_last).requires_grad_(True) if has_res else None
                wg, bg = dv["w"].clone().requires_grad_(True), dv["b"].clone().requires_grad_(True)
                rm, rv = dv["rm"].clone(), dv["rv"].clone()
                with te_mod._det_scope(det):
                    out = _BNActFn.apply(xg, wg, bg, rm, rv, c.momentum, EPS, relu, rg, c.groups, fork != "none")
                    if fork == "both":
                        torch.autograd.backward(list(out), [nchw(dv["dy"]), nchw(dv["dy2"])])
                    else:
                        (out[1] if fork == "alias" else out).backward(nchw(dv["dy"]))
                y = out[0] if fork != "none" else out
                assert fork == "none" or out[1].data_ptr() == y.data_ptr()

                def rows(t):
                    return _h(t.detach().permute(0, 2, 3, 1).reshape(-1, c.C), c)
                yh = rows(y)
                gate = (yh > 0) if relu else None
                ref = bn_ref.layer64(h["x"], h["res"] if has_res else None, h["w"], h["b"], h["rm"], h["rv"], mom, f32(EPS),
                                     relu, h["dy"], h["dy2"] if fork == "both" else None, gate)
                tag = f"relu={int(relu)} res={int(has_res)} fork={fork}"
                errs = {"y": _bf16_units(yh, ref["y"]), "dx": _bf16_units(rows(xg.grad), ref["dx"])}
                for k, got in (("dweight", wg.grad), ("dbias", bg.grad), ("running_mean", rm), ("running_var", rv)):
                    errs[k] = float((_h(got).double() - ref[k]).abs().max()) / max(float(ref[k].abs().max()), 1e-300)
                if has_res and not torch.equal(rows(rg.grad), ref["dres"]):
                    fails.append(f"{tag}: dres is not bf16(dy + dy2) under the device's gate")
                for k, v in errs.items():
                    _record(f"layer/{k}/{name}/{'det' if det else 'default'}/{tag.replace(' ', '_')}", v)
                    _worst(f"layer/{k}", v)
                    if not v <= _limit(f"layer/{k}"):
                        fails.append(f"{tag}: {k} {v:.3g} > {_limit(f'layer/{k}'):.3g}")
    assert not fails, fails


# ---- the deterministic entries, bit for bit -----------------------------------------------------------------------------
# more than one row group (c256_g1_n65: two); more than one channel tile (C = 512, 2048); groups > 1; 64 groups; the grid's
# cap / groups clamp binding (bn_ref.CLAMP_CASE)
DIGEST_CASES = ("c256_g1_n65", "c512_g3_n33", "c2048_g1_n65", "c32_g64_n9", bn_ref.CLAMP_CASE.name)


def _sha(t):
    import hashlib
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def bn_det_digests(name):
    """{launch / output: sha256 of its raw bytes} of every output of the deterministic chain on the case's seeded inputs:
    stats -> fold, apply (relu x residual, running statistics), reduce -> dx (modes 0, 1, 2 x dy2, with and without dres)."""
    c, dv = bn_ref.BY_NAME[name], _dev(name)
    st, nb, tot = _stats(c, dv, True)
    out = {"stats/slab": _sha(st), "fold/out": _sha(tot)}
    for relu in (False, True):
        for res in (None, dv["res"]):
            o = _apply(c, dv, True, st, nb, relu, res)
            for k in ("y", "saved", "rm", "rv"):
                out[f"apply/relu{int(relu)}_res{int(res is not None)}/{k}"] = _sha(getattr(o, k))
    for mode, relu, has_res in MODES:
        fwd = _apply(c, dv, True, st, nb, relu, dv["res"] if has_res else None, running=False)
        for dy2 in (None, dv["dy2"]):
            tag = f"mode{mode}_dy2{int(dy2 is not None)}"
            sums, snb, _ = _reduce(c, dv, True, mode, dy2, fwd)
            out[f"reduce/{tag}/slab"] = _sha(sums)
            for dres in (False, True) if mode != 2 else (False,):
                o = _dx(c, dv, True, mode, dy2, fwd, sums, snb, dres=dres)
                for k in ("dx", "dres", "dw", "db") if dres else ("dx", "dw", "db"):
                    out[f"dx/{tag}_dres{int(dres)}/{k}"] = _sha(getattr(o, k))
    return out


@pytest.mark.parametrize("name", DIGEST_CASES)
def test_bn_det_entries_keep_every_output_bit(name):
    """The ``_det`` kernels are bit-reproducible, so their outputs on fixed inputs are a golden for any change that claims to
    leave the device code alone: tests/golden/bn_det_digests.json, recorded with ``bn_det_digests`` on an MI355X from a
    build of commit bf10b8c (twice, with equal digests).  The atomic entries' last bits are order-free: the fp64 tests above
    hold them."""
    import json
    import os
    from conftest import ROOT
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "bn_det_digests.json")))[name]
    got = bn_det_digests(name)
    assert sorted(got) == sorted(want)
    assert not [k for k in got if got[k] != want[k]]


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_bn_entries_refuse_what_they_do_not_take():
    L = _lib.load()
    t = torch.zeros(1 << 16, device=DEV)
    p, s = t.data_ptr(), _s()
    big = t.numel() * 4

    def every(rows, C, groups, ws_bytes=big, only_det=False):
        calls = {
            "stats": lambda: L.dmm_bn_stats_grouped_bf16(p, rows, C, groups, p, s),
            "apply": lambda: L.dmm_bn_apply_grouped_bf16(p, None, rows, C, groups, p, p, p, None, None, 0.1, EPS, 1, p, p, s),
            "reduce": lambda: L.dmm_bn_bwd_reduce_grouped_bf16(p, None, p, p, rows, C, groups, p, p, p, 1, p, s),
            "dx": lambda: L.dmm_bn_bwd_dx_grouped_bf16(p, None, p, p, rows, C, groups, p, p, p, p, 1, p, None, p, p, s),
            "stats_det": lambda: L.dmm_bn_stats_det_grouped_bf16(p, rows, C, groups, p, ws_bytes, s),
            "apply_det": lambda: L.dmm_bn_apply_det_grouped_bf16(p, None, rows, C, groups, p, ws_bytes, p, p, None, None, 0.1,
                                                                 EPS, 1, p, p, s),
            "reduce_det": lambda: L.dmm_bn_bwd_reduce_det_grouped_bf16(p, None, p, p, rows, C, groups, p, p, p, 1, p, ws_bytes, s),
            "dx_det": lambda: L.dmm_bn_bwd_dx_det_grouped_bf16(p, None, p, p, rows, C, groups, p, p, p, p, ws_bytes, 1, p, None,
                                                               p, p, s),
            "fold_det": lambda: L.dmm_bn_fold_det(p, ws_bytes, rows, C, groups, p, s),
        }
        return {k: f() for k, f in calls.items() if k.endswith("_det") or not only_det}
    assert set(every(130, 32, 65).values()) == {_lib.DMM_ERR_BAD_ARG}             # groups = 65
    assert set(every(64, 32, 3).values()) == {_lib.DMM_ERR_BAD_ARG}               # rows not divisible by groups
    assert set(every(4, 24, 1).values()) == {_lib.DMM_ERR_UNSUPPORTED}            # 256 % (C / 8) != 0
    assert set(every(4, 4096, 1).values()) == {_lib.DMM_ERR_UNSUPPORTED}          # C / 8 > 256
    need = int(L.dmm_bn_det_workspace_bytes(66, 32, 3))
    assert need == 3 * 1 * 2 * 32 * 4
    short = every(66, 32, 3, need - 1, only_det=True)                            # the workspace one byte short
    assert short == dict.fromkeys(("stats_det", "apply_det", "reduce_det", "dx_det", "fold_det"), _lib.DMM_ERR_WORKSPACE)
    # a residual in front of the ReLU needs the output for its gate: mode 2 with dres stays refused
    c = bn_ref.BY_NAME["c32_g1_n7"]
    dv = _dev(c.name)
    fwd = _forward(c, dv, True, None)
    for det in (False, True):
        sums, nb, _ = _reduce(c, dv, det, 2, None, fwd)
        assert _dx(c, dv, det, 2, None, fwd, sums, nb, dres=True, allow=(_lib.DMM_ERR_BAD_ARG,)).rc == _lib.DMM_ERR_BAD_ARG
    torch.cuda.synchronize()
