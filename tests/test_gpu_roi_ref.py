"""``dmm_roialign.hip``'s six kernels against the float64 reference of tests/roi_ref.py: the four C entries driven directly, with
per-level sizes that are no pyramid, then ``roialign4_mean_into`` / ``_RoiAlign4Mean`` / ``FeatureExtractor`` on top of them.
``|got - ref| <= bound`` is asserted for EVERY element (the reference takes the kernel's own fp32 sample coordinates, so it is
never on the other side of a discontinuity and nothing is left out); every bound is derived (roi_ref.bound_*: the rounding
counts are beside the formulas) and none is measured.  The worst error / bound of every case is recorded
(profiles/roi_ref_achieved.jsonl holds an MI355X run): a ratio above 1 is a finding, not a reason to widen a bound."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dmm_net_amd
import roi_ref
from roi_ref import BY_NAME, CASES, inputs
from dmm_net_amd import _lib
from dmm_net_amd.roi_features import FeatureExtractor, _RoiAlign4Mean, _layout, roialign4_mean_into

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TORCH = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
ABI = {"fp32": _lib.DTYPE_F32, "fp16": _lib.DTYPE_F16, "bf16": _lib.DTYPE_BF16}
FWD_NAMES = [c.name for c in CASES]
NHWC_NAMES = [c.name for c in CASES if c.kind == "nhwc"]
BWD_NAMES = [c.name for c in CASES if c.kind == "bwd"]
GRAD_NAMES = ["nchw_c5_fp16_b3", "nchw_c5_bf16_b3", "nchw_c17_bf16_b3", "nchw_c3_fp16_b1"]


def _record(name, v):
    from conftest import record_achieved
    record_achieved("roi_ref/" + name, v)


def _s():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _ref_fwd(name):
    d = inputs(name)
    return roi_ref.fwd64(d["feats"], d["rois"], want_mag=True)


@functools.lru_cache(maxsize=None)
def _ref_bwd(name):
    c, d = BY_NAME[name], inputs(name)
    return roi_ref.bwd64(d["dout"], d["rois"], c.B, c.C, list(c.H), list(c.W))


@functools.lru_cache(maxsize=None)
def _dev(name):
    """The case's inputs on the device, never modified: the levels NCHW-contiguous in the case's type, the same values as
    channels-last tensors, rois and dout."""
    c, d = BY_NAME[name], inputs(name)
    feats = [torch.tensor(f).to(DEV).to(TORCH[c.dtype]).contiguous() for f in d["feats"]]
    for f, h in zip(feats, d["feats"]):
        assert np.array_equal(f.float().cpu().numpy(), h)     # the values are exact in the case's type
    cl = [f.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for f in feats]      # memory [B, H, W, C] whatever the sizes
    return {"feats": feats, "cl": cl, "rois": torch.tensor(d["rois"]).to(DEV).contiguous(),
            "dout": torch.tensor(d["dout"]).to(DEV).contiguous()}


def _arrays(c):
    return ((ctypes.c_int * 4)(*c.H), (ctypes.c_int * 4)(*c.W), (ctypes.c_float * 4)(*roi_ref.SCALES))


def _ptrs(ts):
    return (ctypes.c_void_p * 4)(*[t.data_ptr() for t in ts])


def _forward(entry, c, feats, rois, allow=()):
    """One forward entry -> (status, out); ``out`` starts as NaN: the launch writes every element it owns."""
    Hs, Ws, sc = _arrays(c)
    out = torch.full((rois.shape[0], 4 * c.C), float("nan"), device=DEV)
    rc = _lib.call(entry, DEV, _ptrs(feats), ABI[c.dtype], c.B, c.C, Hs, Ws, sc, rois.data_ptr(), rois.shape[0], out.data_ptr(),
                   _s(), allow=allow)
    return rc, out


def _backward(c, dv, det, init=None):
    """One backward entry into ``init`` (default: zeros) -> the four dfeat tensors."""
    Hs, Ws, sc = _arrays(c)
    R = dv["rois"].shape[0]
    dfs = [torch.zeros((c.B, c.C, c.H[l], c.W[l]), device=DEV) if init is None else init[l].clone() for l in range(4)]
    if det:
        nb = int(_lib.load().dmm_roialign4_mean_bwd_det_workspace_bytes(R, Hs, Ws))
        assert nb == R * 4 * ((max(c.H) + max(c.W)) * 4 + 16)
        ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=DEV)                   # the launch writes all it reads
        _lib.call("dmm_roialign4_mean_bwd_det", DEV, dv["dout"].data_ptr(), c.B, c.C, Hs, Ws, sc, dv["rois"].data_ptr(), R,
                  _ptrs(dfs), ws.data_ptr(), nb, _s())
    else:
        _lib.call("dmm_roialign4_mean_bwd", DEV, dv["dout"].data_ptr(), c.B, c.C, Hs, Ws, sc, dv["rois"].data_ptr(), R,
                  _ptrs(dfs), _s())
    return dfs


def _ratio(fails, what, got, ref, bound):
    """|got - ref| <= bound on EVERY element (a NaN fails); -> the worst error / bound (0 / 0 = 0)."""
    err = np.abs(got.detach().double().cpu().numpy() - ref)
    bad = ~(err <= bound)
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    if bool(bad.any()):
        fails.append(f"{what}: {int(bad.sum())} of {bad.size} elements over their bound, |err| up to {float(np.nanmax(err)):.3g}, "
                     f"{ratio:.3g} x the bound")
    return ratio


# ---- forward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FWD_NAMES)
def test_nchw_forward_against_fp64(name):
    """``dmm_roialign4_mean_fwd`` in every case of the list (the channels-last and backward cases are NCHW inputs too): C of 1, 2,
    3 (the register group clamps to channel C - 1), 5 and 17 (a pass holding one channel), three types, B of 1 and 3, a patch
    exactly 1024 cells wide (one row per tile, the tile's tables full), 40 rows in tiles of 25 + 15 (both asserted from the
    geometry), every roi kind, dead rois and a frame index equal to B."""
    c, dv = BY_NAME[name], _dev(name)
    out64, mag, geo = _ref_fwd(name)
    patches = [(g.ay.hi - g.ay.lo + 1, g.ax.hi - g.ax.lo + 1) for per in geo for g in per if g.live]
    if name == "nchw_wide":
        assert any(pw == 1024 and ph > 1 and roi_ref._tiles(ph, pw) == (1, ph) for ph, pw in patches), sorted(set(patches))[-3:]
    if name == "nchw_tiles":
        assert any(ph * pw > 1024 and roi_ref._tiles(ph, pw)[1] > 1 and ph % roi_ref._tiles(ph, pw)[0] != 0 for ph, pw in patches)
        assert (40, 40) in patches and roi_ref._tiles(40, 40) == (25, 2)
    fails = []
    rc, out = _forward("dmm_roialign4_mean_fwd", c, dv["feats"], dv["rois"])
    r = _ratio(fails, "nchw forward", out, out64, roi_ref.bound_fwd(mag, geo, c.C, "nchw"))
    _record(f"fwd_nchw/{name}", r)
    dead = [i for i, per in enumerate(geo) if not any(g.live for g in per)]
    assert len(dead) >= 3 and float(out[dead].abs().max()) == 0.0
    assert not fails, fails


@pytest.mark.parametrize("name", NHWC_NAMES)
def test_nhwc_forward_against_fp64(name):
    """``dmm_roialign4_mean_nhwc_fwd``: per type 1, 4 and 64 lanes per cell (the fold does nothing at 64), 128 and 192 (two and
    three passes); patches of one cell (the 1 x 1 level), of fewer cells than one workgroup step and of more than four steps;
    held to the float64 reference itself, and ``roialign4_mean_into`` takes this entry for channels-last tensors."""
    c, dv = BY_NAME[name], _dev(name)
    out64, mag, geo = _ref_fwd(name)
    vec = roi_ref.vec_of(c.dtype)
    step = 8 * (64 // (min(c.C, 64 * vec) // vec))
    cells = [(g.ay.hi - g.ay.lo + 1) * (g.ax.hi - g.ax.lo + 1) for per in geo for g in per if g.live]
    assert min(cells) == 1 and any(1 < n < step for n in cells) and max(cells) > 4 * step, (step, sorted(set(cells)))
    fails = []
    rc, out = _forward("dmm_roialign4_mean_nhwc_fwd", c, dv["cl"], dv["rois"])
    r = _ratio(fails, "nhwc forward", out, out64, roi_ref.bound_fwd(mag, geo, c.C, "nhwc", vec))
    _record(f"fwd_nhwc/{name}", r)
    assert _layout(dv["cl"]) == "nhwc"
    into = roialign4_mean_into(dv["rois"], dv["cl"], torch.full_like(out, float("nan")))
    assert torch.equal(into, out)
    assert not fails, fails


def test_nhwc_refusals_take_the_nchw_route():
    """C = 12 in fp32 (3 lanes per cell: no power of two) and a base pointer off by 4 bytes are DMM_ERR_UNSUPPORTED at the
    channels-last entry.  ``_RoiAlign4Mean`` copies such channels-last tensors and gives the reference's values through the NCHW
    kernel, in bound.  ``roialign4_mean_into`` is the route that allocates nothing, so it cannot copy: handed the refused
    channels-last tensors themselves it stops at its own assertion BEFORE any launch (pinned here -- it must never read
    [B, H, W, C] memory as NCHW); handed the same values NCHW-contiguous (a misaligned base included) it takes the NCHW kernel."""
    fails = []
    # (a) C = 12
    c = roi_ref.Case("c12", "nchw", "fp32", 2, 12, roi_ref.SMALL_H, roi_ref.SMALL_W, None)
    gen = np.random.default_rng(12)
    feats = [gen.standard_normal((c.B, c.C, c.H[l], c.W[l])).astype(np.float32) for l in range(4)]
    rois = inputs("nhwc_fp32_lpc64")["rois"]                   # (the same level sizes and B)
    assert BY_NAME["nhwc_fp32_lpc64"].H == c.H and BY_NAME["nhwc_fp32_lpc64"].B == c.B
    out64, mag, geo = roi_ref.fwd64(feats, rois, want_mag=True)
    bound = roi_ref.bound_fwd(mag, geo, c.C, "nchw")
    fd = [torch.from_numpy(f).to(DEV) for f in feats]
    cl = [f.contiguous(memory_format=torch.channels_last) for f in fd]
    rd = torch.tensor(rois).to(DEV)
    rc, _ = _forward("dmm_roialign4_mean_nhwc_fwd", c, cl, rd, allow=(_lib.DMM_ERR_UNSUPPORTED,))
    assert rc == _lib.DMM_ERR_UNSUPPORTED and _layout(cl) == "nchw"
    with pytest.raises(AssertionError):
        roialign4_mean_into(rd, cl, torch.empty((len(rois), 48), device=DEV))
    _record("fwd_nchw/c12_into", _ratio(fails, "C = 12 into", roialign4_mean_into(rd, fd, torch.empty((len(rois), 48), device=DEV)),
                                        out64, bound))
    _record("fwd_nchw/c12_apply", _ratio(fails, "C = 12 apply", _RoiAlign4Mean.apply(rd, *cl), out64, bound))
    # (b) the same values of a committed case, every level 4 bytes off a 16-byte boundary
    name = "nhwc_fp32_lpc4"
    c, dv = BY_NAME[name], _dev(name)
    out64, mag, geo = _ref_fwd(name)
    bound = roi_ref.bound_fwd(mag, geo, c.C, "nchw")

    def shifted(t, nhwc):
        buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=DEV)
        assert buf.data_ptr() % 16 == 0
        v = buf[1:1 + t.numel()]
        if nhwc:
            v = v.view(t.shape[0], t.shape[2], t.shape[3], t.shape[1]).permute(0, 3, 1, 2)
        else:
            v = v.view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v
    off_cl = [shifted(t, True) for t in dv["cl"]]
    rc, _ = _forward("dmm_roialign4_mean_nhwc_fwd", c, off_cl, dv["rois"], allow=(_lib.DMM_ERR_UNSUPPORTED,))
    assert rc == _lib.DMM_ERR_UNSUPPORTED and _layout(off_cl) == "nchw"
    _record("fwd_nchw/misaligned_apply", _ratio(fails, "misaligned apply", _RoiAlign4Mean.apply(dv["rois"], *off_cl), out64, bound))
    with pytest.raises(AssertionError):
        roialign4_mean_into(dv["rois"], off_cl, torch.empty((dv["rois"].shape[0], 4 * c.C), device=DEV))
    off = [shifted(t, False) for t in dv["feats"]]
    got = roialign4_mean_into(dv["rois"], off, torch.empty((dv["rois"].shape[0], 4 * c.C), device=DEV))
    _record("fwd_nchw/misaligned_into", _ratio(fails, "misaligned into", got, out64, bound))
    assert torch.equal(got, _forward("dmm_roialign4_mean_fwd", c, dv["feats"], dv["rois"])[1])
    assert not fails, fails


# ---- backward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("name", BWD_NAMES)
def test_backward_against_fp64(name, det):
    """``dmm_roialign4_mean_bwd`` and ``_bwd_det`` on the same cases: C of 1, 3, 5, 64; 130 identical rois of one frame (the
    gather's chunks of 64, 64 and 2) with dead rois and rois of the other frames between them, a frame index equal to B, levels
    smaller than the largest (idle gather rows).  include/dmm_match.h: both ACCUMULATE into dfeat, which the caller zeroes --
    so zeroed buffers give the adjoint, and buffers that arrive with values keep them: the gradient is added, and a cell no
    roi covers keeps its bits.  The deterministic entry is bit-equal over two calls."""
    c, dv = BY_NAME[name], _dev(name)
    grads, mags, cover, kw = _ref_bwd(name)
    R = dv["rois"].shape[0]
    assert max(int(cv.max()) for cv in cover) > 128

    def bounds(mg):
        return roi_ref.bound_bwd_gather(mg, cover, kw, R) if det else roi_ref.bound_bwd_atomic(mg, cover, kw)
    fails = []
    got = _backward(c, dv, det)
    b0 = bounds(mags)
    worst = max(_ratio(fails, f"dfeat{l}", got[l], grads[l], b0[l]) for l in range(4))
    _record(f"bwd_{'det' if det else 'atomic'}/{name}", worst)
    if det:
        again = _backward(c, dv, True)
        assert all(torch.equal(a, b) for a, b in zip(got, again)), "the deterministic backward differs between two calls"
    gen = torch.Generator().manual_seed(c.C)
    init = [torch.randn(g.shape, generator=gen).to(DEV) for g in grads]
    got = _backward(c, dv, det, init)
    hinit = [t.double().cpu().numpy() for t in init]
    b1 = bounds([mags[l] + np.abs(hinit[l]) for l in range(4)])
    worst = max(_ratio(fails, f"dfeat{l} (accumulated)", got[l], grads[l] + hinit[l], b1[l]) for l in range(4))
    _record(f"bwd_{'det' if det else 'atomic'}_accumulate/{name}", worst)
    for l in range(4):
        idle = torch.from_numpy(cover[l] == 0).to(DEV)[:, None].expand_as(init[l])
        assert bool(idle.any()) or l >= 2
        assert torch.equal(got[l][idle], init[l][idle]), f"level {l}: a cell no roi covers changed"
    assert not fails, fails


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("name", GRAD_NAMES)
def test_autograd_with_half_features(name, det):
    """``_RoiAlign4Mean`` with fp16 / bf16 features that require a gradient: the forward inside the NCHW bound, the gradients
    inside the backward's bound plus ONE rounding to the feature's type, and they arrive in that type."""
    c, dv = BY_NAME[name], _dev(name)
    out64, mag, geo = _ref_fwd(name)
    grads, mags, cover, kw = _ref_bwd(name)
    R = dv["rois"].shape[0]
    feats = [f.clone().requires_grad_(True) for f in dv["feats"]]
    with dmm_net_amd.deterministic(det):
        out = _RoiAlign4Mean.apply(dv["rois"], *feats)
        got = torch.autograd.grad(out, feats, dv["dout"])
    fails = []
    _ratio(fails, "forward", out, out64, roi_ref.bound_fwd(mag, geo, c.C, "nchw"))
    bnd = roi_ref.bound_bwd_gather(mags, cover, kw, R) if det else roi_ref.bound_bwd_atomic(mags, cover, kw)
    worst = 0.0
    for l in range(4):
        assert got[l].dtype == TORCH[c.dtype] and got[l].shape == feats[l].shape
        worst = max(worst, _ratio(fails, f"dfeat{l}", got[l], grads[l], roi_ref.bound_cast(bnd[l], grads[l], c.dtype)))
    _record(f"autograd_{'det' if det else 'atomic'}/{name}", worst)
    assert not fails, fails


# ---- the module's routes ---------------------------------------------------------------------------------------------------
class _Boxes:
    def __init__(self, bbox):
        self.bbox = bbox

    def __len__(self):
        return self.bbox.shape[0]


@pytest.mark.parametrize("name", ["nhwc_bf16_lpc4", "nhwc_fp32_lpc64", "nhwc_fp16_lpc128"])
def test_module_routes_are_the_entries_bit_for_bit(name):
    """Channels-last levels without a gradient: ``_RoiAlign4Mean`` and ``FeatureExtractor`` give the channels-last entry's bits;
    with a gradient they are copied and give the NCHW entry's bits."""
    c, dv = BY_NAME[name], _dev(name)
    nhwc = _forward("dmm_roialign4_mean_nhwc_fwd", c, dv["cl"], dv["rois"])[1]
    nchw = _forward("dmm_roialign4_mean_fwd", c, dv["feats"], dv["rois"])[1]
    assert torch.equal(_RoiAlign4Mean.apply(dv["rois"], *dv["cl"]), nhwc)
    with_grad = [t.detach().clone(memory_format=torch.preserve_format).requires_grad_(True) for t in dv["cl"]]
    assert _layout(with_grad) == "nhwc"
    assert torch.equal(_RoiAlign4Mean.apply(dv["rois"], *with_grad).detach(), nchw)
    # the module takes per-frame box lists: the live rois in frame order
    frame = dv["rois"][:, 0]
    rows = torch.cat([torch.nonzero(frame == b).flatten() for b in range(c.B)])
    boxes = [_Boxes(dv["rois"][frame == b][:, 1:].contiguous()) for b in range(c.B)]
    assert torch.equal(FeatureExtractor()(tuple(dv["cl"]), boxes), nhwc[rows])
    assert torch.equal(FeatureExtractor()(tuple(with_grad), boxes).detach(), nchw[rows])


def test_channels_last_levels_down_to_one_cell_through_the_captured_route():
    """``roialign4_mean_into`` -- what a captured frame step calls, with no copy in front -- on channels-last levels of 8 x 8,
    4 x 4, 2 x 2 and 1 x 1 (a frame of at most 32 x 32 pixels).  The 1 x 1 level is plainly contiguous as well (the same
    memory in both layouts); that must not send the other three levels down the NCHW route."""
    c = roi_ref.Case("tiny", "nhwc", "bf16", 2, 16, (8, 4, 2, 1), (8, 4, 2, 1), None)
    gen = np.random.default_rng(32)
    feats = [roi_ref.round_to(gen.standard_normal((c.B, c.C, c.H[l], c.W[l])), "bf16") for l in range(4)]
    rois = np.asarray([(j % c.B,) + bx for j, bx in enumerate(roi_ref.boxes_of(8, 8, gen))] + [(-1.0, 0.0, 0.0, 32.0, 32.0)],
                      dtype=np.float32)
    out64, mag, geo = roi_ref.fwd64(feats, rois, want_mag=True)
    cl = [torch.from_numpy(f).to(DEV).to(torch.bfloat16).contiguous(memory_format=torch.channels_last) for f in feats]
    assert cl[3].is_contiguous() and not cl[2].is_contiguous()
    rd = torch.from_numpy(rois).to(DEV)
    got = roialign4_mean_into(rd, cl, torch.full((len(rois), 4 * c.C), float("nan"), device=DEV))
    fails = []
    r = _ratio(fails, "1 x 1 level", got, out64, roi_ref.bound_fwd(mag, geo, c.C, "nhwc", 8))
    _record("fwd_nhwc/tiny_1x1_into", r)
    assert not fails, fails
    assert _layout(cl) == "nhwc"
    assert torch.equal(got, _forward("dmm_roialign4_mean_nhwc_fwd", c, cl, rd)[1])
    assert torch.equal(_RoiAlign4Mean.apply(rd, *cl), got)
