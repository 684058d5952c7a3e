"""Guards of the ROI kernels' float64 reference (tests/roi_ref.py) -- no GPU.

The reference is what ``tests/test_gpu_roi_ref.py`` holds the kernels to, so it is itself held here: to a second, non-separable
float64 formulation; to the G12 fixture and the oracle; to the census that makes the cases worth running (every class of
sample, the two discontinuities at exactly -1 and exactly ``size`` among them); its derived bounds to an fp32 emulation of the
kernels' arithmetic, operation by operation; and every mutant to the bound it has to exceed."""
import functools

import numpy as np
import pytest

import roi_ref
from roi_ref import CASES, BY_NAME, F, SCALES, U, gamma, inputs

NAMES = [c.name for c in CASES]
NORM32 = F(1.0) / F(784.0)


def _shape(c):
    return c.B, c.C, list(c.H), list(c.W)


@functools.lru_cache(maxsize=None)
def _fwd(name):
    d = inputs(name)
    return roi_ref.fwd64(d["feats"], d["rois"], want_mag=True)


@functools.lru_cache(maxsize=None)
def _bwd(name):
    c, d = BY_NAME[name], inputs(name)
    return roi_ref.bwd64(d["dout"], d["rois"], *_shape(c))


# ---- the reference against other formulations -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_separable_reference_equals_the_sample_formulation(name):
    """wy' F wx / 784 == the 784 samples with 4 corners each, bin means then the mean of the bins: 1e-12 of sum |terms|, on
    every element (dead rois, frames >= B and outside boxes are exact zeros in both)."""
    d = inputs(name)
    out, mag, _ = _fwd(name)
    alt = roi_ref.fwd64_samples(d["feats"], d["rois"])
    assert bool((np.abs(out - alt) <= 1e-12 * mag).all()), float(np.abs(out - alt).max())
    assert float(np.abs(out).max()) > 1e-3


def test_backward_reference_is_the_adjoint_of_the_forward():
    """<dout, A f> == <A' dout, f> in float64, to 1e-12 of the sum of the magnitudes."""
    for name in ("bwd_c3", "bwd_c64", "nchw_c5_fp32_b3"):
        c, d = BY_NAME[name], inputs(name)
        out, mag, _ = _fwd(name)
        grads = _bwd(name)[0]
        lhs = float((out * d["dout"]).sum())
        rhs = float(sum((g * f.astype(np.float64)).sum() for g, f in zip(grads, d["feats"])))
        assert abs(lhs - rhs) <= 1e-12 * float((mag * np.abs(d["dout"])).sum()), (name, lhs, rhs)


def test_reference_reproduces_g12():
    """G12 (an independent differentiable formulation): ``out`` and ``grad*`` within the fixture's existing 1e-5."""
    from conftest import golden
    g = golden("g12_roialign")
    for k in range(int(g["n"])):
        c = g.group(f"c{k}")
        feats = [c[f"feat{l}"] for l in range(4)]
        B, C = feats[0].shape[:2]
        out = roi_ref.fwd64(feats, c["rois"])
        assert float(np.abs(out - c["out"]).max()) <= 1e-5 * max(1.0, float(np.abs(c["out"]).max())), k
        grads = roi_ref.bwd64(c["wgt"], c["rois"], B, C, [f.shape[2] for f in feats], [f.shape[3] for f in feats])[0]
        for l in range(4):
            ge = c[f"grad{l}"]
            assert float(np.abs(grads[l] - ge).max()) <= 1e-5 * max(1.0, float(np.abs(ge).max())), (k, l)


@pytest.mark.parametrize("name", [c.name for c in CASES if c.kind == "nchw" and c.dtype == "fp32"])
def test_reference_reproduces_the_oracle_off_the_boundaries(name):
    """``oracle.roialign4_mean`` (fp32 per sample) on the live rois without a sample exactly at -1 or ``size``.  Its terms:
    hy, hx (2), hy hx (1), the product with the value (1), the sum of the 4 corners (3), of the 4 samples (3), the fp32 result
    (1); the bin means are exact or float64: gamma(11) x sum |terms|."""
    import oracle
    c, d = BY_NAME[name], inputs(name)
    keep = []
    for r, roi in enumerate(d["rois"]):
        cen = roi_ref.census(roi[None], c.H, c.W)
        on_edge = sum(cen[a][k] for a in "yx" for k in ("at_m1", "at_size"))
        if 0 <= int(roi[0]) < c.B and not on_edge:
            keep.append(r)
    assert len(keep) >= 8
    got = oracle.roialign4_mean([np.ascontiguousarray(f) for f in d["feats"]], np.ascontiguousarray(d["rois"][keep]))
    out, mag, _ = _fwd(name)
    assert bool((np.abs(got - out[keep]) <= gamma(11) * mag[keep]).all())


# ---- the census ---------------------------------------------------------------------------------------------------------
def test_census_every_class_is_populated():
    """Over the case list every class of sample occurs on each axis -- outside, clamped at 0, clamped at the top, interior,
    exactly -1 and exactly ``size`` -- and the exact ones in EVERY case: the comparisons of ``axis_weights`` are exercised
    wherever a kernel runs."""
    tot = {a: dict.fromkeys(roi_ref.CLASSES, 0) for a in "yx"}
    for c in CASES:
        cen = roi_ref.census(inputs(c.name)["rois"], c.H, c.W)
        for a in "yx":
            assert cen[a]["at_m1"] >= 1 and cen[a]["at_size"] >= 1, (c.name, a, cen[a])
            for k in roi_ref.CLASSES:
                tot[a][k] += cen[a][k]
    for a in "yx":
        assert all(v > 0 for v in tot[a].values()), tot
    # the issue's two examples, as the kernel's own coordinates
    ys = roi_ref.coords32(-5.0, 51.0, SCALES[0])
    assert list(ys[:3]) == [-1.0, -0.5, 0.0]
    assert 16.0 in list(roi_ref.coords32(11.0, 67.0, SCALES[0]))
    ax = roi_ref.axis64(11.0, 67.0, SCALES[0], 16)
    assert ax.census["at_size"] == 1 and ax.census["outside"] == 1 and ax.hi == 15


def test_the_tile_cases_hold_the_patches_they_are_named_for():
    """``nchw_wide`` holds a live patch exactly 1024 cells wide on several rows (one row per tile, the tile's tables filled to
    their last entry); ``nchw_tiles`` a 40 x 40 patch in tiles of 25 + 15 rows."""
    def patches(name):
        c = BY_NAME[name]
        geo = roi_ref.geometry(inputs(name)["rois"], c.H, c.W, c.B)
        return [(g.ay.hi - g.ay.lo + 1, g.ax.hi - g.ax.lo + 1) for per in geo for g in per if g.live]
    assert any(pw == 1024 and ph == 3 and roi_ref._tiles(ph, pw) == (1, 3) for ph, pw in patches("nchw_wide"))
    assert (40, 40) in patches("nchw_tiles") and roi_ref._tiles(40, 40) == (25, 2)


def test_fp32_coordinates_lie_within_their_roundings_of_float64():
    """``coords32`` against the same expression in float64: six roundings (end - start, / 14, p bin, the first sum, (i + 0.5)
    bin, the last sum), each relative to a value of at most |start| + len -- and the dyadic boxes are exact."""
    worst = 0.0
    for c in CASES:
        for roi in inputs(c.name)["rois"]:
            for s in SCALES:
                for a, b in ((roi[1], roi[3]), (roi[2], roi[4])):
                    y32 = roi_ref.coords32(float(a), float(b), s).astype(np.float64)
                    y64, size = roi_ref.coords64(float(a), float(b), s)
                    err = float(np.abs(y32 - y64).max())
                    assert err <= float(gamma(roi_ref.COORD_ROUNDINGS)) * size, (c.name, roi, s)
                    worst = max(worst, err / (U * size))
    assert worst > 0.0                                        # (the emulation is not float64 in disguise)
    assert np.array_equal(roi_ref.coords32(-5.0, 51.0, 0.25).astype(np.float64), roi_ref.coords64(-5.0, 51.0, 0.25)[0])


# ---- an fp32 emulation of the kernels ------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """fl32(a b + c) of fp32 arrays: the product of two fp32 values is exact in float64."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _axis32(a, b, scale, size):
    """``axis_weights`` in fp32, sample by sample in the source's order -> (w, lo, hi)."""
    w = np.zeros(size, dtype=np.float32)
    lo, hi = size, -1
    for y in roi_ref.coords32(a, b, scale):
        if y < F(-1.0) or y > F(size):
            continue
        if y <= F(0.0):
            y = F(0.0)
        yl = int(y)
        if yl >= size - 1:
            yh = yl = size - 1
            y = F(yl)
        else:
            yh = yl + 1
        ly = F(y - F(yl))
        hy = F(F(1.0) - ly)
        w[yl] = F(w[yl] + hy)
        w[yh] = F(w[yh] + ly)
        lo, hi = min(lo, yl), max(hi, yh)
    return w, lo, hi


def _axes32(roi, l, g, c):
    wy, h0, h1 = _axis32(float(roi[2]), float(roi[4]), SCALES[l], c.H[l])
    wx, w0, w1 = _axis32(float(roi[1]), float(roi[3]), SCALES[l], c.W[l])
    assert (h0, h1, w0, w1) == (g.ay.lo, g.ay.hi, g.ax.lo, g.ax.hi)      # the reference decided nothing else
    return wy, wx, h0, h1, w0, w1


def _tree(acc):
    """Pairwise fold of the last axis (a power of two) in fp32."""
    while acc.shape[-1] > 1:
        n = acc.shape[-1] // 2
        acc = acc[..., :n] + acc[..., n:]
    return acc[..., 0]


def _chain(wg, v, lanes):
    """Lane-strided fma chains: lane j takes elements j, j + lanes, ... of wg [n] and v [C, n] -> acc [C, lanes]."""
    n = wg.shape[0]
    steps = -(-n // lanes)
    wp = np.zeros(steps * lanes, dtype=np.float32)
    vp = np.zeros((v.shape[0], steps * lanes), dtype=np.float32)
    wp[:n], vp[:, :n] = wg, v
    wp, vp = wp.reshape(steps, lanes), vp.reshape(-1, steps, lanes)
    acc = np.zeros((v.shape[0], lanes), dtype=np.float32)
    for s in range(steps):
        acc = _fma32(wp[s], vp[:, s], acc)
    return acc


def _emulate_fwd(name, form):
    c, d = BY_NAME[name], inputs(name)
    _, _, geo = _fwd(name)
    out = np.zeros((len(geo), 4 * c.C), dtype=np.float32)
    vec = roi_ref.vec_of(c.dtype)
    for r, per in enumerate(geo):
        for l, g in enumerate(per):
            if not g.live:
                continue
            wy, wx, h0, h1, w0, w1 = _axes32(d["rois"][r], l, g, c)
            ph, pw = h1 - h0 + 1, w1 - w0 + 1
            f = d["feats"][l][g.b]
            if form == "nchw":
                rpt, nt = roi_ref._tiles(ph, pw)
                res = None
                for t in range(nt):
                    hb = h0 + t * rpt
                    rows = min(rpt, h1 - hb + 1)
                    wg = (wy[hb:hb + rows, None] * wx[None, w0:w1 + 1]).ravel()
                    acc = _chain(wg, f[:, hb:hb + rows, w0:w1 + 1].reshape(c.C, -1), 64)
                    val = _tree(acc) * NORM32
                    res = val if res is None else res + val
            else:
                cpw = 64 // (min(c.C, 64 * vec) // vec)
                wg = (wy[h0:h1 + 1, None] * wx[None, w0:w1 + 1]).ravel()
                acc = _chain(wg, f[:, h0:h1 + 1, w0:w1 + 1].reshape(c.C, -1), 8 * cpw).reshape(c.C, 8, cpw)
                red = _tree(acc)                               # the shuffle folds of a wave: log2(CPW) levels
                t = red[:, 0]
                for w in range(1, 8):
                    t = t + red[:, w]
                res = t * NORM32
            assert res.dtype == np.float32
            out[r, l * c.C:(l + 1) * c.C] = res
    return out


def _emulate_gather(name):
    c, d = BY_NAME[name], inputs(name)
    geo = roi_ref.geometry(d["rois"], c.H, c.W, c.B)
    R = len(geo)
    grads = []
    for l in range(4):
        df = np.zeros((c.B, c.C, c.H[l], c.W[l]), dtype=np.float32)
        for base in range(0, R, 64):
            acc = np.zeros_like(df)
            for r in range(base, min(base + 64, R)):
                g = geo[r][l]
                if not g.live:
                    continue
                wy, wx, h0, h1, w0, w1 = _axes32(d["rois"][r], l, g, c)
                gn = d["dout"][r, l * c.C:(l + 1) * c.C] * NORM32
                gx = gn[:, None] * wx[None, :]
                new = _fma32(gx[:, None, :], wy[None, :, None], acc[g.b])
                acc[g.b][:, h0:h1 + 1, w0:w1 + 1] = new[:, h0:h1 + 1, w0:w1 + 1]
            df = df + acc
        assert df.dtype == np.float32
        grads.append(df)
    return grads


@pytest.mark.parametrize("name", NAMES)
def test_bounds_hold_for_an_fp32_emulation_of_the_forward(name):
    """The forward kernels' arithmetic redone in numpy fp32 with the same operation counts and a lane-strided order (an fma
    through float64): every element within the bound the GPU test asserts -- the NCHW form in every case, the channels-last
    form where the case's C is inside its envelope."""
    c = BY_NAME[name]
    out, mag, geo = _fwd(name)
    forms = ["nchw"] + (["nhwc"] if c.kind == "nhwc" else [])
    for form in forms:
        got = _emulate_fwd(name, form)
        bound = roi_ref.bound_fwd(mag, geo, c.C, form, roi_ref.vec_of(c.dtype))
        err = np.abs(got.astype(np.float64) - out)
        assert bool((err <= bound).all()), (form, float((err / np.maximum(bound, 1e-300)).max()))
        assert float(err.max()) > 0.0


@pytest.mark.parametrize("name", [c.name for c in CASES if c.kind == "bwd"])
def test_bounds_hold_for_an_fp32_emulation_of_the_gather(name):
    c, d = BY_NAME[name], inputs(name)
    grads, mags, cover, kw = _bwd(name)
    got = _emulate_gather(name)
    bounds = roi_ref.bound_bwd_gather(mags, cover, kw, len(d["rois"]))
    assert max(int(cv.max()) for cv in cover) > 128           # three chunks add to one cell
    for l in range(4):
        err = np.abs(got[l].astype(np.float64) - grads[l])
        assert bool((err <= bounds[l]).all()), (l, float((err / np.maximum(bounds[l], 1e-300)).max()))
        assert float(err.max()) > 0.0


# ---- the mutants ---------------------------------------------------------------------------------------------------------
# mutant: the cases in which it has to exceed the bound (forward: the NCHW bound; backward: the gather's)
MUTANT_CASES = {
    1: ["nchw_c1_fp32_b1", "nchw_c17_bf16_b3", "nhwc_fp16_lpc4", "bwd_c3"],
    2: ["nchw_c1_fp32_b1", "nchw_c17_bf16_b3", "nhwc_fp16_lpc4", "bwd_c3"],
    3: ["nchw_c2_fp16_b1", "nhwc_bf16_lpc1", "bwd_c1"],
    4: ["nchw_c3_fp32_b3", "nhwc_fp32_lpc64", "bwd_c5"],
    5: ["nchw_c4_bf16_b1", "nhwc_fp32_lpc128", "bwd_c64"],
    6: ["nchw_c5_fp16_b3", "nhwc_bf16_lpc192", "bwd_c3"],
    7: ["nchw_c16_fp32_b1", "nchw_wide", "nhwc_fp16_lpc1"],
    8: ["nchw_c17_fp32_b3", "nhwc_fp32_lpc4", "bwd_c5"],
    9: ["nchw_c1_bf16_b3", "nhwc_bf16_lpc64"],
    10: ["nchw_wide", "nchw_tiles"],
    11: ["nchw_c1_fp32_b1", "nchw_c2_fp16_b3", "nchw_c3_bf16_b1", "nchw_c5_fp32_b3", "nchw_c17_fp16_b1"],
    12: ["bwd_c1", "bwd_c64"],
    13: ["bwd_c1", "bwd_c3", "bwd_c5", "bwd_c64"],
}
assert set(MUTANT_CASES) == set(roi_ref.MUTANTS)


@pytest.mark.parametrize("mut", sorted(roi_ref.MUTANTS))
def test_every_mutant_exceeds_the_bound(mut):
    """Each mutant of the reference -- one plausible kernel error -- is further from the reference than the bound allows, on at
    least one element, in EVERY case listed for it: a kernel with that error fails the GPU test there."""
    dirs = roi_ref.MUTANTS[mut][1]
    for name in MUTANT_CASES[mut]:
        c, d = BY_NAME[name], inputs(name)
        if c.kind == "bwd":
            assert "bwd" in dirs, (mut, name)
            grads, mags, cover, kw = _bwd(name)
            bad = roi_ref.bwd64(d["dout"], d["rois"], *_shape(c), mut=mut)[0]
            loose = roi_ref.bound_bwd_atomic(mags, cover, kw)
            tight = roi_ref.bound_bwd_gather(mags, cover, kw, len(d["rois"]))
            over = sum(int((np.abs(bad[l] - grads[l]) > np.maximum(loose[l], tight[l])).sum()) for l in range(4))
        else:
            assert "fwd" in dirs, (mut, name)
            out, mag, geo = _fwd(name)
            bad = roi_ref.fwd64(d["feats"], d["rois"], mut=mut)
            vec = roi_ref.vec_of(c.dtype)
            bound = roi_ref.bound_fwd(mag, geo, c.C, "nchw")
            if c.kind == "nhwc":
                bound = np.maximum(bound, roi_ref.bound_fwd(mag, geo, c.C, "nhwc", vec))
            over = int((np.abs(bad - out) > bound).sum())
        assert over > 0, (mut, roi_ref.MUTANTS[mut][0], name)
