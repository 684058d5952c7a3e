"""float64 reference of the ROI feature kernels (``csrc/dmm_roialign.hip``: the NCHW and channels-last forwards, the atomic and
the deterministic backward), the derived error bounds, the shared case list, the seeded input builders and the mutants --
TEST INFRASTRUCTURE ONLY (no test functions here).  Plain numpy on the host.

The reference DECIDES NOTHING.  ``dmm_roialign.hip`` is compiled with -ffp-contract=off, so every operation of ``axis_weights``
rounds once; the 28 sample coordinates of an axis are redone here in numpy float32, operation by operation in the source's
order (``coords32``), and are therefore the kernel's own bits.  Everything after them is float64 of THOSE coordinates: the
outside test, the clamp at 0, the top clamp, ly, hy, the two weight vectors and their lo / hi range.  A float64 run can then
never stand on the other side of -1 or ``size`` from the kernel, and no element is ever left out of a comparison.

Bounds.  u = 2^-24 (one fp32 rounding), gamma(k) = k u / (1 - k u) (k roundings, Higham).  Each bound is gamma(k) x (the sum of
the magnitudes of the terms that enter the fp32 sum); k is counted from the kernel source and written beside the formula.
gamma(k) itself carries the higher-order products of the k roundings on a term's path ((1 + d)^k - 1 <= gamma(k)); what the
bounds leave out is the float64 evaluation of the magnitudes and of the reference itself (2^-53 relative, eight decimal orders
below u) and underflow: the cases hold no fp32 term in the subnormal range.  ``tests/test_roi_ref_cpu.py`` holds the bounds
against an fp32 emulation of the kernels' arithmetic.
"""
import collections
import functools
import math

import numpy as np

U = 2.0 ** -24
ROUND = {"fp32": 2.0 ** -24, "fp16": 2.0 ** -11, "bf16": 2.0 ** -8}      # unit roundoff: 24, 11 and 8 significand bits
# half the spacing of the type's subnormals (fp16: 2^-24, bf16: 2^-133): a result below the normal range rounds absolutely
TINY = {"fp32": 0.0, "fp16": 2.0 ** -25, "bf16": 2.0 ** -134}
SCALES = (0.25, 0.125, 0.0625, 0.03125)
NS = 28                                                                 # 14 bins x sampling ratio 2
CLASSES = ("outside", "clamp0", "top", "interior", "at_m1", "at_size")
F = np.float32


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


def round_to(a, dtype):
    """float array -> float32 array of values exactly representable in ``dtype`` (round to nearest even)."""
    a = np.asarray(a, dtype=np.float32)
    if dtype == "fp16":
        return a.astype(np.float16).astype(np.float32)
    if dtype == "bf16":
        b = a.view(np.uint32).astype(np.uint64)
        b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
        return b.astype(np.uint32).view(np.float32)
    return a


# ---- coordinates: the kernel's own fp32 bits ----------------------------------------------------------------------------
def coords32(a, b, scale, clamp=True):
    """The 28 sample coordinates of a roi along one axis as ``axis_weights`` computes them, every operation in float32:
    roi * scale (both ends), end - start, the clamp to 1, / 14, then start + p * bin + (i + 0.5) * bin / 2."""
    start, end = F(a) * F(scale), F(b) * F(scale)
    ln = F(end - start)
    if clamp and not ln > F(1):
        ln = F(1)
    bn = F(ln / F(14))
    ys = np.empty(NS, dtype=np.float32)
    for k in range(NS):
        p, i = k >> 1, k & 1
        ys[k] = F(F(start + F(F(p) * bn)) + F(F(F(F(i) + F(0.5)) * bn) / F(2)))
    return ys


def coords64(a, b, scale):
    """The same coordinates from the same fp32 ends, every later operation in float64 -> (ys, |start| + len)."""
    start, end = float(F(a) * F(scale)), float(F(b) * F(scale))
    ln = max(end - start, 1.0)
    bn = ln / 14.0
    ys = np.array([start + (k >> 1) * bn + ((k & 1) + 0.5) * bn / 2.0 for k in range(NS)])
    return ys, abs(start) + ln


# six roundings separate the two: end - start, / 14, p * bin, the first sum, (i + 0.5) * bin, the last sum (roi * scale and / 2
# are exact: powers of two); each is relative to a value of at most |start| + len
COORD_ROUNDINGS = 6

Axis = collections.namedtuple("Axis", "w lo hi cnt census ys")


@functools.lru_cache(maxsize=None)
def axis64(a, b, scale, size, mut=0):
    """The weight vector of one axis in float64 from the fp32 coordinates -> Axis(w [size], lo, hi (hi < lo: no sample inside),
    cnt = the most non-zero additions any one cell received, census, ys).  ``mut``: mutants 1 - 6 (see MUTANTS)."""
    ys = coords32(a, b, scale, clamp=mut != 3)
    w, cnt = np.zeros(size), np.zeros(size, dtype=np.int64)
    lo, hi = size, -1
    census = dict.fromkeys(CLASSES, 0)
    for y in (ys[:-1] if mut == 6 else ys):
        y = float(y)
        if y < -1.0 or y > size or (mut == 1 and y >= size) or (mut == 2 and y <= -1.0):
            census["outside"] += 1
            continue
        census["at_m1"] += y == -1.0
        census["at_size"] += y == size
        klass = "interior"
        if y <= 0.0 and mut != 4:
            y, klass = 0.0, "clamp0"
        yl = int(y)                                           # (int)y truncates toward zero
        if yl >= size - 1 and mut != 5:
            yh = yl = size - 1
            y = float(yl)
            klass = "top" if klass == "interior" else klass
        else:
            yh = yl + 1
        census[klass] += 1
        ly = y - yl
        hy = 1.0 - ly
        for idx, v in ((yl, hy), (yh, ly)):
            if 0 <= idx < size:                               # (only a mutant indexes outside; that term is dropped)
                w[idx] += v
                cnt[idx] += v != 0.0
                lo, hi = min(lo, idx), max(hi, idx)
    w.setflags(write=False)
    return Axis(w, lo, hi, int(cnt.max()), census, ys)


Geo = collections.namedtuple("Geo", "b ay ax live")


def geometry(rois, Hs, Ws, B, mut=0):
    """-> [R][4] Geo: frame, the two axes, and whether the (roi, level) contributes at all (a frame in [0, B) and a sample
    inside on both axes)."""
    sc = list(SCALES)
    if mut == 8:
        sc[1], sc[2] = sc[2], sc[1]
    out = []
    for roi in np.asarray(rois, dtype=np.float32):
        b = int(roi[0])
        per = []
        for l in range(4):
            ay = axis64(float(roi[2]), float(roi[4]), sc[l], int(Hs[l]), mut)
            ax = axis64(float(roi[1]), float(roi[3]), sc[l], int(Ws[l]), mut)
            inside = ay.hi >= ay.lo and ax.hi >= ax.lo
            if mut == 9 and b < 0:
                per.append(Geo(0, ay, ax, inside))
            else:
                per.append(Geo(b, ay, ax, inside and 0 <= b < B))
        out.append(per)
    return out


def census(rois, Hs, Ws):
    """-> {"y": {class: samples}, "x": {...}} summed over every roi and level."""
    tot = {"y": dict.fromkeys(CLASSES, 0), "x": dict.fromkeys(CLASSES, 0)}
    for per in geometry(rois, Hs, Ws, 1 << 30):
        for g in per:
            for k in CLASSES:
                tot["y"][k] += g.ay.census[k]
                tot["x"][k] += g.ax.census[k]
    return tot


# ---- the reference ------------------------------------------------------------------------------------------------------
def _tiles(ph, pw):
    """The NCHW forward's row tiles of a ph x pw patch -> (rows per tile, tiles)."""
    rpt = max(1, min(1024 // pw, ph)) if pw <= 1024 else 1
    return rpt, -(-ph // rpt)


def fwd64(feats, rois, mut=0, want_mag=False):
    """out[r, l C + c] = wy' F wx / 784 in float64 from the exact upcast of the features ([B, C, H, W] arrays, any float type);
    zeros for a dead roi (frame < 0), a frame >= B and an empty patch.  want_mag: also sum |wy| |wx| |f| / 784 and the geometry."""
    B, C = feats[0].shape[:2]
    Hs, Ws = [f.shape[2] for f in feats], [f.shape[3] for f in feats]
    geo = geometry(rois, Hs, Ws, B, mut)
    f64 = [np.asarray(f, dtype=np.float64) for f in feats]
    out, mag = np.zeros((len(geo), 4 * C)), np.zeros((len(geo), 4 * C))
    norm = 783.0 if mut == 7 else 784.0
    for r, per in enumerate(geo):
        for l, g in enumerate(per):
            if not g.live:
                continue
            h0, h1, w0, w1 = g.ay.lo, g.ay.hi, g.ax.lo, g.ax.hi
            wy, wx = g.ay.w[h0:h1 + 1], g.ax.w[w0:w1 + 1]
            if mut == 10:
                rpt, nt = _tiles(h1 - h0 + 1, w1 - w0 + 1)
                wy = np.where(np.arange(len(wy)) >= (nt - 1) * rpt, wy, 0.0)
            patch = f64[l][g.b, :, h0:h1 + 1, w0:w1 + 1]
            out[r, l * C:(l + 1) * C] = np.einsum("h,chw,w->c", wy, patch, wx) / norm
            mag[r, l * C:(l + 1) * C] = np.einsum("h,chw,w->c", np.abs(wy), np.abs(patch), np.abs(wx)) / 784.0
    if mut == 11:                                             # the register group's clamped channels stored past the level's C
        src = out.copy()
        for r, per in enumerate(geo):
            for l in range(3):
                if per[l].live:
                    for j in range(min((-C) % 4, C)):
                        out[r, (l + 1) * C + j] = src[r, l * C + C - 1]
    return (out, mag, geo) if want_mag else out


def fwd64_samples(feats, rois):
    """The second, non-separable formulation, as the legacy definition is written: per bin the 2 x 2 samples, each with its
    outside test on both axes, its clamps and its 4 corners; the bin's mean; then the mean over the 14 x 14 bins.  From the
    same fp32 coordinates.  Its only job is to check ``fwd64``."""
    B, C = feats[0].shape[:2]
    out = np.zeros((len(rois), 4 * C))
    for r, roi in enumerate(np.asarray(rois, dtype=np.float32)):
        b = int(roi[0])
        if not 0 <= b < B:
            continue
        for l, f in enumerate(feats):
            H, W = f.shape[2:]
            data = np.asarray(f[b], dtype=np.float64)

            def prep(ys, size):
                ys = ys.astype(np.float64)
                ok = ~((ys < -1.0) | (ys > size))
                y = np.where(ys <= 0.0, 0.0, ys)
                lo = np.where(ok, y, 0.0).astype(np.int64)
                top = lo >= size - 1
                lo = np.where(top, size - 1, lo)
                hi = np.where(top, size - 1, lo + 1)
                y = np.where(top, lo.astype(np.float64), y)
                ly = y - lo
                return ok, lo, hi, ly, 1.0 - ly
            oky, yl, yh, ly, hy = prep(coords32(float(roi[2]), float(roi[4]), SCALES[l]), H)
            okx, xl, xh, lx, hx = prep(coords32(float(roi[1]), float(roi[3]), SCALES[l]), W)
            v = (data[:, yl][:, :, xl] * np.outer(hy, hx) + data[:, yl][:, :, xh] * np.outer(hy, lx)
                 + data[:, yh][:, :, xl] * np.outer(ly, hx) + data[:, yh][:, :, xh] * np.outer(ly, lx))
            v = v * np.outer(oky, okx)                          # a sample outside on either axis is 0
            bins = v.reshape(C, 14, 2, 14, 2).sum(axis=(2, 4)) / 4.0
            out[r, l * C:(l + 1) * C] = bins.mean(axis=2).mean(axis=1)
    return out


def bwd64(dout, rois, B, C, Hs, Ws, mut=0, init=None):
    """The adjoint: dfeat_l[b, c] = init + sum over the rois r of frame b of dout[r, l C + c] wy_r wx_r' / 784, in float64 ->
    (grads [4] of [B, C, H, W], mags [4] = sum |dout| |wy| |wx| / 784 (+ |init|), cover [4] of [B, H, W] = rois whose patch
    holds the cell, kw = the largest weight-rounding count cy + cx of any live (roi, level))."""
    geo = geometry(rois, Hs, Ws, B, mut)
    d64 = np.asarray(dout, dtype=np.float64)
    grads = [np.zeros((B, C, Hs[l], Ws[l])) for l in range(4)]
    mags = [np.zeros((B, C, Hs[l], Ws[l])) for l in range(4)]
    cover = [np.zeros((B, Hs[l], Ws[l]), dtype=np.int64) for l in range(4)]
    kw = 0
    chunks, rows_of = {}, {}                                  # mutant 13: (level, frame, chunk of 64 rois) -> its sum, its rows
    for r, per in enumerate(geo):
        for l, g in enumerate(per):
            if not g.live:
                continue
            t = np.outer(g.ay.w, g.ax.w) / 784.0
            if mut == 12:                                     # wy and wx transposed (cropped / padded to the level)
                m = max(Hs[l], Ws[l])
                p = np.zeros((m, m))
                p[:Ws[l], :Hs[l]] = t.T
                t = p[:Hs[l], :Ws[l]]
            d = d64[r, l * C:(l + 1) * C][:, None, None]
            if mut == 13:                                     # every chunk of 64 rois OVERWRITES the rows it touches
                key = (l, g.b, r // 64)
                chunks[key] = chunks.get(key, 0.0) + d * t
                rows_of.setdefault(key, set()).update(range(g.ay.lo, g.ay.hi + 1))
            else:
                grads[l][g.b] += d * t
            mags[l][g.b] += np.abs(d) * np.abs(t)
            cover[l][g.b, g.ay.lo:g.ay.hi + 1, g.ax.lo:g.ax.hi + 1] += 1
            kw = max(kw, g.ay.cnt + g.ax.cnt)
    for key in sorted(chunks):                                # (ascending chunk within a level and frame: the last one stays)
        rows = sorted(rows_of[key])
        grads[key[0]][key[1]][:, rows, :] = chunks[key][:, rows, :]
    if init is not None:
        for l in range(4):
            grads[l] += np.asarray(init[l], dtype=np.float64)
            mags[l] += np.abs(np.asarray(init[l], dtype=np.float64))
    return grads, mags, cover, kw


# ---- derived bounds: gamma(k) x the magnitudes; k from the kernel source -----------------------------------------------------
def k_weights(g):
    """One cell's weight wy[h] wx[w]: hy = 1 - ly rounds once (ly = y - y_low is exact) and a cell that receives n non-zero
    terms takes n - 1 rounded additions (the first lands on 0): at most cnt per axis; the product wy wx: 1."""
    return g.ay.cnt + g.ax.cnt + 1


def k_fwd_nchw(g):
    """roialign4_mean_kernel<T, false>: the weight (k_weights); a lane's fma chain over cells e, e + 64, ... of a tile of ne <=
    1024 cells: ceil(ne / 64) <= 16; wave_sum_rows: 6 additions; acc * norm with norm = fl(1 / 784): 2; one addition into
    ``out`` per row tile after the first: tiles - 1."""
    ph, pw = g.ay.hi - g.ay.lo + 1, g.ax.hi - g.ax.lo + 1
    rpt, nt = _tiles(ph, pw)
    return k_weights(g) + -(-(min(rpt, ph) * pw) // 64) + 6 + 2 + (nt - 1)


def k_fwd_nhwc(g, C, vec):
    """roialign4_mean_nhwc_kernel: the weight (k_weights); LPC = min(C, 64 vec) / vec lanes per cell, 64 / LPC cells per wave
    and load, 8 waves: a lane's fma chain holds every (8 x 64 / LPC)-th cell, ceil(ncell / (8 CPW)) terms whatever the unroll
    (the cells past the patch have weight 0: fma(0, v, acc) = acc); the shuffle folds: log2(CPW) additions; the eight waves:
    7 additions; t * norm with norm = fl(1 / 784): 2."""
    ncell = (g.ay.hi - g.ay.lo + 1) * (g.ax.hi - g.ax.lo + 1)
    cpw = 64 // (min(C, 64 * vec) // vec)
    return k_weights(g) + -(-ncell // (8 * cpw)) + int(math.log2(cpw)) + 7 + 2


def bound_fwd(mag, geo, C, form, vec=None):
    """[R, 4 C] bound of a forward: gamma(k of the (roi, level)) x sum |wy| |wx| |f| / 784."""
    k = np.zeros_like(mag)
    for r, per in enumerate(geo):
        for l, g in enumerate(per):
            if g.live:
                k[r, l * C:(l + 1) * C] = k_fwd_nchw(g) if form == "nchw" else k_fwd_nhwc(g, C, vec)
    return gamma(k) * mag


def bound_bwd_atomic(mags, cover, kw):
    """roialign4_mean_kernel<float, true>: a term is g = dout * norm (norm itself rounded: 2), g * wx (1), gx * wy (1) with the
    two weights' own roundings (kw = cy + cx at most); a cell covered by n rois then takes at most n rounded additions, in
    whatever order the atomics land (n - 1 into a zeroed cell): k = kw + 4 + n."""
    return [gamma(kw + 4 + cover[l][:, None]) * mags[l] for l in range(4)]


def bound_bwd_gather(mags, cover, kw, R):
    """roialign4_det_gather_kernel: a term is g = dout * norm (2), g * wx (1), then the fma with wy that adds it to the
    chunk's accumulator (1, counted in the chain); the chain of a chunk holds at most min(n, 64) fmas; every chunk of 64 rois
    adds its accumulator to the cell once: ceil(R / 64) additions at most: k = kw + 3 + min(n, 64) + ceil(R / 64)."""
    return [gamma(kw + 3 + np.minimum(cover[l][:, None], 64) + -(-R // 64)) * mags[l] for l in range(4)]


def bound_cast(bound, ref, dtype):
    """One more rounding of the fp32 result to ``dtype`` (autograd hands the gradient back in the feature's type)."""
    return bound + ROUND[dtype] * (np.abs(ref) + bound) + TINY[dtype] if dtype != "fp32" else bound


# ---- cases ---------------------------------------------------------------------------------------------------------------
# kind: "nchw" / "nhwc" forward, "bwd".  H, W: the four levels, free of each other.
Case = collections.namedtuple("Case", "name kind dtype B C H W extra")
SMALL_H, SMALL_W = (9, 5, 3, 1), (13, 7, 4, 1)
NHWC_LPC = (1, 4, 64, 128, 192)
BWD_BOX = (6.0, 5.0, 30.0, 26.0)                              # the box 130 rois of one frame share


def vec_of(dtype):
    return 4 if dtype == "fp32" else 8


def _cases():
    out = []
    for C in (1, 2, 3, 4, 5, 16, 17):
        for dtype in ("fp32", "fp16", "bf16"):
            for B in (1, 3):
                out.append(Case(f"nchw_c{C}_{dtype}_b{B}", "nchw", dtype, B, C, SMALL_H, SMALL_W, None))
    # a patch exactly 1024 cells wide (one row per tile, the LDS tables filled to their last entry: the "wide" rois of
    # ``inputs``), and a patch above 1024 cells whose 40 rows go in tiles of 25 + 15
    out.append(Case("nchw_wide", "nchw", "fp32", 1, 2, (3, 2, 1, 1), (1024, 512, 256, 128), "wide"))
    out.append(Case("nchw_tiles", "nchw", "bf16", 1, 5, (40, 20, 10, 5), (40, 20, 10, 5), None))
    for dtype in ("fp32", "fp16", "bf16"):
        for lpc in NHWC_LPC:
            # one lane per cell: a workgroup step is 512 cells, "more than four steps" needs a patch above 2048 cells
            H, W = ((48, 6, 2, 1), (48, 5, 3, 1)) if lpc < 64 else (SMALL_H, SMALL_W)
            out.append(Case(f"nhwc_{dtype}_lpc{lpc}", "nhwc", dtype, 2, lpc * vec_of(dtype), H, W, None))
    for C in (1, 3, 5, 64):
        out.append(Case(f"bwd_c{C}", "bwd", "fp32", 3, C, SMALL_H, SMALL_W, "crowd"))
    assert len({c.name for c in out}) == len(out)
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def boxes_of(H0, W0, gen):
    """The roi kinds every case carries, for a level 0 of H0 x W0 cells (image 4 H0 x 4 W0).  The two exact-boundary boxes have
    a scaled length of 14 (level 0: bin = 1) so every coordinate is dyadic and exact in fp32: (-5, 51) gives level-0 samples at
    -1, -0.5, 0, ...; (4 S - 53, 4 S + 3) gives ..., S - 0.5, S, S + 0.5 on a level of S cells."""
    Hi, Wi = 4.0 * H0, 4.0 * W0
    fixed = [(3.0, 4.0, 3.2, 4.1),                            # sub-pixel: the length clamps to 1
             (-400.0, -400.0, -300.0, -300.0),                # outside on every level
             (-40.0, -40.0, -20.0, -20.0),                    # outside on the fine levels only
             (-9.0, -7.0, 14.0, 11.0), (Wi - 10.0, -6.0, Wi + 12.0, 9.0),             # clipped at each corner
             (-8.0, Hi - 9.0, 13.0, Hi + 9.0), (Wi - 10.0, Hi - 9.0, Wi + 12.0, Hi + 9.0),
             (0.0, 0.0, Wi, Hi), (0.0, 0.0, Wi - 1.0, Hi - 1.0),                      # whole frame
             (-5.0, -5.0, 51.0, 51.0),                        # samples exactly at -1
             (4.0 * W0 - 53.0, 4.0 * H0 - 53.0, 4.0 * W0 + 3.0, 4.0 * H0 + 3.0)]      # samples exactly at size
    rnd = []
    for _ in range(3):
        x1, y1 = gen.uniform(-5, Wi - 2), gen.uniform(-5, Hi - 2)
        rnd.append((x1, y1, min(x1 + gen.uniform(0.2, Wi * 0.8), Wi + 6), min(y1 + gen.uniform(0.2, Hi * 0.8), Hi + 6)))
    return fixed + rnd


@functools.lru_cache(maxsize=None)
def inputs(name):
    """Seeded host inputs of one case, never modified: feats [4] of [B, C, H, W] float32 holding values exact in the case's
    type, rois [R, 5] float32, dout [R, 4 C] float32."""
    c = BY_NAME[name]
    gen = np.random.default_rng(sum(map(ord, name)) * 7919 + c.C)
    feats = [round_to(gen.standard_normal((c.B, c.C, c.H[l], c.W[l])), c.dtype) for l in range(4)]
    whole = (0.0, 0.0, 4.0 * c.W[0], 4.0 * c.H[0])
    # (the backward cases keep the roi kinds off their last frame: it receives BWD_BOX alone, and cells there stay uncovered)
    frames = c.B - 1 if c.extra == "crowd" else c.B
    rois = [(j % frames,) + bx for j, bx in enumerate(boxes_of(c.H[0], c.W[0], gen))]
    rois += [(-1.0,) + whole, (float(c.B),) + whole]          # a dead roi, and a frame index equal to B
    if c.extra == "wide":
        rois.append((0.0, -3.0, 1.0, 4.0 * c.W[0] + 2.0, 9.0))
        # scaled start -19.5, length W + 38: the first of the 28 samples lands at -0.54 (clamped into cell 0) and the last at
        # W - 0.46 (cell W - 1), both inside [-1, W]: the patch is exactly W = 1024 cells wide
        rois.append((0.0, -78.0, 1.0, 4.0 * c.W[0] + 74.0, 9.0))
    if c.extra == "crowd":                                    # 130 identical rois of frame 1: the gather's chunks of 64, 64, 2
        for j in range(130):
            rois.append((1.0,) + BWD_BOX)
            if j % 10 == 3:
                rois.append((-1.0,) + BWD_BOX)                # dead, and rois of the other frames, in between
                rois.append((float(j % 3 if j % 3 != 1 else 2),) + BWD_BOX)
        rois.append((float(c.B),) + BWD_BOX)
    rois = np.asarray(rois, dtype=np.float32)
    dout = gen.standard_normal((len(rois), 4 * c.C)).astype(np.float32)
    for a in feats + [rois, dout]:
        a.setflags(write=False)
    return {"feats": feats, "rois": rois, "dout": dout}


# ---- mutants: Python variants of the reference, each one plausible kernel error ---------------------------------------------
# number: (what, the directions it applies to)
MUTANTS = {
    1: ("y >= size excluded", ("fwd", "bwd")),
    2: ("y <= -1 excluded", ("fwd", "bwd")),
    3: ("no clamp of the roi length to 1", ("fwd", "bwd")),
    4: ("no clamp of negative y to 0", ("fwd", "bwd")),
    5: ("top-edge clamp missing", ("fwd", "bwd")),
    6: ("last sample dropped", ("fwd", "bwd")),
    7: ("wrong normaliser (783)", ("fwd",)),
    8: ("two level scales swapped", ("fwd", "bwd")),
    9: ("dead roi not zeroed", ("fwd",)),
    10: ("last row tile overwrites the earlier partial sums", ("fwd",)),
    11: ("the clamped channel written into a live channel", ("fwd",)),
    12: ("backward with wy and wx transposed", ("bwd",)),
    13: ("backward without the chunk accumulation", ("bwd",)),
}
