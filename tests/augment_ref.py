"""The yardstick for the clip augmentation (include/dmm_match.h (15)): the entry's arithmetic in numpy fp32, operation for
operation -- numpy rounds every elementwise fp32 operation once and never contracts a multiply and an add -- for the source
index, the flip, the gather, the boxes with their empty rule, the target planes, the sizes and the matrix chain.
tests/test_augment_cpu.py holds this file to the fixture captured from the reference (tests/golden/augment.npz) under the
near-tie rule written in ``near_tie``; the GPU tests hold the device entry to this file byte for byte."""
import math

import numpy as np

F32 = np.float32


def source_index(m, flip, H, W):
    """Row-major 3 x 3 matrix (any float array, read as fp32), flip flag -> (ri, ci) int64 [H,W]: the source pixel of every
    output pixel."""
    m = np.asarray(m, dtype=F32).reshape(3, 3)
    cr, cc = F32(H / 2.0 - 0.5), F32(W / 2.0 - 0.5)       # formed in double, rounded once
    x = (np.arange(H, dtype=F32) - cr)[:, None]
    y = (np.arange(W, dtype=F32) - cc)[None, :]
    sr = (((m[0, 0] * x) + (m[0, 1] * y)) + m[0, 2]) + cr
    sc = (((m[1, 0] * x) + (m[1, 1] * y)) + m[1, 2]) + cc
    assert sr.dtype == F32 and sc.dtype == F32 and sr.shape == (H, W)
    ri = np.rint(np.minimum(np.maximum(sr, F32(0)), F32(H - 1))).astype(np.int64)      # clamp, THEN round half to even
    ci = np.rint(np.minimum(np.maximum(sc, F32(0)), F32(W - 1))).astype(np.int64)
    if flip:
        ci = W - 1 - ci
    return ri, ci


def near_tie(m, H, W, eps=1e-3):
    """bool [H,W]: the pixels where either clamped source coordinate, computed in float64, lies within ``eps`` of a
    half-integer.  There a last-bit difference in how the coordinate was formed (the reference uses a bmm) may pick the other
    neighbour; everywhere else the rounding is decided."""
    m = np.asarray(m, dtype=np.float64).reshape(3, 3)
    cr, cc = H / 2.0 - 0.5, W / 2.0 - 0.5
    x = (np.arange(H, dtype=np.float64) - cr)[:, None]
    y = (np.arange(W, dtype=np.float64) - cc)[None, :]
    sr = np.clip(m[0, 0] * x + m[0, 1] * y + m[0, 2] + cr, 0, H - 1)
    sc = np.clip(m[1, 0] * x + m[1, 1] * y + m[1, 2] + cc, 0, W - 1)
    frac_r, frac_c = sr - np.floor(sr), sc - np.floor(sc)
    return (np.abs(frac_r - 0.5) <= eps) | (np.abs(frac_c - 0.5) <= eps)


def neighbours(m, flip, H, W):
    """(r_lo, r_hi, c_lo, c_hi), int64 [H,W] each: the two rows and the two columns a near-tie pixel may come from (floor and
    ceiling of the clamped float64 coordinate; the columns after the flip)."""
    m = np.asarray(m, dtype=np.float64).reshape(3, 3)
    cr, cc = H / 2.0 - 0.5, W / 2.0 - 0.5
    x = (np.arange(H, dtype=np.float64) - cr)[:, None]
    y = (np.arange(W, dtype=np.float64) - cc)[None, :]
    sr = np.clip(m[0, 0] * x + m[0, 1] * y + m[0, 2] + cr, 0, H - 1)
    sc = np.clip(m[1, 0] * x + m[1, 1] * y + m[1, 2] + cc, 0, W - 1)
    r_lo, r_hi = np.floor(sr).astype(np.int64), np.ceil(sr).astype(np.int64)
    c_lo, c_hi = np.floor(sc).astype(np.int64), np.ceil(sc).astype(np.int64)
    if flip:
        c_lo, c_hi = W - 1 - c_lo, W - 1 - c_hi
    return r_lo, r_hi, c_lo, c_hi


def warp(planes, ri, ci):
    """[..., H, W] -> [..., H, W]: out[..., r, c] = planes[..., ri[r, c], ci[r, c]]."""
    return np.ascontiguousarray(np.asarray(planes)[..., ri, ci])


def boxes(masks_out, boxes_in):
    """Warped masks [P,H,W], the caller's boxes [P,4] -> (boxes fp32 [P,4] xyxy, valid int32 [P]): the inclusive extent of
    (mask > 0.5), or the caller's box and 0 where no pixel is."""
    P = masks_out.shape[0]
    out = np.array(boxes_in, dtype=F32).reshape(P, 4).copy()
    valid = np.zeros(P, dtype=np.int32)
    for p in range(P):
        rows, cols = np.nonzero(masks_out[p] > F32(0.5))
        if rows.size:
            out[p] = (cols.min(), rows.min(), cols.max(), rows.max())
            valid[p] = 1
    return out, valid


def targets(label, F):
    """Warped annotation uint8 [H,W] -> (planes fp32 [F,H,W], sizes int32 [F]); label 0 is background, labels above F (255
    among them) belong to no plane."""
    planes = np.stack([(label == o + 1) for o in range(F)]).astype(F32) if F else np.zeros((0,) + label.shape, dtype=F32)
    return planes, planes.reshape(F, -1).sum(axis=1).astype(np.int32)


def augment_clip(frames, labels, masks, boxes_in, matrices, flips, F):
    """frames [n,C,H,W] fp32, labels [n,H,W] uint8, masks [n,P,H,W] fp32 (P may be 0), boxes_in [n,P,4], matrices [n,3,3],
    flips [n] -> dict of frames, labels, masks, boxes, box_valid, targets [n,F,H,W], sizes [n,F]."""
    n, H, W = labels.shape
    P = masks.shape[1]
    out = {"frames": np.empty_like(frames), "labels": np.empty_like(labels), "masks": np.empty_like(masks),
           "boxes": np.zeros((n, P, 4), dtype=F32), "box_valid": np.zeros((n, P), dtype=np.int32),
           "targets": np.zeros((n, F, H, W), dtype=F32), "sizes": np.zeros((n, F), dtype=np.int32)}
    for f in range(n):
        ri, ci = source_index(matrices[f], bool(flips[f]), H, W)
        out["frames"][f], out["labels"][f], out["masks"][f] = warp(frames[f], ri, ci), warp(labels[f], ri, ci), warp(masks[f], ri, ci)
        out["boxes"][f], out["box_valid"][f] = boxes(out["masks"][f], np.asarray(boxes_in)[f])
        out["targets"][f], out["sizes"][f] = targets(out["labels"][f], F)
    return out


def reference_rows(targets_, sizes):
    """[n,F,H,W], [n,F] -> float64 [n,F,HW + 1]: the rows sequence_from_masks returns (the planes, then the "object present"
    flag)."""
    n, F = sizes.shape
    return np.concatenate([targets_.reshape(n, F, -1).astype(np.float64), (sizes > 0).astype(np.float64)[:, :, None]], axis=2)


def _mm(a, b):
    """3 x 3 fp32 product, every entry ((a0 b0 + a1 b1) + a2 b2) with one rounding per operation."""
    out = np.empty((3, 3), dtype=F32)
    for i in range(3):
        for j in range(3):
            out[i, j] = ((a[i, 0] * b[0, j]) + (a[i, 1] * b[1, j])) + (a[i, 2] * b[2, j])
    return out


def matrix_chain(rotation, translation, shear, zoom, H, W):
    """Rotate . Translate . Shear . Zoom: degrees, (fraction of H, fraction of W), degrees, (zx, zy) -> fp32 [3,3].  The
    entries are formed in double and rounded to fp32 once; the products are fp32."""
    th = math.pi / 180 * rotation
    R = np.array([[math.cos(th), -math.sin(th), 0], [math.sin(th), math.cos(th), 0], [0, 0, 1]], dtype=F32)
    T = np.array([[1, 0, translation[0] * H], [0, 1, translation[1] * W], [0, 0, 1]], dtype=F32)
    ts = (math.pi * shear) / 180
    S = np.array([[1, -math.sin(ts), 0], [0, math.cos(ts), 0], [0, 0, 1]], dtype=F32)
    Z = np.array([[zoom[0], 0, 0], [0, zoom[1], 0], [0, 0, 1]], dtype=F32)
    return _mm(_mm(_mm(R, T), S), Z)
