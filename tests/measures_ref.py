"""The yardstick for the DAVIS counts (include/dmm_match.h (14)): the six integers of every (frame, object) by the direct
definition -- the boundary map from padded numpy shifts, the dilation with the FULL disk footprint through
``scipy.ndimage.binary_dilation`` -- written without a look at dmm_net_amd/measures.py's host form and sharing nothing with it.
tests/test_measures_cpu.py holds this file to the fixture captured from the reference (tests/golden/measures.npz); the GPU
tests hold the device entry to this file at the shapes the fixture does not have."""
import numpy as np
from scipy import ndimage


def bmap(m):
    """seg2bmap at equal size: m bool [H,W].  p is m with one row and one column of zeros behind it, so the three shifts
    towards the origin are plain slices that read zero where they leave the image."""
    m = np.asarray(m, dtype=bool)
    H, W = m.shape
    p = np.zeros((H + 1, W + 1), dtype=bool)
    p[:H, :W] = m
    east, south, south_east = p[:H, 1:], p[1:, :W], p[1:, 1:]
    b = (m != east) | (m != south) | (m != south_east)
    b[H - 1, :] = m[H - 1, :] != east[H - 1, :]            # the last row, then the last column, then the corner: this order
    b[:, W - 1] = m[:, W - 1] != south[:, W - 1]
    b[H - 1, W - 1] = False
    return b


def disk(radius):
    r = int(radius)
    dy, dx = np.ogrid[-r:r + 1, -r:r + 1]
    return dx * dx + dy * dy <= r * r


def dilate(b, radius):
    """Binary dilation by the disk, zeros outside the image."""
    return ndimage.binary_dilation(b, structure=disk(radius), border_value=0)


def counts(pred, gt, n_obj, radius):
    """uint8 label maps [T,H,W] -> int32 [T,n_obj,6]: #(S & A), #(S | A), #bmap(S), #bmap(A), #(bmap(S) & dil(bmap(A))),
    #(bmap(A) & dil(bmap(S))) with S = (pred == o + 1), A = (gt == o + 1)."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    assert pred.shape == gt.shape and pred.ndim == 3
    T = pred.shape[0]
    out = np.zeros((T, n_obj, 6), dtype=np.int32)
    for t in range(T):
        ids = np.union1d(np.unique(pred[t]), np.unique(gt[t]))
        for o in range(n_obj):
            if o + 1 not in ids:
                continue                                   # neither map has the label: every count is 0
            S, A = pred[t] == o + 1, gt[t] == o + 1
            bs, ba = bmap(S), bmap(A)
            out[t, o] = (np.count_nonzero(S & A), np.count_nonzero(S | A), np.count_nonzero(bs), np.count_nonzero(ba),
                         np.count_nonzero(bs & dilate(ba, radius)), np.count_nonzero(ba & dilate(bs, radius)))
    return out
