"""The DAVIS scores of a clip: region similarity J and boundary accuracy F per object and frame, then mean, recall and decay
per sequence -- the reference's dmm/measures/jaccard.py, f_boundary.py and statistics.py as dmm/dataloader/evaluation.py:31-58
and tools/davis_eval.py drive them.

Both measures are ratios of integer counts.  ``clip_counts`` produces the six counts per (frame, object)
(include/dmm_match.h (14)): on the device through ``dmm_davis_counts_u8`` (two launches, no host read, capturable), on the host
through the numpy / ``scipy.ndimage`` form written here -- same semantics, same integers.  ``scores_from_counts`` turns the
integers into the reference's floats with the reference's divisions and case analysis, so J and F equal its values bit for
bit.  ``ClipScorer`` is the callback for ``video.FrameLoop.run(on_labels=...)``: one entry call per frame into a device table,
one synchronisation in ``results()``.

Out of scope, as in the C entry: the T measure, and the reference's nearest-neighbour resize of a prediction whose size
differs from the annotation's (``ValueError`` here).
"""
from __future__ import annotations

import warnings

import numpy as np

N_COUNTS = 6       # S & A | S or A | n_fg | n_gt | bmap(S) & dil(bmap(A)) | bmap(A) & dil(bmap(S))


# ---- the radius ---------------------------------------------------------------------------------------------------------
def boundary_radius(shape, bound_th=0.008) -> int:
    """f_boundary.py:30-31: ``bound_th`` itself when it is >= 1 (an integer, else ValueError), otherwise
    ``np.ceil(bound_th * np.linalg.norm((H, W)))`` in float64 with exactly that numpy expression."""
    H, W = (int(v) for v in shape[-2:])
    bound_pix = bound_th if bound_th >= 1 else np.ceil(bound_th * np.linalg.norm((H, W)))
    if float(bound_pix) != int(bound_pix):
        raise ValueError(f"bound_th = {bound_th!r} is not a whole number of pixels")
    return int(bound_pix)


# ---- the host form ------------------------------------------------------------------------------------------------------
def seg2bmap(seg: np.ndarray) -> np.ndarray:
    """f_boundary.py:80-140 at equal size: bool [H,W] -> bool [H,W], the boundary offset half a pixel towards the origin."""
    seg = np.asarray(seg).astype(bool)
    e, s, se = np.zeros_like(seg), np.zeros_like(seg), np.zeros_like(seg)
    e[:, :-1] = seg[:, 1:]
    s[:-1, :] = seg[1:, :]
    se[:-1, :-1] = seg[1:, 1:]
    b = seg ^ e | seg ^ s | seg ^ se
    b[-1, :] = seg[-1, :] ^ e[-1, :]
    b[:, -1] = seg[:, -1] ^ s[:, -1]
    b[-1, -1] = 0
    return b


def _disk(radius: int) -> np.ndarray:
    L = np.arange(-radius, radius + 1)
    X, Y = np.meshgrid(L, L)
    return (X * X + Y * Y) <= radius * radius


def _dilate(b: np.ndarray, fp: np.ndarray) -> np.ndarray:
    from scipy import ndimage
    return ndimage.binary_dilation(b, structure=fp)


def _clip_counts_host(pred: np.ndarray, gt: np.ndarray, n_obj: int, radius: int) -> np.ndarray:
    T = pred.shape[0]
    out = np.zeros((T, n_obj, N_COUNTS), dtype=np.int32)
    if pred[0].size == 0:
        return out
    fp = _disk(radius)
    for f in range(T):
        present = set(np.unique(pred[f]).tolist()) | set(np.unique(gt[f]).tolist())
        for o in range(n_obj):
            if o + 1 not in present:
                continue                                  # both masks empty: six zeros
            S, A = pred[f] == o + 1, gt[f] == o + 1
            bS, bA = seg2bmap(S), seg2bmap(A)
            out[f, o] = ((S & A).sum(), (S | A).sum(), bS.sum(), bA.sum(), (bS & _dilate(bA, fp)).sum(),
                         (bA & _dilate(bS, fp)).sum())
    return out


# ---- counts -------------------------------------------------------------------------------------------------------------
def _is_tensor(x) -> bool:
    return type(x).__module__.partition(".")[0] == "torch" and hasattr(x, "is_cuda")


def _label_maps(pred, gt):
    if tuple(pred.shape) != tuple(gt.shape):
        raise ValueError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ in shape (resizing is out of scope)")
    if len(pred.shape) not in (2, 3):
        raise ValueError(f"label maps are [T,H,W] or [H,W], not {tuple(pred.shape)}")
    for name, x in (("pred", pred), ("gt", gt)):
        if "uint8" not in str(x.dtype):
            raise ValueError(f"{name} must be uint8 label maps, not {x.dtype}")


def _counts_into(pred, gt, n_obj: int, radius: int, counts) -> None:
    """The entry on device tensors pred, gt [T,H,W] (dense rows, any frame stride) into counts [T,n_obj,6] (contiguous)."""
    import torch
    from . import _lib
    T, H, W = pred.shape
    fixed = []
    for x in (pred, gt):
        if T and H * W and (x.stride(2) != 1 or x.stride(1) != W or (T > 1 and x.stride(0) < H * W)):
            x = x.contiguous()
        fixed.append(x)
    pred, gt = fixed
    fs = [x.stride(0) if T > 1 and H * W else H * W for x in (pred, gt)]
    stream = torch.cuda.current_stream(pred.device).cuda_stream
    L = _lib.load()
    need = L.dmm_davis_counts_workspace_bytes(T, n_obj, H, W, radius)
    ws = torch.empty(need, dtype=torch.uint8, device=pred.device) if need else None
    _lib.call("dmm_davis_counts_u8", pred.device, pred.data_ptr(), gt.data_ptr(), T, n_obj, H, W, fs[0], fs[1], radius,
              counts.data_ptr(), None if ws is None else ws.data_ptr(), need, stream)


def clip_counts(pred, gt, n_obj: int, radius=None, bound_th=0.008):
    """The six counts of every (frame, object): uint8 label maps [T,H,W] or [H,W] (0 = background, o + 1 = object o; labels
    above ``n_obj`` belong to no object) -> int32 [T,n_obj,6] in the order of include/dmm_match.h (14).  CUDA tensors go
    through the device entry on the current stream without synchronising and give a device tensor; host tensors and numpy
    arrays go through the numpy / scipy form and give what they were (a tensor or an array).  ``radius`` None: the
    reference's ``bound_pix`` for this frame size and ``bound_th`` (``boundary_radius``)."""
    _label_maps(pred, gt)
    n_obj = int(n_obj)
    if n_obj < 0:
        raise ValueError("n_obj is negative")
    r = boundary_radius(pred.shape, bound_th) if radius is None else int(radius)
    if r < 0 or (radius is not None and r != radius):
        raise ValueError(f"radius = {radius!r} is not a whole, non-negative number of pixels")
    tensors = _is_tensor(pred), _is_tensor(gt)
    if any(tensors) and (tensors[0] and pred.is_cuda or tensors[1] and gt.is_cuda):
        import torch
        if not all(tensors) or pred.device != gt.device:
            raise ValueError("pred and gt must be on the same device")
        p3, g3 = (x if x.dim() == 3 else x.unsqueeze(0) for x in (pred, gt))
        counts = torch.empty((p3.shape[0], n_obj, N_COUNTS), dtype=torch.int32, device=pred.device)
        _counts_into(p3, g3, n_obj, r, counts)
        return counts
    p, g = (np.asarray(x.numpy() if _is_tensor(x) else x) for x in (pred, gt))
    p3, g3 = (x if x.ndim == 3 else x[None] for x in (p, g))
    counts = _clip_counts_host(p3, g3, n_obj, r)
    if all(tensors):
        import torch
        return torch.from_numpy(counts)
    return counts


# ---- scores -------------------------------------------------------------------------------------------------------------
def _j_from(n_and: int, n_or: int):
    # jaccard.py:33-37: 1 when both masks are empty, else an integer sum over a float32 sum
    if n_or == 0:
        return 1
    return np.int64(n_and) / np.float32(n_or)


def _f_from(n_fg: int, n_gt: int, fg_match: int, gt_match: int):
    # f_boundary.py:59-76
    if n_fg == 0 and n_gt > 0:
        precision, recall = 1, 0
    elif n_fg > 0 and n_gt == 0:
        precision, recall = 0, 1
    elif n_fg == 0 and n_gt == 0:
        precision, recall = 1, 1
    else:
        precision = np.int64(fg_match) / float(n_fg)
        recall = np.int64(gt_match) / float(n_gt)
    if precision + recall == 0:
        return 0
    return 2 * precision * recall / (precision + recall)


def scores_from_counts(counts):
    """int [T,n_obj,6] (array or tensor, any device: one copy to the host) -> (J, F), float64 numpy [n_obj,T], with the
    reference's case analysis and its float64 divisions (J divides by the union as a float32, as jaccard.py:36-37 sums it:
    the same number up to 2^24 pixels of union)."""
    c = counts.cpu().numpy() if _is_tensor(counts) else np.asarray(counts)
    if c.ndim != 3 or c.shape[2] != N_COUNTS:
        raise ValueError(f"counts are [T,n_obj,{N_COUNTS}], not {c.shape}")
    T, n_obj = c.shape[:2]
    J, F = np.empty((n_obj, T), dtype=np.float64), np.empty((n_obj, T), dtype=np.float64)
    for t in range(T):
        for o in range(n_obj):
            k = [int(v) for v in c[t, o]]
            J[o, t] = _j_from(k[0], k[1])
            F[o, t] = _f_from(k[2], k[3], k[4], k[5])
    return J, F


def db_eval_iou(annotation, segmentation):
    """The reference's name and argument order (jaccard.py:15): binary annotation, binary segmentation -> J."""
    a, s = (np.asarray(x).astype(bool) for x in (annotation, segmentation))
    if a.shape != s.shape:
        raise ValueError(f"annotation {a.shape} and segmentation {s.shape} differ in shape (resizing is out of scope)")
    c = clip_counts(s.astype(np.uint8), a.astype(np.uint8), 1, radius=0)
    return float(scores_from_counts(c)[0][0, 0])


def db_eval_boundary(foreground_mask, gt_mask, bound_th=0.008):
    """The reference's name and argument order (f_boundary.py:14): binary segmentation FIRST, binary annotation second -> F."""
    s, a = (np.asarray(x).astype(bool) for x in (foreground_mask, gt_mask))
    if a.shape != s.shape:
        raise ValueError(f"foreground_mask {s.shape} and gt_mask {a.shape} differ in shape (resizing is out of scope)")
    c = clip_counts(s.astype(np.uint8), a.astype(np.uint8), 1, bound_th=bound_th)
    return float(scores_from_counts(c)[1][0, 0])


# ---- statistics (statistics.py) -------------------------------------------------------------------------------------------
def mean(X):
    """Average ignoring NaN."""
    return np.nanmean(X)


def recall(X, threshold=0.5):
    """Fraction of the values above ``threshold``."""
    return mean(np.array(X) > threshold)


def decay(X, n_bins=4):
    """Performance loss over time: the mean of the first quarter minus the mean of the last (statistics.py:22-29, which
    always reads four bins).  The reference casts its bin indices to 8 bits; this does not, so the two are identical for
    sequences of up to 255 scored frames and this one stays right beyond."""
    ids = np.round(np.linspace(1, len(X), n_bins + 1) + 1e-10) - 1
    ids = ids.astype(np.int64)
    D_bins = [X[ids[i]:ids[i + 1] + 1] for i in range(0, 4)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        return np.nanmean(D_bins[0]) - np.mean(D_bins[3])


def std(X):
    """Standard deviation."""
    return np.std(X)


_statistics = {"decay": decay, "mean": mean, "recall": recall, "std": std}


def sequence_results(raw):
    """evaluation.py:44-56 for one measure: ``raw`` [n_obj,T] scores of ALL frames of a sequence -> {'raw': per object the
    scores of frames 1 .. T-2 with NaN at both ends (T values again), 'decay' / 'mean' / 'recall' / 'std': one float per
    object over frames 1 .. T-2}.  The first frame is given and the last is not annotated for scoring: the reference never
    scores either."""
    raw = np.asarray(raw, dtype=np.float64)
    if raw.ndim != 2:
        raise ValueError(f"raw is [n_obj,T], not {raw.shape}")
    scored = [[float(v) for v in r[1:-1]] for r in raw]
    results = {"raw": [[np.nan] + r + [np.nan] for r in scored]}
    for stat, fn in _statistics.items():
        results[stat] = [float(fn(r)) for r in scored]
    return results


# ---- the frame loop's callback ----------------------------------------------------------------------------------------------
class ClipScorer:
    """Scores label maps against ``gt_labels`` [B,T,H,W] (uint8, on the device) as they are produced.  ``scorer(b, t, labels)``
    -- the signature of ``FrameLoop.run(on_labels=...)`` -- is one entry call into row (b, t) of a device table [B,T,n_obj,6],
    on the current stream (the stream the callback runs under), with no synchronisation; (b, t) pairs never scored stay zero,
    which reads as "both empty".  ``results()`` synchronises once."""

    def __init__(self, gt_labels, n_obj: int, radius=None, bound_th=0.008):
        import torch
        if not (_is_tensor(gt_labels) and gt_labels.is_cuda and gt_labels.dim() == 4 and gt_labels.dtype == torch.uint8):
            raise ValueError("gt_labels is a uint8 device tensor [B,T,H,W]")
        self.gt = gt_labels.contiguous()
        self.n_obj = int(n_obj)
        self.radius = boundary_radius(gt_labels.shape, bound_th) if radius is None else int(radius)
        B, T = gt_labels.shape[:2]
        self.counts = torch.zeros((B, T, self.n_obj, N_COUNTS), dtype=torch.int32, device=gt_labels.device)

    def __call__(self, b: int, t: int, labels) -> None:
        if tuple(labels.shape) != tuple(self.gt.shape[2:]):
            raise ValueError(f"labels {tuple(labels.shape)} and the annotation {tuple(self.gt.shape[2:])} differ in shape")
        if str(labels.dtype) != "torch.uint8":
            raise ValueError(f"labels must be uint8, not {labels.dtype}")
        _counts_into(labels.unsqueeze(0), self.gt[b, t].unsqueeze(0), self.n_obj, self.radius, self.counts[b, t].unsqueeze(0))

    def results(self):
        """-> one dict per video: {'J': [n_obj,T], 'F': [n_obj,T], 'J_seq': sequence_results(J), 'F_seq': sequence_results(F)}."""
        table = self.counts.cpu().numpy()                  # the one synchronisation
        out = []
        for b in range(table.shape[0]):
            J, F = scores_from_counts(table[b])
            out.append({"J": J, "F": F, "J_seq": sequence_results(J), "F_seq": sequence_results(F)})
        return out
