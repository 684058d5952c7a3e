"""The DAVIS scores of a clip: region similarity J and boundary accuracy F per object and frame, then mean, recall and decay
per sequence -- the reference's dmm/measures/jaccard.py, f_boundary.py and statistics.py as dmm/dataloader/evaluation.py:31-58
and tools/davis_eval.py drive them.

Both measures are ratios of integer counts.  ``clip_counts`` produces the six counts per (frame, object)
(include/dmm_match.h (14)): on the device through ``dmm_davis_counts_u8`` (two launches, no host read, capturable), on the host
through the numpy / ``scipy.ndimage`` form written here -- same semantics, same integers.  ``scores_from_counts`` turns the
integers into the reference's floats with the reference's divisions and case analysis, so J and F equal its values bit for
bit.  ``ClipScorer`` is the callback for ``video.FrameLoop.run(on_labels=...)``: one entry call per frame into a device table,
one synchronisation in ``results()``.

A prediction whose size differs from the annotation's is scored the way the reference scores it when ``resize=True`` (or
``ClipScorer(pred_size=...)``) asks for it: both measures first resize the prediction to the annotation's shape with
``Image.resize((w, h), Image.NEAREST)`` (jaccard.py:28-32, f_boundary.py:34-38).  That is PIL's ``ImagingScaleAffine``, which
walks the source coordinate by repeated double additions; ``nearest_table`` is that rule in numpy, and include/dmm_match.h
(14b) and (14d) are its device forms: the index tables, and one gather pass into a frame of the annotation's size that (14)
then scores.  Without the argument, differing shapes raise ``ValueError`` as before.

Out of scope, as in the C entries: the T measure.
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


# ---- the nearest resize ---------------------------------------------------------------------------------------------------
def nearest_table(n_in: int, n_out: int) -> np.ndarray:
    """The source index of each of ``n_out`` destination samples of an axis of ``n_in``: int32 [n_out], the rule of
    include/dmm_match.h (14b) -- ``a = n_in / n_out`` in double, ``o = a * 0.5``, then ``tab[i] = int(o); o += a`` with the
    additions made ONE AFTER THE OTHER (``np.add.accumulate`` adds in sequence).  This is what PIL's NEAREST resize does; it
    is not ``floor((i + 0.5) * n_in / n_out)``, which differs from it by one on many size pairs (448 -> 854 among them)."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 0 or n_out < 0:
        raise ValueError("negative axis length")
    if n_out == 0:
        return np.zeros(0, dtype=np.int32)
    a = np.float64(n_in) / np.float64(n_out)
    steps = np.full(n_out, a, dtype=np.float64)
    steps[0] = a * 0.5
    o = np.add.accumulate(steps)
    return np.where(o < 0, -1, o.astype(np.int64)).astype(np.int32)


def resize_labels_host(labels: np.ndarray, size) -> np.ndarray:
    """numpy [..,Hs,Ws] -> [..,H,W]: ``out[.., y, x] = labels[.., tab_y[y], tab_x[x]]``, 0 where an index leaves the source."""
    labels = np.asarray(labels)
    H, W = (int(v) for v in size)
    Hs, Ws = labels.shape[-2:]
    ty, tx = nearest_table(Hs, H), nearest_table(Ws, W)
    ok = ((ty >= 0) & (ty < Hs))[:, None] & ((tx >= 0) & (tx < Ws))[None, :]
    out = np.zeros(labels.shape[:-2] + (H, W), dtype=labels.dtype)
    if Hs * Ws and H * W:
        out[...] = np.where(ok, labels[..., np.clip(ty, 0, Hs - 1)[:, None], np.clip(tx, 0, Ws - 1)[None, :]], 0)
    return out


def nearest_tables(pred_size, size, device):
    """(14b): the two index tables of one size pair as ONE int32 device tensor [H + W] (rows, then columns), on the current
    stream.  Build it once per size pair and hand it to every call that resizes."""
    import torch
    from . import _lib
    (Hs, Ws), (H, W) = (tuple(int(v) for v in s) for s in (pred_size, size))
    tables = torch.empty((H + W,), dtype=torch.int32, device=device)
    _lib.call("dmm_nearest_index_tables_i32", tables.device, Hs, Ws, H, W, tables.data_ptr() if H + W else None,
              torch.cuda.current_stream(tables.device).cuda_stream)
    return tables


def _dense_frames(x):
    """A device tensor [T,H,W] -> (the tensor with dense rows, its frame stride in elements)."""
    T, H, W = x.shape
    if T and H * W and (x.stride(2) != 1 or x.stride(1) != W or (T > 1 and x.stride(0) < H * W)):
        x = x.contiguous()
    return x, (x.stride(0) if T > 1 and H * W else H * W)


def resize_labels_device(labels, size, tables=None):
    """(14d) on a uint8 device tensor [T,Hs,Ws] -> a new [T,H,W], on the current stream without synchronising.  ``tables`` =
    ``nearest_tables((Hs, Ws), size, device)`` when the caller keeps them; else they are built here (one more launch)."""
    import torch
    from . import _lib
    H, W = (int(v) for v in size)
    T, Hs, Ws = labels.shape
    if T * H * W == 0 or Hs * Ws == 0:                      # nothing to write, or nothing to read: every index leaves the source
        return torch.zeros((T, H, W), dtype=torch.uint8, device=labels.device)
    if tables is None:
        tables = nearest_tables((Hs, Ws), (H, W), labels.device)
    if not (tables.numel() == H + W and tables.dtype == torch.int32 and tables.device == labels.device):
        raise ValueError(f"tables are int32 [{H + W}] on {labels.device}: nearest_tables(({Hs}, {Ws}), ({H}, {W}), device)")
    src, fs = _dense_frames(labels)
    out = torch.empty((T, H, W), dtype=torch.uint8, device=labels.device)
    _lib.call("dmm_resize_labels_nearest_u8", labels.device, src.data_ptr(), Hs, Ws, fs, out.data_ptr(), H, W, H * W,
              tables.data_ptr(), T, torch.cuda.current_stream(labels.device).cuda_stream)
    return out


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


def _label_maps(pred, gt, resize=False):
    if not resize and tuple(pred.shape) != tuple(gt.shape):
        raise ValueError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ in shape (resize=True resizes the "
                         "prediction as the reference does)")
    if len(pred.shape) != len(gt.shape) or tuple(pred.shape[:-2]) != tuple(gt.shape[:-2]):
        raise ValueError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ in their frames")
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
    (pred, fs_pred), (gt, fs_gt) = _dense_frames(pred), _dense_frames(gt)
    stream = torch.cuda.current_stream(pred.device).cuda_stream
    L = _lib.load()
    need = L.dmm_davis_counts_workspace_bytes(T, n_obj, H, W, radius)
    ws = torch.empty(need, dtype=torch.uint8, device=pred.device) if need else None
    _lib.call("dmm_davis_counts_u8", pred.device, pred.data_ptr(), gt.data_ptr(), T, n_obj, H, W, fs_pred, fs_gt, radius,
              counts.data_ptr(), None if ws is None else ws.data_ptr(), need, stream)


def clip_counts(pred, gt, n_obj: int, radius=None, bound_th=0.008, resize=False):
    """The six counts of every (frame, object): uint8 label maps [T,H,W] or [H,W] (0 = background, o + 1 = object o; labels
    above ``n_obj`` belong to no object) -> int32 [T,n_obj,6] in the order of include/dmm_match.h (14).  CUDA tensors go
    through the device entry on the current stream without synchronising and give a device tensor; host tensors and numpy
    arrays go through the numpy / scipy form and give what they were (a tensor or an array).  ``radius`` None: the
    reference's ``bound_pix`` for this frame size and ``bound_th`` (``boundary_radius``).

    ``resize=True`` accepts a prediction [..,Hs,Ws] of another size than the annotation [..,H,W] and scores it as the
    reference does: resized to H x W by PIL's NEAREST rule (``nearest_table``), on the device through (14b) and (14d) into
    a buffer that (14) then reads, on the host through ``resize_labels_host``; at equal sizes it changes nothing.  Each
    device call builds the index tables again (one more launch, a serial walk of H + W additions): a caller that scores
    many clips of one size pair keeps them instead -- ``ClipScorer(pred_size=...)``, or ``nearest_tables`` with
    ``resize_labels_device`` and the equal-size call.  The reference takes ``bound_pix`` from the prediction's shape BEFORE
    it resizes (f_boundary.py:30-31), so ``radius`` None is ``boundary_radius(pred.shape)`` here too: 5 for a 255 x 448
    prediction, not the 8 of its 480 x 854 annotation.  To score with the annotation's radius, as the official DAVIS
    toolkit does, pass ``radius=boundary_radius(gt.shape)``."""
    _label_maps(pred, gt, resize)
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
        if tuple(p3.shape[1:]) != tuple(g3.shape[1:]):
            p3 = resize_labels_device(p3, g3.shape[1:])
        _counts_into(p3, g3, n_obj, r, counts)
        return counts
    p, g = (np.asarray(x.numpy() if _is_tensor(x) else x) for x in (pred, gt))
    p3, g3 = (x if x.ndim == 3 else x[None] for x in (p, g))
    if p3.shape[1:] != g3.shape[1:]:
        p3 = resize_labels_host(p3, g3.shape[1:])
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


def db_eval_iou(annotation, segmentation, resize=False):
    """The reference's name and argument order (jaccard.py:15): binary annotation, binary segmentation -> J.  ``resize=True``:
    a segmentation of another shape is resized to the annotation's first, as jaccard.py:28-32 does."""
    a, s = (np.asarray(x).astype(bool) for x in (annotation, segmentation))
    if a.shape != s.shape and not resize:
        raise ValueError(f"annotation {a.shape} and segmentation {s.shape} differ in shape (resize=True resizes the "
                         "segmentation as the reference does)")
    c = clip_counts(s.astype(np.uint8), a.astype(np.uint8), 1, radius=0, resize=resize)
    return float(scores_from_counts(c)[0][0, 0])


def db_eval_boundary(foreground_mask, gt_mask, bound_th=0.008, resize=False):
    """The reference's name and argument order (f_boundary.py:14): binary segmentation FIRST, binary annotation second -> F.
    ``resize=True``: a segmentation of another shape is resized to the annotation's first, as f_boundary.py:34-38 does, and
    ``bound_pix`` comes from the segmentation's shape before the resize, as f_boundary.py:30-31 takes it."""
    s, a = (np.asarray(x).astype(bool) for x in (foreground_mask, gt_mask))
    if a.shape != s.shape and not resize:
        raise ValueError(f"foreground_mask {s.shape} and gt_mask {a.shape} differ in shape (resize=True resizes the "
                         "segmentation as the reference does)")
    c = clip_counts(s.astype(np.uint8), a.astype(np.uint8), 1, bound_th=bound_th, resize=resize)
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


def dataset_results(per_video):
    """evaluation.py:104-108: the dataset's figures from its sequences'.  ``per_video``: one entry per sequence (a list, or a
    dict by sequence name), each ``{'J_seq': sequence_results(J), 'F_seq': sequence_results(F)}`` as ``ClipScorer.results()``
    gives them -> ``{'J': {'mean', 'recall', 'decay'}, 'F': {...}}``, each ``float(np.mean(np.hstack(...)))`` over the
    sequences' per-object values -- every object of every sequence weighs the same.  Host only."""
    videos = list(per_video.values()) if isinstance(per_video, dict) else list(per_video)
    if not videos:
        raise ValueError("no sequences")
    out = {}
    for measure in ("J", "F"):
        out[measure] = {}
        for statistic in ("mean", "recall", "decay"):
            raw_data = np.hstack([v[measure + "_seq"][statistic] for v in videos])
            out[measure][statistic] = float(np.mean(raw_data))
    return out


# ---- the frame loop's callback ----------------------------------------------------------------------------------------------
class ClipScorer:
    """Scores label maps against ``gt_labels`` [B,T,H,W] (uint8, on the device) as they are produced.  ``scorer(b, t, labels)``
    -- the signature of ``FrameLoop.run(on_labels=...)`` -- is one entry call into row (b, t) of a device table [B,T,n_obj,6]
    (after one resize call, with ``pred_size``),
    on the current stream (the stream the callback runs under), with no synchronisation; (b, t) pairs never scored stay zero,
    which reads as "both empty".  ``results()`` synchronises once.

    ``pred_size=(Hs, Ws)``: the labels arrive at that size (the model's) and are scored against the annotation's H x W as
    ``clip_counts(resize=True)`` scores them.  The index tables are built once, here; ``radius`` None is then
    ``boundary_radius(pred_size)``, the reference's quirk (``clip_counts``)."""

    def __init__(self, gt_labels, n_obj: int, radius=None, bound_th=0.008, pred_size=None):
        import torch
        if not (_is_tensor(gt_labels) and gt_labels.is_cuda and gt_labels.dim() == 4 and gt_labels.dtype == torch.uint8):
            raise ValueError("gt_labels is a uint8 device tensor [B,T,H,W]")
        self.gt = gt_labels.contiguous()
        self.n_obj = int(n_obj)
        self.size = tuple(int(v) for v in (gt_labels.shape[2:] if pred_size is None else pred_size))
        if len(self.size) != 2 or min(self.size) < 0:
            raise ValueError(f"pred_size is (Hs, Ws), not {pred_size!r}")
        self.radius = boundary_radius(self.size, bound_th) if radius is None else int(radius)
        self.tables = None
        if self.size != tuple(gt_labels.shape[2:]):
            self.tables = nearest_tables(self.size, gt_labels.shape[2:], gt_labels.device)
        B, T = gt_labels.shape[:2]
        self.counts = torch.zeros((B, T, self.n_obj, N_COUNTS), dtype=torch.int32, device=gt_labels.device)

    def __call__(self, b: int, t: int, labels) -> None:
        if tuple(labels.shape) != self.size:
            raise ValueError(f"labels {tuple(labels.shape)} are not of the scorer's size {self.size} (the annotation's "
                             f"{tuple(self.gt.shape[2:])}; pred_size= names another)")
        if str(labels.dtype) != "torch.uint8":
            raise ValueError(f"labels must be uint8, not {labels.dtype}")
        labels = labels.unsqueeze(0)
        if self.tables is not None:
            labels = resize_labels_device(labels, self.gt.shape[2:], self.tables)
        _counts_into(labels, self.gt[b, t].unsqueeze(0), self.n_obj, self.radius, self.counts[b, t].unsqueeze(0))

    def results(self):
        """-> one dict per video: {'J': [n_obj,T], 'F': [n_obj,T], 'J_seq': sequence_results(J), 'F_seq': sequence_results(F)}."""
        table = self.counts.cpu().numpy()                  # the one synchronisation
        out = []
        for b in range(table.shape[0]):
            J, F = scores_from_counts(table[b])
            out.append({"J": J, "F": F, "J_seq": sequence_results(J), "F_seq": sequence_results(F)})
        return out
