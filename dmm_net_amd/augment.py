"""The augmentation of training clips on the device: the reference's flip and nearest-neighbour affine warp of the image, the
annotation and every pasted proposal mask (dmm/dataloader/dataset.py:222-258), the proposals' boxes from their warped masks and
the target rows of ``sequence_from_masks`` (dataset.py:300-338), all from ONE pass over the output pixels
(``dmm_augment_clip_f32``, include/dmm_match.h (15): at most three launches, no host read, capturable).

``affine_matrix`` builds a frame's matrix the way the reference's lazy ``RandomAffine`` chain does (bit-equal for the same
parameters), ``draw_clip_params`` draws a clip's parameters in the reference's order, ``augment_clip`` runs the entry.  Build
the dataset with ``augment=False``, upload the raw clip, and call ``augment_clip`` after collate.

Deviation from the reference: label 0 is ALWAYS background here.  On a frame with no background pixel at all the reference's
``np.unique(annot)[1:]`` (dataset.py:311) drops the smallest object id instead; that quirk is not reproduced.

The frames it takes -- resized, ``ToTensor``'d and normalised -- come from ``frames.ClipPreparer`` (include/dmm_match.h (16)).

Out of scope: the transform library's bilinear mode (the reference's datasets always pass ``interp='nearest'``), image decode
and ``random_select_frames``.
"""
from __future__ import annotations

import math

from . import _lib


def affine_matrix(rotation, translation, shear, zoom, H, W):
    """Rotate . Translate . Shear . Zoom -> torch.FloatTensor [3,3] on the CPU: ``rotation`` and ``shear`` in degrees,
    ``translation`` = (fraction of H, fraction of W) (``Translate`` scales by ``size(1)`` and ``size(2)``), ``zoom`` = (zx, zy).
    The entries and the fp32 ``mm`` chain are the reference's (transforms.py:84-90, 300-303, 456-461, 573-576, 715-718)."""
    import torch
    theta = math.pi / 180 * rotation
    rot = torch.FloatTensor([[math.cos(theta), -math.sin(theta), 0],
                             [math.sin(theta), math.cos(theta), 0],
                             [0, 0, 1]])
    th, tw = (translation, translation) if not isinstance(translation, (tuple, list)) else translation
    tra = torch.FloatTensor([[1, 0, th * H],
                             [0, 1, tw * W],
                             [0, 0, 1]])
    theta = (math.pi * shear) / 180
    she = torch.FloatTensor([[1, -math.sin(theta), 0],
                             [0, math.cos(theta), 0],
                             [0, 0, 1]])
    zx, zy = (zoom, zoom) if not isinstance(zoom, (tuple, list)) else zoom
    zoo = torch.FloatTensor([[zx, 0, 0],
                             [0, zy, 0],
                             [0, 0, 1]])
    return rot.mm(tra).mm(she).mm(zoo)


def draw_clip_params(rng, T, rotation=10, translation=0.1, shear=0.1, zoom=(0.7, 1.4), *, H, W):
    """One clip's draws from ``rng`` (a ``random.Random``) in the reference's order: the flip (``rng.random() < 0.5``), then per
    frame the rotation, the height and width translations, the shear and the two zooms with ``rng.uniform`` -- ``1 + 6 T``
    draws.  The defaults are the reference's (args.py:98-101, with the zoom range of davis2017.py:89).  ``H``, ``W``: the frame
    size the translations scale with.  -> (flip, matrices [T,3,3] fp32 on the CPU)."""
    import torch
    th, tw = (translation, translation) if not isinstance(translation, (tuple, list)) else translation
    flip = rng.random() < 0.5
    mats = []
    for _ in range(T):
        deg = rng.uniform(-rotation, rotation)
        dh = rng.uniform(-th, th)
        dw = rng.uniform(-tw, tw)
        sh = rng.uniform(-shear, shear)
        zx = rng.uniform(zoom[0], zoom[1])
        zy = rng.uniform(zoom[0], zoom[1])
        mats.append(affine_matrix(deg, (dh, dw), sh, (zx, zy), H, W))
    return flip, (torch.stack(mats) if mats else torch.zeros((0, 3, 3)))


class AugmentedClip:
    """What ``augment_clip`` returns: ``frames`` [n,C,H,W] fp32, ``labels`` [n,H,W] uint8, ``masks`` [n,P,H,W] fp32, ``boxes``
    [n,P,4] fp32 xyxy, ``box_valid`` [n,P] int32 (0: the warped mask is empty and the input box was kept), ``targets``
    [n,F,H,W] fp32 and ``sizes`` [n,F] int32 -- device tensors, valid once the stream has run."""
    __slots__ = ("frames", "labels", "masks", "boxes", "box_valid", "targets", "sizes")

    def __init__(self, frames, labels, masks, boxes, box_valid, targets, sizes):
        self.frames, self.labels, self.masks, self.boxes = frames, labels, masks, boxes
        self.box_valid, self.targets, self.sizes = box_valid, targets, sizes

    @property
    def sw(self):
        """The "object present" weights, fp32 [n,F]: (sizes > 0), computed on the device."""
        return (self.sizes > 0).float()

    def reference_targets(self):
        """fp32 [n,F,HW + 1]: the layout ``sequence_from_masks`` returns and trainer.py slices -- the HW target values of
        each object, then its ``sw``."""
        n, F = self.sizes.shape
        import torch
        return torch.cat([self.targets.reshape(n, F, -1), self.sw.unsqueeze(2)], dim=2)


def _strided(x, dense_dims):
    """``x`` as the ABI can address it: the last two dimensions dense rows, strides before them at least a plane (a stride of
    a dimension of size 1 is free); otherwise a contiguous copy."""
    H, W = x.shape[-2:]
    ok = H * W == 0 or ((W == 1 or x.stride(-1) == 1) and (H == 1 or x.stride(-2) == W))
    for d in range(dense_dims):
        ok = ok and (x.shape[d] <= 1 or x.stride(d) >= H * W)
    return x if ok else x.contiguous()


def _stride(x, d):
    H, W = x.shape[-2:]
    return x.stride(d) if x.shape[d] > 1 else H * W * (x.shape[1] if d == 0 and x.dim() == 4 else 1)


def augment_clip(frames, labels, masks=None, boxes=None, *, matrices, flip, max_obj=5, out=None):
    """Warp ``n`` frames, each by its own matrix.  ``frames`` [n,C,H,W] fp32, ``labels`` [n,H,W] uint8, ``masks`` [n,P,H,W]
    fp32 soft masks with their ``boxes`` [n,P,4] fp32 xyxy (both None: no proposals), ``matrices`` [n,3,3] fp32 (host or
    device), ``flip`` a bool or [n] (the reference flips a whole clip), ``max_obj`` = F, the target planes per frame
    (``maxseqlen``).  Non-contiguous views are taken as they are where their strides fit the ABI and copied otherwise; the
    inputs are never written.  ``out``: a previous result for the same shapes, written again (a captured graph replays it).
    Runs on the current stream without synchronising.  -> ``AugmentedClip``."""
    import torch
    for name, x in (("frames", frames), ("labels", labels), ("masks", masks), ("boxes", boxes)):
        if x is not None and not x.is_cuda:
            raise _lib.DmmError(f"dmm_net_amd.augment needs tensors on an MI355X device (no CPU fallback): {name} is on the host")
    if frames.dim() != 4 or frames.dtype != torch.float32:
        raise ValueError(f"frames are fp32 [n,C,H,W], not {frames.dtype} {tuple(frames.shape)}")
    n, C, H, W = frames.shape
    if tuple(labels.shape) != (n, H, W) or labels.dtype != torch.uint8:
        raise ValueError(f"labels are uint8 {(n, H, W)}, not {labels.dtype} {tuple(labels.shape)}")
    if (masks is None) != (boxes is None):
        raise ValueError("masks and boxes come together")
    dev = frames.device
    if masks is None:
        masks = torch.empty((n, 0, H, W), dtype=torch.float32, device=dev)
        boxes = torch.empty((n, 0, 4), dtype=torch.float32, device=dev)
    if masks.dim() != 4 or tuple(masks.shape[0:1] + masks.shape[2:]) != (n, H, W) or masks.dtype != torch.float32:
        raise ValueError(f"masks are fp32 [n,P,H,W] with n, H, W = {(n, H, W)}, not {masks.dtype} {tuple(masks.shape)}")
    P, F = masks.shape[1], int(max_obj)
    if tuple(boxes.shape) != (n, P, 4) or boxes.dtype != torch.float32:
        raise ValueError(f"boxes are fp32 {(n, P, 4)}, not {boxes.dtype} {tuple(boxes.shape)}")
    if F < 0:
        raise ValueError("max_obj is negative")
    matrices = torch.as_tensor(matrices)
    if tuple(matrices.shape) != (n, 3, 3):
        raise ValueError(f"matrices are [n,3,3] with n = {n}, not {tuple(matrices.shape)}")
    matrices = matrices.to(device=dev, dtype=torch.float32, non_blocking=True).contiguous()
    if isinstance(flip, (bool, int)):
        flips = None if not flip else torch.ones(n, dtype=torch.int32, device=dev)
    else:
        flips = torch.as_tensor(flip)
        if tuple(flips.shape) != (n,):
            raise ValueError(f"flip is a bool or [n] with n = {n}, not {tuple(flips.shape)}")
        flips = (flips != 0).to(device=dev, dtype=torch.int32, non_blocking=True).contiguous()

    frames, labels, masks = _strided(frames, 2), _strided(labels, 1), _strided(masks, 2)
    boxes = boxes.contiguous()
    if out is None:
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        out = AugmentedClip(e((n, C, H, W), torch.float32), e((n, H, W), torch.uint8), e((n, P, H, W), torch.float32),
                            e((n, P, 4), torch.float32), e((n, P), torch.int32), e((n, F, H, W), torch.float32),
                            e((n, F), torch.int32))
    else:
        want = {"frames": (n, C, H, W), "labels": (n, H, W), "masks": (n, P, H, W), "boxes": (n, P, 4), "box_valid": (n, P),
                "targets": (n, F, H, W), "sizes": (n, F)}
        for k, shape in want.items():
            t = getattr(out, k)
            if tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
                raise ValueError(f"out.{k} is {tuple(t.shape)} on {t.device}, not a contiguous {shape} on {dev}")
    if n == 0 or H * W == 0:                               # the entry has nothing to do: no pixel, so no mask pixel either
        out.boxes.copy_(boxes)
        out.box_valid.zero_()
        out.sizes.zero_()
        return out

    L = _lib.load()
    need = L.dmm_augment_clip_workspace_bytes(n, C, P, F, H, W)
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    stream = torch.cuda.current_stream(dev).cuda_stream
    HW = H * W
    _lib.call("dmm_augment_clip_f32", dev,
              ptr(frames), _stride(frames, 0), _stride(frames, 1), ptr(out.frames), C * HW, HW,
              ptr(labels), _stride(labels, 0), ptr(out.labels), HW,
              ptr(masks), _stride(masks, 0), _stride(masks, 1), ptr(out.masks), P * HW, HW,
              ptr(boxes), ptr(out.boxes), ptr(out.box_valid), ptr(out.targets), ptr(out.sizes),
              ptr(matrices), ptr(flips), n, C, P, F, H, W, ptr(ws), need, stream)
    return out
