"""Frames as the encoders take them, from decoded images, on the device: PIL's resize of an 8-bit RGB frame, then
``ToTensor`` and ``Normalize`` -- what the reference's dataset workers do per frame (dmm/dataloader/dataset.py:202-219 with the
transforms composed at train.py:76-77 and eval.py:51-52), through ``dmm_prepare_frames_u8`` / ``dmm_prepare_frames_nearest_u8``
(include/dmm_match.h (16): at most two launches, no host read, capturable).

For 8-bit images PIL's resize is integer arithmetic on fixed-point coefficient tables with a ``uint8`` rounding between its
horizontal and its vertical pass, and ``ToTensor`` + ``Normalize`` of a ``uint8`` has 256 possible values per channel: the
device result equals the host pipeline bit for bit.  ``resample_tables`` forms PIL's tables, ``normalise_lut`` the 3 x 256
values with torch's own operations in the reference's order, ``resize_frames_host`` is the rule in numpy (the CPU tests'
subject and the device tests' second witness), ``prepare_frames`` runs the entry and ``ClipPreparer`` keeps the tables, the
look-up table and the workspace of one size pair and resizes the annotation beside the frames (``measures.
resize_labels_device``).  Build the dataset with ``inputRes=None, transform=None``, upload the decoded ``uint8`` frames, then
``ClipPreparer`` followed by ``augment_clip``.

Which filter the reference ran is the caller's choice: ``img.resize(size)`` without a filter is BICUBIC on Pillow from 7.0 on
and was NEAREST before (the authors' 2019 environment most likely), so all three are here.

Out of scope: JPEG decode, PIL's BOX / HAMMING / LANCZOS filters, ``reducing_gap``, non-RGB modes, bf16 or channels-last
outputs.
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib
from .measures import nearest_table, nearest_tables, resize_labels_device

FILTERS = ("nearest", "bilinear", "bicubic")
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
PRECISION_BITS = 22          # 32 - 8 - 2: PIL's fixed point for 8-bit channels


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_SUPPORT = {"bilinear": (_bilinear, 1.0), "bicubic": (_bicubic, 2.0)}


def _check_filter(filter):
    if filter not in FILTERS:
        raise ValueError(f"filter is one of {FILTERS}, not {filter!r}")
    return filter


def resample_tables(n_in, n_out, filter):
    """PIL's coefficient tables of one axis (``precompute_coeffs`` + ``normalize_coeffs_8bpc``), in IEEE double and in the
    order include/dmm_match.h (16) states -> (bounds int32 [n_out,2] = (lo, cnt), coef int32 [n_out,ksize]).  Pure host."""
    n_in, n_out = int(n_in), int(n_out)
    if filter not in _SUPPORT:
        raise ValueError(f"resample_tables: filter is 'bilinear' or 'bicubic', not {filter!r}")
    if n_in <= 0 or n_out <= 0:
        raise ValueError(f"resample_tables: axis lengths are positive, not {n_in} -> {n_out}")
    fn, filter_support = _SUPPORT[filter]
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = filter_support * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    coef = np.zeros((n_out, ksize), dtype=np.int32)
    one = float(1 << PRECISION_BITS)
    for i in range(n_out):
        center = (i + 0.5) * scale
        ss = 1.0 / fs
        lo = max(int(center - support + 0.5), 0)           # (int() truncates toward zero, as the C cast does)
        cnt = min(int(center + support + 0.5), n_in) - lo
        w = [fn((k + lo - center + 0.5) * ss) for k in range(cnt)]
        ww = 0.0
        for v in w:                                        # left to right (sum() compensates on newer Pythons)
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        coef[i, :cnt] = [int(v * one + 0.5) if v >= 0 else int(v * one - 0.5) for v in w]
        bounds[i] = (lo, cnt)
    return bounds, coef


def normalise_lut(mean=MEAN, std=STD):
    """fp32 [3,256] on the CPU: ``ToTensor`` then ``Normalize`` of every byte value, with torch's own operations in the
    reference's order -- ``byte.float().div(255)``, then ``.sub(mean[c]).div(std[c])`` with fp32 ``mean`` / ``std``."""
    import torch
    mean, std = (torch.as_tensor(v, dtype=torch.float32).reshape(-1) for v in (mean, std))
    if mean.numel() != 3 or std.numel() != 3:
        raise ValueError("mean and std have one value per RGB channel")
    v = torch.arange(256, dtype=torch.uint8).float().div(255)
    return v[None, :].repeat(3, 1).sub(mean[:, None]).div(std[:, None]).contiguous()


def _pass_host(x, axis, n_out, filter):
    """One pass of the rule along ``axis`` of a uint8 array."""
    bounds, coef = resample_tables(x.shape[axis], n_out, filter)
    idx = np.minimum(bounds[:, :1].astype(np.int64) + np.arange(coef.shape[1]), x.shape[axis] - 1)     # (cnt .. : coef is 0)
    taps = np.moveaxis(np.take(x, idx, axis=axis), (axis, axis + 1), (-2, -1)).astype(np.int64)        # [.., n_out, ksize]
    acc = (1 << (PRECISION_BITS - 1)) + (taps * coef.astype(np.int64)).sum(-1)
    return np.moveaxis(np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8), -1, axis)


def resize_frames_host(frames_u8, size, filter="bicubic"):
    """numpy uint8 [..,Hs,Ws,3] -> [..,H,W,3]: the rule of include/dmm_match.h (16) -- ``Image.resize((W, H), filter)`` of
    every frame, bit for bit.  The horizontal pass first, the uint8 rounding between the passes, a pass whose axis keeps its
    size skipped; ``nearest`` through ``measures.nearest_table``, an index outside the source reading as 0."""
    x = np.asarray(frames_u8)
    _check_filter(filter)
    if x.dtype != np.uint8 or x.ndim < 3 or x.shape[-1] != 3:
        raise ValueError(f"frames are uint8 [..,Hs,Ws,3], not {x.dtype} {x.shape}")
    H, W = (int(v) for v in size)
    Hs, Ws = x.shape[-3:-1]
    if H < 0 or W < 0:
        raise ValueError("negative size")
    if filter == "nearest":
        ty, tx = nearest_table(Hs, H), nearest_table(Ws, W)
        ok = ((ty >= 0) & (ty < Hs))[:, None] & ((tx >= 0) & (tx < Ws))[None, :]
        out = np.zeros(x.shape[:-3] + (H, W, 3), dtype=np.uint8)
        if Hs * Ws and H * W:
            out[...] = np.where(ok[..., None], x[..., np.clip(ty, 0, Hs - 1)[:, None], np.clip(tx, 0, Ws - 1)[None, :], :], 0)
        return out
    if H * W == 0 or int(np.prod(x.shape[:-3])) == 0:
        return np.zeros(x.shape[:-3] + (H, W, 3), dtype=np.uint8)
    if Hs * Ws == 0:
        raise ValueError("an empty image has nothing to resample")
    if Ws != W:
        x = _pass_host(x, x.ndim - 2, W, filter)
    if Hs != H:
        x = _pass_host(x, x.ndim - 3, H, filter)
    return np.ascontiguousarray(x)


class FrameTables:
    """The device tables of one size pair and filter: ``bounds_x`` / ``coef_x`` (Ws -> W) and ``bounds_y`` / ``coef_y``
    (Hs -> H), each None when its axis keeps its size, or ``nearest`` (int32 [H + W], (14b)); and ``lut``, fp32 [3,256].
    Read-only once built: every call for the pair can share them."""

    def __init__(self, src_size, size, filter="bicubic", mean=MEAN, std=STD, device="cuda"):
        import torch
        (Hs, Ws), (H, W) = (tuple(int(v) for v in s) for s in (src_size, size))
        if min(Hs, Ws, H, W) < 0:
            raise ValueError("negative size")
        self.src_size, self.size, self.filter = (Hs, Ws), (H, W), _check_filter(filter)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.DmmError("dmm_net_amd.frames needs an MI355X device (no CPU fallback): the tables live on the device")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.bounds_x = self.coef_x = self.bounds_y = self.coef_y = self.nearest = None
        self.ksize_x = self.ksize_y = 0
        specs = [(normalise_lut(mean, std).reshape(-1).numpy(), torch.float32)]
        if filter == "nearest":
            self.nearest = nearest_tables((Hs, Ws), (H, W), self.device)
        elif H * W and Hs * Ws:
            host = {}
            if Ws != W:
                host["x"] = resample_tables(Ws, W, filter)
            if Hs != H:
                host["y"] = resample_tables(Hs, H, filter)
            for b, c in host.values():
                specs += [(b.reshape(-1), torch.int32), (c.reshape(-1), torch.int32)]
        up = _lib.small_to_device_many(specs, self.device)                  # one pinned staging buffer, one copy
        self.lut = up[0].view(3, 256)
        if filter != "nearest" and H * W and Hs * Ws:
            it = iter(up[1:])
            for ax, (b, c) in host.items():
                setattr(self, "bounds_" + ax, next(it).view(-1, 2))
                setattr(self, "coef_" + ax, next(it).view(c.shape))
                setattr(self, "ksize_" + ax, int(c.shape[1]))

    def workspace_bytes(self, n):
        if self.filter == "nearest":
            return 0
        return int(_lib.load().dmm_prepare_frames_workspace_bytes(int(n), *self.src_size, *self.size))


def _source(frames_u8):
    """``frames_u8`` as the ABI can address it -- dense pixels, a row stride of at least a row, a frame stride of at least the
    rows it spans -- or a contiguous copy.  -> (tensor, frame stride, row stride)."""
    n, Hs, Ws, _ = frames_u8.shape
    x = frames_u8
    if x.numel():
        rs = x.stride(1) if Hs > 1 else 3 * Ws
        fs = x.stride(0) if n > 1 else Hs * rs
        if not ((Ws == 1 or x.stride(2) == 3) and x.stride(3) == 1 and rs >= 3 * Ws and fs >= Hs * rs):
            x = x.contiguous()
            rs, fs = 3 * Ws, 3 * Ws * Hs
        return x, fs, rs
    return x, 3 * Ws * Hs, 3 * Ws


def _check_frames(frames_u8):
    """Wrong dtypes and shapes are ``ValueError``s, as in ``augment_clip``; a host tensor is the package's ``DmmError``."""
    import torch
    if not isinstance(frames_u8, torch.Tensor) or frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or frames_u8.dtype != torch.uint8:
        what = (f"{frames_u8.dtype} {tuple(frames_u8.shape)}" if isinstance(frames_u8, torch.Tensor) else type(frames_u8).__name__)
        raise ValueError(f"frames are uint8 [n,Hs,Ws,3], not {what}")
    if not frames_u8.is_cuda:
        raise _lib.DmmError("dmm_net_amd.frames needs tensors on an MI355X device (no CPU fallback): frames_u8 is on the host")


def _run(frames_u8, tables, out, return_u8, workspace):
    """The entry call behind ``prepare_frames`` and ``ClipPreparer``.  -> (fp32 [n,3,H,W], uint8 [n,H,W,3] or None)."""
    import torch
    _check_frames(frames_u8)
    dev = frames_u8.device
    n, Hs, Ws, _ = frames_u8.shape
    H, W = tables.size
    if tables.src_size != (Hs, Ws) or tables.device != dev:
        raise ValueError(f"tables are for {tables.src_size} -> {tables.size} on {tables.device}, the frames are {(Hs, Ws)} on {dev}")
    if tables.filter != "nearest" and Hs * Ws == 0 and H * W != 0:
        raise ValueError("an empty image has nothing to resample")
    if out is None:
        out = torch.empty((n, 3, H, W), dtype=torch.float32, device=dev)
    else:
        if tuple(out.shape) != (n, 3, H, W) or out.dtype != torch.float32 or out.device != dev:
            raise ValueError(f"out is fp32 {(n, 3, H, W)} on {dev}, not {out.dtype} {tuple(out.shape)} on {out.device}")
        if out.numel() and not ((W == 1 or out.stride(3) == 1) and (H == 1 or out.stride(2) == W)
                                and out.stride(1) >= H * W and (n == 1 or out.stride(0) >= H * W)):
            raise ValueError(f"out has dense rows and strides of at least a plane, not strides {out.stride()}")
    u8 = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev) if return_u8 else None
    if n * H * W == 0:
        return out, u8
    src, fs, rs = _source(frames_u8)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    HW = H * W
    outs = (ptr(tables.lut), out.data_ptr(), max(out.stride(0), HW), max(out.stride(1), HW), ptr(u8), 3 * HW)
    if tables.filter == "nearest":
        _lib.call("dmm_prepare_frames_nearest_u8", dev, ptr(src), fs, rs, n, 3, Hs, Ws, H, W, ptr(tables.nearest), *outs, stream)
        return out, u8
    need = tables.workspace_bytes(n)
    if need and (workspace is None or workspace.numel() * workspace.element_size() < need):
        workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
    _lib.call("dmm_prepare_frames_u8", dev, ptr(src), fs, rs, n, 3, Hs, Ws, H, W, ptr(tables.bounds_x), ptr(tables.coef_x),
              tables.ksize_x, ptr(tables.bounds_y), ptr(tables.coef_y), tables.ksize_y, *outs,
              ptr(workspace) if need else None, need, stream)
    return out, u8


def prepare_frames(frames_u8, size, *, filter="bicubic", mean=MEAN, std=STD, tables=None, out=None, return_u8=False):
    """``uint8 [n,Hs,Ws,3]`` decoded frames on the device -> fp32 ``[n,3,H,W]``: ``Image.resize((W, H), filter)``,
    ``ToTensor()`` and ``Normalize(mean, std)`` of every frame, bit for bit; with ``return_u8`` also the resized image itself,
    ``uint8 [n,H,W,3]``, as a second result.  ``size`` = (H, W).  ``tables``: a ``FrameTables`` of the size pair when the
    caller keeps one (its filter, mean and std hold); else one is built here (a host loop and one upload per call).  ``out``:
    an fp32 ``[n,3,H,W]`` with dense rows -- a slice of a larger batch is fine -- written instead of a new tensor (a captured
    graph replays it).  Non-contiguous frames are taken as they are where their strides fit the ABI and copied otherwise;
    they are never written.  Runs on the current stream without synchronising."""
    _check_filter(filter)
    _check_frames(frames_u8)
    H, W = (int(v) for v in size)
    if tables is None:
        tables = FrameTables(frames_u8.shape[1:3], (H, W), filter, mean, std, frames_u8.device)
    elif tables.size != (H, W):
        raise ValueError(f"tables are for {tables.src_size} -> {tables.size}, not -> {(H, W)}")
    res, u8 = _run(frames_u8, tables, out, return_u8, None)
    return (res, u8) if return_u8 else res


class ClipPreparer:
    """One size pair's preparation, set up once: the coefficient tables of both axes, the nearest tables of the annotation,
    the look-up table and (from the first call on) the workspace.  ``preparer(frames_u8, labels_u8=None, out=None)`` ->
    ``(frames fp32 [n,3,H,W], labels uint8 [n,H,W] or None)``: exactly what ``augment_clip(frames, labels, ...)``,
    ``TrainEncoder.forward`` and ``FrameLoop.run`` accept.  The labels go through ``measures.resize_labels_device`` --
    ``annot.resize((W, H), Image.NEAREST)`` of dataset.py:213-215."""

    def __init__(self, src_size, size, filter="bicubic", mean=MEAN, std=STD, device="cuda"):
        self.tables = FrameTables(src_size, size, filter, mean, std, device)
        self.src_size, self.size = self.tables.src_size, self.tables.size
        self.label_tables = (self.tables.nearest if filter == "nearest" else
                             nearest_tables(self.src_size, self.size, self.tables.device))
        self.workspace = None

    def __call__(self, frames_u8, labels_u8=None, out=None):
        import torch
        n = frames_u8.shape[0] if isinstance(frames_u8, torch.Tensor) and frames_u8.dim() == 4 else 0
        need = self.tables.workspace_bytes(n)
        if need and (self.workspace is None or self.workspace.numel() < need):
            self.workspace = torch.empty((need,), dtype=torch.uint8, device=self.tables.device)
        frames, _ = _run(frames_u8, self.tables, out, False, self.workspace)
        labels = None
        if labels_u8 is not None:
            if not labels_u8.is_cuda:
                raise _lib.DmmError("dmm_net_amd.frames needs tensors on an MI355X device (no CPU fallback): labels_u8 is on the host")
            if labels_u8.dtype != torch.uint8 or tuple(labels_u8.shape) != (n,) + self.src_size:
                raise ValueError(f"labels are uint8 {(n,) + self.src_size}, not {labels_u8.dtype} {tuple(labels_u8.shape)}")
            labels = resize_labels_device(labels_u8, self.size, self.label_tables)
        return frames, labels
