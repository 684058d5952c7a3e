"""Batched device ops of the matching layer: thin tensor-level wrappers over the C ABI.

Every function takes CUDA(=HIP) tensors, enqueues on the current torch stream of their device and
returns fresh tensors.  B frames per call; ``n_valid`` / ``m_valid`` (int32 [B], optional) make the
batch ragged.  No function here has a CPU implementation: CPU tensors raise.
"""
from __future__ import annotations

import ctypes
import threading
from collections import namedtuple
from typing import Optional, Tuple

import torch

from . import _lib
from .determinism import is_deterministic

_DT = {torch.float32: _lib.DTYPE_F32, torch.float16: _lib.DTYPE_F16, torch.bfloat16: _lib.DTYPE_BF16}


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream(t: torch.Tensor):
    return torch.cuda.current_stream(t.device).cuda_stream


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.DmmError("dmm_net_amd ops need tensors on an MI355X device (no CPU fallback)")


def _plane_rows(t: torch.Tensor) -> torch.Tensor:
    """[..., K, H, W] as the C ABI reads planes: the H*W elements of a plane contiguous, the plane stride at least H*W.  A
    tensor that is laid out so (``alloc_planes`` strides, slices along the batch or plane axis) and an empty one are passed as
    they are; any other is copied.  (Strides and shape are read once each: the one-frame calls are host bound.)"""
    s, n = t.stride(), t.shape
    if (s[-1] == 1 and s[-2] == n[-1] and s[-3] >= n[-2] * n[-1]) or t.numel() == 0:
        return t
    return t.contiguous()


def _planes(t: torch.Tensor) -> Tuple[torch.Tensor, int, int]:
    """[B,K,H,W] with contiguous H*W planes -> (tensor, frame stride, plane stride) in elements."""
    assert t.dim() == 4, t.shape
    t = _plane_rows(t)
    return t, t.stride(0), t.stride(1)


def _planes3(t: torch.Tensor):
    """[K,H,W] with contiguous H*W planes -> (tensor, plane stride in elements)."""
    assert t.dim() == 3, t.shape
    t = _plane_rows(t)
    return t, t.stride(0)


def _batch_planes(t: torch.Tensor, one_frame: bool = False):
    """[B,K,H,W] planes, or with ``one_frame`` the [K,H,W] planes of a batch of one -> (tensor, K, frame stride, plane stride)."""
    t = _plane_rows(t)
    s = t.stride()
    if one_frame:
        assert len(s) == 3, t.shape
        return t, t.shape[0], t.shape[0] * s[0], s[0]
    assert len(s) == 4, t.shape
    return t, t.shape[1], s[0], s[1]


def _cf(t):
    return None if t is None else t.contiguous().float()


def _count_tables(B, N, M, dev, dual=False):
    """inter [B,M,N], area_p [B,N], area_t [B,M] int32 (``dual``: + inter2, area_t2 of the second template set)."""
    i32 = dict(dtype=torch.int32, device=dev)
    one = (torch.empty((B, M, N), **i32), torch.empty((B, N), **i32), torch.empty((B, M), **i32))
    return one + (torch.empty((B, M, N), **i32), torch.empty((B, M), **i32)) if dual else one


def alloc_planes(B: int, K: int, H: int, W: int, dtype, device, align_bytes: int = 128, fill=None) -> torch.Tensor:
    """[B,K,H,W] mask planes whose PLANE STRIDE is rounded up to ``align_bytes`` (every plane then starts on a 128-byte
    line).  255 x 255 planes are an odd number of elements: contiguous 16-bit planes alternate between dword-aligned and
    2-bytes-off starts, and every 2 KiB run of a misaligned plane straddles one extra 128-byte line (+5.4 % HBM traffic in
    the count kernel at BASELINE configs[4], profiles/r03).  The C ABI takes the plane stride (``sp_n`` / ``so_m``), so a
    producer that owns its buffers just allocates them this way; H*W elements of a plane stay contiguous."""
    es = torch.empty((), dtype=dtype).element_size()
    q = max(1, align_bytes // es)
    S = (H * W + q - 1) // q * q
    buf = torch.empty((B, K, S), dtype=dtype, device=device)
    if fill is not None:
        buf.fill_(fill)
    return torch.as_strided(buf, (B, K, H, W), (K * S, S, W, 1))


class FramePlanes:
    """Proposal planes of B frames held as ONE TENSOR PER FRAME (the reference's ``prop_m[bid]``, dmm_model.py:58 / :111)
    plus the device pointer table the ``*_frames`` entry points of the C ABI take -- the frames go through one launch
    without being copied into a [B, Nmax, H, W] batch first.  Frame b has ``planes[b].shape[0]`` planes (ragged: pass
    ``n_valid``); all frames share H, W, dtype and the plane stride."""

    def __init__(self, planes, table="build"):
        """``table``: "build" uploads the pointer table here; None defers it -- the caller uploads ``addresses()`` together
        with its other small tables (``_lib.small_to_device_many``) and assigns ``.table``."""
        planes = list(planes)
        assert len(planes) > 0
        H, W = int(planes[0].shape[-2]), int(planes[0].shape[-1])
        self.dtype, self.device = planes[0].dtype, planes[0].device
        assert self.dtype in _DT, self.dtype
        fixed = []
        for t in planes:
            _need_gpu(t)
            assert t.dim() == 3 and tuple(t.shape[-2:]) == (H, W) and t.dtype == self.dtype and t.device == self.device
            fixed.append(_plane_rows(t))
        strides = {int(t.stride(0)) for t in fixed if t.shape[0] > 1}
        if len(strides) > 1:                         # mixed plane strides: densify the odd ones
            fixed = [t if (t.shape[0] <= 1 or t.stride(0) == H * W) else t.contiguous() for t in fixed]
            strides = {int(t.stride(0)) for t in fixed if t.shape[0] > 1}
            if len(strides) > 1:
                fixed = [t.contiguous() for t in fixed]
                strides = {H * W}
        self.planes = fixed                          # keeps the storage alive
        self.plane_stride = strides.pop() if strides else H * W
        self.H, self.W, self.B = H, W, len(fixed)
        self.N = max(int(t.shape[0]) for t in fixed)
        self.counts = [int(t.shape[0]) for t in fixed]
        # one small H2D copy; frames without planes get a valid dummy address (never dereferenced: n_valid = 0)
        self.table = _lib.small_to_device(self.addresses(), torch.int64, self.device) if table == "build" else table

    def addresses(self):
        any_ptr = next((t.data_ptr() for t in self.planes if t.shape[0]), 0)
        return [t.data_ptr() if t.shape[0] else any_ptr for t in self.planes]

    def n_valid(self) -> torch.Tensor:
        return _lib.small_to_device(self.counts, torch.int32, self.device)

    def stacked(self) -> torch.Tensor:
        """[B, N, H, W] copy (zero planes beyond a frame's count) -- only for paths without a pointer-table kernel."""
        out = self.planes[0].new_zeros((self.B, self.N, self.H, self.W))
        for b, t in enumerate(self.planes):
            out[b, :t.shape[0]] = t
        return out


def _proposal_planes(masks_p, one_frame: bool = False):
    """The proposal planes of a call, whatever holds them: a [B,N,H,W] tensor, a ``FramePlanes`` or, with ``one_frame``, a
    [N,H,W] tensor -> (address, torch dtype, B, N, H, W, frame stride, plane stride, device, what keeps the address alive).
    For a ``FramePlanes`` the address is its pointer table's and the frame stride is ``_lib.FRAME_TABLE``, as the one-call
    training entries take it; the granular ``*_frames`` entries take the plane stride alone (``_sp``)."""
    if isinstance(masks_p, FramePlanes):
        fp = masks_p
        return fp.table.data_ptr(), fp.dtype, fp.B, fp.N, fp.H, fp.W, _lib.FRAME_TABLE, fp.plane_stride, fp.device, fp
    _need_gpu(masks_p)
    t, N, sp_b, sp_n = _batch_planes(masks_p, one_frame)
    return t.data_ptr(), t.dtype, 1 if one_frame else t.shape[0], N, t.shape[-2], t.shape[-1], sp_b, sp_n, t.device, t


def _sp(sp_b, sp_n):
    """-> (is a pointer table, the proposal strides of a granular entry: the ``*_frames`` entries have no frame stride)."""
    return (True, (sp_n,)) if sp_b == _lib.FRAME_TABLE else (False, (sp_b, sp_n))


def padded_width(N: int, M: int) -> int:
    """Pp = solver width after the reference's zero padding (match_model.py:109-113)."""
    return N if N > M else M + 1


def iou_counts(masks_p, masks_t: torch.Tensor, n_valid=None, m_valid=None):
    """-> inter [B,M,N] i32, area_p [B,N] i32, area_t [B,M] i32 (match_helper.py:9-28 on all pairs).  masks_p: [B,N,H,W]
    tensor or ``FramePlanes`` (then with ``n_valid``)."""
    p, dt, B, N, H, W, sp_b, sp_n, dev, _keep = _proposal_planes(masks_p)
    frames, sp = _sp(sp_b, sp_n)
    _need_gpu(masks_t)
    assert dt == masks_t.dtype and dt in _DT and (n_valid is not None or not frames)
    masks_t, st_b, st_m = _planes(masks_t)
    M = masks_t.shape[1]
    assert masks_t.shape[0] == B and tuple(masks_t.shape[2:]) == (H, W)
    inter, ap, at = _count_tables(B, N, M, dev)
    _lib.call("dmm_iou_counts_frames" if frames else "dmm_iou_counts", dev, p, _ptr(masks_t), _DT[dt], B, N, M, H * W, *sp,
              st_b, st_m, _ptr(n_valid), _ptr(m_valid), _ptr(inter), _ptr(ap), _ptr(at), _stream(masks_t))
    return inter, ap, at


def pack_words(HW: int) -> int:
    """uint64 words per packed plane of HW pixels (DMM_PACKED1 ballot layout)."""
    return 4 * ((HW + 255) // 256)


def ragged_blocks(blocks):
    """-> (contiguous blocks, their addresses as the pointer table of ``ragged_pad`` wants them)."""
    blocks = [b.contiguous() for b in blocks]
    any_ptr = next((b.data_ptr() for b in blocks if b.shape[0]), 0)
    return blocks, [b.data_ptr() if b.shape[0] else any_ptr for b in blocks]


def ragged_pad(blocks, P_max: int, counts: torch.Tensor, table: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-video blocks [P_b, ...] (same trailing shape and dtype, 4-byte multiples per row) -> [B, P_max, ...] with
    zeros from row P_b on, in ONE launch (``dmm_ragged_pad``): the batching step of the per-video driver.
    counts: [B] int32 on the device (= the n_valid the ragged kernels take anyway).  ``table`` (optional): the blocks'
    addresses already on the device (``ragged_blocks`` + ``_lib.small_to_device_many``; the blocks must then be the
    contiguous ones ``ragged_blocks`` returned)."""
    if table is None:
        blocks, addrs = ragged_blocks(blocks)
    first = blocks[0]
    _need_gpu(first, counts)
    tail = tuple(first.shape[1:])
    row_bytes = first.element_size()
    for d in tail:
        row_bytes *= int(d)
    out = torch.empty((len(blocks), int(P_max)) + tail, dtype=first.dtype, device=first.device)
    if row_bytes % 4 != 0 or any(tuple(b.shape[1:]) != tail or b.dtype != first.dtype for b in blocks):
        raise ValueError("ragged_pad: blocks must share dtype and trailing shape, rows of a multiple of 4 bytes")
    if table is None:
        table = _lib.small_to_device(addrs, torch.int64, first.device)
    _lib.call("dmm_ragged_pad", first.device, _ptr(table), _ptr(counts), len(blocks), int(P_max), row_bytes, _ptr(out),
              _stream(first))
    return out                                        # (the blocks are read in stream order: no keep-alive needed)


def pack_masks(masks: torch.Tensor) -> torch.Tensor:
    """[B,K,H,W] soft masks -> [B,K,words] int64 bit planes of (x > 0.5) in the library's ballot layout."""
    _need_gpu(masks)
    masks, s_b, s_k = _planes(masks)
    B, K, H, W = masks.shape
    if s_b != K * s_k:
        masks = masks.contiguous()
        s_k = H * W
    wd = pack_words(H * W)
    out = torch.empty((B, K, wd), dtype=torch.int64, device=masks.device)
    _lib.call("dmm_pack_masks", masks.device, _ptr(masks), _DT[masks.dtype], B * K, H * W, s_k, _ptr(out), wd,
              _stream(masks))
    return out


def iou_counts_packed(packed_p: torch.Tensor, packed_t: torch.Tensor, HW: int, n_valid=None, m_valid=None):
    """iou_counts on DMM_PACKED1 planes ([B,N,words], [B,M,words] int64): identical integer tables, 1/32 of the bytes."""
    _need_gpu(packed_p, packed_t)
    assert packed_p.dtype == torch.int64 and packed_t.dtype == torch.int64
    packed_p, packed_t = packed_p.contiguous(), packed_t.contiguous()
    B, N, wd = packed_p.shape
    M = packed_t.shape[1]
    assert wd == pack_words(HW) and packed_t.shape[2] == wd
    dev = packed_p.device
    inter, ap, at = _count_tables(B, N, M, dev)
    _lib.call("dmm_iou_counts", dev, _ptr(packed_p), _ptr(packed_t), _lib.DTYPE_PACKED1, B, N, M, HW, N * wd, wd, M * wd,
              wd, _ptr(n_valid), _ptr(m_valid), _ptr(inter), _ptr(ap), _ptr(at), _stream(packed_p))
    return inter, ap, at


def iou_counts_dual(masks_p, masks_t: torch.Tensor, masks_t2: torch.Tensor, n_valid=None, m_valid=None):
    """One pass over the proposal planes (tensor or ``FramePlanes``) against TWO template sets (templates + training
    targets).  -> (inter, area_p, area_t), (inter2, area_t2)."""
    p, dt, B, N, H, W, sp_b, sp_n, dev, _keep = _proposal_planes(masks_p)
    frames, sp = _sp(sp_b, sp_n)
    _need_gpu(masks_t, masks_t2)
    assert dt == masks_t.dtype == masks_t2.dtype and dt in _DT and (n_valid is not None or not frames)
    assert masks_t.shape == masks_t2.shape
    masks_t, st_b, st_m = _planes(masks_t)
    masks_t2, st2_b, st2_m = _planes(masks_t2)
    M = masks_t.shape[1]
    inter, ap, at, inter2, at2 = _count_tables(B, N, M, dev, dual=True)
    _lib.call("dmm_iou_counts_dual_frames" if frames else "dmm_iou_counts_dual", dev, p, _ptr(masks_t), _ptr(masks_t2),
              _DT[dt], B, N, M, H * W, *sp, st_b, st_m, st2_b, st2_m, _ptr(n_valid), _ptr(m_valid), _ptr(inter), _ptr(ap),
              _ptr(at), _ptr(inter2), _ptr(at2), _stream(masks_t))
    return (inter, ap, at), (inter2, at2)


def feature_normalize(x: torch.Tensor, want_norms: bool = False):
    """x [..., D] fp32 -> x / max(||x||, 1e-8) (and the clamped norms)."""
    _need_gpu(x)
    x = x.contiguous().float()
    D = x.shape[-1]
    rows = x.numel() // max(D, 1)
    out = torch.empty_like(x)
    norms = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device) if want_norms else None
    _lib.call("dmm_feature_normalize_f32", x.device, _ptr(x), rows, D, _ptr(out), _ptr(norms), _stream(x))
    return (out, norms) if want_norms else out


def cosine(featn_t: torch.Tensor, featn_p: torch.Tensor, n_valid=None, m_valid=None) -> torch.Tensor:
    """cos [B,M,N] of normalised rows featn_t [B,M,D], featn_p [B,N,D] (match_helper.py:59-63)."""
    _need_gpu(featn_t, featn_p)
    featn_t, featn_p = featn_t.contiguous().float(), featn_p.contiguous().float()
    B, M, D = featn_t.shape
    N = featn_p.shape[1]
    out = torch.empty((B, M, N), dtype=torch.float32, device=featn_t.device)
    _lib.call("dmm_cosine_f32", featn_t.device, _ptr(featn_t), _ptr(featn_p), B, N, M, D, _ptr(n_valid), _ptr(m_valid),
              _ptr(out), _stream(featn_t))
    return out


def cosine_features(feat_t: torch.Tensor, feat_p: torch.Tensor) -> torch.Tensor:
    """get_cosine_score (match_helper.py:51-64) from RAW features feat_t [B,M,D], feat_p [B,N,D] -> cos [B,M,N]: one
    fused launch inside its envelope (dense, N >= 2, D % 64 == 0; D = 256 / 512 / 1024 with the D axis over the lanes),
    else normalise x 2 + cosine.  Bit identical either way."""
    _need_gpu(feat_t, feat_p)
    feat_t, feat_p = feat_t.contiguous().float(), feat_p.contiguous().float()
    B, M, D = feat_t.shape
    N = feat_p.shape[1]
    out = torch.empty((B, M, N), dtype=torch.float32, device=feat_t.device)
    rc = _lib.call("dmm_cosine_features_f32", feat_t.device, _ptr(feat_t), _ptr(feat_p), B, N, M, D, _ptr(out),
                   _stream(feat_t), allow=(_lib.DMM_ERR_UNSUPPORTED,))
    if rc == _lib.DMM_ERR_UNSUPPORTED:                        # outside the fused kernel's envelope
        return cosine(feature_normalize(feat_t), feature_normalize(feat_p))
    return out


def _solver_out(B, N, M, dev, per_frame: str):
    """The result dict of the solver wrappers: sim [B,M,N], R and Rb [B,M,Pp], match_score and det_score [B,M] fp32, and
    the int32 [B] tensor named ``per_frame`` (iters / status)."""
    Pp = padded_width(N, M)
    f32 = dict(dtype=torch.float32, device=dev)
    out = dict(sim=torch.empty((B, M, N), **f32), R=torch.empty((B, M, Pp), **f32), Rb=torch.empty((B, M, Pp), **f32),
               match_score=torch.empty((B, M), **f32), det_score=torch.empty((B, M), **f32))
    out[per_frame] = torch.empty((B,), dtype=torch.int32, device=dev)
    return out


def relax_match(cos, inter, area_p, area_t, score_p, *, score_weight, max_iter, proj_iter, lr, is_test,
                n_valid=None, m_valid=None, want_x=False, state="f32"):
    """Similarity mix + relaxed assignment + scores for B frames.  cos [B,M,N] = feature_sim.
    Returns dict(sim, R, Rb, match_score, det_score, iters, X).  ``state="f16"``: the opt-in tolerance mode with the
    solver state in packed fp16 and fp32 sums (``dmm_relax_match_f16s``, BASELINE configs[4]); the default reproduces
    the reference bit for bit.  Tables outside the fast kernels' envelope (M > 32 or Pp > 256) go through
    ``dmm_relax_match_any_f32`` (general solver, state in a scratch tensor allocated here) -- fp32 state only."""
    _need_gpu(cos, inter)
    B, M, N = cos.shape
    Pp = padded_width(N, M)
    dev = cos.device
    out = _solver_out(B, N, M, dev, "iters")
    out["X"] = torch.empty((B, M, Pp), dtype=torch.float32, device=dev) if want_x else None
    cos, score_p = _cf(cos), _cf(score_p)
    assert state in ("f32", "f16")
    args = (_ptr(cos), _ptr(inter), _ptr(area_p), _ptr(area_t), _ptr(score_p), B, N, M, _ptr(n_valid), _ptr(m_valid),
            float(score_weight), int(max_iter), int(proj_iter), float(lr), int(is_test), _ptr(out["sim"]),
            _ptr(out["R"]), _ptr(out["Rb"]), _ptr(out["match_score"]), _ptr(out["det_score"]), _ptr(out["iters"]),
            _ptr(out["X"]))
    if state == "f32" and (M > _lib.MAX_TEMPLATES or Pp > _lib.MAX_PROPOSALS):
        scratch = torch.empty((int(_lib.load().dmm_relax_any_scratch_bytes(B, N, M)),), dtype=torch.uint8, device=dev)
        _lib.call("dmm_relax_match_any_f32", dev, *args, _ptr(scratch), scratch.numel(), _stream(cos))
        scratch.record_stream(torch.cuda.current_stream(dev))
    else:
        _lib.call("dmm_relax_match_f32" if state == "f32" else "dmm_relax_match_f16s", dev, *args, _stream(cos))
    return out


def relax_match_bwd(sim, score_p, dRb, d_match_score, d_det_score, *, max_iter, proj_iter, lr, is_test,
                    n_valid=None, m_valid=None) -> torch.Tensor:
    """d loss / d sim [B,M,N] of ``relax_match`` (reverse sweep through the taped solver iterations)."""
    _need_gpu(sim)
    sim = sim.contiguous().float()
    B, M, N = sim.shape
    dev = sim.device
    dRb, d_match_score, d_det_score, score_p = _cf(dRb), _cf(d_match_score), _cf(d_det_score), _cf(score_p)
    L = _lib.load()
    nbytes = int(L.dmm_relax_bwd_workspace_bytes(B, N, M, int(max_iter), int(proj_iter)))
    ws = torch.empty((max(nbytes, 8),), dtype=torch.uint8, device=dev)
    out = torch.empty((B, M, N), dtype=torch.float32, device=dev)
    _lib.call("dmm_relax_match_bwd_f32", dev, _ptr(sim), _ptr(score_p), B, N, M, _ptr(n_valid), _ptr(m_valid),
              int(max_iter), int(proj_iter), float(lr), int(is_test), _ptr(dRb), _ptr(d_match_score), _ptr(d_det_score),
              _ptr(out), _ptr(ws), ws.numel(), _stream(sim))
    return out


def feature_sim_bwd(dsim, cos, gt, d_loss, score_weight, feat_t, feat_p, featn_t, featn_p, norm_t, norm_p,
                    n_valid=None, m_valid=None):
    """-> (g_feat_t [B,M,D], g_feat_p [B,N,D]): backward of cosine + (1 - w) mix + matching-loss mse in one launch
    (``dmm_feature_sim_bwd_f32``).  gt / d_loss None = no matching loss."""
    _need_gpu(dsim, feat_t, feat_p)
    dsim, cos, gt, d_loss = _cf(dsim), _cf(cos), _cf(gt), _cf(d_loss)
    feat_t, feat_p, featn_t, featn_p = _cf(feat_t), _cf(feat_p), _cf(featn_t), _cf(featn_p)
    norm_t, norm_p = _cf(norm_t), _cf(norm_p)
    B, M, N = dsim.shape
    D = feat_p.shape[-1]
    g_t, g_p = torch.empty_like(feat_t), torch.empty_like(feat_p)
    if gt is None or d_loss is None:
        gt = d_loss = cos_arg = None
    else:
        cos_arg = cos
    _lib.call("dmm_feature_sim_bwd_f32", dsim.device, _ptr(dsim), _ptr(cos_arg), _ptr(gt), _ptr(d_loss),
              float(score_weight), _ptr(feat_t), _ptr(feat_p), _ptr(featn_t), _ptr(featn_p), _ptr(norm_t), _ptr(norm_p), B,
              N, M, D, _ptr(n_valid), _ptr(m_valid), _ptr(g_t), _ptr(g_p), _stream(dsim))
    return g_t, g_p


def _greedy_init_any(C: torch.Tensor, rows_valid=None, cols_valid=None):
    """relax_matching(C, 0, 0, 0) -- the greedy one-hot initialisation alone (relax_match.py:45-55), what
    compute_matching_loss asks for (match_helper.py:44) -- for tables OUTSIDE the solver kernels' envelope: a handful of
    device tensor ops (order-free: max, first argmin over rows per column, first argmin over columns per row; torch's
    argmin returns the first minimal index).  Inside the envelope ``dmm_relax_solve_f32`` does it in its prologue."""
    B, n, m = C.shape
    dev = C.device
    rv = torch.full((B,), n, dtype=torch.int64, device=dev) if rows_valid is None else rows_valid.long()
    cv = torch.full((B,), m, dtype=torch.int64, device=dev) if cols_valid is None else cols_valid.long()
    live = (torch.arange(n, device=dev)[None, :, None] < rv[:, None, None]) & \
           (torch.arange(m, device=dev)[None, None, :] < cv[:, None, None])
    inf = torch.tensor(float("inf"), device=dev)
    cmax = torch.where(live, C, -inf).flatten(1).max(1)[0]                               # C.max() over the live block
    col_best = torch.where(live, C, inf).argmin(1)                                       # [B, m]: first argmin over rows
    keep = torch.arange(n, device=dev)[None, :, None] == col_best[:, None, :]
    crm = torch.where(live, torch.where(keep, C, cmax[:, None, None].expand_as(C)), inf)
    idx = crm.argmin(2)                                                                  # [B, n]: first argmin over columns
    X = torch.zeros_like(C)
    X.scatter_(2, idx[:, :, None], 1.0)
    X = torch.where(live & (torch.arange(n, device=dev)[None, :, None] < rv[:, None, None]), X, torch.zeros_like(X))
    X = X * ((rv > 0) & (cv > 0))[:, None, None].to(X.dtype)
    return dict(X=X, R=X.clone(), cost=torch.zeros((B, 1), dtype=torch.float32, device=dev),
                iters=torch.zeros((B,), dtype=torch.int32, device=dev))


def relax_solve(C: torch.Tensor, max_iter: int, proj_iter: int, lr: float, rows_valid=None, cols_valid=None):
    """relax_matching on cost matrices C [B,n,m] -> dict(X, R, cost [B,max_iter+1], iters [B]).
    rows_valid / cols_valid (int32 [B]) restrict each frame to its top-left live block."""
    _need_gpu(C)
    C = C.contiguous().float()
    B, n, m = C.shape
    if (n > _lib.MAX_TEMPLATES or m > _lib.MAX_PROPOSALS) and max_iter == 0:
        return _greedy_init_any(C, rows_valid, cols_valid)
    X = torch.empty_like(C)
    R = torch.empty_like(C)
    cost = torch.zeros((B, max_iter + 1), dtype=torch.float32, device=C.device)
    iters = torch.empty((B,), dtype=torch.int32, device=C.device)
    _lib.call("dmm_relax_solve_f32", C.device, _ptr(C), B, n, m, _ptr(rows_valid), _ptr(cols_valid), int(max_iter),
              int(proj_iter), float(lr), _ptr(X), _ptr(R), _ptr(cost), _ptr(iters), _stream(C))
    return dict(X=X, R=R, cost=cost, iters=iters)


LSAP_INVALID, LSAP_INFEASIBLE = 1, 2          # dmm_lsap_f32's status codes
_LSAP_MESSAGES = {LSAP_INVALID: "matrix contains invalid numeric entries", LSAP_INFEASIBLE: "cost matrix is infeasible"}


def lsap_envelope(nr: int, nc: int) -> bool:
    """Tables ``dmm_lsap_f32`` solves (after the transpose of a tall table)."""
    nr, nc = min(nr, nc), max(nr, nc)
    return nr <= _lib.MAX_TEMPLATES and nc <= _lib.MAX_PROPOSALS


def check_lsap_status(status: torch.Tensor, where: str = "") -> None:
    """Raise scipy's ``ValueError`` if a frame's assignment failed (reads the 4*B status bytes: one sync); nothing while a
    stream capture is in progress (the status tensor is read after the graph has run)."""
    if torch.cuda.is_current_stream_capturing():
        return
    st = status.cpu()
    bad = torch.nonzero(st).flatten()
    if bad.numel():
        code = int(st[bad[0]])
        raise ValueError(f"{_LSAP_MESSAGES.get(code, f'linear_sum_assignment status {code}')} ({where}frame {int(bad[0])})")


def _lsap_host(C, rows_valid, cols_valid):
    """scipy per frame: tables outside the kernel's envelope."""
    import numpy as np
    from scipy.optimize import linear_sum_assignment as lsa
    B, nr, nc = C.shape
    c = C.detach().cpu().numpy()
    rv = [nr] * B if rows_valid is None else rows_valid.cpu().tolist()
    cv = [nc] * B if cols_valid is None else cols_valid.cpu().tolist()
    col = np.full((B, nr), -1, np.int32)
    st = np.zeros((B,), np.int32)
    for b in range(B):
        try:
            r, k = lsa(c[b, :rv[b], :cv[b]])
        except ValueError as e:
            st[b] = LSAP_INFEASIBLE if "infeasible" in str(e) else LSAP_INVALID
            continue
        col[b, r] = k
    col_t = torch.from_numpy(col).to(C.device)
    X = torch.zeros((B, nr, nc), dtype=torch.float32, device=C.device)
    X.scatter_(2, col_t.clamp_min(0).long()[:, :, None], (col_t >= 0).float()[:, :, None])
    return X, col_t, torch.from_numpy(st).to(C.device)


def _i32(t):
    return None if t is None else t.to(torch.int32).contiguous()


def linear_sum_assignment(C: torch.Tensor, rows_valid=None, cols_valid=None, maximize: bool = False):
    """scipy.optimize.linear_sum_assignment for B tables at once: C [B,nr,nc] -> (X [B,nr,nc] one-hot float32,
    col_of_row [B,nr] int32 with -1 for an unassigned row, status [B] int32: 0 ok, LSAP_INVALID, LSAP_INFEASIBLE).
    The same assignment as scipy, ties included (``dmm_lsap_f32``: fp64 on the float32 costs).  rows_valid / cols_valid
    (int32 [B]) restrict frame b to its top-left block.  A tall table (nr > nc) is solved through its transpose, as scipy
    does; tables outside the kernel's envelope (more than 32 x 256 after that) run scipy per frame on the host.  No status
    is read here: ``check_lsap_status`` raises like scipy."""
    _need_gpu(C)
    C = C.float()
    if maximize:
        C = -C
    B, nr, nc = C.shape
    if not lsap_envelope(nr, nc):
        return _lsap_host(C, rows_valid, cols_valid)
    if nr > nc:
        X_t, _, st = linear_sum_assignment(C.transpose(1, 2), cols_valid, rows_valid)
        X = X_t.transpose(1, 2).contiguous()
        col = torch.where(X.sum(2) > 0, X.argmax(2), -1).to(torch.int32)
        return X, col, st
    C = C.contiguous()
    X = torch.empty((B, nr, nc), dtype=torch.float32, device=C.device)
    col = torch.empty((B, nr), dtype=torch.int32, device=C.device)
    st = torch.empty((B,), dtype=torch.int32, device=C.device)
    _lib.call("dmm_lsap_f32", C.device, _ptr(C), B, nr, nc, _ptr(_i32(rows_valid)), _ptr(_i32(cols_valid)), _ptr(X),
              _ptr(col), _ptr(st), _stream(C))
    return X, col, st


def hungarian_match(cos, inter, area_p, area_t, score_p, *, score_weight, is_test, n_valid=None, m_valid=None,
                    check=True):
    """``relax_match`` with the exact assignment (algo 'hun', ``dmm_hungarian_match_f32``): the same sim, C = -sim padded
    to each frame's live width, R = Rb = the one-hot assignment scipy picks.  Returns dict(sim, R, Rb, match_score,
    det_score, status).  ``check``: raise scipy's ValueError for a failed frame (reads the status: one sync, skipped
    while a stream capture is in progress).  M <= 32 and Pp <= 256 only (DmmError otherwise)."""
    _need_gpu(cos, inter)
    B, M, N = cos.shape
    dev = cos.device
    out = _solver_out(B, N, M, dev, "status")
    cos, score_p = _cf(cos), _cf(score_p)
    _lib.call("dmm_hungarian_match_f32", dev, _ptr(cos), _ptr(inter), _ptr(area_p), _ptr(area_t), _ptr(score_p), B, N, M,
              _ptr(n_valid), _ptr(m_valid), float(score_weight), int(is_test), _ptr(out["sim"]), _ptr(out["R"]),
              _ptr(out["Rb"]), _ptr(out["match_score"]), _ptr(out["det_score"]), _ptr(out["status"]), _stream(cos))
    if check:
        check_lsap_status(out["status"])
    return out


def mask_mix(Rb: torch.Tensor, masks_p, n_valid=None, m_valid=None, out_dtype=None, shared: bool = False) -> torch.Tensor:
    """full_outmask [B,M,H,W] = Rb [B,M,Pp] @ masks_p [B,N,H*W] (zero planes for the padded columns); masks_p: tensor or
    ``FramePlanes`` (fp32 output only; ``n_valid`` defaults to the frames' own counts).
    ``shared``: the rows of Rb share planes (train mode keeps every R > 0.01): every plane of the union of the rows'
    supports is streamed once (``dmm_mask_mix_shared_*``); same result bit for bit."""
    p, dt, B, N, H, W, sp_b, sp_n, _dev, _keep = _proposal_planes(masks_p)
    frames, sp = _sp(sp_b, sp_n)
    _need_gpu(Rb)
    M, Pp = Rb.shape[1], Rb.shape[2]
    Rb = _cf(Rb)
    out_dtype = out_dtype or torch.float32
    if frames:
        if n_valid is None:                          # frames are ragged by construction: never read past a short one
            n_valid = masks_p.n_valid()
        if out_dtype != torch.float32:
            raise ValueError("mask_mix on per-frame plane tables writes fp32 (dmm_mask_mix_frames)")
    out = torch.empty((B, M, H, W), dtype=out_dtype, device=Rb.device)
    _lib.call(("dmm_mask_mix_shared" if shared else "dmm_mask_mix") + ("_frames" if frames else "_to"), Rb.device, _ptr(Rb),
              p, _DT[dt], B, N, M, Pp, H * W, *sp, _ptr(n_valid), _ptr(m_valid), _ptr(out),
              *(() if frames else (_DT[out_dtype],)), M * H * W, H * W, _stream(Rb))
    return out


def mask_mix_bwd(Rb: torch.Tensor, masks_p, dout: torch.Tensor, n_valid=None, m_valid=None, det=None):
    """dRb [B,M,Pp] = dout [B,M,H,W] . masks_p [B,N,H,W] on the support of Rb (zeros elsewhere); masks_p: tensor or
    ``FramePlanes``.  ``det``: the deterministic entry (None: the mode as it resolves now; autograd callers pass the decision
    of their forward)."""
    if det is None:
        det = is_deterministic()
    p, dt, B, N, H, W, sp_b, sp_n, _dev, _keep = _proposal_planes(masks_p)
    frames, sp = _sp(sp_b, sp_n)
    _need_gpu(Rb, dout)
    M, Pp = Rb.shape[1], Rb.shape[2]
    Rb = _cf(Rb)
    if frames and n_valid is None:
        n_valid = masks_p.n_valid()
    dout = _cf(dout).view(B, M, H * W)
    dRb = torch.empty((B, M, Pp), dtype=torch.float32, device=Rb.device)
    entry = "dmm_mask_mix_bwd_frames" if frames else "dmm_mask_mix_bwd"
    args = (_ptr(Rb), p, _DT[dt], _ptr(dout), B, N, M, Pp, H * W, *sp, _ptr(n_valid), _ptr(m_valid), _ptr(dRb))
    if det:
        ws = _det_mix_ws(B, N, M, Pp, H * W, Rb.device)
        _lib.call(entry + "_det", Rb.device, *args, _ptr(ws), ws.numel(), _stream(Rb))
    else:
        _lib.call(entry, Rb.device, *args, _stream(Rb))
    return dRb


def _det_mix_ws(B, N, M, Pp, HW, device) -> torch.Tensor:
    """The slab of the deterministic mix backward (zeroed by the entry itself)."""
    n = int(_lib.load().dmm_mask_mix_bwd_det_workspace_bytes(B, N, M, Pp, HW))
    return torch.empty((max(n, 16),), dtype=torch.uint8, device=device)


_WORKSPACES = {}
_WS_STATE = {}                       # (device, stream) -> ((B, N, M, D), ctypes.c_int): dmm_match_forward_ws's note
# HIP stream capture is process-global by default: a second host thread that touches the runtime while one captures
# aborts the process.  Captures are serialised and run in thread-local capture mode (nn.DataParallel-style callers).
_CAPTURE_LOCK = threading.Lock()
_WS_NEED = {}                        # (B, N, M, D) [+ solver setting] -> workspace bytes (a C call saved per layer call)


def _need_cached(key, size_fn, *args) -> int:
    """``size_fn(*args)`` bytes, asked once per ``key`` (the host-bound one-frame and training calls)."""
    need = _WS_NEED.get(key)
    if need is None:
        need = _WS_NEED[key] = int(size_fn(*args))
    return need


def _cached_ws(key, need, dev):
    """The workspace cached under ``key`` = (device index, stream[, tag]), at least ``need`` bytes: grown, never shrunk.
    A new buffer holds nothing the library knows about: the note kept for the old one goes with it."""
    ws = _WORKSPACES.get(key)
    if ws is None or ws.numel() < need:
        ws = _WORKSPACES[key] = torch.empty((max(need, 256),), dtype=torch.uint8, device=dev)
        _WS_STATE.pop(key, None)
    return ws


def _forward_ws(dev, stream, shape, need):
    """``dmm_match_forward_ws``'s workspace of (device, stream) and the library's note about what the previous call left in
    THIS workspace, ``need`` bytes for tables of ``shape`` = (B, N, M, D) -> (workspace, byref(note) | None).  The note only
    holds for the same table layout, so another shape starts from "unknown".  A call recorded into a graph is replayed
    behind our back, on this workspace: a capturing stream ends note keeping for its workspace for good."""
    key = (dev.index, stream)
    ws = _cached_ws(key, need, dev)
    if torch.cuda.is_current_stream_capturing() or _WS_STATE.get(key) == "captured":
        _WS_STATE[key] = "captured"
        return ws, None
    noted, note = _WS_STATE.get(key, (None, None))
    if noted != shape:
        note = ctypes.c_int(0)
        _WS_STATE[key] = (shape, note)
    return ws, ctypes.byref(note)


def match_forward(masks_p, masks_t, feat_p, feat_t, score_p, *, score_weight, max_iter, proj_iter, lr, is_test,
                  n_valid=None, m_valid=None, return_tables=False):
    """The whole forward of B frames as ONE C-ABI call (``dmm_match_forward``: counts -> normalise -> cosine -> solver
    -> mix on the current stream): fresh output tensors, intermediates in a workspace cached per (device, stream).
    The inference path of ``MatchModel`` (no autograd bookkeeping, 1 ctypes call instead of 7, no per-call
    intermediate allocations).  Returns (full_outmask [B,M,H,W], match_score [B,M], det_score [B,M], iters [B]) and, with
    ``return_tables``, a dict of sim [B,M,N], R and Rb [B,M,Pp].  ANY N and M: tables outside the envelope of the fast
    kernels (M <= 32, Pp = max(N, M + 1) <= 256) take the general kernels of ``dmm_wide.hip`` inside the same call."""
    _need_gpu(masks_p, masks_t, feat_p, feat_t, score_p)
    assert masks_p.dtype == masks_t.dtype and masks_p.dtype in _DT
    masks_p, sp_b, sp_n = _planes(masks_p)
    masks_t, st_b, st_m = _planes(masks_t)
    B, N, H, W = masks_p.shape
    M, D = masks_t.shape[1], feat_p.shape[-1]
    feat_p, feat_t, score_p = _cf(feat_p), _cf(feat_t), _cf(score_p)
    dev = masks_p.device
    stream = _stream(masks_p)
    ws, note = _forward_ws(dev, stream, (B, N, M, D), int(_lib.load().dmm_workspace_bytes(B, N, M, D)))
    f32 = dict(dtype=torch.float32, device=dev)
    full = torch.empty((B, M, H, W), **f32)
    ms, ds = torch.empty((B, M), **f32), torch.empty((B, M), **f32)
    iters = torch.empty((B,), dtype=torch.int32, device=dev)
    tables = None
    if return_tables:
        Pp = padded_width(N, M)
        tables = {"sim": torch.empty((B, M, N), **f32), "R": torch.empty((B, M, Pp), **f32),
                  "Rb": torch.empty((B, M, Pp), **f32)}
    tp = (lambda k: _ptr(tables[k])) if tables else (lambda k: None)
    _lib.call("dmm_match_forward_ws", dev, _ptr(masks_p), _ptr(masks_t), _DT[masks_p.dtype], _ptr(feat_p), _ptr(feat_t),
              _ptr(score_p), B, N, M, H * W, D, sp_b, sp_n, st_b, st_m, _ptr(n_valid), _ptr(m_valid), float(score_weight),
              int(max_iter), int(proj_iter), float(lr), int(is_test), _ptr(full), _ptr(ms), _ptr(ds), tp("sim"), tp("R"),
              tp("Rb"), _ptr(iters), _ptr(ws), ws.numel(), note, stream)
    if return_tables:
        return full, ms, ds, iters, tables
    return full, ms, ds, iters


def match_forward_frame(proposed_mask, mask_last, feat_p, feat_t, score_p, *, score_weight, max_iter, proj_iter, lr, is_test):
    """ONE frame exactly as the reference's evaluator hands it over (``MatchModel.forward`` without targets,
    dmm_model.py:75-77): proposed_mask [P,H,W], mask_last [O,H,W], feat_p [P,D], feat_t [O,D], score_p [P] ->
    (full_outmask [O,H,W], match_score [O], det_score [O]).  ``match_forward`` with B = 1 minus everything a one-frame
    call does not need on the HOST (the call is host bound otherwise): no unsqueeze / index views around the C call, no
    iteration-count or table outputs, three allocations."""
    _need_gpu(proposed_mask, mask_last, feat_p, feat_t, score_p)
    pm, tm = proposed_mask, mask_last
    assert pm.dtype == tm.dtype and pm.dtype in _DT and pm.dim() == 3 and tm.dim() == 3
    pm, tm = _plane_rows(pm), _plane_rows(tm)
    N, H, W = pm.shape
    M, D = tm.shape[0], feat_p.shape[-1]
    feat_p, feat_t, score_p = feat_p.contiguous().float(), feat_t.contiguous().float(), score_p.contiguous().float()
    dev = pm.device
    stream = torch.cuda.current_stream(dev).cuda_stream
    shape = (1, N, M, D)
    ws, note = _forward_ws(dev, stream, shape, _need_cached(shape, _lib.load().dmm_workspace_bytes, *shape))
    full = torch.empty((M, H, W), dtype=torch.float32, device=dev)
    ms = torch.empty((M,), dtype=torch.float32, device=dev)
    ds = torch.empty((M,), dtype=torch.float32, device=dev)
    _lib.call("dmm_match_forward_ws", dev, pm.data_ptr(), tm.data_ptr(), _DT[pm.dtype], feat_p.data_ptr(),
              feat_t.data_ptr(), score_p.data_ptr(), 1, N, M, H * W, D, N * pm.stride(0) if N else 0, pm.stride(0),
              M * tm.stride(0) if M else 0, tm.stride(0), None, None, score_weight, max_iter, proj_iter, lr, is_test,
              full.data_ptr(), ms.data_ptr(), ds.data_ptr(), None, None, None, None, ws.data_ptr(), ws.numel(), note, stream)
    return full, ms, ds


def match_train_forward(masks_p, masks_t, targets, feat_p, feat_t, score_p, n_valid, m_valid, *, score_weight, max_iter,
                        proj_iter, lr, is_test, one_frame=False, want_tape=True):
    """The training call of B frames as ONE C-ABI call (``dmm_match_train_forward``, include/dmm_match.h (5d)): feature
    similarity -> counts against templates AND targets -> solver -> mix -> matching loss.  masks_p: [B,N,H,W] tensor or
    ``FramePlanes``; targets [B,M,H,W] of the masks' dtype or None.  ``one_frame``: the tensors are ONE frame without the
    batch axis, as the reference's trainer hands them over (masks_p [N,H,W], masks_t / targets [M,H,W], feat_p [N,D],
    feat_t [M,D], score_p [N]) and so are the results -- no unsqueeze / select views around the call.  Returns None when the
    shape is outside the entry's envelope (the caller then runs the granular ops), else
    (full [B,M,H,W], match_score [B,M], det_score [B,M], cost_loss [B] | None, iters [B], saved, taped) with ``saved`` = the
    flat fp32 block cos | sim | Rb | gt (| the solver's tape, 256-byte aligned) that ``match_train_backward`` reads and
    ``taped`` = whether the forward's solver kernel kept its tape there (tables of <= 64 solver columns: the backward then
    does not re-run the solver).  ``want_tape=False`` (no gradient will be asked for): the untaped solver kernels."""
    p_ptr, dt, B, N, H, W, sp_b, sp_n, dev, _keep = _proposal_planes(masks_p, one_frame)
    masks_t, M, st_b, st_m = _batch_planes(masks_t, one_frame)
    D = feat_p.shape[-1]
    Pp = padded_width(N, M)
    if M > _lib.MAX_TEMPLATES or Pp > _lib.MAX_PROPOSALS or B > 65535 or N == 0 or M == 0 or B == 0 or dt not in _DT \
            or masks_t.dtype != dt:
        return None
    sg_b = sg_m = 0
    g_ptr = None
    if targets is not None:
        if targets.dtype != dt:
            targets = targets.to(dt)
        targets, _, sg_b, sg_m = _batch_planes(targets, one_frame)
        g_ptr = targets.data_ptr()
    L = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    need = _need_cached(("tf", B, N, M, D), L.dmm_match_train_forward_workspace_bytes, B, N, M, D)
    ws = _cached_ws((dev.index, stream, "train_fwd"), need, dev)
    f32 = dict(dtype=torch.float32, device=dev)
    lead = () if one_frame else (B,)
    full = torch.empty(lead + (M, H, W), **f32)
    ms, ds = torch.empty(lead + (M,), **f32), torch.empty(lead + (M,), **f32)
    loss = torch.empty(lead, **f32) if targets is not None else None
    iters = torch.empty((B,), dtype=torch.int32, device=dev)
    n_cs, n_rb = B * M * N, B * M * Pp
    tape_off, tape_bytes = _train_tape_layout(L, B, N, M, max_iter, proj_iter)
    if not want_tape:
        tape_bytes = 0
    saved = torch.empty((tape_off // 4 + tape_bytes // 4,), **f32)
    sp = saved.data_ptr()
    taped = ctypes.c_int(0)
    rc = _lib.call("dmm_match_train_forward", dev, p_ptr, masks_t.data_ptr(), g_ptr, _DT[dt], feat_p.data_ptr(),
                   feat_t.data_ptr(), score_p.data_ptr(), B, N, M, H * W, D, sp_b, sp_n, st_b, st_m, sg_b, sg_m,
                   _ptr(n_valid), _ptr(m_valid), score_weight, max_iter, proj_iter, lr, is_test, full.data_ptr(),
                   ms.data_ptr(), ds.data_ptr(), _ptr(loss), iters.data_ptr(), sp, sp + 4 * n_cs, sp + 8 * n_cs,
                   (sp + 8 * n_cs + 4 * n_rb) if targets is not None else None, ws.data_ptr(), ws.numel(),
                   (sp + tape_off) if tape_bytes else None, tape_bytes, ctypes.byref(taped), stream,
                   allow=(_lib.DMM_ERR_UNSUPPORTED,))
    if rc == _lib.DMM_ERR_UNSUPPORTED:                        # nothing was launched
        return None
    return full, ms, ds, loss, iters, saved, int(taped.value)


def _train_tape_layout(L, B, N, M, max_iter, proj_iter):
    """-> (byte offset of the solver's tape inside the training call's saved block, its size; 0 = not taped)."""
    k = ("tt", B, N, M, max_iter, proj_iter)
    got = _WS_NEED.get(k)
    if got is None:
        n_cs, n_rb = B * M * N, B * M * padded_width(N, M)
        off = -(-(4 * (3 * n_cs + n_rb)) // 256) * 256
        nbytes = int(L.dmm_match_train_tape_bytes(B, N, M, int(max_iter), int(proj_iter)))
        # the tape is sized for max_iter x proj_iter sweeps whatever the solver executes (the shipped default 400 x 50 is
        # 10 MB per frame, held until the backward): past _TAPE_MAX_BYTES per call the backward re-runs the solver instead
        got = _WS_NEED[k] = (off, nbytes if nbytes <= _TAPE_MAX_BYTES else 0)
    return got


_TAPE_MAX_BYTES = 32 << 20          # (held until the backward, per frame step alive in the autograd graph)


def match_train_backward(masks_p, feat_p, feat_t, score_p, saved, has_loss, d_full, d_ms, d_ds, d_loss, n_valid, m_valid,
                         M, *, score_weight, max_iter, proj_iter, lr, is_test, one_frame=False, iters=None, taped=0, det=None):
    """-> (g_feat_t [B,M,D], g_feat_p [B,N,D]): the whole backward of ``match_train_forward`` as ONE C-ABI call
    (``dmm_match_train_backward``, (5e)): normalise both feature sets -> mix backward -> taped solver backward ->
    feature-similarity backward.  ``saved`` is the forward's block; d_* may be None.  ``one_frame``: as in the forward.
    ``iters`` / ``taped``: the forward's iteration counts and its ``taped`` flag -- with them the solver's backward walks the
    tape inside ``saved`` instead of re-running the solver."""
    p_ptr, dt, B, N, H, W, sp_b, sp_n, dev, _keep = _proposal_planes(masks_p, one_frame)
    D = feat_p.shape[-1]
    Pp = padded_width(N, M)
    n_cs, n_rb = B * M * N, B * M * Pp
    L = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    if det is None:                       # (the _det entry: its mix backward folds a slab in a fixed order)
        det = is_deterministic()
    if det:                               # (its slab depends on the dispatch options too: sized per call, a host function)
        need = int(L.dmm_match_train_backward_det_workspace_bytes(B, N, M, D, max_iter, proj_iter, H * W))
    else:
        need = _need_cached(("tb", B, N, M, D, max_iter, proj_iter), L.dmm_match_train_backward_workspace_bytes, B, N, M, D,
                            max_iter, proj_iter)
    ws = _cached_ws((dev.index, stream, "train_bwd"), need, dev)
    d_full, d_ms, d_ds, d_loss = _cf(d_full), _cf(d_ms), _cf(d_ds), _cf(d_loss)
    use_loss = has_loss and d_loss is not None
    g_t, g_p = torch.empty_like(feat_t), torch.empty_like(feat_p)
    sp = saved.data_ptr()
    tape_off, tape_bytes = _train_tape_layout(L, B, N, M, max_iter, proj_iter)
    walk = bool(taped) and iters is not None and tape_bytes > 0 and saved.numel() * 4 >= tape_off + tape_bytes
    _lib.call("dmm_match_train_backward_det" if det else "dmm_match_train_backward", dev, p_ptr, _DT[dt], feat_p.data_ptr(),
              feat_t.data_ptr(), score_p.data_ptr(), sp if use_loss else None, sp + 4 * n_cs, sp + 8 * n_cs,
              (sp + 8 * n_cs + 4 * n_rb) if use_loss else None, _ptr(d_full), _ptr(d_ms), _ptr(d_ds),
              _ptr(d_loss) if use_loss else None, B, N, M, H * W, D, sp_b, sp_n, _ptr(n_valid), _ptr(m_valid), score_weight,
              max_iter, proj_iter, lr, is_test, g_t.data_ptr(), g_p.data_ptr(), ws.data_ptr(), ws.numel(),
              (sp + tape_off) if walk else None, _ptr(iters) if walk else None, int(walk), stream)
    return g_t, g_p


def _loss_planes(t: torch.Tensor):
    """[B,K,HW] or [B,K,H,W] -> (the tensor as the C ABI reads its planes, frame stride, plane stride, K, HW).  What passes
    ``_plane_rows`` goes in as it is: a ``y_mask[:, :n_obj]`` slice, ``alloc_planes`` strides."""
    if t.dim() == 3:
        t = t.unsqueeze(2)
    t, s_b, s_k = _planes(t)
    return t, s_b, s_k, t.shape[1], t.shape[2] * t.shape[3]


def mask_iou_loss(pred: torch.Tensor, target: torch.Tensor, sw: torch.Tensor, valid=None, n_obj=None, keep: bool = True):
    """The soft-IoU mask loss of the first ``n_obj`` planes of every frame with the logged hard IoU, two launches and no host
    read (``dmm_mask_iou_loss_fwd``, include/dmm_match.h (13): objectives.py:25-35 on hungarian.py:62-86, trainer.py:188-196 /
    :205-206 / :281-300).  pred [B,>=n_obj,HW] or [B,>=n_obj,H,W] fp32 probabilities; target the same with fp32 / fp16 / bf16
    values; sw [B,>=n_obj] sample weights; valid [B,O] or None (then the two hard scalars are 0); n_obj: target's planes by
    default.  -> (loss, hard_valid, hard_all: 0-dim; cost [B,n_obj]; hard [B,n_obj]; the workspace block
    ``mask_iou_loss_bwd`` reads).  ``keep``: the block is the caller's until its backward has run (a fresh tensor); False: no
    gradient will be asked for, the block is the cached one of (device, stream)."""
    _need_gpu(pred, target, sw, valid)
    assert pred.dtype == torch.float32 and target.dtype in _DT, (pred.dtype, target.dtype)
    pred, sb_p, so_p, Kp, HW = _loss_planes(pred)
    target, sb_t, so_t, Kt, HW_t = _loss_planes(target)
    B = pred.shape[0]
    n_obj = Kt if n_obj is None else int(n_obj)
    assert target.shape[0] == B and HW_t == HW and 0 < n_obj <= min(Kp, Kt) and B > 0 and HW > 0, (pred.shape, target.shape, n_obj)
    sw = sw.float()
    if sw.dim() != 2 or sw.stride(1) != 1:
        sw = sw.reshape(B, -1).contiguous()
    assert sw.shape[0] == B and sw.shape[1] >= n_obj, sw.shape
    O = n_obj
    if valid is not None:
        valid = valid.to(torch.int32).contiguous()
        O = valid.shape[1]
        assert valid.dim() == 2 and valid.shape[0] == B and O >= n_obj, valid.shape
    dev = pred.device
    stream = _stream(pred)
    need = _need_cached(("ml", B, n_obj, HW), _lib.load().dmm_mask_iou_loss_workspace_bytes, B, n_obj, HW)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev) if keep else _cached_ws((dev.index, stream, "mask_loss"), need, dev)
    R = B * n_obj
    out = torch.empty((3 + 2 * R,), dtype=torch.float32, device=dev)            # scalars | cost | hard: one allocation
    op = out.data_ptr()
    _lib.call("dmm_mask_iou_loss_fwd", dev, pred.data_ptr(), sb_p, so_p, target.data_ptr(), _DT[target.dtype], sb_t, so_t,
              sw.data_ptr(), sw.stride(0), _ptr(valid), B, O, n_obj, HW, op + 12, op + 12 + 4 * R, op, ws.data_ptr(), ws.numel(),
              stream)
    return out[0], out[1], out[2], out[3:3 + R].view(B, n_obj), out[3 + R:].view(B, n_obj), ws


def mask_iou_loss_bwd(target: torch.Tensor, ws: torch.Tensor, d_loss: torch.Tensor, pred_shape, n_obj: int) -> torch.Tensor:
    """d loss / d pred of ``mask_iou_loss`` in ``pred_shape``, one launch (``dmm_mask_iou_loss_bwd``): d_loss (0-dim, on the
    device) times the closed-form gradient for the first ``n_obj`` planes of every frame, zeros for the others.  ``target``
    and ``ws`` as the forward took and left them."""
    _need_gpu(target, ws, d_loss)
    target, sb_t, so_t, _Kt, HW = _loss_planes(target)
    B, O = int(pred_shape[0]), int(pred_shape[1])
    d_loss = d_loss.float().contiguous()
    dpred = torch.empty(tuple(pred_shape), dtype=torch.float32, device=target.device)
    _lib.call("dmm_mask_iou_loss_bwd", target.device, target.data_ptr(), _DT[target.dtype], sb_t, so_t, d_loss.data_ptr(), B, O,
              int(n_obj), HW, ws.data_ptr(), ws.numel(), dpred.data_ptr(), O * HW, HW, _stream(target))
    return dpred


def match_forward_packed(masks_p, packed_p, masks_t, feat_p, feat_t, score_p, n_valid, m_valid, *, score_weight, max_iter,
                         proj_iter, lr, is_test, out=None, workspace=None):
    """``match_forward`` with the proposal side of the cost pass on the 1-bit planes ``packed_p`` [B,N,words] the caller
    holds next to the soft planes (``proposals.ProposalSlots``); ``dmm_match_forward_packed``.  ``out`` = (full [B,M,H,W],
    match_score [B,M], det_score [B,M], iters [B]) and ``workspace`` (uint8) may be caller-owned: then nothing is
    allocated (a captured frame step).  Returns the ``out`` tuple."""
    _need_gpu(masks_p, packed_p, masks_t, feat_p, feat_t, score_p)
    assert masks_p.dtype == masks_t.dtype and masks_p.dtype in _DT and packed_p.dtype == torch.int64
    masks_p, sp_b, sp_n = _planes(masks_p)
    masks_t, st_b, st_m = _planes(masks_t)
    B, N, H, W = masks_p.shape
    M, D = masks_t.shape[1], feat_p.shape[-1]
    assert packed_p.is_contiguous() and packed_p.shape == (B, N, pack_words(H * W))
    assert feat_p.is_contiguous() and feat_t.is_contiguous() and score_p.is_contiguous()
    assert feat_p.dtype == feat_t.dtype == score_p.dtype == torch.float32
    dev = masks_p.device
    L = _lib.load()
    need = int(L.dmm_workspace_bytes_packed(B, N, M, D, H * W))
    if workspace is None:
        workspace = _cached_ws((dev.index, _stream(masks_p), "packed"), need, dev)
    assert workspace.numel() >= need
    if out is None:
        f32 = dict(dtype=torch.float32, device=dev)
        out = (torch.empty((B, M, H, W), **f32), torch.empty((B, M), **f32), torch.empty((B, M), **f32),
               torch.empty((B,), dtype=torch.int32, device=dev))
    full, ms, ds, iters = out
    assert full.is_contiguous() and full.shape == (B, M, H, W) and full.dtype == torch.float32
    wd = packed_p.shape[2]
    _lib.call("dmm_match_forward_packed", dev, _ptr(masks_p), _ptr(packed_p), _ptr(masks_t), _DT[masks_p.dtype],
              _ptr(feat_p), _ptr(feat_t), _ptr(score_p), B, N, M, H * W, D, sp_b, sp_n, N * wd, wd, st_b, st_m, _ptr(n_valid),
              _ptr(m_valid), float(score_weight), int(max_iter), int(proj_iter), float(lr), int(is_test), _ptr(full),
              _ptr(ms), _ptr(ds), None, None, None, _ptr(iters), _ptr(workspace), workspace.numel(), _stream(masks_p))
    return out


def match_solve_packed(packed_p, packed_t, feat_p, feat_t, score_p, n_valid, m_valid, HW, *, score_weight, max_iter,
                        proj_iter, lr, is_test, out, workspace):
    """Cost + assignment on 1-bit planes of BOTH sides, no mix (``dmm_match_solve_packed``): packed_p [B,N,words],
    packed_t [B,M,words]; ``out`` = (Rb [B,M,Pp], match_score [B,M], det_score [B,M], iters [B]) caller-owned, like the
    workspace (>= dmm_workspace_bytes): nothing is allocated -- the middle of a captured frame step."""
    _need_gpu(packed_p, packed_t, feat_p, feat_t, score_p)
    B, N, wd = packed_p.shape
    M, D = packed_t.shape[1], feat_p.shape[-1]
    assert packed_p.is_contiguous() and packed_t.is_contiguous() and packed_t.shape == (B, M, wd) and wd == pack_words(HW)
    assert feat_p.is_contiguous() and feat_t.is_contiguous() and score_p.is_contiguous()
    Rb, ms, ds, iters = out
    assert Rb.is_contiguous() and Rb.shape == (B, M, padded_width(N, M))
    assert workspace.numel() >= int(_lib.load().dmm_workspace_bytes(B, N, M, D))
    _lib.call("dmm_match_solve_packed", packed_p.device, _ptr(packed_p), _ptr(packed_t), _ptr(feat_p), _ptr(feat_t),
              _ptr(score_p), B, N, M, int(HW), D, _ptr(n_valid), _ptr(m_valid), float(score_weight), int(max_iter),
              int(proj_iter), float(lr), int(is_test), _ptr(Rb), _ptr(ms), _ptr(ds), None, None, _ptr(iters),
              _ptr(workspace), workspace.numel(), _stream(packed_p))
    return out


def match_solve_packed_hun(packed_p, packed_t, feat_p, feat_t, score_p, n_valid, m_valid, HW, *, score_weight, is_test,
                           out, status, workspace):
    """``match_solve_packed`` with the exact assignment (algo 'hun', ``dmm_match_solve_packed_hun``): ``out`` = (Rb,
    match_score, det_score, ...) and ``status`` [B] int32 caller-owned, nothing allocated or read (a captured step)."""
    _need_gpu(packed_p, packed_t, feat_p, feat_t, score_p)
    B, N, wd = packed_p.shape
    M, D = packed_t.shape[1], feat_p.shape[-1]
    assert packed_p.is_contiguous() and packed_t.is_contiguous() and packed_t.shape == (B, M, wd) and wd == pack_words(HW)
    assert feat_p.is_contiguous() and feat_t.is_contiguous() and score_p.is_contiguous()
    Rb, ms, ds = out[:3]
    assert Rb.is_contiguous() and Rb.shape == (B, M, padded_width(N, M))
    assert status.dtype == torch.int32 and status.is_contiguous() and status.shape == (B,)
    assert workspace.numel() >= int(_lib.load().dmm_workspace_bytes(B, N, M, D))
    _lib.call("dmm_match_solve_packed_hun", packed_p.device, _ptr(packed_p), _ptr(packed_t), _ptr(feat_p), _ptr(feat_t),
              _ptr(score_p), B, N, M, int(HW), D, _ptr(n_valid), _ptr(m_valid), float(score_weight), int(is_test),
              _ptr(Rb), _ptr(ms), _ptr(ds), None, None, _ptr(status), _ptr(workspace), workspace.numel(),
              _stream(packed_p))
    return out


# what one ``ForwardPlan.run`` hands to its launches: the checked inputs, the planes' dtype code and strides, and
# cfg = (score_weight, max_iter, proj_iter, lr, is_test) as the C ABI takes them
_PlanRun = namedtuple("_PlanRun", "masks_p masks_t feat_p feat_t score_p dt sp_b sp_n st_b st_m n_valid m_valid cfg")


class ForwardPlan:
    """Pre-allocated forward of B same-shaped frames: nothing is allocated or synchronised per call.

    Two execution shapes:

    * ``pipeline=False`` -- one ``dmm_match_forward`` C call, all kernels back to back on the current stream;
      With ``graph=True`` (small batches, where a frame step is launch / latency bound) the sequence is captured into
      a HIP graph the second time in a row ``run`` sees the same tensors (same addresses and strides) and replayed
      from then on -- one graph launch instead of 7 kernel launches (``graph_fork=True`` also runs the two independent
      branches of the layer, IoU counts (masks) | feature similarity, side by side before the solver joins them).
      Up to 4 tensor sets are kept (each captured graph holds references to its tensors); other calls launch directly.
    * ``pipeline=True``  -- "streaming lane + latency lane".  The batch is split in two halves A, B.  The
      current stream runs only the HBM-bound kernels, serialised at full bandwidth:
      cost(A) -> cost(B) -> mix(A) -> mix(B)  (A, B = the two halves of the batch).  A side stream runs the latency-bound ones:
      normalise + cosine (all frames) -> solver(A) (after cost(A)) -> solver(B) (after cost(B)).
      solver(A) hides under cost(B), solver(B) under mix(A); HIP events carry the dependencies, there is no
      host synchronisation, and every output is complete in current-stream order when ``run`` returns.
    """

    def __init__(self, B, N, M, H, W, D, device, mask_dtype=torch.float32, want_tables=False, pipeline=None,
                 split=0.5, time_kernels=False, graph=None, out_dtype=None, parts=2, graph_fork=False,
                 solver_state="f32", out_plane_align=0):
        self.B, self.N, self.M, self.H, self.W, self.D = B, N, M, H, W, D
        self.Pp = padded_width(N, M)
        self.device = torch.device(device)
        self.mask_dtype = mask_dtype
        # "f16": dmm_relax_match_f16s (packed-fp16 solver state, fp32 sums; opt-in tolerance mode of BASELINE configs[4]).
        # Its <= 128 VGPRs let it share a SIMD with the streaming kernels, so wide tables can take the 2-lane schedule.
        assert solver_state in ("f32", "f16")
        self.solver_state = solver_state
        self.solver_entry = "dmm_relax_match_f32" if solver_state == "f32" else "dmm_relax_match_f16s"
        # default: two lanes for large batches whose solver fits beside the streaming kernels (one wave per frame, exact
        # row count: M <= 16, Pp <= 64); the multi-wave solvers of wide tables hold up to 256 VGPRs per wave and only
        # serialise with them (config 5, fp32 state: 2.26 ms single stream vs 2.37 ms two lanes per 256 frames)
        # (round 5, tools/config5_probe.py: with the fp16-state solver the wide tables of config 5 run 3.05 ms per 512 frames
        # on one stream against 3.08-3.46 on two lanes -- the solver's waves slow the CUs they land on and the statically
        # partitioned count launch waits for its slowest CU -- so wide tables take one stream whatever the solver state)
        auto = B >= 64 and M <= 16 and self.Pp <= 64
        self.pipeline = auto if pipeline is None else bool(pipeline)
        # time_kernels: the single-stream form issues the granular C-ABI calls (same kernels as dmm_match_forward) so
        # that HIP events can bracket the cost and mix launches; bench.py sets kernel_events = {} per timed step
        # out_dtype: fp32 (default, the nn.Module boundary) or the planes' own 16-bit type (config 5: the matched masks
        # are the next frame's fp16 templates); the fused single C call writes fp32 only -> granular launches otherwise
        self.out_dtype = out_dtype or torch.float32
        assert self.out_dtype in (torch.float32, mask_dtype)
        self.time_kernels = bool(time_kernels) or self.out_dtype != torch.float32 or solver_state != "f32"
        self.kernel_events = None
        # opt-in: it only pays for callers that present the SAME tensors again (static buffers: bench loops, serving
        # loops over GraphedEncoder outputs); a frame loop with fresh proposal tensors would capture and never replay
        self.graph_mode = bool(graph) and not self.pipeline and not self.time_kernels
        # graph_fork: feature branch on a second stream inside the captured graph.  It paid while the feature similarity
        # took as long as the counts (18 us vs 19 us at B = 1); with the lanes kernel (10 us) and the small-chunk count
        # launch (round 2) the ~18 us a cross-queue fork + join costs is more than the branch saves: default off
        self.graph_fork = bool(graph_fork)
        self._graphs, self._last_key = {}, None                   # key -> (graph, tensors it holds addresses of, ws in / out)
        # dmm_match_forward_ws: what the last call of this plan left in ITS workspace (DMM_WS_UNKNOWN / _TABLES_ZERO).
        # From _TABLES_ZERO a handful of dense frames start their counts without a clearing launch (include/dmm_match.h 5a').
        self._ws_state = ctypes.c_int(0)
        L = _lib.load()
        f32 = dict(dtype=torch.float32, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        # out_plane_align: plane stride of full_outmask rounded up to that many bytes (alloc_planes) -- the matched masks of
        # config 5 are the next frame's 16-bit templates, so their producer writes them line aligned
        if out_plane_align:
            self.full_outmask = alloc_planes(B, M, H, W, self.out_dtype, self.device, int(out_plane_align))
        else:
            self.full_outmask = torch.empty((B, M, H, W), dtype=self.out_dtype, device=self.device)
        self.so_b, self.so_m = self.full_outmask.stride(0), self.full_outmask.stride(1)
        # the fused C call writes contiguous fp32 only: aligned output planes take the granular launches -- which cannot be
        # the graph-replay form, so asking for both is an error rather than a silent downgrade
        if out_plane_align and graph:
            raise ValueError("ForwardPlan(out_plane_align=..., graph=True): line-aligned output planes are written by the "
                             "granular launches only (no HIP-graph replay); drop one of the two")
        self.time_kernels = self.time_kernels or bool(out_plane_align)
        self.graph_mode = self.graph_mode and not out_plane_align
        self.match_score = torch.empty((B, M), **f32)
        self.det_score = torch.empty((B, M), **f32)
        self.iters = torch.empty((B,), **i32)
        self.sim = torch.empty((B, M, N), **f32)
        self.R = torch.empty((B, M, self.Pp), **f32) if want_tables else None
        self.Rb = torch.empty((B, M, self.Pp), **f32)
        if not self.pipeline:
            self.ws_bytes = int(L.dmm_workspace_bytes(B, N, M, D))
            self.workspace = torch.empty((self.ws_bytes,), dtype=torch.uint8, device=self.device)
            if self.time_kernels or self.graph_mode:
                if self.graph_mode:
                    with _lib.device_guard(self.device):
                        self.side = torch.cuda.Stream(device=self.device)
                self.counts = [torch.empty((B * (M * N + N + M),), **i32)]
                self.halves = [(0, B)]
                self.pn = torch.empty((B, N, D), **f32)
                self.tn = torch.empty((B, M, D), **f32)
                self.cos = torch.empty((B, M, N), **f32)
            return
        # ``parts`` equal slices of the batch (2 = halves A, B; with split != 0.5 the first slice takes that fraction).
        # Measured at B = 1024, config 2: 1:1 gives 255 k frames/s, 7:1 only 245 k (the normalise / cosine kernels then
        # overlap one long cost launch and slow it down by what they cost alone).
        parts = max(1, min(int(parts), B))
        if parts == 2 and B > 1:
            cut = min(B - 1, max(1, int(round(B * split))))
            self.halves = [(0, cut), (cut, B)]
        else:
            edges = [round(B * k / parts) for k in range(parts + 1)]
            self.halves = [(edges[k], edges[k + 1]) for k in range(parts) if edges[k + 1] > edges[k]]
        # inter | area_p | area_t of one half are contiguous -> one memset per cost launch
        self.counts = [torch.empty(((e - b) * (M * N + N + M),), **i32) for (b, e) in self.halves]
        self.pn = torch.empty((B, N, D), **f32)
        self.tn = torch.empty((B, M, D), **f32)
        self.cos = torch.empty((B, M, N), **f32)
        with _lib.device_guard(self.device):
            # (stream priorities make no measurable difference here: 261.1 / 262.0 k frames/s at priority 0 / -1)
            self.side = torch.cuda.Stream(device=self.device)
            self.ev_start = torch.cuda.Event()
            self.ev_cost = [torch.cuda.Event() for _ in self.halves]
            self.ev_solved = [torch.cuda.Event() for _ in self.halves]

    def schedule_name(self) -> str:
        if self.pipeline:
            return "streaming lane (cost, mix) + latency lane (normalise, cosine, solver) on 2 HIP streams" + \
                (" [fp16-state solver]" if self.solver_state == "f16" else "")
        if self.graph_mode:
            if not self._graphs:
                return "single stream (HIP graph armed: captured on the 2nd call with the same tensors)"
            return "HIP graph replay (IoU counts | feature similarity in parallel -> solver -> mix)" if self.graph_fork \
                else "HIP graph replay (feature similarity + IoU counts [one launch at <= 8 dense frames] -> solver -> mix, one chain)"
        return "single stream"

    def _launch_forked(self, r):
        """Granular launches, the form that is captured into the HIP graph (``graph_fork``: feature branch on the side
        stream, fork / join by stream waits)."""
        main = torch.cuda.current_stream(self.device)
        ms = main.cuda_stream
        if not self.graph_fork:
            # one chain: the fused C call (its feature-similarity launch also clears the count tables: no memset node)
            self._fused(r, None, ms)
            return
        side = self.side
        side.wait_stream(main)
        self._feature_sim(r.feat_p, r.feat_t, r.n_valid, r.m_valid, side.cuda_stream)
        self._counts(r, 0, self.B, ms)
        main.wait_stream(side)
        self._solve(r, 0, self.B, ms)
        self._mix(r, 0, self.B, ms)

    # ---- the launches: one method each, on the frames [b, e) of the batch (the whole batch is (0, B): every offset zero) ----
    @staticmethod
    def _at(t, b, per_frame):
        """Address of frame ``b`` in ``t``, ``per_frame`` elements a frame (None stays None)."""
        return None if t is None else t.data_ptr() + t.element_size() * b * per_frame

    def _counts(self, r, b, e, stream):
        inter, ap, at = self._tables(b, e)
        _lib.call("dmm_iou_counts", None, self._at(r.masks_p, b, r.sp_b), self._at(r.masks_t, b, r.st_b), r.dt, e - b, self.N,
                  self.M, self.H * self.W, r.sp_b, r.sp_n, r.st_b, r.st_m, self._at(r.n_valid, b, 1), self._at(r.m_valid, b, 1),
                  _ptr(inter), _ptr(ap), _ptr(at), stream)

    def _solve(self, r, b, e, stream):
        N, M, Pp, at_ = self.N, self.M, self.Pp, self._at
        inter, ap, at = self._tables(b, e)
        _lib.call(self.solver_entry, None, at_(self.cos, b, M * N), _ptr(inter), _ptr(ap), _ptr(at), at_(r.score_p, b, N), e - b,
                  N, M, at_(r.n_valid, b, 1), at_(r.m_valid, b, 1), *r.cfg, at_(self.sim, b, M * N), at_(self.R, b, M * Pp),
                  at_(self.Rb, b, M * Pp), at_(self.match_score, b, M), at_(self.det_score, b, M), at_(self.iters, b, 1), None,
                  stream)

    def _mix(self, r, b, e, stream):
        _lib.call("dmm_mask_mix_to", None, self._at(self.Rb, b, self.M * self.Pp), self._at(r.masks_p, b, r.sp_b), r.dt, e - b,
                  self.N, self.M, self.Pp, self.H * self.W, r.sp_b, r.sp_n, self._at(r.n_valid, b, 1), self._at(r.m_valid, b, 1),
                  self._at(self.full_outmask, b, self.so_b), _DT[self.out_dtype], self.so_b, self.so_m, stream)

    def _fused(self, r, guard, stream):
        """The whole batch as one ``dmm_match_forward_ws`` call on the plan's workspace (``guard``: the device to call under)."""
        _lib.call("dmm_match_forward_ws", guard, _ptr(r.masks_p), _ptr(r.masks_t), r.dt, _ptr(r.feat_p), _ptr(r.feat_t),
                  _ptr(r.score_p), self.B, self.N, self.M, self.H * self.W, self.D, r.sp_b, r.sp_n, r.st_b, r.st_m,
                  _ptr(r.n_valid), _ptr(r.m_valid), *r.cfg, _ptr(self.full_outmask), _ptr(self.match_score),
                  _ptr(self.det_score), _ptr(self.sim), _ptr(self.R), _ptr(self.Rb), _ptr(self.iters), _ptr(self.workspace),
                  self.ws_bytes, ctypes.byref(self._ws_state), stream)

    def _mark(self, name, stream, begin):
        """HIP event on ``stream`` before / after a kernel launch when bench.py asked for kernel timing."""
        if self.kernel_events is None:
            return
        e = torch.cuda.Event(enable_timing=True)
        e.record(stream)
        if begin:
            self.kernel_events.setdefault(name, []).append([e, None])
        else:
            self.kernel_events[name][-1][1] = e

    def _feature_sim(self, feat_p, feat_t, n_valid, m_valid, stream):
        """cos[B,M,N] into self.cos on ``stream``: the fused one-launch kernel for dense batches inside its envelope,
        normalise + normalise + cosine otherwise."""
        B, N, M, D = self.B, self.N, self.M, self.D
        if n_valid is None and m_valid is None:
            if _lib.call("dmm_cosine_features_f32", None, _ptr(feat_t), _ptr(feat_p), B, N, M, D, _ptr(self.cos), stream,
                         allow=(_lib.DMM_ERR_UNSUPPORTED,)) == _lib.DMM_OK:
                return
        _lib.call("dmm_feature_normalize_f32", None, _ptr(feat_p), B * N, D, _ptr(self.pn), None, stream)
        _lib.call("dmm_feature_normalize_f32", None, _ptr(feat_t), B * M, D, _ptr(self.tn), None, stream)
        _lib.call("dmm_cosine_f32", None, _ptr(self.tn), _ptr(self.pn), B, N, M, D, _ptr(n_valid), _ptr(m_valid),
                  _ptr(self.cos), stream)

    def _tables(self, b, e):
        """inter | area_p | area_t of the slice [b, e) (one of ``self.halves``)."""
        nb, M, N = e - b, self.M, self.N
        c = self.counts[self.halves.index((b, e))]
        return c[:nb * M * N], c[nb * M * N:nb * (M * N + N)], c[nb * (M * N + N):]

    def run(self, masks_p, masks_t, feat_p, feat_t, score_p, *, score_weight=0.3, max_iter=20, proj_iter=5, lr=0.1,
            is_test=1, n_valid=None, m_valid=None):
        _need_gpu(masks_p, masks_t, feat_p, feat_t, score_p)
        masks_p, sp_b, sp_n = _planes(masks_p)
        masks_t, st_b, st_m = _planes(masks_t)
        B, N, M, H, W = self.B, self.N, self.M, self.H, self.W
        assert masks_p.shape == (B, N, H, W) and masks_t.shape == (B, M, H, W)
        assert masks_p.dtype == self.mask_dtype and masks_t.dtype == self.mask_dtype
        assert feat_p.is_contiguous() and feat_t.is_contiguous() and score_p.is_contiguous()
        assert feat_p.dtype == torch.float32 and feat_t.dtype == torch.float32 and score_p.dtype == torch.float32
        cfg = (float(score_weight), int(max_iter), int(proj_iter), float(lr), int(is_test))
        r = _PlanRun(masks_p, masks_t, feat_p, feat_t, score_p, _DT[self.mask_dtype], sp_b, sp_n, st_b, st_m, n_valid, m_valid, cfg)
        if self.graph_mode and not torch.cuda.is_current_stream_capturing():
            key = (masks_p.data_ptr(), masks_t.data_ptr(), feat_p.data_ptr(), feat_t.data_ptr(), score_p.data_ptr(),
                   sp_b, sp_n, st_b, st_m, _ptr(n_valid), _ptr(m_valid), cfg)
            hit = self._graphs.get(key)
            # a captured call must find the workspace in the state it was captured with; if something else ran in between
            # (another tensor set, a direct call that took a different path) this call goes directly -- which heals it
            if hit is not None and hit[2] in (0, self._ws_state.value):
                hit[0].replay()
                self._ws_state.value = hit[3]
                return self.full_outmask, self.match_score, self.det_score
            if hit is None and key == self._last_key and len(self._graphs) < 4:
                # second call in a row on the same tensors: capture (the first one ran directly = the warm-up)
                ws_in = self._ws_state.value
                with _CAPTURE_LOCK, torch.cuda.device(self.device):
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, capture_error_mode="thread_local"):
                        self._launch_forked(r)
                ws_out = self._ws_state.value                       # what a replay leaves (nothing ran during the capture)
                self._ws_state.value = ws_in
                # the graph holds raw addresses: keep the tensors alive with it
                self._graphs[key] = (g, (masks_p, masks_t, feat_p, feat_t, score_p, n_valid, m_valid), ws_in, ws_out)
                g.replay()
                self._ws_state.value = ws_out
                return self.full_outmask, self.match_score, self.det_score
            self._last_key = key
        if not self.pipeline and self.time_kernels:
            with _lib.device_guard(self.device):
                main = torch.cuda.current_stream(self.device)
                ms = main.cuda_stream
                self._mark("cost", main, True)
                self._counts(r, 0, B, ms)
                self._mark("cost", main, False)
                self._feature_sim(feat_p, feat_t, n_valid, m_valid, ms)
                self._mark("solver", main, True)
                self._solve(r, 0, B, ms)
                self._mark("solver", main, False)
                self._mark("mix", main, True)
                self._mix(r, 0, B, ms)
                self._mark("mix", main, False)
            return self.full_outmask, self.match_score, self.det_score
        if not self.pipeline:
            self._fused(r, self.device, _stream(masks_p))
            return self.full_outmask, self.match_score, self.det_score

        with _lib.device_guard(self.device):
            main = torch.cuda.current_stream(self.device)
            side = self.side
            ms, ss = main.cuda_stream, side.cuda_stream
            self.ev_start.record(main)
            # ---- latency lane: normalise + cosine for every frame --------------------------------------------
            side.wait_event(self.ev_start)
            self._feature_sim(feat_p, feat_t, n_valid, m_valid, ss)
            # ---- streaming lane: cost(A), cost(B) ------------------------------------------------------------
            for h, (b, e) in enumerate(self.halves):
                self._mark("cost", main, True)
                self._counts(r, b, e, ms)
                self._mark("cost", main, False)
                self.ev_cost[h].record(main)
            # ---- latency lane: solver(h) as soon as cost(h) is done ------------------------------------------
            for h, (b, e) in enumerate(self.halves):
                side.wait_event(self.ev_cost[h])
                self._solve(r, b, e, ss)
                self.ev_solved[h].record(side)
            # ---- streaming lane: mix(A) after solver(A), mix(B) after solver(B) ------------------------------
            for h, (b, e) in enumerate(self.halves):
                main.wait_event(self.ev_solved[h])
                self._mark("mix", main, True)
                self._mix(r, b, e, ms)
                self._mark("mix", main, False)
        return self.full_outmask, self.match_score, self.det_score


# ---- the deterministic mode's own 3x3 convolution (include/dmm_match.h (10d)) -------------------------------------------
def conv3x3_bf16(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, stride: int = 1, *, out=None,
                 workspace=None) -> torch.Tensor:
    """3x3 / padding 1 convolution by ``dmm_conv3x3_bf16`` (MFMA implicit GEMM, fp32 accumulation, bias added in fp32, one
    rounding; deterministic: bit-identical call after call, and an image's result does not depend on its batch).
    x: [B, ci, H, W] bf16 channels-last; w: [co, ci, 3, 3] bf16 channels-last; bias: bf16 [co] or None -> y [B, co, Ho, Wo]
    bf16 channels-last.  The data gradient of the convolution is the same call on dy with the flipped, transposed weight
    (``flip(w, (2, 3)).transpose(0, 1)``; stride 2: on dy spread over zeros to the input's size, at stride 1).
    ``out`` / ``workspace`` (uint8, >= ``dmm_conv3x3_workspace_bytes``) may be caller-owned; by default both are fresh."""
    _need_gpu(x, w, bias)
    cl = torch.channels_last
    B, ci, H, W = x.shape
    co = w.shape[0]
    if x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16 or tuple(w.shape) != (co, ci, 3, 3):
        raise _lib.DmmError("conv3x3_bf16 takes bf16 x [B, ci, H, W] and w [co, ci, 3, 3]")
    if ci % 64 or co % 64 or ci <= 0 or co <= 0 or stride not in (1, 2):
        raise _lib.DmmError(f"conv3x3_bf16: ci = {ci}, co = {co}, stride = {stride} is outside the kernel's envelope")
    x, w = x.contiguous(memory_format=cl), w.contiguous(memory_format=cl)
    if bias is not None:
        if bias.dtype != torch.bfloat16 or tuple(bias.shape) != (co,):
            raise _lib.DmmError("conv3x3_bf16 takes a bf16 bias [co]")
        bias = bias.contiguous()
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if out is None:
        out = torch.empty((B, co, Ho, Wo), dtype=torch.bfloat16, device=x.device, memory_format=cl)
    elif tuple(out.shape) != (B, co, Ho, Wo) or out.dtype != torch.bfloat16 or not out.is_contiguous(memory_format=cl):
        raise _lib.DmmError("conv3x3_bf16: out must be bf16 channels-last [B, co, Ho, Wo]")
    need = _need_cached(("c3", B, H, W, ci, co, stride), _lib.load().dmm_conv3x3_workspace_bytes, B, H, W, ci, co, stride)
    if workspace is None and need:
        workspace = torch.empty((need,), dtype=torch.uint8, device=x.device)
    _lib.call("dmm_conv3x3_bf16", x.device, _ptr(x), _ptr(w), _ptr(bias), B, H, W, ci, co, int(stride), _ptr(out),
              _ptr(workspace) if need else None, workspace.numel() if need else 0, _stream(x))
    return out


def conv3x3_dgrad_bf16(dy: torch.Tensor, wt: torch.Tensor, in_hw: Tuple[int, int], stride: int = 1) -> torch.Tensor:
    """The data gradient of ``conv3x3_bf16(x, w, stride=stride)`` for x of ``in_hw`` = (H, W), as a forward convolution:
    ``wt`` = ``flip(w, (2, 3)).transpose(0, 1)`` ([ci, co, 3, 3] bf16 channels-last; ``dmm_wprep3x3_bf16``'s dstT) applied at
    stride 1 to dy -- at stride 2 to dy spread over zeros to [B, co, H, W] (``dmm_upsample2_zero_bf16``), which is exact:
    the taps that meet a zero contribute nothing."""
    _need_gpu(dy, wt)
    H, W = int(in_hw[0]), int(in_hw[1])
    B, co = dy.shape[0], dy.shape[1]
    if stride not in (1, 2) or tuple(dy.shape[2:]) != ((H - 1) // stride + 1, (W - 1) // stride + 1):
        raise _lib.DmmError("conv3x3_dgrad_bf16: dy does not belong to an input of in_hw at this stride")
    dy = dy.contiguous(memory_format=torch.channels_last)
    if stride == 2:
        if dy.dtype != torch.bfloat16:
            raise _lib.DmmError("conv3x3_dgrad_bf16 takes a bf16 dy")
        full = torch.empty((B, co, H, W), dtype=dy.dtype, device=dy.device, memory_format=torch.channels_last)
        _lib.call("dmm_upsample2_zero_bf16", dy.device, _ptr(dy), B, H, W, co, _ptr(full), _stream(dy))
        dy = full
    return conv3x3_bf16(dy, wt, None, 1)


# ---- the narrow 3x3 convolutions of the deterministic mode (include/dmm_match.h (10e)) -----------------------------------
def conv3x3_narrow_bf16(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *, out=None) -> torch.Tensor:
    """3x3 / padding 1 / stride 1 convolution by ``dmm_conv3x3_narrow_bf16`` for widths that are multiples of 32 (MFMA implicit
    GEMM, fp32 accumulation, bias added in fp32, one rounding; no split of the reduction and no workspace; deterministic:
    bit-identical call after call, and an image's result does not depend on its batch).
    x: [B, ci, H, W] bf16 channels-last; w: [co, ci, 3, 3] bf16 channels-last; bias: bf16 [co] or None -> y [B, co, H, W] bf16
    channels-last.  ``out`` may be caller-owned; by default it is fresh."""
    _need_gpu(x, w, bias)
    cl = torch.channels_last
    if x.dim() != 4 or w.dim() != 4:
        raise _lib.DmmError("conv3x3_narrow_bf16 takes bf16 x [B, ci, H, W] and w [co, ci, 3, 3]")
    B, ci, H, W = x.shape
    co = w.shape[0]
    if x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16 or tuple(w.shape) != (co, ci, 3, 3):
        raise _lib.DmmError("conv3x3_narrow_bf16 takes bf16 x [B, ci, H, W] and w [co, ci, 3, 3]")
    if ci % 32 or co % 32 or ci <= 0 or co <= 0:
        raise _lib.DmmError(f"conv3x3_narrow_bf16: ci = {ci}, co = {co} is outside the kernel's envelope")
    x, w = x.contiguous(memory_format=cl), w.contiguous(memory_format=cl)
    if bias is not None:
        if bias.dtype != torch.bfloat16 or tuple(bias.shape) != (co,):
            raise _lib.DmmError("conv3x3_narrow_bf16 takes a bf16 bias [co]")
        bias = bias.contiguous()
    if out is None:
        out = torch.empty((B, co, H, W), dtype=torch.bfloat16, device=x.device, memory_format=cl)
    elif tuple(out.shape) != (B, co, H, W) or out.dtype != torch.bfloat16 or not out.is_contiguous(memory_format=cl):
        raise _lib.DmmError("conv3x3_narrow_bf16: out must be bf16 channels-last [B, co, H, W]")
    _lib.call("dmm_conv3x3_narrow_bf16", x.device, _ptr(x), _ptr(w), _ptr(bias), B, H, W, ci, co, _ptr(out), _stream(x))
    return out


def conv3x3_narrow_dgrad_bf16(dy: torch.Tensor, wt: torch.Tensor) -> torch.Tensor:
    """The data gradient of ``conv3x3_narrow_bf16(x, w)`` as a forward convolution: at stride 1 / padding 1,
    dx[b, ci, h, w] = sum dy[b, co, h - kh + 1, w - kw + 1] * w[co, ci, kh, kw] is the same 3x3 / padding 1 convolution of dy
    with ``wt`` = ``flip(w, (2, 3)).transpose(0, 1)`` ([ci, co, 3, 3] bf16 channels-last; ``dmm_wprep3x3_bf16``'s dstT)."""
    return conv3x3_narrow_bf16(dy, wt, None)


def wgrad3x3_narrow_bf16(dy: torch.Tensor, x: torch.Tensor, *, out=None, workspace=None) -> torch.Tensor:
    """The weight gradient of ``conv3x3_narrow_bf16(x, w)`` by ``dmm_wgrad3x3_narrow_bf16``: dy [B, co, H, W] and x [B, ci, H, W]
    bf16 channels-last, widths multiples of 32 -> fp32 [co, ci, 3, 3] (the parameter's own layout), overwritten; implicit patch
    matrix, row slabs folded in a fixed order, no atomics.  ``out`` / ``workspace`` (uint8, >=
    ``dmm_wgrad3x3_narrow_workspace_bytes``) may be caller-owned; by default both are fresh."""
    _need_gpu(dy, x)
    cl = torch.channels_last
    if dy.dim() != 4 or x.dim() != 4 or dy.dtype != torch.bfloat16 or x.dtype != torch.bfloat16 \
            or dy.shape[0] != x.shape[0] or tuple(dy.shape[2:]) != tuple(x.shape[2:]):
        raise _lib.DmmError("wgrad3x3_narrow_bf16 takes bf16 dy [B, co, H, W] and x [B, ci, H, W]")
    B, ci, H, W = x.shape
    co = dy.shape[1]
    if ci % 32 or co % 32 or ci <= 0 or co <= 0:
        raise _lib.DmmError(f"wgrad3x3_narrow_bf16: ci = {ci}, co = {co} is outside the kernel's envelope")
    dy, x = dy.contiguous(memory_format=cl), x.contiguous(memory_format=cl)
    if out is None:
        out = torch.empty((co, ci, 3, 3), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (co, ci, 3, 3) or out.dtype != torch.float32 or not out.is_contiguous():
        raise _lib.DmmError("wgrad3x3_narrow_bf16: out must be fp32 contiguous [co, ci, 3, 3]")
    need = _need_cached(("w3n", B, H, W, ci, co), _lib.load().dmm_wgrad3x3_narrow_workspace_bytes, B, H, W, ci, co)
    if workspace is None:
        workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=x.device)
    _lib.call("dmm_wgrad3x3_narrow_bf16", x.device, _ptr(dy), _ptr(x), B, H, W, ci, co, _ptr(out), _ptr(workspace),
              workspace.numel(), _stream(x))
    return out


# ---- the 7x7 / stride 2 stem of the deterministic mode (include/dmm_match.h (10f)) ----------------------------------------
def _stem_image(x: torch.Tensor, what: str) -> torch.Tensor:
    if x.dim() != 4 or x.dtype != torch.bfloat16 or x.shape[1] != 3:
        raise _lib.DmmError(f"{what} takes a bf16 x [B, 3, H, W]")
    return x.contiguous(memory_format=torch.channels_last)


def conv7x7s2_stem_bf16(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *, out=None) -> torch.Tensor:
    """The 7x7 / stride 2 / padding 3 stem convolution (3 -> 64) by ``dmm_conv7x7s2_stem_bf16`` (MFMA implicit GEMM over 7 kernel
    rows x 32 lanes, 21 of them real; fp32 accumulation, bias added in fp32, one rounding; no split of the reduction and no
    workspace; deterministic: bit-identical call after call, and an image's result does not depend on its batch).
    x: [B, 3, H, W] bf16 channels-last; w: [64, 3, 7, 7] bf16 channels-last; bias: bf16 [64] or None -> y [B, 64, Ho, Wo] bf16
    channels-last, Ho = (H - 1) // 2 + 1.  ``out`` may be caller-owned; by default it is fresh."""
    _need_gpu(x, w, bias)
    cl = torch.channels_last
    x = _stem_image(x, "conv7x7s2_stem_bf16")
    if w.dtype != torch.bfloat16 or tuple(w.shape) != (64, 3, 7, 7):
        raise _lib.DmmError("conv7x7s2_stem_bf16 takes a bf16 w [64, 3, 7, 7]")
    w = w.contiguous(memory_format=cl)
    if bias is not None:
        if bias.dtype != torch.bfloat16 or tuple(bias.shape) != (64,):
            raise _lib.DmmError("conv7x7s2_stem_bf16 takes a bf16 bias [64]")
        bias = bias.contiguous()
    B, _, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if out is None:
        out = torch.empty((B, 64, Ho, Wo), dtype=torch.bfloat16, device=x.device, memory_format=cl)
    elif tuple(out.shape) != (B, 64, Ho, Wo) or out.dtype != torch.bfloat16 or not out.is_contiguous(memory_format=cl):
        raise _lib.DmmError("conv7x7s2_stem_bf16: out must be bf16 channels-last [B, 64, Ho, Wo]")
    _lib.call("dmm_conv7x7s2_stem_bf16", x.device, _ptr(x), _ptr(w), _ptr(bias), B, H, W, _ptr(out), _stream(x))
    return out


def wgrad7x7s2_stem_bf16(dy: torch.Tensor, x: torch.Tensor, *, out=None, workspace=None) -> torch.Tensor:
    """The weight gradient of ``conv7x7s2_stem_bf16(x, w)`` by ``dmm_wgrad7x7s2_stem_bf16``: dy [B, 64, Ho, Wo] and x [B, 3, H, W]
    bf16 channels-last -> fp32 [64, 3, 7, 7] (the parameter's own layout), overwritten; implicit patch matrix, pixel slabs
    folded in a fixed order, no atomics.  ``out`` / ``workspace`` (uint8, >= ``dmm_wgrad7x7s2_stem_workspace_bytes``) may be
    caller-owned; by default both are fresh."""
    _need_gpu(dy, x)
    x = _stem_image(x, "wgrad7x7s2_stem_bf16")
    B, _, H, W = x.shape
    if dy.dim() != 4 or dy.dtype != torch.bfloat16 or tuple(dy.shape) != (B, 64, (H - 1) // 2 + 1, (W - 1) // 2 + 1):
        raise _lib.DmmError("wgrad7x7s2_stem_bf16 takes a bf16 dy [B, 64, Ho, Wo] that belongs to x")
    dy = dy.contiguous(memory_format=torch.channels_last)
    if out is None:
        out = torch.empty((64, 3, 7, 7), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (64, 3, 7, 7) or out.dtype != torch.float32 or not out.is_contiguous():
        raise _lib.DmmError("wgrad7x7s2_stem_bf16: out must be fp32 contiguous [64, 3, 7, 7]")
    need = _need_cached(("w7s", B, H, W), _lib.load().dmm_wgrad7x7s2_stem_workspace_bytes, B, H, W)
    if workspace is None:
        workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=x.device)
    _lib.call("dmm_wgrad7x7s2_stem_bf16", x.device, _ptr(dy), _ptr(x), B, H, W, _ptr(out), _ptr(workspace), workspace.numel(),
              _stream(x))
    return out
