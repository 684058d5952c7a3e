"""References for the refine step of training (no test functions here): closed forms of what ``dmm_mask_pyramid_bwd_f32``,
``dmm_upsample_bilinear_bwd_f32`` and ``dmm_refine_train_finish[_bwd]_f32`` compute, written dtype-generic in torch / numpy
so that they can be evaluated in fp64, and the trainer's object loop restated in torch ops.

* The pyramid: k nested ceil-mode 2x2 pools = the maximum over the clipped 2^k x 2^k window; under ATen's first-maximum
  rule applied pool by pool the gradient goes to the pixel that, among the window's maxima, has the smallest Z-ORDER code
  (bits of (y, x) inside the window interleaved, y above x).
* The bilinear upsample (align_corners = True): per axis every destination index touches source ``i0`` with ``l0`` and
  ``i0 + step`` with ``l1``; the backward gathers, per source index, over the contiguous range of destination indices that
  touch it.
* The finish: torch's default nearest interpolation reads source ``min(floor(dst * (in / out)), in - 1)``; the backward sums
  the contiguous block of destination pixels that read a source pixel, times p (1 - p).
"""
import numpy as np
import torch
import torch.nn.functional as F

LEVELS = (5, 4, 3, 2)                                            # coarsest first: the order of the pyramid's outputs


# ---- the pyramid ------------------------------------------------------------------------------------------------------
def zorder_codes(k):
    """[2^k, 2^k] int64: the Z-order code of (y, x), the y bit above the x bit at every level."""
    n = 1 << k
    y, x = torch.meshgrid(torch.arange(n), torch.arange(n), indexing="ij")
    code = torch.zeros(n, n, dtype=torch.int64)
    for bit in range(k):
        code |= (((y >> bit) & 1) << (2 * bit + 1)) | (((x >> bit) & 1) << (2 * bit))
    return code


def pyramid_winners(plane, k):
    """plane [..., H, W] -> (iy, ix) [..., hk, wk]: the pixel of every clipped 2^k window the gradient descends to."""
    H, W = plane.shape[-2:]
    n = 1 << k
    hk, wk = -(-H // n), -(-W // n)
    pad = F.pad(plane, (0, wk * n - W, 0, hk * n - H), value=float("-inf"))
    lead = pad.shape[:-2]
    win = pad.reshape(*lead, hk, n, wk, n).transpose(-3, -2).reshape(*lead, hk, wk, n * n)      # row-major inside a window
    code = zorder_codes(k).reshape(-1).to(plane.device)
    top = win.max(-1, keepdim=True)[0]
    best = torch.where(win == top, code, torch.full_like(code, n * n)).min(-1)[1]                # the maximum of least code
    iy = best // n + (torch.arange(hk, device=plane.device) * n).view(hk, 1)
    ix = best % n + (torch.arange(wk, device=plane.device) * n).view(1, wk)
    return iy, ix


def pyramid_bwd_closed_form(prev_mask, init_pred, d_outs, n_obj, H, W):
    """The planes [B, O, H*W | H, W] and the gradients of the four levels ([n_obj, B, 3, hk, wk], coarsest first, None =
    zeros) -> (d_prev, d_init) [B, n_obj, H, W] in the gradients' dtype (levels added in the order 2, 3, 4, 5)."""
    res = []
    for c, src in ((0, prev_mask), (2, init_pred)):
        B = src.shape[0]
        plane = src[:, :n_obj].reshape(B, n_obj, H, W)
        dtype = next(d.dtype for d in d_outs if d is not None)
        grad = torch.zeros(B * n_obj * H * W, dtype=dtype, device=plane.device)
        base = (torch.arange(B * n_obj, device=plane.device) * (H * W)).view(B, n_obj, 1, 1)
        for k, d in sorted(zip(LEVELS, d_outs)):
            if d is None:
                continue
            iy, ix = pyramid_winners(plane, k)
            g = d[:, :, c].transpose(0, 1)                                      # [B, n_obj, hk, wk]
            grad.index_put_(((base + iy * W + ix).reshape(-1),), g.reshape(-1), accumulate=True)
        res.append(grad.view(B, n_obj, H, W))
    return tuple(res)


def nested_pools(prev_mask, ref_mask, init_pred, n_obj, H, W):
    """The trainer's pools on all objects: -> 4 tensors [n_obj, B, 3, hk, wk], coarsest first."""
    B = prev_mask.shape[0]
    m = torch.stack([t[:, :n_obj].reshape(B, n_obj, H, W) for t in (prev_mask, ref_mask, init_pred)], 2)
    m = m.transpose(0, 1).reshape(n_obj * B, 3, H, W)
    m = F.max_pool2d(m, (2, 2), ceil_mode=True)
    out = []
    for _ in range(4):
        m = F.max_pool2d(m, (2, 2), ceil_mode=True)
        out.append(m.view(n_obj, B, 3, *m.shape[-2:]))
    return out[::-1]


# ---- the bilinear upsample ----------------------------------------------------------------------------------------------
def bilinear_taps(n_in, n_out, dtype=np.float64):
    """Per destination index: (i0, step, l0, l1) of align_corners = True, every operation rounded in ``dtype``."""
    one = dtype(1)
    scale = dtype(n_in - 1) / dtype(n_out - 1) if n_out > 1 else dtype(0)
    s = (scale * np.arange(n_out).astype(dtype)).astype(dtype)
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    step = (i0 < n_in - 1).astype(np.int64)
    l1 = (s - i0.astype(dtype)).astype(dtype)
    return i0, step, (one - l1).astype(dtype), l1


def gather_range(n_in, n_out, dtype=np.float64):
    """Per source index the first and last destination index that touches it, and whether all between do."""
    i0, step, _, _ = bilinear_taps(n_in, n_out, dtype)
    lo, hi, solid = [], [], True
    for i in range(n_in):
        touch = np.nonzero((i0 == i) | (i0 + step == i))[0]
        lo.append(int(touch[0]))
        hi.append(int(touch[-1]))
        solid = solid and len(touch) == touch[-1] - touch[0] + 1
    return lo, hi, solid


def bilinear_matrix(n_in, n_out, dtype, device="cpu"):
    """[n_out, n_in]: the weight of source i in destination o."""
    np_dtype = np.float32 if dtype == torch.float32 else np.float64
    i0, step, l0, l1 = bilinear_taps(n_in, n_out, np_dtype)
    m = np.zeros((n_out, n_in), dtype=np_dtype)
    o = np.arange(n_out)
    np.add.at(m, (o, i0), l0)
    np.add.at(m, (o, i0 + step), l1)
    return torch.from_numpy(m).to(device)


def bilinear_bwd_closed_form(d_dst, h, w):
    """d_dst [B, C, H, W] -> d_src [B, C, h, w] = My^T d_dst Mx in d_dst's dtype."""
    H, W = d_dst.shape[-2:]
    my, mx = bilinear_matrix(h, H, d_dst.dtype, d_dst.device), bilinear_matrix(w, W, d_dst.dtype, d_dst.device)
    return torch.einsum("Yy,bcYX,Xx->bcyx", my, d_dst, mx)


# ---- the finish -----------------------------------------------------------------------------------------------------------
def nearest_index(n_in, n_out):
    """Per destination index the source index torch's default (nearest) interpolation reads: fp32, as ATen computes it."""
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)


def train_finish_closed_form(logits, O, H, W):
    B, n_obj, h, w = logits.shape
    iy = torch.from_numpy(nearest_index(h, H)).to(logits.device)
    ix = torch.from_numpy(nearest_index(w, W)).to(logits.device)
    outs = logits.new_zeros((B, O, H, W))
    outs[:, :n_obj] = torch.sigmoid(logits[:, :, iy][:, :, :, ix])
    return outs


def train_finish_bwd_closed_form(logits, d_outs):
    B, n_obj, h, w = logits.shape
    H, W = d_outs.shape[-2:]
    iy = torch.from_numpy(nearest_index(h, H)).to(logits.device)
    ix = torch.from_numpy(nearest_index(w, W)).to(logits.device)
    rows = torch.zeros((B, n_obj, h, W), dtype=d_outs.dtype, device=logits.device).index_add_(2, iy, d_outs[:, :n_obj])
    acc = torch.zeros((B, n_obj, h, w), dtype=d_outs.dtype, device=logits.device).index_add_(3, ix, rows)
    p = torch.sigmoid(logits.to(d_outs.dtype))
    return p * (1 - p) * acc


# ---- the trainer's object loop ------------------------------------------------------------------------------------------
def trainer_refine(decoder, feats, prev_thid, init_pred, prev_mask, sw_mask, y_mask, valid, ref_mask, n_obj, only_temporal=False,
                   iou_weight=1.0):
    """The reference trainer's refine step restated in torch ops on ``decoder`` (whatever form its ``forward`` takes) ->
    (loss, {'hard_iou', 'loss_miou'}, outs_pad [B, O, HW], thid)."""
    from dmm_net_amd.losses import hard_iou, softIoULoss
    B, O, H, W = init_pred.shape
    HW = H * W
    spatial, thid, planes = None, [], []
    for t in range(n_obj):
        temporal = None
        if prev_thid is not None:
            assert len(prev_thid) == n_obj
            temporal = prev_thid[t]
            if only_temporal:
                spatial = None
        m = torch.cat([prev_mask[:, t].reshape(B, 1, HW), ref_mask[:, t].reshape(B, 1, HW), init_pred[:, t].reshape(B, 1, HW)],
                      dim=2).view(B, 3, H, W)
        m = F.max_pool2d(m, (2, 2), ceil_mode=True)
        pyr = []
        for _ in range(len(feats)):
            m = F.max_pool2d(m, (2, 2), ceil_mode=True)
            pyr.append(m)
        out_mask, hidden = decoder(feats, pyr[::-1], spatial, temporal)
        thid.append([hc[0] for hc in hidden])
        spatial = hidden
        planes.append(F.interpolate(out_mask, (H, W)).view(B, -1))
    out = torch.sigmoid(torch.cat(planes, 1).view(B, n_obj, -1))
    sw = sw_mask[:, :n_obj].contiguous().float()
    y = y_mask[:, :n_obj].contiguous()
    loss_miou = softIoULoss()(y.view(-1, HW), out.view(-1, HW), sw.view(-1, 1), need_sigmoid=0)
    with torch.no_grad():
        nv = valid.sum()
        hard = hard_iou(y.view(-1, HW), out.view(-1, HW)).view(B, n_obj)
        hard = hard.sum() / (nv + 1e-6) if nv > 0 else torch.zeros_like(hard).sum()
    outs_pad = out.new_zeros(B, O, HW)
    outs_pad[:, :n_obj] = out
    return iou_weight * loss_miou, {"hard_iou": hard, "loss_miou": loss_miou}, outs_pad, thid
