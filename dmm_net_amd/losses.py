"""The mask losses of the trainer's frame step on the fused path: ``softIoULoss`` (the reference's criterion,
dmm/utils/objectives.py:25-35 on dmm/utils/hungarian.py:62-86) and ``mask_step_losses`` (the criterion plus the hard IoU the
trainer logs beside it: dmm/modules/trainer.py:188-196 + :205-206 on the matching layer's output, :281-300 on the refine
decoder's).

Device tensors with fp32 predictions go through ``dmm_mask_iou_loss_fwd`` / ``_bwd`` (include/dmm_match.h (13)): two
launches forward, one backward, no host read -- a frame step with its loss can be captured into a graph.  CPU tensors, and
predictions that are not fp32, run the STOCK form written here: the reference's tensor ops, with its
``masked_select(costs, sw.byte())`` read as the bool mask torch 1.x took it for (current torch refuses a uint8 mask).  The
stock form is also what the tests and ``tools/mask_loss_timing.py`` hold the fused path against.
"""
from __future__ import annotations

import torch
import torch.nn as nn


def soft_iou_costs(y_true: torch.Tensor, y_pred: torch.Tensor, e: float = 1e-6) -> torch.Tensor:
    """softIoU (hungarian.py:62-86) with need_sigmoid = 0: [R,HW], [R,HW] -> cost [R]."""
    num = (y_pred * y_true).sum(1, True)
    den = (y_pred + y_true - y_pred * y_true).sum(1, True) + e
    return (1 - num / den).view(-1)


def select_mean(costs: torch.Tensor, sw: torch.Tensor) -> torch.Tensor:
    """objectives.py:31-34: the mean over the rows whose weight is set, over all rows when none is (one host read)."""
    costs = costs.view(-1, 1)
    if (sw.data > 0).any():
        return torch.mean(torch.masked_select(costs, sw.view(-1, 1).byte().bool()))
    return torch.mean(costs)


def hard_iou(y_true: torch.Tensor, y_pred: torch.Tensor) -> torch.Tensor:
    """compute_iou_binary_mask_2D (match_helper.py:9-28): [R,HW], [R,HW] -> iou [R], no gradient."""
    with torch.no_grad():
        a, s = y_true > 0.5, y_pred > 0.5
        union = (a | s).float().sum(1) + 1e-6
        return (a & s).float().sum(1) / union


def _fused(pred: torch.Tensor) -> bool:
    return pred.is_cuda and pred.dtype == torch.float32


def _fused_target(t: torch.Tensor) -> torch.Tensor:
    return t if t.dtype in (torch.float32, torch.float16, torch.bfloat16) else t.float()


class softIoULoss(nn.Module):
    """The reference's criterion with the reference's call: ``forward(y_true [R,HW], y_pred [R,HW], sw [R,1],
    need_sigmoid=1)`` -> the mean cost of the selected rows.  ``need_sigmoid`` must be false, as softIoU asserts
    (hungarian.py:76-78)."""

    def forward(self, y_true, y_pred, sw, need_sigmoid=1):
        assert (not need_sigmoid), need_sigmoid
        if not _fused(y_pred):
            return select_mean(soft_iou_costs(y_true.to(y_pred.dtype), y_pred), sw)
        from .autograd import mask_iou_loss
        return mask_iou_loss(y_pred.unsqueeze(0), _fused_target(y_true).unsqueeze(0), sw.reshape(1, -1))[0]


def mask_step_losses_stock(y_mask, pred, sw_mask, tplt_valid, n_obj=None):
    """``mask_step_losses`` as the reference's tensor ops (two host reads)."""
    B, O = y_mask.shape[0], y_mask.shape[1]
    n = O if n_obj is None else int(n_obj)
    HW = y_mask[0, 0].numel()
    y = y_mask[:, :n].reshape(B * n, HW).to(pred.dtype)
    p = pred[:, :n].reshape(B * n, HW)
    cost = soft_iou_costs(y, p)
    loss = select_mean(cost, sw_mask[:, :n].reshape(-1, 1))
    with torch.no_grad():
        hard = hard_iou(y, p).view(B, n)
        nv = tplt_valid.sum()
        if nv > 0:
            hard_valid = (hard * tplt_valid[:, :n].float()).sum() / (nv + 1e-6)
            hard_all = hard.sum() / (nv + 1e-6)
        else:
            hard_valid = hard_all = torch.zeros_like(hard).sum()
    return loss, hard_valid, hard_all, cost.detach().view(B, n), hard


def mask_step_losses(y_mask, pred, sw_mask, tplt_valid, n_obj=None):
    """One call for the mask loss of a frame step and what the trainer logs with it.  y_mask [B,O,HW] (or [B,O,H,W]) targets,
    pred [B,>=n_obj,...] probabilities of the same plane size, sw_mask [B,O] sample weights, tplt_valid [B,O] valid flags;
    ``n_obj`` (default O): the leading planes of every frame that are compared, as the refine loss compares the decoder's
    ``total_obj`` outputs (trainer.py:281-283).  -> (loss, hard_valid, hard_all, cost [B,n_obj], hard [B,n_obj]):
      loss        the criterion's value, differentiable in ``pred``                   (trainer.py:205-206, :289-293)
      hard_valid  sum of hard IoU over valid templates / (number of valid + 1e-6)     (trainer.py:188-196, hard_iou1)
      hard_all    sum of hard IoU over the compared planes / (the same denominator)   (trainer.py:296-300, hard_iou0)
    Both hard figures are 0 when no template is valid."""
    if not _fused(pred):
        return mask_step_losses_stock(y_mask, pred, sw_mask, tplt_valid, n_obj)
    from .autograd import mask_iou_loss
    return mask_iou_loss(pred, _fused_target(y_mask), sw_mask, tplt_valid, n_obj)
