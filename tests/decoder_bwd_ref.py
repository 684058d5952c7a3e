"""The closed-form backward of the fused LSTM cell (include/dmm_match.h (12e)) in torch ops, dtype-generic (no test
functions here).  It is what ``dmm_clstm_gates_bwd_f32`` implements, written the way the header states it: the gates are
recomputed from the cell's inputs, planes in the order 0, 2, 1; tests/test_decoder_train_cpu.py holds it against fp64 autograd
of ``gates_torch``, so the formulas are pinned without a device."""
import torch
import torch.nn.functional as F


def shifted(m, dy, dx):
    """m [B, h, w] -> s with s[b, y, x] = m[b, y + dy - 1, x + dx - 1], 0 outside the plane."""
    return F.pad(m, (1, 1, 1, 1))[:, dy:dy + m.shape[1], dx:dx + m.shape[2]]


def gates_bwd_closed_form(pre, masks, w_mask, cell_prev, d_hidden, d_cell):
    """-> (d_pre [B, 4*Hd, h, w], d_cell_prev [B, Hd, h, w] or None, d_masks [B, 3, h, w], d_w_mask [4*Hd, 9])."""
    B, C4, h, w = pre[0].shape
    Hd = C4 // 4
    g0 = pre[0]
    for p in pre[1:]:
        g0 = g0 + p
    zero = torch.zeros((B, Hd, h, w), dtype=g0.dtype, device=g0.device)
    u = zero if d_hidden is None else d_hidden / 3
    v = zero if d_cell is None else d_cell / 3
    wq = w_mask.view(4, Hd, 9)
    ds, dcr = {}, {}
    for k in (0, 2, 1):
        taps = torch.stack([shifted(masks[:, k], j // 3, j % 3) for j in range(9)], 1)           # [B, 9, h, w]
        s = g0.view(B, 4, Hd, h, w) + torch.einsum("qcj,bjyx->bqcyx", wq, taps)
        i, r, o, g = torch.sigmoid(s[:, 0]), torch.sigmoid(s[:, 1]), torch.sigmoid(s[:, 2]), torch.tanh(s[:, 3])
        c_k = i * g if cell_prev is None else r * cell_prev + i * g
        t_k = torch.tanh(c_k)
        dc = v + u * o * (1 - t_k * t_k)
        ds_in = dc * g * i * (1 - i)
        ds_rem = zero if cell_prev is None else dc * cell_prev * r * (1 - r)
        ds_out = u * t_k * o * (1 - o)
        ds_cell = dc * i * (1 - g * g)
        ds[k] = torch.stack([ds_in, ds_rem, ds_out, ds_cell], 1)                                  # [B, 4, Hd, h, w]
        dcr[k] = dc * r
    d_pre = ((ds[0] + ds[2]) + ds[1]).reshape(B, 4 * Hd, h, w)
    d_cell_prev = None if cell_prev is None else (dcr[0] + dcr[2]) + dcr[1]
    d_w = torch.zeros((4, Hd, 9), dtype=g0.dtype, device=g0.device)
    d_masks = torch.zeros((B, 3, h, w), dtype=g0.dtype, device=g0.device)
    for k in (0, 2, 1):
        for j in range(9):
            dy, dx = j // 3, j % 3
            d_w[:, :, j] += (ds[k] * shifted(masks[:, k], dy, dx)[:, None, None]).sum((0, 3, 4))
            # d_masks[y', x'] takes ds at (y' - dy + 1, x' - dx + 1): the shift by (2 - dy, 2 - dx)
            t = (ds[k] * wq[None, :, :, j, None, None]).sum((1, 2))                              # [B, h, w]
            d_masks[:, k] += shifted(t, 2 - dy, 2 - dx)
    return d_pre, d_cell_prev, d_masks, d_w.reshape(4 * Hd, 9)
