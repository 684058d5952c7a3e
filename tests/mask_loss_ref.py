"""Reference of the fused mask loss (include/dmm_match.h (13)), written from its formulas:

    I_r = sum p y      U_r = sum (p + y - p y) + 1e-6      cost_r = 1 - I_r / U_r
    sel_r = (uint8)sw_r != 0 if any sw > 0, else 1         K = sum sel_r         loss = (1 / K) sum sel_r cost_r
    hard_r = float(#(p > 0.5 & y > 0.5)) / (float(#(p > 0.5 | y > 0.5)) + 1e-6)
    nv = sum valid over all B * O slots;  hard_valid = sum hard_r valid_r / (nv + 1e-6), hard_all = sum hard_r / (nv + 1e-6)
    d loss / d p = sel_r / K * (I_r - (U_r + I_r) y) / U_r^2

``reference`` evaluates the soft part in fp64 (numpy) and the hard part exactly: integer counts, then the fp32 formula with
the one addition order the kernels document (a thread's rows r, r + 256, ... in ascending order, a balanced tree over each
wave's 64 lanes, waves in order), so the hard figures are compared BIT FOR BIT.  Also here: the case list of the GPU tests
and the bound rule (the decoder's: through fp64, against the stock fp32 form's own error).
"""
import numpy as np

F32 = np.float32
EPS32 = F32(1e-6)
HW_OF = lambda chunk: (1, 3, 35, 255, chunk - 1, chunk, chunk + 1, 2 * chunk + 5)      # 255 = 15 x 17: odd, 4-byte-aligned rows
BON = ((1, 1, 1), (2, 3, 3), (2, 5, 2), (4, 5, 5))                                     # (B, O, n_obj)
WEIGHTS = ("all", "none", "mixed", "one")
VALIDS = ("mixed", "zero")


def block_fold(vals):
    """fp32 sum of ``vals`` in the finish kernel's order: 256 threads, thread l adds rows l, l + 256, ... in ascending order;
    a balanced binary tree over the 64 lanes of each wave; waves 0..3 in order."""
    part = np.zeros(256, F32)
    for r, v in enumerate(np.asarray(vals, F32).reshape(-1)):
        part[r % 256] = part[r % 256] + v
    waves = []
    for w in range(4):
        v = part[64 * w:64 * w + 64].copy()
        while v.size > 1:
            v = v[0::2] + v[1::2]
        waves.append(v[0])
    t = waves[0]
    for w in waves[1:]:
        t = F32(t + w)
    return F32(t)


def selection(sw):
    """sel [B, n] (bool) from the weights of the compared planes: sw.byte() != 0 when any weight is > 0, else every row."""
    sw = np.asarray(sw, F32)
    if (sw > 0).any():
        return (np.trunc(sw).astype(np.int64) & 0xFF) != 0
    return np.ones(sw.shape, bool)


def hard_counts(pred, target):
    """[..., HW] x 2 -> (#(p > 0.5 & y > 0.5), #(p > 0.5 | y > 0.5)) int64 [...]; the operands as fp32 VALUES."""
    hp, hy = np.asarray(pred, F32) > F32(0.5), np.asarray(target, F32) > F32(0.5)
    return (hp & hy).sum(-1), (hp | hy).sum(-1)


def reference(pred, target, sw, valid, n_obj, g=1.0):
    """pred [B, Kp, HW] fp32, target [B, Kt, HW] (values), sw [B, >= n_obj], valid [B, O] int or None -> dict of the fp64 soft
    outputs (cost [B, n], loss, dpred [B, Kp, HW] for an upstream gradient g), the exact hard outputs in fp32 (hard [B, n],
    hard_valid, hard_all), and sel [B, n]."""
    pred, target = np.asarray(pred), np.asarray(target)
    B, Kp, HW = pred.shape
    n = int(n_obj)
    p, y = pred[:, :n].astype(np.float64), target[:, :n].astype(np.float64)
    I = (p * y).sum(-1)
    U = (p + y - p * y).sum(-1) + 1e-6
    cost = 1.0 - I / U
    sel = selection(np.asarray(sw)[:, :n])
    K = float(sel.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = np.float64(cost[sel].sum()) / K
        coef = np.where(sel, 1.0 / K if K else 0.0, 0.0)
    dpred = np.zeros(pred.shape, np.float64)
    dpred[:, :n] = g * coef[..., None] * (I[..., None] - (U + I)[..., None] * y) / (U * U)[..., None]
    ca, co = hard_counts(pred[:, :n], target[:, :n])
    hard = (ca.astype(F32) / (co.astype(F32) + EPS32)).astype(F32)
    if valid is None:
        nv, vn = F32(0), np.zeros((B, n), F32)
    else:
        valid = np.asarray(valid)
        nv, vn = block_fold(valid.astype(F32)), valid[:, :n].astype(F32)
    if nv > 0:
        hard_valid = F32(block_fold(hard * vn) / F32(nv + EPS32))
        hard_all = F32(block_fold(hard) / F32(nv + EPS32))
    else:
        hard_valid = hard_all = F32(0)
    return dict(cost=cost, loss=loss, dpred=dpred, hard=hard, hard_valid=hard_valid, hard_all=hard_all, sel=sel, I=I, U=U,
                counts=(ca, co))


def closed_form_gradient(pred, target, sw, n_obj, g=1.0):
    return reference(pred, target, sw, None, n_obj, g)["dpred"]


def make_case(B, O, n_obj, HW, weights="mixed", valids="mixed", seed=0):
    """Seeded inputs of one case (numpy): pred [B, O, HW] uniform in [0, 1.3) (train-mode full_outmask can exceed 1), target
    [B, O, HW] mostly binary with a few quarter values (exact in fp16 / bf16), a tenth of the pixels exactly 0.5 on both
    sides; with three rows or more, row 1 is empty on both sides and row 2 has an empty prediction and a non-empty target.
    sw [B, O] by ``weights`` (all / none / mixed / one set / 'frac': values in (0, 1) only), valid [B, O] int32 by ``valids``."""
    rng = np.random.RandomState(1000 * seed + 7 * HW + 131 * B + 17 * O + n_obj)
    pred = (rng.rand(B, O, HW) * 1.3).astype(F32)
    target = (rng.rand(B, O, HW) > 0.5).astype(F32)
    quarter = rng.rand(B, O, HW) < 0.05
    target[quarter] = rng.choice([0.25, 0.75], size=int(quarter.sum())).astype(F32)
    half = rng.rand(B, O, HW) < 0.1
    pred[half], target[half] = 0.5, 0.5
    if B * n_obj >= 3:
        rows = [(r // n_obj, r % n_obj) for r in (1, 2)]
        pred[rows[0]], target[rows[0]] = 0.0, 0.0
        pred[rows[1]] = 0.0
        target[rows[1]][0] = 1.0
    sw = np.zeros((B, O), F32)
    if weights == "all":
        sw[:] = 1.0
    elif weights == "mixed":
        sw[:] = (rng.rand(B, O) > 0.5).astype(F32)
        sw[0, 0], sw[-1, n_obj - 1] = 1.0, 0.0 if B * n_obj > 1 else 1.0
    elif weights == "one":
        sw[B - 1, n_obj - 1] = 1.0
    elif weights == "frac":
        sw[:] = 0.5
    else:
        assert weights == "none", weights
    valid = np.zeros((B, O), np.int32)
    if valids == "mixed":
        valid[:] = rng.rand(B, O) > 0.4
        valid[0, 0] = 1
    else:
        assert valids == "zero", valids
    return pred, target, sw, valid


def ulp(x):
    return float(np.spacing(F32(abs(float(x)))))


def bound(e_stock, largest):
    """The decoder rule: a kernel alone may be off by 2 e_stock + 1 ulp (fp32) of the largest output; e_stock = the stock
    fp32 form's own error against the fp64 evaluation of the same inputs.  Where e_stock is 0 the ulp carries it."""
    return 2.0 * float(e_stock) + ulp(largest)
