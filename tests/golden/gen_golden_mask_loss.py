#!/usr/bin/env python3
"""Capture the mask-loss fixture ``mask_loss.npz`` from the REFERENCE's own criterion.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_mask_loss.py <checkout of ZENGXH/DMM_Net>

Imports ``softIoULoss`` (dmm/utils/objectives.py) and ``compute_iou_binary_mask_2D`` (dmm/utils/match_helper.py) from the
checkout and calls them (torch CPU, fp32) on seeded inputs of at most 6 rows x 35 pixels with the sample weights all set,
none set and mixed.  Stored per case: the inputs, the criterion's value, softIoU's per-row costs, autograd's gradient of the
value with respect to the prediction, and the hard IoUs.  Data only: no reference source text is stored.

Two shims, neither of which holds arithmetic under test:
  * ``munkres`` -- dmm/utils/hungarian.py imports it at module level for its ``match`` helper, which nothing here calls; the
    package is absent, so an empty stand-in module with a ``Munkres`` name is installed.
  * ``torch.masked_select`` -- the criterion passes ``sw.byte()`` as the mask.  torch 1.x read a uint8 mask as a bool mask;
    current torch refuses it ("expected BoolTensor for mask").  The wrapper converts a uint8 mask with ``.bool()`` and
    passes everything else through: the torch 1.x meaning.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def main(ref):
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref)
    munkres = types.ModuleType("munkres")
    munkres.Munkres = type("Munkres", (), {})
    sys.modules.setdefault("munkres", munkres)
    stock_select = torch.masked_select

    def masked_select(input, mask, **kw):
        return stock_select(input, mask.bool() if mask.dtype == torch.uint8 else mask, **kw)

    torch.masked_select = masked_select
    from dmm.utils.objectives import softIoULoss
    from dmm.utils.hungarian import softIoU
    from dmm.utils.match_helper import compute_iou_binary_mask_2D

    crit = softIoULoss()
    out = {}
    g = torch.Generator().manual_seed(20261019)
    weights = {"all": [1, 1, 1, 1, 1, 1], "none": [0, 0, 0, 0, 0, 0], "mixed": [1, 0, 0, 1, 1, 0]}
    for name, w in weights.items():
        R, HW = 6, 35
        pred = (torch.rand(R, HW, generator=g) * 1.3).float()
        y = (torch.rand(R, HW, generator=g) > 0.5).float()
        half = torch.rand(R, HW, generator=g) < 0.1                  # pixels at exactly 0.5 on both sides
        pred[half], y[half] = 0.5, 0.5
        pred[1], y[1] = 0.0, 0.0                                     # both empty
        pred[2] = 0.0                                                # empty prediction, non-empty target
        sw = torch.tensor(w, dtype=torch.float32).view(-1, 1)
        p = pred.clone().requires_grad_(True)
        loss = crit(y, p, sw, need_sigmoid=0)
        loss.backward()
        out[name + "/pred"], out[name + "/target"], out[name + "/sw"] = pred.numpy(), y.numpy(), sw.numpy()
        out[name + "/loss"] = loss.detach().numpy()
        out[name + "/cost"] = softIoU(y, pred, need_sigmoid=0).detach().numpy()
        out[name + "/dpred"] = p.grad.numpy()
        out[name + "/hard"] = compute_iou_binary_mask_2D(y, pred).numpy()
    torch.masked_select = stock_select
    path = os.path.join(HERE, "mask_loss.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
