#!/usr/bin/env python3
"""Capture ``measures_resized.npz`` from the REFERENCE's own measures, called with predictions and annotations of DIFFERENT
shapes: the case in which jaccard.py:28-32 and f_boundary.py:34-38 resize the prediction with PIL's NEAREST first.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_measures_resized.py <checkout of ZENGXH/DMM_Net>

The loader of the reference's modules and the morphology stand-in are those of gen_golden_measures.py (imported, see its
docstring); PIL must be present.  Two clips of 3 frames and 3 objects: 24 x 40 -> 45 x 76 (up) and 16 x 20 -> 12 x 15 (down).
Stored per clip: the two label maps, the prediction resized as PIL makes it (``Image.fromarray(pred).resize((w, h),
Image.NEAREST)``; the generator asserts that every per-object binary resize the reference makes equals that map == id), the
radius (``bound_pix`` on the PREDICTION's shape, where f_boundary.py:30-31 takes it), and per (frame, object) the reference's
J and F and the four boundary sums n_fg, n_gt, sum(fg_match), sum(gt_match) behind its F.  The generator also asserts that on
each axis of each pair PIL's index table differs from floor((i + 0.5) * n_in / n_out).  Data only: no reference source text.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden_measures import _blob, _load, _morphology  # noqa: E402


def _pil_table(n_in, n_out):
    from PIL import Image
    ramp = np.arange(n_in, dtype=np.int32)[None, :]
    return np.array(Image.fromarray(ramp, "I").resize((n_out, 1), Image.NEAREST)).astype(np.int32)[0]


def _pil_resize(lab, H, W):
    from PIL import Image
    return np.array(Image.fromarray(lab.astype(np.uint8)).resize((W, H), Image.NEAREST))


def _labels(rng, H, W, n_obj):
    lab = np.zeros((H, W), dtype=np.uint8)
    spots = [(0, 0), (H - 1, W - 1), (H / 2, W / 2)]
    for o in range(n_obj):
        cy, cx = spots[o]
        lab[_blob(rng, H, W, cy + rng.uniform(-1, 1), cx + rng.uniform(-1, 1), H * rng.uniform(0.3, 0.45),
                  W * rng.uniform(0.3, 0.45))] = o + 1
    lab[0, W - 1] = lab[H - 1, 0] = n_obj
    return lab


def main(ref):
    sys.dont_write_bytecode = True
    if not hasattr(np, "bool"):
        np.bool = bool
    form = _morphology()
    jac, fb = _load(ref, "jaccard"), _load(ref, "f_boundary")
    from skimage.morphology import binary_dilation, disk

    rng = np.random.default_rng(20261020)
    specs = [("up24x40to45x76", 3, (24, 40), (45, 76), 3), ("down16x20to12x15", 3, (16, 20), (12, 15), 3)]
    out = {"morphology": np.array(form), "clips": np.array([s[0] for s in specs])}
    for name, T, (Hs, Ws), (H, W), n_obj in specs:
        for n_in, n_out in ((Hs, H), (Ws, W)):
            closed = np.floor((np.arange(n_out) + 0.5) * n_in / n_out).astype(np.int32)
            assert not np.array_equal(_pil_table(n_in, n_out), closed), (n_in, n_out)
        gt = np.stack([_labels(rng, H, W, n_obj) for _ in range(T)])
        pred = np.stack([_labels(rng, Hs, Ws, n_obj) for _ in range(T)])
        pred[1][pred[1] == 2] = 0                           # object 1 missing from one prediction
        bound_th = 0.008
        bound_pix = np.ceil(bound_th * np.linalg.norm(pred[0].shape))
        resized = np.stack([_pil_resize(pred[t], H, W) for t in range(T)])
        J, F = np.zeros((n_obj, T)), np.zeros((n_obj, T))
        sums = np.zeros((T, n_obj, 4), dtype=np.int64)
        for t in range(T):
            for o in range(n_obj):
                an, sg = gt[t] == o + 1, pred[t] == o + 1
                J[o, t] = jac.db_eval_iou(an, sg)
                F[o, t] = fb.db_eval_boundary(sg, an, bound_th)
                sg_r = _pil_resize(sg, H, W).astype(bool)   # what the reference itself resized
                assert np.array_equal(sg_r, resized[t] == o + 1), (name, t, o)
                fg_b, gt_b = fb.seg2bmap(sg_r), fb.seg2bmap(an)
                fg_dil, gt_dil = binary_dilation(fg_b, disk(bound_pix)), binary_dilation(gt_b, disk(bound_pix))
                n_fg, n_gt, fg_m, gt_m = np.sum(fg_b), np.sum(gt_b), np.sum(fg_b * gt_dil), np.sum(gt_b * fg_dil)
                sums[t, o] = (n_fg, n_gt, fg_m, gt_m)
                if n_fg > 0 and n_gt > 0:                   # the sums are the ones behind the reference's F
                    p, r = fg_m / float(n_fg), gt_m / float(n_gt)
                    assert F[o, t] == (0 if p + r == 0 else 2 * p * r / (p + r)), (name, t, o)
        out[name + "/pred"], out[name + "/gt"], out[name + "/resized"] = pred, gt, resized
        out[name + "/n_obj"], out[name + "/radius"] = np.array(n_obj), np.array(int(bound_pix))
        out[name + "/J"], out[name + "/F"], out[name + "/sums"] = J, F, sums
    path = os.path.join(HERE, "measures_resized.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", "morphology:", form)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
