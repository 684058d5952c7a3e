#!/usr/bin/env python3
"""Capture the DAVIS-measures fixture ``measures.npz`` from the REFERENCE's own measures.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_measures.py <checkout of ZENGXH/DMM_Net>

Loads ``dmm/measures/jaccard.py``, ``f_boundary.py`` and ``statistics.py`` from the checkout by file path (the package's
``__init__`` pulls in more than the measures need) and calls ``db_eval_iou``, ``db_eval_boundary``, ``seg2bmap``, ``mean``,
``recall`` and ``decay`` on seeded label-map clips, per object as dmm/dataloader/evaluation.py:44-46 does (``an == obj_id``,
``sg == obj_id``).  Stored per clip: the two label maps, the radius (the reference's ``bound_pix`` expression on the frame
shape), and per (frame, object) the reference's J and F, its ``seg2bmap`` of both masks (bit-packed) and the four boundary
sums of f_boundary.py:52-57 -- n_fg, n_gt, sum(fg_match), sum(gt_match) -- taken with the reference's ``seg2bmap`` and the
same two morphology calls f_boundary.py:47-50 makes; the generator asserts that these sums give back the F the reference
returned.  Per object: mean, recall and decay over the scored J sequences, and over seeded sequences of every length from 4
to 40.  Data only: no reference source text is stored.

Two shims, neither of which holds arithmetic under test:
  * ``np.bool = bool`` -- only where numpy has no ``np.bool`` (1.24 to 1.26 dropped the alias the reference's
    ``astype(np.bool)`` uses; numpy 2 has the name again, as its own bool type, and is left alone).
  * ``skimage.morphology`` -- when skimage is absent, a stand-in module with ``disk(r)`` = the footprint ``x*x + y*y <= r*r``
    on ``arange(-r, r + 1)`` and ``binary_dilation(img, fp)`` = ``scipy.ndimage.binary_dilation(img, structure=fp)``, which is
    what skimage itself calls.  ``morphology`` in the file records which form was used ("skimage" or "scipy-stand-in").
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(ref, name):
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(ref, "dmm", "measures", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _morphology():
    try:
        import skimage.morphology  # noqa: F401
        return "skimage"
    except ImportError:
        from scipy import ndimage
        sk, mo = types.ModuleType("skimage"), types.ModuleType("skimage.morphology")

        def disk(radius):
            L = np.arange(-radius, radius + 1)
            X, Y = np.meshgrid(L, L)
            return np.array((X ** 2 + Y ** 2) <= radius ** 2, dtype=np.uint8)

        def binary_dilation(image, footprint=None):
            return ndimage.binary_dilation(image, structure=footprint)

        mo.disk, mo.binary_dilation, sk.morphology = disk, binary_dilation, mo
        sys.modules["skimage"], sys.modules["skimage.morphology"] = sk, mo
        return "scipy-stand-in"


def _blob(rng, H, W, cy, cx, ry, rx):
    """A seeded blob: an ellipse whose rim is roughened by a few harmonics."""
    y, x = np.mgrid[0:H, 0:W]
    ang = np.arctan2(y - cy, x - cx)
    rim = 1.0 + sum(rng.uniform(-0.18, 0.18) * np.cos(k * ang + rng.uniform(0, 6.28)) for k in (2, 3, 5))
    return ((y - cy) / max(ry, 0.5)) ** 2 + ((x - cx) / max(rx, 0.5)) ** 2 <= rim ** 2


def _annotation(rng, H, W, n_obj):
    """Objects that between them lie flush with all four edges and all four corners."""
    lab = np.zeros((H, W), dtype=np.uint8)
    spots = [(0, 0), (H - 1, W - 1), (H / 2, W / 2)]
    for o in range(n_obj):
        cy, cx = spots[o]
        lab[_blob(rng, H, W, cy + rng.uniform(-1, 1), cx + rng.uniform(-1, 1), H * rng.uniform(0.3, 0.45),
                  W * rng.uniform(0.3, 0.45))] = o + 1
    lab[0, W - 1] = lab[H - 1, 0] = n_obj                   # the other two corners
    return lab


def _shift(lab, dy, dx):
    out = np.zeros_like(lab)
    H, W = lab.shape
    ys, yd = (slice(0, H - dy), slice(dy, H)) if dy >= 0 else (slice(-dy, H), slice(0, H + dy))
    xs, xd = (slice(0, W - dx), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, W + dx))
    out[yd, xd] = lab[ys, xs]
    return out


def _clip(rng, T, H, W, n_obj):
    gt = np.stack([_annotation(rng, H, W, n_obj) for _ in range(T)])
    pred = np.zeros_like(gt)
    for t in range(T):
        kind = t % 4
        if kind == 0:                                       # the annotation, a few pixels off
            pred[t] = _shift(gt[t], int(rng.integers(-3, 4)), int(rng.integers(-3, 4)))
        elif kind == 1:                                     # an unrelated blob per object
            for o in range(n_obj):
                pred[t][_blob(rng, H, W, rng.uniform(0, H), rng.uniform(0, W), H * 0.3, W * 0.3)] = o + 1
        elif kind == 2:                                     # nothing
            pass
        else:                                               # everything is object 1
            pred[t] = 1
    return pred, gt


def main(ref):
    sys.dont_write_bytecode = True
    if not hasattr(np, "bool"):
        np.bool = bool
    form = _morphology()
    jac, fb, st = _load(ref, "jaccard"), _load(ref, "f_boundary"), _load(ref, "statistics")
    from skimage.morphology import binary_dilation, disk

    rng = np.random.default_rng(20261019)
    specs = [("c33x65", 6, 33, 65, 3), ("c96x128", 5, 96, 128, 2), ("c130x257", 3, 130, 257, 3), ("c75x100", 1, 75, 100, 2),
             ("c300x400", 1, 300, 400, 3), ("c1x70", 1, 1, 70, 2), ("c70x1", 1, 70, 1, 2), ("c1x1", 1, 1, 1, 2)]
    out = {"morphology": np.array(form), "clips": np.array([s[0] for s in specs])}
    for name, T, H, W, n_obj in specs:
        if min(H, W) == 1:
            gt = rng.integers(0, n_obj + 1, size=(T, H, W)).astype(np.uint8)
            pred = rng.integers(0, n_obj + 1, size=(T, H, W)).astype(np.uint8)
        else:
            pred, gt = _clip(rng, T, H, W, n_obj)
        bound_th = 0.008
        bound_pix = bound_th if bound_th >= 1 else np.ceil(bound_th * np.linalg.norm(gt[0].shape))
        J, F = np.zeros((n_obj, T)), np.zeros((n_obj, T))
        sums = np.zeros((T, n_obj, 4), dtype=np.int64)
        bmaps = np.zeros((T, n_obj, 2, H, W), dtype=bool)
        for t in range(T):
            for o in range(n_obj):
                an, sg = gt[t] == o + 1, pred[t] == o + 1
                J[o, t] = jac.db_eval_iou(an, sg)
                F[o, t] = fb.db_eval_boundary(sg, an, bound_th)
                fg_b, gt_b = fb.seg2bmap(sg), fb.seg2bmap(an)
                fg_dil, gt_dil = binary_dilation(fg_b, disk(bound_pix)), binary_dilation(gt_b, disk(bound_pix))
                n_fg, n_gt, fg_m, gt_m = np.sum(fg_b), np.sum(gt_b), np.sum(fg_b * gt_dil), np.sum(gt_b * fg_dil)
                sums[t, o] = (n_fg, n_gt, fg_m, gt_m)
                bmaps[t, o, 0], bmaps[t, o, 1] = fg_b, gt_b
                if n_fg > 0 and n_gt > 0:                   # the sums are the ones behind the reference's F
                    p, r = fg_m / float(n_fg), gt_m / float(n_gt)
                    assert F[o, t] == (0 if p + r == 0 else 2 * p * r / (p + r)), (name, t, o)
        out[name + "/pred"], out[name + "/gt"] = pred, gt
        out[name + "/n_obj"], out[name + "/radius"] = np.array(n_obj), np.array(int(bound_pix))
        out[name + "/J"], out[name + "/F"], out[name + "/sums"] = J, F, sums
        out[name + "/bmaps"] = np.packbits(bmaps.reshape(-1))
        if T >= 6:                                          # the statistics of the scored frames, evaluation.py:46-49
            for stat in ("mean", "recall", "decay"):
                out[f"{name}/J_{stat}"] = np.array([float(getattr(st, stat)(list(J[o, 1:-1]))) for o in range(n_obj)])
    for L in range(4, 41):
        X = rng.uniform(0, 1, size=L).round(3)
        X[rng.integers(0, L)] = 0.5                         # a value on the recall threshold
        out[f"stats/{L}/X"] = X
        for stat in ("mean", "recall", "decay"):
            out[f"stats/{L}/{stat}"] = np.array(float(getattr(st, stat)(list(X))))
    path = os.path.join(HERE, "measures.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", "morphology:", form)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
