#!/usr/bin/env python3
"""Capture the clip-augmentation fixture ``augment.npz`` from the REFERENCE's own transforms.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_augment.py <checkout of ZENGXH/DMM_Net>

Loads ``dmm/dataloader/transforms/transforms.py`` and ``utils.py`` from the checkout by file path (as the two modules of a
stand-in package, so that the first can import the second; they need only torch and numpy) and ``dmm/utils/utils.py`` for
``binmask_to_bbox_xyxy_pt`` (its imports of yaml, torchvision and maskrcnn_benchmark, none of which that function touches, are
answered by empty stand-in modules where the real ones are absent).  Per clip it does what dmm/dataloader/dataset.py:168 and
:222-258 do:
  * seeds ``random``, draws the clip's flip (``random.random() < 0.5``), then per frame calls the reference's lazy
    ``RandomAffine`` (rotation 10, translation 0.1, shear 0.1, zoom (0.7, 1.4)) for the frame's matrix; the six parameters of
    every frame are drawn again from the same seed in the reference's order, and the generator asserts that the reference's
    ``Rotate . Translate . Shear . Zoom`` lazy chain on them gives the same matrix bit for bit;
  * after the drawn frames come the special ones: the identity, a translation that pushes every source coordinate past the
    edge, a 90-degree rotation;
  * flips image, annotation and masks with ``np.flip`` on axis 2 when the clip flips, warps them with
    ``Affine(m, interp='nearest')``, takes ``binmask_to_bbox_xyxy_pt((mask > 0.5).float())`` of every warped mask (``[]`` =
    empty: the input box stays, valid 0);
  * restates ``sequence_from_masks`` (dataset.py:300-338, the DAVIS branch; the dataset class itself needs the whole
    package) on the warped annotation for ``maxseqlen`` = F.  Every frame keeps a background pixel: see the deviation noted in
    dmm_net_amd/augment.py.
Stored: inputs, seed, flip, parameters, matrices, the warped planes, boxes with their valid flags, and the target rows.
Data only: no reference source text is stored.

Near-tie pixels (tests/augment_ref.py ``near_tie``: a clamped source coordinate, in float64, within 1e-3 of a half-integer) are
where a last-bit difference in the coordinate decides the neighbour.  The generator asserts that no frame of 1000 pixels or
more has above 1.5 % of them (pick another seed otherwise) and stores every frame's count; frames below 1000 pixels are exempt
from the share -- a 1 x 9 frame under the identity has none, under a half-pixel shift all nine.
"""
import importlib.util
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import augment_ref  # noqa: E402

RANGES = dict(rotation=10, translation=0.1, shear=0.1, zoom=(0.7, 1.4))


def _load_transforms(ref):
    d = os.path.join(ref, "dmm", "dataloader", "transforms")
    pkg = types.ModuleType("ref_tf")
    pkg.__path__ = [d]
    sys.modules["ref_tf"] = pkg
    mods = {}
    for name in ("utils", "transforms"):
        spec = importlib.util.spec_from_file_location("ref_tf." + name, os.path.join(d, name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules["ref_tf." + name] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods["transforms"]


def _load_box_utils(ref):
    for name, attrs in (("yaml", ()), ("torchvision", ("transforms",)), ("torchvision.transforms", ()),
                        ("maskrcnn_benchmark", ()), ("maskrcnn_benchmark.structures", ()),
                        ("maskrcnn_benchmark.structures.bounding_box", ("BoxList",))):
        try:
            importlib.import_module(name)
        except ImportError:
            m = types.ModuleType(name)
            for a in attrs:
                setattr(m, a, sys.modules.get(name + "." + a, None))
            sys.modules[name] = m
    spec = importlib.util.spec_from_file_location("ref_box_utils", os.path.join(ref, "dmm", "utils", "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _sequence_from_masks(annot, max_seq_len):
    """dataset.py:300-338, DAVIS branch, restated: float annotation [H,W] -> rows [max_seq_len, HW + 1] float64."""
    instance_ids = np.unique(annot)[1:]
    if len(instance_ids) > 0:
        instance_ids = instance_ids[:-1] if instance_ids[-1] == 255 else instance_ids
    h, w = annot.shape
    total = len(instance_ids)
    max_id = int(np.max(instance_ids)) if total > 0 else 0
    num = max(max_seq_len, max_id)
    gt_seg, sw = np.zeros((num, h * w)), np.zeros((num, 1))
    for i in range(total):
        k = int(instance_ids[i])
        aux = np.zeros((h, w))
        aux[annot == k] = 1
        gt_seg[k - 1, :] = np.reshape(aux, h * w)
        sw[k - 1] = 1
    return np.concatenate((gt_seg[:max_seq_len], sw[:max_seq_len]), axis=1)


def _inputs(rng, T, H, W, P, n_labels):
    """Image: channel 0 numbers the pixels (every gather is identifiable), the others are coarse ramps.  Annotation: blocks of
    labels 0 .. n_labels with 255 sprinkled in and a background pixel kept.  Masks: soft blobs on a 1/8 grid, 0.5 among them."""
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([np.stack([(y * W + x + t).astype(np.float32), ((y // 3) - t).astype(np.float32) * 0.5,
                              ((x // 5) + 2 * t).astype(np.float32) * 0.25]) for t in range(T)])
    lab = np.zeros((T, H, W), dtype=np.uint8)
    for t in range(T):
        bs = int(rng.choice([1, 3, 5]))
        coarse = rng.integers(0, n_labels + 1, size=(-(-H // bs), -(-W // bs)))
        coarse[rng.random(coarse.shape) < 0.35] = 0
        coarse[rng.random(coarse.shape) < 0.04] = 255
        lab[t] = np.kron(coarse, np.ones((bs, bs), dtype=np.int64))[:H, :W]
        lab[t, H // 2, W // 2] = lab[t, H - 1, 0] = lab[t, H - 1, W - 1] = 0      # (the all-clamped frame reads one corner)
    masks = np.zeros((T, P, H, W), dtype=np.float32)
    boxes = np.zeros((T, P, 4), dtype=np.float32)
    for t in range(T):
        for p in range(P):
            cy, cx = rng.uniform(0, H), rng.uniform(0, W)
            ry, rx = max(1.0, H * rng.uniform(0.1, 0.4)), max(1.0, W * rng.uniform(0.1, 0.4))
            d = ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2
            masks[t, p] = np.round(np.clip(1.25 - d, 0, 1) * 8) / 8
            if p == P - 1 and P > 1:
                masks[t, p] = np.minimum(masks[t, p], 0.5)  # never above the threshold: warps to "empty"
            boxes[t, p] = (rng.integers(0, W), rng.integers(0, H), W - 1, H - 1)
    return img, lab, masks, boxes


def main(ref):
    sys.dont_write_bytecode = True
    tf = _load_transforms(ref)
    box_utils = _load_box_utils(ref)
    rng = np.random.default_rng(20261019)
    # name, drawn frames, H, W, P, F, labels in the annotation, seed of `random`
    specs = [("c37x53_p6", 3, 37, 53, 6, 5, 6, 11), ("c37x53_p1", 2, 37, 53, 1, 1, 2, 17), ("c16x64_p0", 2, 16, 64, 0, 5, 5, 13),
             ("c1x1_p1", 1, 1, 1, 1, 1, 1, 14), ("c1x9_p6", 1, 1, 9, 6, 5, 3, 15), ("c9x1_p0", 1, 9, 1, 0, 1, 2, 19)]
    out = {"clips": np.array([s[0] for s in specs])}
    for name, T_drawn, H, W, P, F, n_labels, seed in specs:
        probe = torch.zeros(3, H, W)
        random.seed(seed)
        flip = random.random() < 0.5
        ra = tf.RandomAffine(rotation_range=RANGES["rotation"], translation_range=RANGES["translation"],
                             shear_range=RANGES["shear"], zoom_range=RANGES["zoom"], lazy=True)
        mats = [ra(probe) for _ in range(T_drawn)]
        random.seed(seed)                                   # the same draws again, by name
        assert (random.random() < 0.5) == flip
        params = []
        for t in range(T_drawn):
            deg = random.uniform(-RANGES["rotation"], RANGES["rotation"])
            dh = random.uniform(-RANGES["translation"], RANGES["translation"])
            dw = random.uniform(-RANGES["translation"], RANGES["translation"])
            sh = random.uniform(-RANGES["shear"], RANGES["shear"])
            zx = random.uniform(*RANGES["zoom"])
            zy = random.uniform(*RANGES["zoom"])
            params.append((deg, dh, dw, sh, zx, zy))
        # the special frames: identity | every source coordinate past the bottom-right edge | a quarter turn
        params += [(0.0, 0.0, 0.0, 0.0, 1.0, 1.0), (0.0, 1.0, 1.0, 0.0, 1.0, 1.0), (90.0, 0.0, 0.0, 0.0, 1.0, 1.0)]
        chain = []
        for deg, dh, dw, sh, zx, zy in params:
            m = tf.Rotate(deg, lazy=True)(probe)
            for step in (tf.Translate([dh, dw], lazy=True), tf.Shear(sh, lazy=True), tf.Zoom([zx, zy], lazy=True)):
                m = m.mm(step(probe))
            chain.append(m)
        for t in range(T_drawn):
            assert torch.equal(mats[t], chain[t]), (name, t)
        mats = chain
        T = len(mats)
        img, lab, masks, boxes_in = _inputs(rng, T, H, W, P, n_labels)

        w_img, w_lab, w_masks = np.empty_like(img), np.empty_like(lab), np.empty_like(masks)
        boxes, valid = boxes_in.copy(), np.zeros((T, P), dtype=np.int32)
        rows = np.zeros((T, F, H * W + 1))
        ties = np.zeros(T, dtype=np.int64)
        for t in range(T):
            i_t, a_t, m_t = img[t], lab[t][None], masks[t]
            if flip:                                        # dataset.py:222-225
                i_t, a_t, m_t = np.flip(i_t, axis=2).copy(), np.flip(a_t, axis=2).copy(), np.flip(m_t, axis=2).copy()
            fn = tf.Affine(mats[t], interp="nearest")
            o_img, o_annot = fn(torch.from_numpy(i_t), torch.from_numpy(a_t).float())
            w_img[t] = o_img.numpy()
            annot = o_annot.numpy().squeeze(0)
            w_lab[t] = annot.astype(np.uint8)
            assert (w_lab[t] == annot).all() and (w_lab[t] == 0).any()
            for p in range(P):
                bin_mask = fn(torch.from_numpy(m_t[p]).view(1, H, W))[0]
                w_masks[t, p] = bin_mask.numpy()
                bin_mask = (bin_mask > 0.5).float()
                if bin_mask.sum() == 0:
                    continue
                boxes[t, p] = box_utils.binmask_to_bbox_xyxy_pt(bin_mask.float())
                valid[t, p] = 1
            rows[t] = _sequence_from_masks(annot, F)
            ties[t] = int(augment_ref.near_tie(mats[t].numpy(), H, W).sum())
            if H * W >= 1000:
                assert ties[t] <= 0.015 * H * W, (name, t, ties[t], "pick another seed")
        print(f"{name}: flip {flip}, near-tie pixels per frame {ties.tolist()} of {H * W}, empty masks {int((valid == 0).sum())}")
        g = {"frames": img, "labels": lab, "masks": masks, "boxes_in": boxes_in, "seed": np.array(seed), "flip": np.array(flip),
             "drawn": np.array(T_drawn), "F": np.array(F), "params": np.array(params, dtype=np.float64),
             "matrices": torch.stack(mats).numpy(), "out_frames": w_img, "out_labels": w_lab, "out_masks": w_masks,
             "out_boxes": boxes, "out_box_valid": valid, "out_rows": np.packbits(rows.astype(bool).reshape(-1)),
             "near_tie": ties}
        assert np.isin(rows, (0.0, 1.0)).all()
        for k, v in g.items():
            out[f"{name}/{k}"] = v
    path = os.path.join(HERE, "augment.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < 200_000


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
