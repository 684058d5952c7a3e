"""Times the augmentation of one config-4 clip set on the GPU against the numpy restatement on the host, and prints ONE JSON line.

    python tools/augment_timing.py [--out FILE] [--repeats 5] [--iters 20] [--lib OTHER_BUILD.so]

12 frames of 255 x 448, C = 3 image planes, P = 50 proposal masks, F = 5 target planes; matrices drawn with the reference's
default ranges, the clip flipped.
  device   ``augment.augment_clip(..., out=...)`` on device tensors (dmm_augment_clip_f32: the clearing launch, the warp, the
           box finish), HIP events, min / median / max over ``repeats`` windows of ``iters`` calls after a warm-up, in us
  bytes    the algorithmic traffic: every input plane read once, every output plane, target plane and box written once --
             n * H * W * ((4 C + 1 + 4 P) + (4 C + 1 + 4 P + 4 F)) + n * P * (16 + 4) + n * F * 4
           (image and mask planes fp32, the annotation uint8, targets fp32; boxes fp32 x 4 with an int32 flag; sizes int32),
           against the median time and the 8 TB/s peak.  A gather does not read its input once -- lines are shared between
           neighbouring pixels and fetched again by other workgroups -- so this is a floor on the traffic, not a count of it.
  host     the wall time of tests/augment_ref.py's ``augment_clip`` for the same clip on ONE thread of the same box
``--lib``: load another build of the library (csrc/dmm_augment.hip compiled with another ``-DDMM_AUG_TILE_W=``, linked with the
same objects) instead of the in-tree one.  The device outputs are compared with the host's, byte for byte, before anything is reported."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import augment_ref  # noqa: E402
from dmm_net_amd import _lib, augment  # noqa: E402

PEAK_BYTES_PER_S = 8e12
STEP_MS = 13.31                                            # TrainEncoder's config-4 step (README)


def windows(fn, repeats, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(1e3 * a.elapsed_time(b) / iters)
    return {"min": min(out), "median": statistics.median(out), "max": max(out)}


def clip(n, C, H, W, P):
    rng = np.random.default_rng(4)
    y, x = np.mgrid[0:H, 0:W]
    frames = rng.standard_normal((n, C, H, W)).astype(np.float32)
    labels = np.zeros((n, H, W), dtype=np.uint8)
    masks = np.zeros((n, P, H, W), dtype=np.float32)
    for f in range(n):
        for o in range(3):
            cy, cx = H * (0.3 + 0.2 * o) + f, W * (0.2 + 0.3 * o) + 2 * f
            labels[f][((y - cy) / (0.2 * H)) ** 2 + ((x - cx) / (0.12 * W)) ** 2 <= 1] = o + 1
        for p in range(P):
            cy, cx, ry, rx = rng.uniform(0, H), rng.uniform(0, W), H * rng.uniform(0.05, 0.3), W * rng.uniform(0.05, 0.3)
            masks[f, p] = np.clip(1.3 - ((y - cy) / ry) ** 2 - ((x - cx) / rx) ** 2, 0, 1)
    boxes = np.zeros((n, P, 4), dtype=np.float32)
    return frames, labels, masks, boxes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "augment_timing needs an MI355X"
    if a.lib:
        _lib.use_library(a.lib)
    torch.set_num_threads(1)
    n, C, H, W, P, F = 12, 3, 255, 448, 50, 5
    frames, labels, masks, boxes = clip(n, C, H, W, P)
    flip, mats = augment.draw_clip_params(random.Random(4), n, H=H, W=W)
    flip = True
    t0 = time.perf_counter()
    want = augment_ref.augment_clip(frames, labels, masks, boxes, mats.numpy(), [flip] * n, F)
    host_s = time.perf_counter() - t0
    d = [torch.from_numpy(x).to("cuda:0") for x in (frames, labels, masks, boxes)]
    dm, df = mats.to("cuda:0"), torch.ones(n, dtype=torch.int32, device="cuda:0")
    out = augment.augment_clip(*d, matrices=dm, flip=df, max_obj=F)
    for k in ("frames", "labels", "masks", "boxes", "box_valid", "targets", "sizes"):
        assert np.array_equal(getattr(out, k).cpu().numpy(), want[k]), f"device {k} differs from the host restatement"
    dev_us = windows(lambda: augment.augment_clip(*d, matrices=dm, flip=df, max_obj=F, out=out), a.repeats, a.iters)
    nbytes = n * H * W * ((4 * C + 1 + 4 * P) + (4 * C + 1 + 4 * P + 4 * F)) + n * P * (16 + 4) + n * F * 4
    rate = nbytes / (dev_us["median"] * 1e-6)
    res = {"what": "augmentation of one config-4 clip set", "library": a.lib or "in-tree", "frames": n, "C": C, "P": P, "F": F,
           "H": H, "W": W, "unit": "us per clip set", "repeats": a.repeats, "iters": a.iters, "device_us": dev_us,
           "algorithmic_bytes": nbytes, "bytes_per_s": rate, "fraction_of_8TBps": rate / PEAK_BYTES_PER_S,
           "fraction_of_13.31ms_step": dev_us["median"] * 1e-3 / STEP_MS, "host_restatement_one_thread_s": host_s}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
