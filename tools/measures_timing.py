"""Times the DAVIS counts of one clip on the GPU against the host yardstick, and prints ONE JSON line.

    python tools/measures_timing.py [--out FILE] [--repeats 5] [--iters 10] [--host-frames 4]

36 frames x 3 objects at 480 x 854 and at 255 x 448 (blob annotations, predictions a few pixels off), the radius the
reference takes for the size (8 and 5).  Per size:
  device   ``measures.clip_counts`` on device label maps (dmm_davis_counts_u8: the clearing launch + the counts), HIP events,
           min / median / max over ``repeats`` windows of ``iters`` calls after a warm-up, in us per clip
  host     the wall time of tests/measures_ref.py's ``counts`` -- the full-footprint scipy.ndimage form -- on ONE thread of the
           same box, measured on the first ``host-frames`` frames and scaled to the clip (it is linear in the frames)
  bytes    what the kernel must read: 2 * T * H * W label bytes, times the passes it makes over them (one per object, times
           the halo rows and words a band re-reads: the tiling rule of include/dmm_match.h (14) evaluated here), against the
           median time
The device counts of the timed frames are compared with the host's before anything is reported."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import measures_ref  # noqa: E402
from dmm_net_amd import measures  # noqa: E402

LDS_WORDS = 1280          # csrc/dmm_measures.hip kMeasCap


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


def blobs(rng, T, H, W, n_obj):
    y, x = np.mgrid[0:H, 0:W]
    gt = np.zeros((T, H, W), dtype=np.uint8)
    for t in range(T):
        for o in range(n_obj):
            cy, cx = H * (0.25 + 0.25 * o) + 2 * t, W * (0.2 + 0.3 * o) + 3 * t
            ang = np.arctan2(y - cy, x - cx)
            rim = 1 + 0.2 * np.cos(3 * ang + t) + 0.1 * np.cos(7 * ang + o)
            gt[t][((y - cy) / (0.2 * H)) ** 2 + ((x - cx) / (0.15 * W)) ** 2 <= rim ** 2] = o + 1
    pred = np.roll(gt, (3, -4), axis=(1, 2))
    pred[:, :, : W // 8] = 0
    return pred, gt


def passes(H, W, radius, n_obj):
    """How often the kernel reads a label byte: per object, the in-image rows and words of every workgroup's region."""
    bh = min(H, min(64, max(16, 3 * radius + 8)))
    rows, wpr = bh + 2 * radius + 1, -(-W // 64)
    tw = min(wpr, LDS_WORDS // rows - 2)
    row_reads = sum(min(H, y0 + bh + radius + 1) - max(0, y0 - radius) for y0 in range(0, H, bh))
    word_reads = sum(min(wpr, c0 + tw + 1) - max(0, c0 - 1) for c0 in range(0, wpr, tw))
    return n_obj * (row_reads / H) * (word_reads / wpr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--host-frames", type=int, default=4)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "measures_timing needs an MI355X"
    torch.set_num_threads(1)
    T, n_obj = 36, 3
    res = {"what": "DAVIS counts of one clip", "frames": T, "objects": n_obj, "unit": "us per clip", "repeats": a.repeats,
           "iters": a.iters, "host_frames_measured": a.host_frames, "sizes": {}}
    for H, W in ((480, 854), (255, 448)):
        rng = np.random.default_rng(H)
        pred, gt = blobs(rng, T, H, W, n_obj)
        radius = measures.boundary_radius((H, W))
        dp, dg = torch.from_numpy(pred).to("cuda:0"), torch.from_numpy(gt).to("cuda:0")
        k = a.host_frames
        t0 = time.perf_counter()
        want = measures_ref.counts(pred[:k], gt[:k], n_obj, radius)
        host_s = (time.perf_counter() - t0) * T / k
        got = measures.clip_counts(dp, dg, n_obj).cpu().numpy()
        assert np.array_equal(got[:k], want), "device counts differ from the host yardstick"
        dev_us = windows(lambda: measures.clip_counts(dp, dg, n_obj), a.repeats, a.iters)
        p = passes(H, W, radius, n_obj)
        nbytes = 2 * T * H * W * p
        res["sizes"][f"{H}x{W}"] = {"radius": radius, "device_us": dev_us, "host_one_thread_s": host_s,
                                    "label_bytes": 2 * T * H * W, "passes": p, "bytes_read": nbytes,
                                    "bytes_per_s": nbytes / (dev_us["median"] * 1e-6)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
