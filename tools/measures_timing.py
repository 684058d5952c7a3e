"""Times the DAVIS counts of one clip on the GPU against the host yardstick, and prints ONE JSON line.

    python tools/measures_timing.py [--out FILE] [--repeats 5] [--iters 10] [--host-frames 4] [--pred-size 255x448]

36 frames x 3 objects at 480 x 854 and at 255 x 448 (blob annotations, predictions a few pixels off), the radius the
reference takes for the size (8 and 5).  Per size:
  device   ``measures.clip_counts`` on device label maps (dmm_davis_counts_u8: the clearing launch + the counts), HIP events,
           min / median / max over ``repeats`` windows of ``iters`` calls after a warm-up, in us per clip
  host     the wall time of tests/measures_ref.py's ``counts`` -- the full-footprint scipy.ndimage form -- on ONE thread of the
           same box, measured on the first ``host-frames`` frames and scaled to the clip (it is linear in the frames)
  bytes    what the kernel must read: 2 * T * H * W label bytes, times the passes it makes over them (one per object, times
           the halo rows and words a band re-reads: the tiling rule of include/dmm_match.h (14) evaluated here), against the
           median time
The device counts of the timed frames are compared with the host's before anything is reported.

``--pred-size HsxWs`` adds "resized": the same clip's predictions at Hs x Ws scored against the 480 x 854 annotations
(include/dmm_match.h (14b), (14d), (14)), tables prebuilt, the radius the reference takes for the prediction's size:
  resize     (14d) ``dmm_resize_labels_nearest_u8`` alone, into a 480 x 854 buffer
  two_step   (14d), then (14) on the buffer (resize + clear + counts), tables prebuilt: what ``ClipScorer(pred_size=...)`` runs
  public     ``measures.clip_counts(pred, gt, n_obj, resize=True)`` itself: (14b) on every call as well (it keeps no tables)
each once over the whole clip and once frame by frame (36 calls, the way ``ClipScorer`` makes them), in us per clip; the counts
are compared with the host yardstick on the numpy-resized prediction first.  (The fused route this was measured against, the
counts kernel with its prediction load a gather, is not in the library: profiles/r13_davis_resized.md.)"""
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
from dmm_net_amd import video  # noqa: E402

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


def resized(a, T, n_obj, pred_size, size=(480, 854)):
    """The shipped route of a (Hs, Ws) clip against ``size`` annotations, and its resize alone."""
    (Hs, Ws), (H, W) = pred_size, size
    pred, _ = blobs(np.random.default_rng(Hs), T, Hs, Ws, n_obj)
    _, gt = blobs(np.random.default_rng(H), T, H, W, n_obj)
    radius = measures.boundary_radius((Hs, Ws))
    dp, dg = torch.from_numpy(pred).to("cuda:0"), torch.from_numpy(gt).to("cuda:0")
    tables = measures.nearest_tables((Hs, Ws), (H, W), dp.device)
    counts = torch.empty((T, n_obj, measures.N_COUNTS), dtype=torch.int32, device=dp.device)

    def resize():
        video.resize_labels(dp, (H, W), tables=tables)

    def two_step():
        measures._counts_into(video.resize_labels(dp, (H, W), tables=tables), dg, n_obj, radius, counts)

    def public():
        measures.clip_counts(dp, dg, n_obj, resize=True)

    def resize_frames():
        for t in range(T):
            video.resize_labels(dp[t:t + 1], (H, W), tables=tables)

    def two_step_frames():
        for t in range(T):
            measures._counts_into(video.resize_labels(dp[t:t + 1], (H, W), tables=tables), dg[t:t + 1], n_obj, radius,
                                  counts[t:t + 1])

    k = a.host_frames
    host_resized = measures.resize_labels_host(pred[:k], (H, W))
    want = measures_ref.counts(host_resized, gt[:k], n_obj, radius)
    assert np.array_equal(video.resize_labels(dp[:k], (H, W), tables=tables).cpu().numpy(), host_resized)
    out = {"pred_size": f"{Hs}x{Ws}", "size": f"{H}x{W}", "radius": radius}
    for name, fn in (("two_step", two_step), ("two_step_frames", two_step_frames)):
        counts.fill_(-1)
        fn()
        assert np.array_equal(counts[:k].cpu().numpy(), want), name + ": device counts differ from the host yardstick"
    assert np.array_equal(measures.clip_counts(dp[:k], dg[:k], n_obj, resize=True).cpu().numpy(), want)
    for name, fn in (("resize", resize), ("two_step", two_step), ("public", public), ("resize_frames", resize_frames),
                     ("two_step_frames", two_step_frames)):
        out[name + "_us"] = windows(fn, a.repeats, a.iters)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pred-size", default=None, help="HsxWs: also time the resized routes against 480x854 annotations")
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
    if a.pred_size:
        res["resized"] = resized(a, T, n_obj, tuple(int(v) for v in a.pred_size.lower().split("x")))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
