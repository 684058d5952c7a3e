"""Times the preparation of one config-4 clip set on the GPU against the same work on one host thread, and prints ONE JSON line.

    python tools/prepare_timing.py [--out FILE] [--repeats 5] [--iters 20] [--filter bicubic]

12 decoded frames of 720 x 1280 (uint8, interleaved RGB) with their annotations -> 255 x 448: the resize, ToTensor and
Normalize of the frames (dmm_prepare_frames_u8: the horizontal and the vertical launch) and the nearest resize of the
annotations (dmm_resize_labels_nearest_u8), through ``frames.ClipPreparer`` with ``out=``.
  device   HIP events, min / median / max over ``repeats`` windows of ``iters`` calls after a warm-up, in us: the whole call
           (``clip_us``), the frames alone (``frames_us``) and the annotations alone (``labels_us``)
  bytes    the algorithmic traffic of the frames: the source read once, the uint8 intermediate [Hs, W, 3] written once and
           read once, the fp32 planes written once --
             n * (3 Hs Ws + 2 * 3 Hs W + 12 H W)
           against ``frames_us``' median and the 8 TB/s peak.  The vertical pass reads every intermediate row once per output
           row whose taps cover it (about ksize / scale times, from the caches), so this is a floor on the traffic.
  host     the wall time of the same clip set on ONE thread of the same box: Pillow's ``Image.resize`` + the reference's
           ``ToTensor`` / ``Normalize`` operations in torch where Pillow imports (``host_path`` = "pillow"), otherwise
           ``frames.resize_frames_host`` (``"numpy restatement"``); the best of three runs
The device frames and labels are compared with the host's, bit for bit, before anything is reported."""
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
from dmm_net_amd import frames as F, measures  # noqa: E402

PEAK_BYTES_PER_S = 8e12
STEP_MS = 13.31                                            # TrainEncoder's config-4 step (README)
AUGMENT_US = 145.1                                         # augment_clip on the same clip set (profiles/r10_augment.md)


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


def clip(n, Hs, Ws):
    """Frames with smooth structure, edges and sensor-like noise; annotations with three ellipses that move."""
    rng = np.random.default_rng(14)
    y, x = np.mgrid[0:Hs, 0:Ws].astype(np.float32)
    frames = np.zeros((n, Hs, Ws, 3), dtype=np.uint8)
    labels = np.zeros((n, Hs, Ws), dtype=np.uint8)
    for f in range(n):
        for c in range(3):
            base = 128 + 90 * np.sin(x * (0.011 + 0.004 * c) + 0.3 * f) * np.cos(y * (0.017 - 0.003 * c)) + 30 * ((x // 64 + y // 48) % 2)
            frames[f, :, :, c] = np.clip(base + rng.normal(0, 6, (Hs, Ws)), 0, 255).astype(np.uint8)
        for o in range(3):
            cy, cx = Hs * (0.3 + 0.2 * o) + 3 * f, Ws * (0.2 + 0.3 * o) + 5 * f
            labels[f][((y - cy) / (0.2 * Hs)) ** 2 + ((x - cx) / (0.12 * Ws)) ** 2 <= 1] = o + 1
    return frames, labels


def host_prepare(frames, labels, size, filter, lut):
    """-> (fp32 [n,3,H,W], uint8 [n,H,W], the path's name)."""
    H, W = size
    try:
        from PIL import Image
        flt = {"nearest": Image.NEAREST, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}[filter]
        mean, std = (torch.tensor(v, dtype=torch.float32).view(3, 1, 1) for v in (F.MEAN, F.STD))
        out, lab = [], []
        for f in range(frames.shape[0]):
            img = np.array(Image.fromarray(frames[f]).resize((W, H), flt))
            out.append(torch.from_numpy(img).permute(2, 0, 1).contiguous().float().div(255).sub_(mean).div_(std))
            lab.append(np.array(Image.fromarray(labels[f]).resize((W, H), Image.NEAREST)))
        return torch.stack(out), np.stack(lab), "pillow"
    except ImportError:
        u8 = torch.from_numpy(F.resize_frames_host(frames, size, filter)).long()
        planes = torch.stack([lut[c][u8[..., c]] for c in range(3)], 1)
        return planes, measures.resize_labels_host(labels, size), "numpy restatement"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--filter", default="bicubic", choices=F.FILTERS)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "prepare_timing needs an MI355X"
    torch.set_num_threads(1)
    n, (Hs, Ws), (H, W) = 12, (720, 1280), (255, 448)
    frames, labels = clip(n, Hs, Ws)
    lut = F.normalise_lut()
    host_s = []
    for _ in range(3):
        t0 = time.perf_counter()
        want, want_lab, path = host_prepare(frames, labels, (H, W), a.filter, lut)
        host_s.append(time.perf_counter() - t0)
    dev = "cuda:0"
    d_frames, d_labels = torch.from_numpy(frames).to(dev), torch.from_numpy(labels).to(dev)
    prep = F.ClipPreparer((Hs, Ws), (H, W), a.filter, device=dev)
    out = torch.empty((n, 3, H, W), dtype=torch.float32, device=dev)
    got, got_lab = prep(d_frames, d_labels, out=out)
    assert torch.equal(got.cpu().view(torch.int32), want.contiguous().view(torch.int32)), "device frames differ from the host's"
    assert np.array_equal(got_lab.cpu().numpy(), want_lab), "device labels differ from the host's"
    clip_us = windows(lambda: prep(d_frames, d_labels, out=out), a.repeats, a.iters)
    frames_us = windows(lambda: prep(d_frames, out=out), a.repeats, a.iters)
    labels_us = windows(lambda: measures.resize_labels_device(d_labels, (H, W), prep.label_tables), a.repeats, a.iters)
    nbytes = n * (3 * Hs * Ws + 2 * 3 * Hs * W + 12 * H * W)
    rate = nbytes / (frames_us["median"] * 1e-6)
    res = {"what": "preparation of one config-4 clip set", "frames": n, "src": [Hs, Ws], "dst": [H, W], "filter": a.filter,
           "unit": "us per clip set", "repeats": a.repeats, "iters": a.iters, "clip_us": clip_us, "frames_us": frames_us,
           "labels_us": labels_us, "algorithmic_bytes_frames": nbytes, "bytes_per_s": rate,
           "fraction_of_8TBps": rate / PEAK_BYTES_PER_S, "fraction_of_13.31ms_step": clip_us["median"] * 1e-3 / STEP_MS,
           "times_augment_clip_145.1us": clip_us["median"] / AUGMENT_US, "host_path": path,
           "host_one_thread_s": {"best": min(host_s), "all": host_s}, "workspace_bytes": prep.tables.workspace_bytes(n)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
