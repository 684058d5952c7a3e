#!/usr/bin/env python3
"""algo 'hun' on the device against scipy on the host.

1. ops.linear_sum_assignment (dmm_lsap_f32, HIP events) at B in {1, 64, 512, 1024} for 50 x 10 costs (templates x padded
   proposals: the 10 x 50 table of 10 templates) and 20 x 200, against scipy per frame on the host (wall time, the table
   already on the host).
2. DMM_Model.inference and .forward + backward for 4 videos of 255 x 448, 50 proposals, 5 templates, algo 'hun', with
   autograd._DEVICE_LSAP on (device assignment) and off (scipy route): wall us per call, medians of 20.
3. FrameLoop on the fixed-slot step (one graph replay per frame) for 4 videos of 255 x 448, 24 frames, 5 templates,
   50 proposal slots: ms per frame step under 'hun' and under 'relax'."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from scipy.optimize import linear_sum_assignment as scipy_lsa

from dmm_net_amd import autograd, ops, synth

dev = "cuda:0"


def events_us(fn, n=50, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def wall_us(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(ts)


g = torch.Generator(device=dev).manual_seed(0)
for nr, nc in ((10, 50), (20, 200)):
    for B in (1, 64, 512, 1024):
        C = -torch.rand((B, nr, nc), generator=g, device=dev)
        d = events_us(lambda: ops.linear_sum_assignment(C))
        c = C.cpu().numpy().astype(np.float32)
        t0 = time.perf_counter()
        for b in range(B):
            scipy_lsa(c[b])
        h = (time.perf_counter() - t0) * 1e6
        print(f"lsap {nr:2d} x {nc:3d}  B={B:5d}: device {d:9.1f} us ({d / B:7.2f} us/frame)   "
              f"scipy host {h:9.1f} us ({h / B:7.2f} us/frame)", flush=True)


class _Props:
    def __init__(self, mask, scores):
        self._f = {"mask": mask, "scores": scores}

    def __len__(self):
        return self._f["mask"].shape[0]

    def fields(self):
        return list(self._f.keys())

    def get_field(self, k):
        return self._f[k]


from dmm_net_amd.dmm_model import DMM_Model  # noqa: E402

B, F, P, H, W, D = 4, 5, 50, 255, 448, 512
frames = [synth.make_frame(P, F, H, W, D, seed=900 + b, kind="structured", with_targets=True) for b in range(B)]
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
feats = torch.cat([t(fr.proposed_feature) for fr in frames], 0).requires_grad_(True)
props = [_Props(t(fr.proposed_mask).unsqueeze(1), t(fr.proposal_score)) for fr in frames]
valid = torch.ones((B, F), device=dev)
ml = torch.stack([t(fr.mask_last_occurence) for fr in frames], 0)
targets = [t(fr.targets) for fr in frames]
tf = [t(fr.template_feature).requires_grad_(True) for fr in frames]
cfg = {"matching": {"algo": "hun"}, "relax_max_iter": 10, "relax_proj_iter": 5, "relax_learning_rate": 0.1,
       "score_weight": 0.3}
infos = {"args": None, "shape": None, "extra_frame": [0] * B, "valid": valid}
for route in (True, False):
    autograd._DEVICE_LSAP = route
    ev = DMM_Model(cfg, is_test=1, feature_extractor=lambda bf, pr: feats.detach())
    tr = DMM_Model(cfg, is_test=0, feature_extractor=lambda bf, pr: feats)

    def inf():
        with torch.no_grad():
            ev.inference(infos, props, None, ml, {b: {"feat": [tf[b].detach()]} for b in range(B)})

    def fwd_bwd():
        out = tr(None, props, None, ml, {b: {"feat": [tf[b]]} for b in range(B)}, valid, targets)
        (out[0].sum() + sum(out[2])).backward()

    print(f"DMM_Model 4 x {H} x {W}, {P} x {F}, 'hun', device assignment={route}: inference {wall_us(inf):8.0f} us   "
          f"forward+backward {wall_us(fwd_bwd):8.0f} us", flush=True)
autograd._DEVICE_LSAP = True

# 3. FrameLoop (fixed-slot step, one graph replay per frame): ms per frame step, 'hun' against 'relax'
import torch.nn.functional as Fn  # noqa: E402

from dmm_net_amd import proposals as prop, video  # noqa: E402
from dmm_net_amd.roi_features import FeatureExtractor  # noqa: E402


class _PoolEncoder:
    def __init__(self, C=8):
        self.mul = torch.linspace(0.5, 1.5, C, device=dev).view(1, C, 1, 1)

    def __call__(self, x):
        g_ = x.mean(1, keepdim=True)
        lv = tuple(Fn.avg_pool2d(g_, s, ceil_mode=True) * self.mul for s in (4, 8, 16, 32))
        return {"backbone_feature": lv, "refine_input_feat": lv}


rng = np.random.default_rng(0)
T, O = 24, 5


def _raw(n):
    x1, y1 = rng.uniform(0, W - 64, n), rng.uniform(0, H - 64, n)
    bx = np.stack([x1, y1, np.minimum(x1 + rng.uniform(20, 120, n), W - 1), np.minimum(y1 + rng.uniform(20, 100, n), H - 1)], 1)
    bl = prop.SimpleBoxList(torch.from_numpy(bx.astype(np.float32)), (W, H))
    bl.add_field("scores", torch.from_numpy(rng.random(n).astype(np.float32)))
    bl.add_field("mask", torch.from_numpy((rng.random((n, 1, 28, 28)) * 0.6 + 0.4).astype(np.float32)))
    return bl


clip_frames = torch.randn(B, T, 3, H, W, device=dev)
clip_props = [[_raw(80) for _ in range(T)] for _ in range(B)]
first = torch.zeros(B, O, H, W, device=dev)
for b in range(B):
    for o in range(O):
        y0, x0 = int(rng.integers(0, H - 60)), int(rng.integers(0, W - 60))
        first[b, o, y0:y0 + 50, x0:x0 + 55] = 1.0
first = first.view(B, O, H * W)
for algo in ("relax", "hun"):
    c = dict(cfg, matching={"algo": algo})
    lp = video.FrameLoop(_PoolEncoder(), DMM_Model(c, is_test=1, feature_extractor=FeatureExtractor()), nms_thresh=0.4,
                         max_proposals=50)
    assert lp._slots_ok(clip_frames, clip_props, O)
    us = wall_us(lambda: lp.run(clip_frames, first, clip_props), n=5, warm=2)
    print(f"FrameLoop 4 x {H} x {W}, {T} frames, {O} templates, algo {algo!r}: {us / T / 1e3:.3f} ms per frame step",
          flush=True)
