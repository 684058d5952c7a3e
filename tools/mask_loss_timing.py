"""Times the mask loss of one frame step on the GPU, forward + backward, and prints ONE JSON line.

    python tools/mask_loss_timing.py [--out FILE] [--repeats 5] [--iters 20]

4 videos x 5 objects x 255 x 448, fp32 predictions and targets, mixed sample weights.  HIP events, warm-up, then min / median /
max over ``repeats`` windows of ``iters`` steps, in us per step (loss * 18 -> backward to the prediction):
  (a) stock   the reference's tensor ops (losses.mask_step_losses_stock: trainer.py:188-208 with the bool-mask reading)
  (b) fused   losses.mask_step_losses (dmm_mask_iou_loss_fwd / _bwd)
  (c) graph   the fused step replayed from one captured graph (the stock form reads the host twice: it cannot be captured)
with the GPU kernels per step of each (torch.profiler; the library's own count for the fused entries), the stock form
once more at the end (the spread of the baseline under the same conditions), and the forward entry (partials + finish
launch) and the backward launch alone with their algorithmic bytes per second."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dmm_net_amd import _lib, losses, ops  # noqa: E402
from dmm_net_amd.graphs import SafeGraph  # noqa: E402

G = 18.0


def windows(fn, repeats, iters, warmup=10):
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


def kernels_per_step(fn, steps=5):
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
        return sum(e.count for e in prof.key_averages() if e.self_device_time_total > 0) / steps
    except Exception as e:                                   # the profiler is a convenience here, the timings are not
        return f"unavailable ({type(e).__name__})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mask_loss_timing needs an MI355X"
    dev = "cuda:0"
    B, O, H, W = 4, 5, 255, 448
    HW = H * W
    torch.manual_seed(0)
    pred = (torch.rand(B, O, H, W, device=dev) * 1.3).requires_grad_(True)
    y = (torch.rand(B, O, HW, device=dev) > 0.5).float()
    sw = (torch.rand(B, O, device=dev) > 0.3).float()
    sw[0, 0] = 1.0
    valid = (torch.rand(B, O, device=dev) > 0.3).to(torch.int32)
    valid[0, 0] = 1
    res = {"what": "mask loss of one frame step, forward + backward", "B": B, "objects": O, "H": H, "W": W,
           "unit": "us per step", "repeats": a.repeats, "iters": a.iters}

    def step_of(fn):
        def step():
            out = fn(y, pred, sw, valid)
            (dp,) = torch.autograd.grad(out[0] * G, pred)
            return out, dp
        return step

    stock, fused = step_of(losses.mask_step_losses_stock), step_of(losses.mask_step_losses)
    res["stock"] = windows(stock, a.repeats, a.iters)
    res["fused"] = windows(fused, a.repeats, a.iters)
    L = _lib.load()
    c0 = int(L.dmm_launch_count())
    fused()
    res["fused_library_launches_per_step"] = int(L.dmm_launch_count()) - c0
    res["fused_gpu_kernels_per_step"] = kernels_per_step(fused)
    res["stock_gpu_kernels_per_step"] = kernels_per_step(stock)
    torch.cuda.synchronize()
    g = SafeGraph()
    with g.capture():
        kept = fused()
    res["graph"] = windows(g.replay, a.repeats, a.iters)
    del kept
    res["stock_again"] = windows(stock, a.repeats, a.iters)

    # ---- the entries alone ---------------------------------------------------------------------------------------
    with torch.no_grad():
        p = pred.detach()
        k = windows(lambda: ops.mask_iou_loss(p, y, sw, valid, keep=False), a.repeats, 50)
        nbytes = 2 * 4 * B * O * HW
        res["entry_fwd_partials_plus_finish_us"] = dict(k, bytes=nbytes, bytes_per_s=nbytes / (k["median"] * 1e-6))
        ws = ops.mask_iou_loss(p, y, sw, valid)[5]
        d_loss = torch.full((), G, device=dev)
        k = windows(lambda: ops.mask_iou_loss_bwd(y, ws, d_loss, p.shape, O), a.repeats, 50)
        res["entry_bwd_us"] = dict(k, bytes=nbytes, bytes_per_s=nbytes / (k["median"] * 1e-6))
    spread = res["stock"]["max"] - res["stock"]["min"]
    res["stock_spread"] = spread
    res["fused_median_below_stock_median_by_more_than_stock_spread"] = bool(
        res["stock"]["median"] - res["fused"]["median"] > spread)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
