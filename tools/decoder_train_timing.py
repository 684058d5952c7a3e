"""Times one training step of the refine decoder on the GPU, stock form beside ``fused_train``, and prints ONE JSON line.

    python tools/decoder_train_timing.py [--out FILE] [--repeats 3] [--iters 5] [--dtype fp32|bf16]

Config 4's sizes: 4 videos of 255 x 448, hidden 128, 'concat', 5 objects chained as the trainer chains them (object t's
spatial state is object t - 1's hidden), temporal hiddens present.  One step = forward of the five decoder calls + backward
of the sum of their upsampled sigmoids, gradients to every parameter and skip map.  HIP events after warm-up, min / median /
max over ``repeats`` windows of ``iters`` steps, in ms per step; ``torch.cuda.max_memory_allocated`` of one step per form;
and the cell's backward kernel alone at the coarsest and the finest level (us per call, with and without the two
reductions).

``--dtype bf16`` adds, in the same run, ``fused_train_bf16``: the same step with ``decoder.train_dtype = torch.bfloat16`` on bf16
skip maps and temporal hiddens, then ``fused_train`` once more (``fused_train_again``: the fp32 form's spread under the same
conditions), the device time of the kernels of one step of each form, and the cell's bf16 backward kernel beside the fp32 one."""
import argparse
import json
import os
import statistics
import sys
import types

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dmm_net_amd import decoder as D  # noqa: E402


def windows(fn, repeats, iters, warmup=3):
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
        out.append(a.elapsed_time(b) / iters)
    return {"min": min(out), "median": statistics.median(out), "max": max(out)}


def device_time_ms(fn):
    """The summed device time of the kernels of one call of ``fn`` (``torch.profiler``), in ms."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    total = 0.0
    for e in prof.events():
        if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower():
            total += float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0))
    return total / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "decoder_train_timing needs an MI355X"
    dev = "cuda:0"
    B, n_obj, H, W, hidden = 4, 5, 255, 448, 128
    torch.manual_seed(0)
    args = types.SimpleNamespace(hidden_size=hidden, kernel_size=3, dropout=0.0, skip_mode="concat", prev_mask_d=1, use_gpu=True)
    dec = D.RSISMask(args).eval().to(dev)
    sizes = D.pyramid_sizes(H, W)
    ch = [hidden, hidden, hidden // 2, hidden // 4]
    feats = [torch.randn((B, c) + s, device=dev, requires_grad=True) for c, s in zip(ch, sizes)]
    masks = [[torch.rand((B, 3) + s, device=dev) for s in sizes] for _ in range(n_obj)]
    temporal = [[0.5 * torch.randn((B, d) + s, device=dev).tanh() for d, s in zip(dec.skip_dims_out, sizes)]
                for _ in range(n_obj)]
    leaves = feats + list(dec.parameters())

    def make(feats, temporal, leaves):
        def step():
            spatial, loss = None, 0
            for t in range(n_obj):
                out_mask, spatial = dec(feats, masks[t], spatial, temporal[t])
                loss = loss + torch.sigmoid(F.interpolate(out_mask, (H, W)).float()).sum()
            return torch.autograd.grad(loss, leaves)
        return step
    step = make(feats, temporal, leaves)

    res = {"what": "refine decoder training step (forward + backward)", "B": B, "objects": n_obj, "H": H, "W": W,
           "hidden": hidden, "skip_mode": "concat", "unit": "ms per step", "repeats": a.repeats, "iters": a.iters}

    def measure(fused_train, step=step):
        dec.fused_train = fused_train
        t = windows(step, a.repeats, a.iters)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step()
        torch.cuda.synchronize()
        t["max_memory_allocated_MiB"] = torch.cuda.max_memory_allocated() / 2 ** 20
        t["held_before_the_step_MiB"] = base / 2 ** 20
        return t

    res["stock"] = measure(False)
    c0 = dec.conv_calls
    res["fused_train"] = measure(True)
    res["fused_train_convolutions_per_step"] = (dec.conv_calls - c0) // (3 + a.repeats * a.iters + 1)
    res["stock_convolutions_per_step"] = n_obj * (3 * 4 + 1)
    res["stock_again"] = measure(False)                       # the spread of the baseline under the same conditions
    dec.fused_train = False
    spread = max(res["stock"]["max"], res["stock_again"]["max"]) - min(res["stock"]["min"], res["stock_again"]["min"])
    res["stock_spread"] = spread
    res["fused_train_faster_than_stock_by_more_than_its_spread"] = bool(
        min(res["stock"]["min"], res["stock_again"]["min"]) - res["fused_train"]["max"] > spread)

    us = lambda d: {k: 1e3 * v for k, v in d.items()}
    with torch.no_grad():
        for lvl in (0, 3):
            Hd, (h, w) = dec.skip_dims_out[lvl], sizes[lvl]
            pre = [torch.randn(B, 4 * Hd, h, w, device=dev) for _ in range(3)]
            cp, dh, dc = (torch.randn(B, Hd, h, w, device=dev) for _ in range(3))
            wm = torch.randn(4 * Hd, 9, device=dev) * 0.3
            for label, need in (("all_outputs", (True, True, True)), ("no_d_masks", (True, False, True)),
                                ("d_pre_d_cell_prev_only", (True, False, False))):
                res[f"kernel_clstm_gates_bwd_level{lvl}_{label}_us"] = us(windows(
                    lambda: D.clstm_gates_bwd(pre, masks[0][lvl], wm, cp, dh, dc, need=need), a.repeats, 50))
                if a.dtype == "bf16":
                    pre16, dh16 = [p.to(torch.bfloat16) for p in pre], dh.to(torch.bfloat16)
                    res[f"kernel_clstm_gates_bwd_bf16_level{lvl}_{label}_us"] = us(windows(
                        lambda: D.clstm_gates_bwd(pre16, masks[0][lvl], wm, cp, dh16, dc, need=need), a.repeats, 50))
    if a.dtype == "bf16":
        bf16 = torch.bfloat16
        feats16 = [f.detach().to(bf16).requires_grad_(True) for f in feats]
        temporal16 = [[t.to(bf16) for t in ts] for ts in temporal]
        step16 = make(feats16, temporal16, feats16 + list(dec.parameters()))
        dec.train_dtype = bf16
        c0 = dec.conv_calls
        res["fused_train_bf16"] = measure(True, step16)
        res["fused_train_bf16_convolutions_per_step"] = (dec.conv_calls - c0) // (3 + a.repeats * a.iters + 1)
        res["fused_train_bf16_kernel_time_ms"] = device_time_ms(step16)
        dec.train_dtype = torch.float32
        res["fused_train_again"] = measure(True)
        res["fused_train_kernel_time_ms"] = device_time_ms(step)
        dec.fused_train = False
        lo = min(res["fused_train"]["min"], res["fused_train_again"]["min"])
        hi = max(res["fused_train"]["max"], res["fused_train_again"]["max"])
        res["fused_train_spread"] = hi - lo
        res["fused_train_bf16_faster_than_fused_train_by_more_than_its_spread"] = bool(lo - res["fused_train_bf16"]["max"] > hi - lo)
        res["fused_train_bf16_slower_than_fused_train_by_more_than_its_spread"] = bool(res["fused_train_bf16"]["min"] - hi > hi - lo)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
