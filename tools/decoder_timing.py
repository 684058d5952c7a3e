"""Times the refine decoder's frame step on the GPU (dmm_net_amd/decoder.py) and prints ONE JSON line.

    python tools/decoder_timing.py [--out FILE] [--repeats 5] [--iters 20]

4 videos of 255 x 448, 5 objects, hidden 128, 'concat', steady state (temporal state present).  HIP events, warm-up, then
min / median / max over ``repeats`` windows of ``iters`` steps, in ms per frame step:
  (a) stock   the reference's op-for-op form on the GPU (what the reference's module does) -- the baseline
  (b) fused   the fused form, eager
  (c) graph   the fused form replayed from one captured graph
and the four kernels of csrc/dmm_decoder.hip alone (us per launch; the two streaming ones with their algorithmic bytes and
the fraction of the 8 TB/s HBM peak those bytes / event time come to), plus the launch counts of one fused frame step."""
import argparse
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dmm_net_amd import _lib, decoder as D  # noqa: E402

HBM_PEAK = 8.0e12


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
        out.append(a.elapsed_time(b) / iters)
    return {"min": min(out), "median": statistics.median(out), "max": max(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "decoder_timing needs an MI355X"
    dev = "cuda:0"
    B, O, n_obj, H, W, hidden = 4, 5, 5, 255, 448, 128
    torch.manual_seed(0)
    args = types.SimpleNamespace(hidden_size=hidden, kernel_size=3, dropout=0.0, skip_mode="concat", prev_mask_d=1, use_gpu=True)
    dec = D.RSISMask(args).eval().to(dev)
    sizes = D.pyramid_sizes(H, W)
    ch = [hidden, hidden, hidden // 2, hidden // 4]
    feats = {"refine_input_feat": tuple(torch.randn((B, c) + s, device=dev) for c, s in zip(ch, sizes))}
    prev_mask = (torch.rand(B, O, H * W, device=dev) > 0.6).float()
    y_mask = torch.zeros(B, O, H * W, device=dev)
    init_pred = torch.rand(B, O, H, W, device=dev)
    hist = torch.rand(B, O, H, W, device=dev)
    valid = torch.ones(B, O, dtype=torch.long, device=dev)
    res = {"what": "refine decoder frame step", "B": B, "objects": n_obj, "H": H, "W": W, "hidden": hidden,
           "skip_mode": "concat", "unit": "ms per frame step", "repeats": a.repeats, "iters": a.iters}

    with torch.no_grad():
        def make(fused):
            dec.fused = fused
            step = D.RefineStep(dec)
            st = [None]

            def fn():
                dec.fused = fused
                _, _, st[0] = step(feats, prev_mask, y_mask, init_pred, hist, valid, st[0])
            return step, fn
        _, stock_fn = make(False)
        res["stock"] = windows(stock_fn, a.repeats, a.iters)
        step, fused_fn = make(True)
        res["fused"] = windows(fused_fn, a.repeats, a.iters)
        torch.cuda.synchronize()
        c0, l0 = dec.conv_calls, int(_lib.load().dmm_launch_count())
        fused_fn()
        res["fused_convolutions_per_step"] = dec.conv_calls - c0
        res["fused_kernel_launches_per_step"] = int(_lib.load().dmm_launch_count()) - l0
        res["stock_convolutions_per_step"] = n_obj * (3 * 4 + 1)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fused_fn()
        res["graph"] = windows(g.replay, a.repeats, a.iters)
        # alternate once more: the spread of the baseline under the same conditions
        res["stock_again"] = windows(stock_fn, a.repeats, a.iters)
        dec.fused = True

        # ---- the kernels alone -------------------------------------------------------------------------------------
        us = lambda d: {k: 1e3 * v for k, v in d.items()}
        pyr = D.mask_pyramid(prev_mask, y_mask, init_pred, n_obj, H, W)
        k = us(windows(lambda: D.mask_pyramid(prev_mask, y_mask, init_pred, n_obj, H, W, out=pyr), a.repeats, 50))
        nbytes = 4 * (3 * B * n_obj * H * W + sum(p.numel() for p in pyr))
        res["kernel_mask_pyramid_us"] = dict(k, bytes=nbytes, hbm_fraction=nbytes / (k["median"] * 1e-6) / HBM_PEAK)
        h3, w3 = sizes[-1]
        logits = torch.randn(n_obj * B, 1, 2 * h3, 2 * w3, device=dev).view(n_obj, B, 2 * h3, 2 * w3).transpose(0, 1)
        outs, v32 = torch.empty(B, O, H, W, device=dev), valid.to(torch.int32)
        k = us(windows(lambda: D.refine_finish(logits, v32, outs, hist, n_obj), a.repeats, 50))
        nbytes = 4 * (2 * B * O * H * W + logits.numel())
        res["kernel_refine_finish_us"] = dict(k, bytes=nbytes, hbm_fraction=nbytes / (k["median"] * 1e-6) / HBM_PEAK)
        for lvl in (0, 3):
            Hd, (h, w) = dec.skip_dims_out[lvl], sizes[lvl]
            pre = [torch.randn(B, 4 * Hd, h, w, device=dev) for _ in range(3)]
            cp, hd, cl = (torch.randn(B, Hd, h, w, device=dev) for _ in range(3))
            wm = torch.randn(4 * Hd, 9, device=dev)
            res[f"kernel_clstm_gates_level{lvl}_us"] = us(windows(
                lambda: D.clstm_gates(pre, pyr[lvl][0], wm, cp, hd, cl), a.repeats, 50))
        src = torch.randn(B, dec.skip_dims_out[2], *sizes[2], device=dev)
        dst = torch.empty(B, dec.skip_dims_out[2] + dec.skip_dims_out[3], *sizes[3], device=dev)
        res["kernel_upsample_into_level3_us"] = us(windows(lambda: D.upsample_bilinear_into(src, dst, 0, "write"), a.repeats, 50))
    spread = res["stock"]["max"] - res["stock"]["min"]
    res["stock_spread"] = spread
    res["fused_faster_than_stock_by_more_than_its_spread"] = bool(res["stock"]["min"] - res["fused"]["max"] > spread)
    res["graph_faster_than_stock_by_more_than_its_spread"] = bool(res["stock"]["min"] - res["graph"]["max"] > spread)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
