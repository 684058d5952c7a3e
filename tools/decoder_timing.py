"""Times the refine decoder's frame step on the GPU (dmm_net_amd/decoder.py) and prints ONE JSON line.

    python tools/decoder_timing.py [--out FILE] [--repeats 5] [--iters 20] [--dtype {fp32,bf16}]

4 videos of 255 x 448, 5 objects, hidden 128, 'concat', steady state (temporal state present).  HIP events, warm-up, then
min / median / max over ``repeats`` windows of ``iters`` steps, in ms per frame step:
  (a) stock   the reference's op-for-op form on the GPU (what the reference's module does) -- the baseline
  (b) fused   the fused form, eager
  (c) graph   the fused form replayed from one captured graph
and the four kernels of csrc/dmm_decoder.hip alone (us per launch; the two streaming ones with their algorithmic bytes and
the fraction of the 8 TB/s HBM peak those bytes / event time come to), plus the launch counts of one fused frame step.

``--dtype bf16`` (the default, fp32, prints what it always printed): the fused step with ``compute_dtype = torch.bfloat16`` on
bf16 feature maps, eager and replayed from a graph, and IN THE SAME RUN the fp32 fused step, eager and replayed, measured
before and after it (the comparison point and its spread); the three 16-bit kernels alone beside their fp32 siblings at the
same shapes, each with its algorithmic bytes; the convolution and launch counts of one step of either form."""
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


def emit(res, out):
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


def bf16_report(a):
    """``--dtype bf16``: the bf16 fused step against the fp32 fused step of the same run, and the 16-bit kernels alone."""
    dev = "cuda:0"
    B, O, n_obj, H, W, hidden = 4, 5, 5, 255, 448, 128
    torch.manual_seed(0)
    args = types.SimpleNamespace(hidden_size=hidden, kernel_size=3, dropout=0.0, skip_mode="concat", prev_mask_d=1, use_gpu=True)
    dec32 = D.RSISMask(args).eval().to(dev)
    dec16 = D.RSISMask(args).eval().to(dev)
    dec16.load_state_dict(dec32.state_dict())
    dec16.compute_dtype = torch.bfloat16
    sizes = D.pyramid_sizes(H, W)
    ch = [hidden, hidden, hidden // 2, hidden // 4]
    maps32 = tuple(torch.randn((B, c) + s, device=dev) for c, s in zip(ch, sizes))
    maps = {"fp32": {"refine_input_feat": maps32}, "bf16": {"refine_input_feat": tuple(m.to(torch.bfloat16) for m in maps32)}}
    prev_mask = (torch.rand(B, O, H * W, device=dev) > 0.6).float()
    y_mask = torch.zeros(B, O, H * W, device=dev)
    init_pred = torch.rand(B, O, H, W, device=dev)
    hist = torch.rand(B, O, H, W, device=dev)
    valid = torch.ones(B, O, dtype=torch.long, device=dev)
    res = {"what": "refine decoder frame step, bf16 against fp32 (fused form)", "dtype": "bf16", "B": B, "objects": n_obj, "H": H,
           "W": W, "hidden": hidden, "skip_mode": "concat", "unit": "ms per frame step", "repeats": a.repeats, "iters": a.iters}
    with torch.no_grad():
        fns, graphs = {}, {}
        for name, dec in (("fp32", dec32), ("bf16", dec16)):
            step, st = D.RefineStep(dec), [None]

            def fn(step=step, st=st, feats=maps[name]):
                _, _, st[0] = step(feats, prev_mask, y_mask, init_pred, hist, valid, st[0])
            fns[name] = fn
        res["fused_fp32"] = windows(fns["fp32"], a.repeats, a.iters)
        res["fused_bf16"] = windows(fns["bf16"], a.repeats, a.iters)
        res["fused_fp32_again"] = windows(fns["fp32"], a.repeats, a.iters)
        for name, dec in (("fp32", dec32), ("bf16", dec16)):
            torch.cuda.synchronize()
            c0, l0 = dec.conv_calls, int(_lib.load().dmm_launch_count())
            fns[name]()
            res[f"{name}_convolutions_per_step"] = dec.conv_calls - c0
            res[f"{name}_kernel_launches_per_step"] = int(_lib.load().dmm_launch_count()) - l0
            torch.cuda.synchronize()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                fns[name]()
        res["graph_fp32"] = windows(graphs["fp32"].replay, a.repeats, a.iters)
        res["graph_bf16"] = windows(graphs["bf16"].replay, a.repeats, a.iters)
        res["graph_fp32_again"] = windows(graphs["fp32"].replay, a.repeats, a.iters)

        # ---- the three 16-bit kernels alone, each beside its fp32 sibling at the same shape ---------------------------------
        us = lambda d: {k: 1e3 * v for k, v in d.items()}
        pyr = D.mask_pyramid(prev_mask, y_mask, init_pred, n_obj, H, W)
        h3, w3 = sizes[-1]
        v32 = valid.to(torch.int32)
        outs = torch.empty(B, O, H, W, device=dev)
        for name, dt, es in (("fp32", torch.float32, 4), ("bf16", torch.bfloat16, 2)):
            new = lambda *shape: torch.randn(shape, device=dev).to(dt)
            logits = new(n_obj * B, 1, 2 * h3, 2 * w3).view(n_obj, B, 2 * h3, 2 * w3).transpose(0, 1)
            k = us(windows(lambda: D.refine_finish(logits, v32, outs, hist, n_obj), a.repeats, 50))
            res[f"kernel_refine_finish_{name}_us"] = dict(k, bytes=4 * 2 * B * O * H * W + es * logits.numel())
            for lvl in (0, 3):
                Hd, (h, w) = dec32.skip_dims_out[lvl], sizes[lvl]
                pre = [new(B, 4 * Hd, h, w) for _ in range(3)]
                hd = new(B, Hd, h, w)
                cp, cl = (torch.randn(B, Hd, h, w, device=dev) for _ in range(2))
                wm = torch.randn(4 * Hd, 9, device=dev)
                k = us(windows(lambda: D.clstm_gates(pre, pyr[lvl][0], wm, cp, hd, cl), a.repeats, 50))
                # three addends in, the hidden out (16-bit in the bf16 form); masks, stencil, both cells fp32
                nbytes = es * (3 * 4 + 1) * B * Hd * h * w + 4 * (3 * B * h * w + 36 * Hd + 2 * B * Hd * h * w)
                res[f"kernel_clstm_gates_level{lvl}_{name}_us"] = dict(k, bytes=nbytes)
            src = new(B, dec32.skip_dims_out[2], *sizes[2])
            dst = new(B, dec32.skip_dims_out[2] + dec32.skip_dims_out[3], *sizes[3])
            k = us(windows(lambda: D.upsample_bilinear_into(src, dst, 0, "write"), a.repeats, 50))
            res[f"kernel_upsample_into_level3_{name}_us"] = dict(k, bytes=es * (src.numel() + src.shape[0] * src.shape[1] * dst.shape[2] * dst.shape[3]))
    for form in ("fused", "graph"):
        f32, f32b, b16 = res[f"{form}_fp32"], res[f"{form}_fp32_again"], res[f"{form}_bf16"]
        spread = max(f32["max"] - f32["min"], f32b["max"] - f32b["min"], b16["max"] - b16["min"])
        res[f"{form}_larger_spread"] = spread
        # a speed-up is claimed only when the medians differ by more than the larger min-max spread, against BOTH fp32 runs
        res[f"{form}_bf16_faster_by_more_than_the_spread"] = bool(min(f32["median"], f32b["median"]) - b16["median"] > spread)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "decoder_timing needs an MI355X"
    if a.dtype == "bf16":
        return emit(bf16_report(a), a.out)
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
    emit(res, a.out)


if __name__ == "__main__":
    main()
