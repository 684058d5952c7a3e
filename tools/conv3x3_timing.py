#!/usr/bin/env python3
"""Per-layer time of the deterministic mode's own 3x3 convolution (``ops.conv3x3_bf16`` = dmm_conv3x3_bf16) on the in-envelope
3x3 shapes of config 4 -- ResNet-101 body and heads at 12 x 3 x 255 x 448 -- beside ``F.conv2d`` with and without
``cudnn.deterministic``.  HIP-event time per call over a window of launches after a warm-up; FLOP = 2 * B * Ho * Wo * co * 9 *
ci, so TFLOP/s is the algorithm's work over the call's device time (a call of a split reduction is two launches).

    python tools/conv3x3_timing.py [--frames 12] [--out FILE.json] [--skip-library-det] [--narrow-only] [--stem-only]

Then the NARROW shapes (``ops.conv3x3_narrow_bf16`` = dmm_conv3x3_narrow_bf16; the level-2 heads at frames x 64 x 112: 256 -> 32
and 32 -> 128 forward, 32 -> 256 and 128 -> 32 as their data gradients): the own kernel beside ``F.conv2d`` with and without
``cudnn.deterministic`` and beside the unfold + ``mm`` route the "own" setting takes, and the narrow weight gradient
(``ops.wgrad3x3_narrow_bf16``) beside unfold + ``mm``.

Then the 7x7 / stride 2 STEM (3 -> 64 at frames x 255 x 448; ``ops.conv7x7s2_stem_bf16`` = dmm_conv7x7s2_stem_bf16 beside
``_conv_as_gemm``, ``ops.wgrad7x7s2_stem_bf16`` beside unfold + ``mm``): min / median / max over windows that alternate between
the two routes, and the bytes each direction must move (x + w + y, or dy + x + dw) over the median as a bandwidth and as a
fraction of the HBM peak.

Prints three markdown tables and one JSON line; needs an MI355X."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shapes(frames):
    """(ci, co, stride, H, W) -> how many convolutions of a ResNet-101 encoder step have it (forward hooks on one pass)."""
    import torch
    import torch.nn as nn
    from dmm_net_amd.encoder import FeatureEncoder
    from dmm_net_amd.train_encoder import _wgrad_ok
    enc = FeatureEncoder("resnet101").to("cuda:0").eval()
    seen, hooks = {}, []

    def hook(m, inp, out):
        k = (m.in_channels, m.out_channels, m.stride[0], inp[0].shape[2], inp[0].shape[3])
        seen[k] = seen.get(k, 0) + 1
    for m in enc.modules():
        if isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3) and m.padding == (1, 1) and _wgrad_ok(m):
            hooks.append(m.register_forward_hook(hook))
    with torch.no_grad():
        enc(torch.randn(frames, 3, 255, 448, device="cuda:0"))
    for h in hooks:
        h.remove()
    del enc
    torch.cuda.empty_cache()
    return seen


def timed(fn, budget_ms=200.0, max_iters=200):
    """Device time per call in ms: warm up, size the window from a first call, then one event pair round the window."""
    import torch
    for _ in range(2):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    n = int(max(3, min(max_iters, budget_ms / max(a.elapsed_time(b), 1e-3))))
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


NARROW = [(256, 32), (32, 128), (32, 256), (128, 32)]      # (ci, co) at frames x 64 x 112


def narrow_rows(frames, skip_library_det):
    """The narrow shapes: forward / data gradient (the same entry) and weight gradient, own kernels beside the other routes."""
    import torch
    import torch.nn.functional as F
    from dmm_net_amd import ops
    from dmm_net_amd.train_encoder import _conv_as_gemm
    cl = torch.channels_last
    H, W = 64, 112
    g = torch.Generator(device="cuda:0").manual_seed(1)
    rows = []
    for ci, co in NARROW:
        x = torch.randn((frames, ci, H, W), generator=g, device="cuda:0").bfloat16().contiguous(memory_format=cl)
        w = (torch.randn((co, ci, 3, 3), generator=g, device="cuda:0") / (3 * ci ** 0.5)).bfloat16().contiguous(memory_format=cl)
        dy = torch.randn((frames, co, H, W), generator=g, device="cuda:0").bfloat16().contiguous(memory_format=cl)
        flop = 2.0 * frames * H * W * co * 9 * ci
        own = timed(lambda: ops.conv3x3_narrow_bf16(x, w, None))
        unfold = timed(lambda: _conv_as_gemm(x, w, None, (1, 1), (1, 1)), budget_ms=100.0, max_iters=50)
        with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=False):
            lib = timed(lambda: F.conv2d(x, w, None, 1, 1))
            same = float((ops.conv3x3_narrow_bf16(x, w, None).float() - F.conv2d(x, w, None, 1, 1).float()).abs().max())
        lib_det = None
        if not skip_library_det:
            with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
                lib_det = timed(lambda: F.conv2d(x, w, None, 1, 1), budget_ms=60.0, max_iters=20)
        wg_own = timed(lambda: ops.wgrad3x3_narrow_bf16(dy, x))

        def wg_unfold():                                 # _DetConvFn's weight gradient
            cols = F.unfold(x, (3, 3), 1, 1, 1).transpose(1, 2).reshape(frames * H * W, ci * 9)
            return torch.mm(dy.permute(0, 2, 3, 1).reshape(frames * H * W, co).t(), cols)
        wg_un = timed(wg_unfold, budget_ms=100.0, max_iters=50)
        rows.append({"ci": ci, "co": co, "H": H, "W": W, "gflop": round(flop / 1e9, 3), "own_ms": round(own, 4),
                     "own_tflops": round(flop / own / 1e9, 1), "unfold_mm_ms": round(unfold, 4), "library_ms": round(lib, 4),
                     "library_det_ms": None if lib_det is None else round(lib_det, 4), "max_abs_own_minus_library": same,
                     "wgrad_own_ms": round(wg_own, 4), "wgrad_unfold_mm_ms": round(wg_un, 4)})
        del x, w, dy
        torch.cuda.empty_cache()
    print()
    print("| ci | co | H x W | GFLOP | own ms | own TFLOP/s | unfold + mm ms | F.conv2d ms | F.conv2d deterministic ms | "
          "wgrad own ms | wgrad unfold + mm ms |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['ci']} | {r['co']} | {r['H']} x {r['W']} | {r['gflop']} | {r['own_ms']} | {r['own_tflops']} | "
              f"{r['unfold_mm_ms']} | {r['library_ms']} | {r['library_det_ms']} | {r['wgrad_own_ms']} | {r['wgrad_unfold_mm_ms']} |")
    return rows


HBM_PEAK = 8.0e12                        # bytes / s (MI355X)


def stem_rows(frames, windows=7):
    """The stem at config 4's size: own forward beside ``_conv_as_gemm``, own weight gradient beside unfold + ``mm``; each route
    timed in ``windows`` windows, the two routes of a direction alternating, -> min / median / max per call."""
    import statistics
    import torch
    import torch.nn.functional as F
    from dmm_net_amd import ops
    from dmm_net_amd.train_encoder import _conv_as_gemm
    cl = torch.channels_last
    H, W = 255, 448
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    g = torch.Generator(device="cuda:0").manual_seed(2)
    x = torch.randn((frames, 3, H, W), generator=g, device="cuda:0").bfloat16().contiguous(memory_format=cl)
    w = (torch.randn((64, 3, 7, 7), generator=g, device="cuda:0") / 147 ** 0.5).bfloat16().contiguous(memory_format=cl)
    dy = torch.randn((frames, 64, Ho, Wo), generator=g, device="cuda:0").bfloat16().contiguous(memory_format=cl)
    M = frames * Ho * Wo

    def wg_unfold():                                     # _DetConvFn's weight gradient
        cols = F.unfold(x, (7, 7), 1, 3, 2).transpose(1, 2).reshape(M, 147)
        return torch.mm(dy.permute(0, 2, 3, 1).reshape(M, 64).t(), cols)
    must = {"forward": x.numel() * 2 + w.numel() * 2 + M * 64 * 2, "wgrad": M * 64 * 2 + x.numel() * 2 + 64 * 147 * 4}
    pairs = {"forward": (lambda: ops.conv7x7s2_stem_bf16(x, w, None), lambda: _conv_as_gemm(x, w, None, (2, 2), (3, 3))),
             "wgrad": (lambda: ops.wgrad7x7s2_stem_bf16(dy, x), wg_unfold)}
    rows = []
    for what, (own, route) in pairs.items():
        t = {"own": [], "unfold_mm": []}
        for _ in range(windows):
            t["own"].append(timed(own, budget_ms=100.0))
            t["unfold_mm"].append(timed(route, budget_ms=100.0, max_iters=50))
        row = {"what": what, "frames": frames, "H": H, "W": W, "must_move_mb": round(must[what] / 1e6, 2)}
        for k, v in t.items():
            med = statistics.median(v)
            row[k] = {"min_ms": round(min(v), 4), "median_ms": round(med, 4), "max_ms": round(max(v), 4),
                      "must_move_tb_s": round(must[what] / med / 1e9, 3),
                      "fraction_of_hbm_peak": round(must[what] / (med * 1e-3) / HBM_PEAK, 3)}
        rows.append(row)
    y_own, y_route = ops.conv7x7s2_stem_bf16(x, w, None).float(), _conv_as_gemm(x, w, None, (2, 2), (3, 3)).float()
    dw_own, dw_route = ops.wgrad7x7s2_stem_bf16(dy, x), wg_unfold().float().view(64, 3, 7, 7)
    rows[0]["max_abs_own_minus_unfold_mm"] = float((y_own - y_route).abs().max())
    rows[1]["max_abs_own_minus_unfold_mm"] = float((dw_own - dw_route).abs().max())
    rows[1]["max_abs_dw"] = float(dw_own.abs().max())
    print()
    print("| stem | must move MB | route | min ms | median ms | max ms | TB/s of must-move | of HBM peak |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        for k in ("own", "unfold_mm"):
            q = r[k]
            print(f"| {r['what']} | {r['must_move_mb']} | {k} | {q['min_ms']} | {q['median_ms']} | {q['max_ms']} | "
                  f"{q['must_move_tb_s']} | {q['fraction_of_hbm_peak']} |")
    return rows


def main():
    import torch
    import torch.nn.functional as F
    from dmm_net_amd import ops
    if not torch.cuda.is_available():
        sys.exit("conv3x3_timing needs an MI355X")
    a = sys.argv[1:]
    frames = int(a[a.index("--frames") + 1]) if "--frames" in a else 12
    cl = torch.channels_last
    rows = []
    g = torch.Generator(device="cuda:0").manual_seed(0)
    if "--stem-only" in a:
        summary = {"frames": frames, "stem_rows": stem_rows(frames)}
        print(json.dumps(summary), flush=True)
        if "--out" in a:
            with open(a[a.index("--out") + 1], "w") as f:
                json.dump(summary, f, indent=1)
        return
    wide = {} if "--narrow-only" in a else shapes(frames)
    for (ci, co, stride, H, W), count in sorted(wide.items(), key=lambda kv: (-kv[0][3], kv[0])):
        x = torch.randn((frames, ci, H, W), generator=g, device="cuda:0").bfloat16().contiguous(memory_format=cl)
        w = (torch.randn((co, ci, 3, 3), generator=g, device="cuda:0") / (3 * ci ** 0.5)).bfloat16().contiguous(memory_format=cl)
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        flop = 2.0 * frames * Ho * Wo * co * 9 * ci
        own = timed(lambda: ops.conv3x3_bf16(x, w, None, stride))
        with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=False):
            lib = timed(lambda: F.conv2d(x, w, None, stride, 1))
            same = float((ops.conv3x3_bf16(x, w, None, stride).float() - F.conv2d(x, w, None, stride, 1).float()).abs().max())
        lib_det = None
        if "--skip-library-det" not in a:
            with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
                lib_det = timed(lambda: F.conv2d(x, w, None, stride, 1), budget_ms=60.0, max_iters=20)
        rows.append({"ci": ci, "co": co, "stride": stride, "H": H, "W": W, "count": count, "gflop": round(flop / 1e9, 3),
                     "own_ms": round(own, 4), "own_tflops": round(flop / own / 1e9, 1), "library_ms": round(lib, 4),
                     "library_det_ms": None if lib_det is None else round(lib_det, 4), "max_abs_own_minus_library": same})
    print("| ci | co | stride | H x W in | per step | GFLOP | own ms | own TFLOP/s | F.conv2d ms | F.conv2d deterministic ms |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['ci']} | {r['co']} | {r['stride']} | {r['H']} x {r['W']} | {r['count']} | {r['gflop']} | {r['own_ms']} | "
              f"{r['own_tflops']} | {r['library_ms']} | {r['library_det_ms']} |")
    tot = lambda k: round(sum(r[k] * r["count"] for r in rows if r[k] is not None), 3)
    summary = {"frames": frames, "forward_sum_ms": {"own": tot("own_ms"), "library": tot("library_ms"),
                                                   "library_det": tot("library_det_ms")}, "rows": rows,
               "narrow_rows": narrow_rows(frames, "--skip-library-det" in a), "stem_rows": stem_rows(frames)}
    print(json.dumps(summary), flush=True)
    if "--out" in a:
        with open(a[a.index("--out") + 1], "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
