"""Times one refine training step on the GPU in three forms and prints ONE JSON line.

    python tools/refine_train_timing.py [--out FILE] [--repeats 3] [--iters 5] [--no-profile] [--dtype fp32|bf16]

Config 4's sizes: 4 videos of 255 x 448, hidden 128, 'concat', 5 objects, TWO frames chained as the trainer chains them
(frame 1's ``prev_mask`` is frame 0's ``outs``, attached; the temporal hiddens carry their graph), so the cross-frame
gradient through the pyramid is live.  One step = both frames' forward with the mask loss + the backward of the summed loss
to every parameter, every skip map and both frames' ``init_pred``.

  (a) ``loop_stock``        the trainer's loop on the stock decoder
  (b) ``loop_fused_train``  the same loop on ``decoder.fused_train = True`` (torch ops around the fused cell)
  (c) ``step``              ``RefineTrainStep`` on its fused route

HIP events after warm-up, min / median / max over ``repeats`` windows of ``iters`` steps, ms per step; (b) is measured twice,
before and after (c), and its spread is taken over both.  ``torch.cuda.max_memory_allocated`` of one step per form, and the
kernels of one step of (b) and (c) by device time from ``torch.profiler``.

``--dtype bf16`` adds, in the same run, (d) ``step_bf16``: the step with ``decoder.train_dtype = torch.bfloat16`` on bf16 skip maps
(what a trainer behind a bf16 encoder hands over), then (c) once more (``step_again``: the fp32 step's spread under the same
conditions), the kernels of one bf16 step, and every 16-bit training kernel beside its fp32 sibling at the finest level's sizes
(us per call)."""
import argparse
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dmm_net_amd import decoder as D  # noqa: E402


class TrainerLoop(D.RefineTrainStep):
    """The step pinned to its stock route: the trainer's loop on ``decoder.forward``, whatever form that takes."""

    def _fused(self, *a):
        self.last_route = "stock"
        return self._stock(*a)


def windows(fn, repeats, iters, warmup=2):
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


def kernel_table(fn, top=24):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    rows = {}
    for e in prof.events():
        if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower():
            t = float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0))
            r = rows.setdefault(e.name, [0, 0.0])
            r[0] += 1
            r[1] += t
    total = sum(t for _, t in rows.values())
    table = sorted(rows.items(), key=lambda kv: -kv[1][1])[:top]
    return {"device_time_ms": total / 1e3, "launches": sum(n for n, _ in rows.values()),
            "kernels": [{"name": k[:96], "calls": n, "ms": t / 1e3} for k, (n, t) in table]}


def kernel_pairs(dec, B, n_obj, O, H, W, repeats, iters=50):
    """Every 16-bit training kernel beside its fp32 sibling, us per call: the cell's backward and the upsample's at the finest
    level, the trainer's finish and its backward on conv_out's output for all objects."""
    dev = "cuda:0"
    Hd, (h, w) = dec.skip_dims_out[3], D.pyramid_sizes(H, W)[3]
    r = lambda *s: torch.randn(s, device=dev)
    pre, cp, dh, dc = [r(B, 4 * Hd, h, w) for _ in range(3)], r(B, Hd, h, w), r(B, Hd, h, w), r(B, Hd, h, w)
    masks, wm = torch.rand(B, 3, h, w, device=dev), r(4 * Hd, 9) * 0.3
    d_up = r(B, dec.skip_dims_out[2], h, w)
    h2, w2 = D.pyramid_sizes(H, W)[2]
    logits, d_outs = r(n_obj * B, 1, 2 * h, 2 * w).view(n_obj, B, 2 * h, 2 * w).transpose(0, 1), r(B, O, H, W)
    out = {}
    with torch.no_grad():
        for name, to in (("fp32", lambda t: t), ("bf16", lambda t: t.to(torch.bfloat16))):
            p16, dh16, up16, lg16 = [to(p) for p in pre], to(dh), to(d_up), to(logits.contiguous()).view(B, n_obj, 2 * h, 2 * w)
            for label, fn in (("clstm_gates_bwd_all_outputs", lambda: D.clstm_gates_bwd(p16, masks, wm, cp, dh16, dc)),
                              ("clstm_gates_bwd_d_pre_d_cell_prev_only",
                               lambda: D.clstm_gates_bwd(p16, masks, wm, cp, dh16, dc, need=(True, False, False))),
                              ("upsample_bilinear_bwd", lambda: D.upsample_bilinear_bwd(up16, 0, up16.shape[1], h2, w2)),
                              ("refine_train_finish", lambda: D.refine_train_finish(lg16, O, H, W)),
                              ("refine_train_finish_bwd", lambda: D.refine_train_finish_bwd(lg16, d_outs))):
                out[f"{label}_{name}"] = {k: 1e3 * v for k, v in windows(fn, repeats, iters).items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "refine_train_timing needs an MI355X"
    dev = "cuda:0"
    B, O, n_obj, H, W, hidden, T = 4, 6, 5, 255, 448, 128, 2
    torch.manual_seed(0)
    args = types.SimpleNamespace(hidden_size=hidden, kernel_size=3, dropout=0.0, skip_mode="concat", prev_mask_d=1, use_gpu=True)
    dec = D.RSISMask(args).eval().to(dev)
    sizes = D.pyramid_sizes(H, W)
    ch = [hidden, hidden, hidden // 2, hidden // 4]
    frames = [{"feats": [torch.randn((B, c) + s, device=dev, requires_grad=True) for c, s in zip(ch, sizes)],
               "y_mask": (torch.rand(B, O, H * W, device=dev) > 0.6).float(),
               "init_pred": torch.rand(B, O, H, W, device=dev, requires_grad=True)} for _ in range(T)]
    valid = torch.zeros(B, O, dtype=torch.long, device=dev)
    valid[:, :n_obj] = 1
    valid[1, 2] = 0
    sw = valid.float()
    leaves = [t for fr in frames for t in fr["feats"] + [fr["init_pred"]]] + list(dec.parameters())

    def make(step, frames=frames, leaves=leaves):
        def run():
            ref_mask = frames[0]["y_mask"]
            prev_mask, state, total = ref_mask, None, 0
            for fr in frames:
                loss, _, outs, state = step(fr["feats"], prev_mask, ref_mask, fr["init_pred"], fr["y_mask"], sw, valid, state)
                total = total + loss
                prev_mask = outs
            return torch.autograd.grad(total, leaves)
        return run

    res = {"what": "refine training step, two frames (forward + loss + backward)", "B": B, "O": O, "objects": n_obj, "H": H,
           "W": W, "hidden": hidden, "skip_mode": "concat", "frames": T, "unit": "ms per step", "repeats": a.repeats,
           "iters": a.iters}

    def measure(step, fused_train, **kw):
        dec.fused_train = fused_train
        fn = make(step, **kw)
        t = windows(fn, a.repeats, a.iters)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        t["max_memory_allocated_MiB"] = torch.cuda.max_memory_allocated() / 2 ** 20
        t["held_before_the_step_MiB"] = base / 2 ** 20
        t["route"] = step.last_route
        return t

    loop, step = TrainerLoop(dec), D.RefineTrainStep(dec)
    res["loop_stock"] = measure(loop, False)
    res["loop_fused_train"] = measure(loop, True)
    c0 = dec.conv_calls
    res["step"] = measure(step, True)
    res["step_convolutions_per_step"] = (dec.conv_calls - c0) // (2 + a.repeats * a.iters + 1)
    res["loop_fused_train_again"] = measure(loop, True)
    assert res["step"]["route"] == "fused" and res["loop_fused_train"]["route"] == "stock"
    b_min = min(res["loop_fused_train"]["min"], res["loop_fused_train_again"]["min"])
    b_max = max(res["loop_fused_train"]["max"], res["loop_fused_train_again"]["max"])
    res["loop_fused_train_spread"] = b_max - b_min
    res["step_spread"] = res["step"]["max"] - res["step"]["min"]
    res["step_faster_than_loop_fused_train_by_more_than_its_spread"] = bool(b_min - res["step"]["max"] > b_max - b_min)
    if not a.no_profile:
        for name, st in (("loop_fused_train", loop), ("step", step)):
            dec.fused_train = True
            try:
                res[f"profile_{name}"] = kernel_table(make(st))
            except Exception as e:                                    # the timing above stands without the table
                res[f"profile_{name}_error"] = repr(e)
    if a.dtype == "bf16":
        bf16 = torch.bfloat16
        frames16 = [dict(fr, feats=[f.detach().to(bf16).requires_grad_(True) for f in fr["feats"]]) for fr in frames]
        low = dict(frames=frames16, leaves=[t for fr in frames16 for t in fr["feats"] + [fr["init_pred"]]] + list(dec.parameters()))
        dec.train_dtype = bf16
        c0 = dec.conv_calls
        res["step_bf16"] = measure(step, True, **low)
        res["step_bf16_convolutions_per_step"] = (dec.conv_calls - c0) // (2 + a.repeats * a.iters + 1)
        if not a.no_profile:
            try:
                res["profile_step_bf16"] = kernel_table(make(step, **low))
            except Exception as e:
                res["profile_step_bf16_error"] = repr(e)
        dec.train_dtype = torch.float32
        res["step_again"] = measure(step, True)
        assert res["step_bf16"]["route"] == "fused" and res["step_again"]["route"] == "fused"
        s_min, s_max = min(res["step"]["min"], res["step_again"]["min"]), max(res["step"]["max"], res["step_again"]["max"])
        res["step_fp32_spread"] = s_max - s_min
        res["step_bf16_faster_than_step_by_more_than_its_spread"] = bool(s_min - res["step_bf16"]["max"] > s_max - s_min)
        res["step_bf16_slower_than_step_by_more_than_its_spread"] = bool(res["step_bf16"]["min"] - s_max > s_max - s_min)
        res["kernels_us"] = kernel_pairs(dec, B, n_obj, O, H, W, a.repeats)
    dec.fused_train = False
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
