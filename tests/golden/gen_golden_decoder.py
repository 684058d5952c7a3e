"""Writes tests/golden/g23_refine_decoder{,_sum,_chain}.npz from the reference's own decoder (three files: each stays below
the size limit of a committed file; keys '<mode>/...' of 'concat' in the first, of 'sum' in the second, 'chain/...' in the third).

    python tests/golden/gen_golden_decoder.py <path to a checkout of the reference>

The reference's ``RSISMask`` (dmm/modules/base.py:71-188, with dmm/modules/clstm.py) is imported from the checkout at
generation time behind module stubs (base.py imports maskrcnn_benchmark and torchvision at module level and the decoder
touches neither).  The fixture holds arrays and names only:

  <mode>/param/<name>          the module's parameters by the reference's names (mode = concat | sum; hidden 32, 3x3).
                               Default initialisation under a fixed seed, rounded to fp16-representable values and stored
                               as fp16 (exact; loaded back as fp32) -- two modes of fp32 weights would not fit a fixture.
  <mode>/skip<i>, mask<i>      refine_input_feat / mask_lstm of a 47 x 66 image, 2 videos (levels 2 x 3 .. 12 x 17)
  <mode>/sp<i>_h, sp<i>_c, tm<i>   a spatial state and temporal hiddens
  <mode>/<case>/out_mask, h<i>, c<i>             the reference's fp32 outputs, case = the state combination:
                               nn (no state), sn (spatial), nt (temporal), st (both)
  <mode>/<case>/f64/...        the same from a .double() copy of the module on the same inputs
  <mode>/<case>/e_ref/...      max |fp32 - fp64| per output
  chain/...                    the concat module: 3 objects over 2 time steps of a 29 x 43 image driven like evaluator.py:179-212,
                               one invalid (video, object) pair: inputs, ``outs`` and ``mask_hist_new`` per step (fp32,
                               fp64, e_ref), and the number of temporal hidden lists.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))


def stub_and_import(ref_root):
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    mod("maskrcnn_benchmark")
    mod("maskrcnn_benchmark.layers", nms=None)
    mod("maskrcnn_benchmark.layers.misc", interpolate=F.interpolate)
    mod("maskrcnn_benchmark.structures")
    mod("maskrcnn_benchmark.structures.bounding_box", BoxList=None)
    mod("maskrcnn_benchmark.structures.image_list", to_image_list=None)
    mod("maskrcnn_benchmark.modeling")
    mod("maskrcnn_benchmark.modeling.detector", build_detection_model=None)
    mod("maskrcnn_benchmark.config", cfg=None)
    mod("maskrcnn_benchmark.utils")
    mod("maskrcnn_benchmark.utils.checkpoint", DetectronCheckpointer=None)
    mod("maskrcnn_benchmark.data", transforms=types.SimpleNamespace())
    mod("torchvision", transforms=types.SimpleNamespace())
    sys.path.insert(0, ref_root)
    from dmm.modules.base import RSISMask
    return RSISMask


def make_args(skip_mode, hidden=32):
    return types.SimpleNamespace(hidden_size=hidden, kernel_size=3, dropout=0.0, skip_mode=skip_mode, prev_mask_d=1,
                                 use_gpu=False)


def level_sizes(H, W):
    return [(-(-H // (1 << k)), -(-W // (1 << k))) for k in (5, 4, 3, 2)]


def np32(t):
    return t.detach().to(torch.float32).numpy()


def record(out, prefix, res32, res64):
    def flat(res):
        om, hl = res
        d = {"out_mask": om}
        for i, (h, c) in enumerate(hl):
            d[f"h{i}"], d[f"c{i}"] = h, c
        return d
    a, b = flat(res32), flat(res64)
    for k in a:
        out[f"{prefix}/{k}"] = np32(a[k])
        out[f"{prefix}/f64/{k}"] = b[k].detach().numpy()
        out[f"{prefix}/e_ref/{k}"] = np.float64((a[k].double() - b[k]).abs().max().item())


def main():
    ref_root = sys.argv[1]
    RSISMask = stub_and_import(ref_root)
    torch.set_num_threads(8)
    out = {}
    B, hidden = 2, 32
    sizes = level_sizes(47, 66)
    skip_ch = [hidden, hidden, hidden // 2, hidden // 4]
    dims = [hidden, hidden // 2, hidden // 4, hidden // 8]
    decoders = {}
    with torch.no_grad():
        for mi, mode in enumerate(("concat", "sum")):
            torch.manual_seed(2300 + mi)
            dec = RSISMask(make_args(mode)).eval()
            for p in dec.parameters():
                p.copy_(p.half().float())
            for name, p in dec.state_dict().items():
                out[f"{mode}/param/{name}"] = p.numpy().astype(np.float16)
                assert np.array_equal(out[f"{mode}/param/{name}"].astype(np.float32), p.numpy())
            dec64 = RSISMask(make_args(mode)).eval().double()
            dec64.load_state_dict({k: v.double() for k, v in dec.state_dict().items()}, strict=True)
            decoders[mode] = (dec, dec64)
            g = torch.Generator().manual_seed(2310 + mi)
            feats = [torch.randn((B, c) + s, generator=g) for c, s in zip(skip_ch, sizes)]
            masks = [torch.rand((B, 3) + s, generator=g) for s in sizes]
            spatial = [[0.5 * torch.randn((B, d) + s, generator=g).tanh(), torch.randn((B, d) + s, generator=g)]
                       for d, s in zip(dims, sizes)]
            temporal = [0.5 * torch.randn((B, d) + s, generator=g).tanh() for d, s in zip(dims, sizes)]
            for i in range(4):
                out[f"{mode}/skip{i}"], out[f"{mode}/mask{i}"] = np32(feats[i]), np32(masks[i])
                out[f"{mode}/sp{i}_h"], out[f"{mode}/sp{i}_c"] = np32(spatial[i][0]), np32(spatial[i][1])
                out[f"{mode}/tm{i}"] = np32(temporal[i])
            dbl = lambda ts: [t.double() for t in ts]
            for case, sp, tm in (("nn", None, None), ("sn", spatial, None), ("nt", None, temporal),
                                 ("st", spatial, temporal)):
                r32 = dec(feats, masks, None if sp is None else [list(s) for s in sp], tm)
                r64 = dec64(dbl(feats), dbl(masks), None if sp is None else [dbl(s) for s in sp],
                            None if tm is None else dbl(tm))
                record(out, f"{mode}/{case}", r32, r64)

        # ---- the object chain ----------------------------------------------------------------------------------------
        dec, dec64 = decoders["concat"]
        H, W, O, T = 29, 43, 4, 2
        sizes = level_sizes(H, W)
        g = torch.Generator().manual_seed(2390)
        valid = torch.tensor([[1, 1, 1, 0], [1, 0, 1, 0]])                      # (video 1, object 1) is invalid
        steps, feats_t = [], []
        for _ in range(T):
            feats_t.append([torch.randn((B, c) + s, generator=g) for c, s in zip(skip_ch, sizes)])
            prev_mask = (torch.rand((B, O, H * W), generator=g) > 0.6).float()
            y_mask = (torch.rand((B, O, H * W), generator=g) > 0.6).float()
            init_pred = torch.rand((B, O, H, W), generator=g).half().float()
            hist = torch.rand((B, O, H, W), generator=g).half().float()
            steps.append((prev_mask, y_mask, init_pred, hist))
        out["chain/valid"] = valid.numpy().astype(np.int64)
        out["chain/size"] = np.array([H, W], dtype=np.int64)
        for t in range(T):
            for i in range(4):
                out[f"chain/t{t}/skip{i}"] = np32(feats_t[t][i])
            pm, ym, ip, hi = steps[t]
            out[f"chain/t{t}/prev_mask"], out[f"chain/t{t}/y_mask"] = pm.numpy().astype(np.uint8), ym.numpy().astype(np.uint8)
            out[f"chain/t{t}/init_pred"], out[f"chain/t{t}/mask_hist"] = ip.numpy().astype(np.float16), hi.numpy().astype(np.float16)

        results = {}
        for name, d, dtype in (("f32", dec, torch.float32), ("f64", dec64, torch.float64)):
            prev_thid, res = None, []
            for t in range(T):
                feats = [f.to(dtype) for f in feats_t[t]]
                # one time step at a time so that each step sees its own features; the temporal state is handed on
                (r,), thid = _one_step(d, feats, steps[t], valid, H, W, dtype, prev_thid)
                res.append(r)
                prev_thid = thid
            results[name] = (res, prev_thid)
        for t in range(T):
            for k, idx in (("outs", 0), ("mask_hist_new", 1)):
                a, b = results["f32"][0][t][idx], results["f64"][0][t][idx]
                out[f"chain/t{t}/{k}"] = np32(a)
                out[f"chain/t{t}/f64/{k}"] = b.numpy()
                out[f"chain/t{t}/e_ref/{k}"] = np.float64((a.double() - b).abs().max().item())
        out["chain/n_thid"] = np.int64(len(results["f32"][1]))

    for fname, prefix in (("g23_refine_decoder", "concat/"), ("g23_refine_decoder_sum", "sum/"),
                          ("g23_refine_decoder_chain", "chain/")):
        part = {k: v for k, v in out.items() if k.startswith(prefix)}
        path = os.path.join(HERE, fname + ".npz")
        np.savez_compressed(path, **part)
        print("wrote", path, os.path.getsize(path), "bytes,", len(part), "arrays")
        assert os.path.getsize(path) < (1 << 20)
    for k in sorted(out):
        if "/e_ref/" in k:
            print(f"  {k} = {float(out[k]):.3e}")


def _one_step(decoder, feats, step, valid, H, W, dtype, prev_thid):
    """drive_chain for one time step, starting from ``prev_thid``."""
    B, O = valid.shape
    n_obj = max(1, int((valid.sum(0) > 0).sum()))
    maxpool = nn.MaxPool2d((2, 2), ceil_mode=True)
    up = nn.UpsamplingBilinear2d(size=(H, W))
    prev_mask, y_mask, init_pred, hist = step
    hist_new = hist.clone().to(dtype)
    hidden_spatial, thid, out_masks = None, [], []
    for t in range(n_obj):
        hidden_temporal = prev_thid[t] if prev_thid is not None else None
        m = torch.cat([prev_mask[:, t].view(B, 1, H * W), y_mask[:, t].view(B, 1, H * W),
                       init_pred[:, t].reshape(B, 1, H * W)], dim=2).view(B, 3, H, W).to(dtype)
        m = maxpool(m)
        pyr = []
        for _ in range(len(feats)):
            m = maxpool(m)
            pyr.append(m)
        out_mask, hidden = decoder(feats, list(reversed(pyr)), hidden_spatial, hidden_temporal)
        hidden_spatial = hidden
        thid.append([h[0] for h in hidden])
        out_mask = up(out_mask)
        for b in range(B):
            if valid[b, t]:
                hist_new[b, t:t + 1] = torch.sigmoid(out_mask[b])
        out_masks.append(out_mask.view(B, -1))
    outs = torch.sigmoid(torch.cat(out_masks, 1).view(B, n_obj, -1))
    pad = outs.new_zeros(B, O, H * W)
    pad[:, :n_obj] = outs
    return [(pad, hist_new)], thid


if __name__ == "__main__":
    main()
