"""The feature-similarity backward (``dmm_feature_sim_bwd_f32``: a row form, a per-frame form and a wave-per-row form behind
option FEAT_BWD_FRAME) and the training call's whole backward against float64 autograd (tests/bwd_ref.py) -- a reference
outside the kernels; test_gpu_parity.py compares the three forms with each other only.

Bound: max |got - ref| <= 2e-5 * max |ref| per gradient tensor.  A zero feature row, a row under the eps clamp and
a row scaled by 1e4 have gradients 1e8 times larger / 1e4 times smaller than their neighbours', so the tensor-wide bound
would say nothing about the one or about the others: those rows are held to the same 2e-5 of THEIR largest entry, and
the tensor-wide bound is taken over the ordinary rows.
"""
import numpy as np
import pytest
import torch

import bwd_ref
from conftest import record_achieved
from dmm_net_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 2e-5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _read_int(name):
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "dmm_net_amd", "csrc", "dmm_cosine.hip")) as fh:
        return int(re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", fh.read()).group(1))


WAVE_MAX_B = _read_int("kFeatBwdWaveMaxB")      # by batch size (option -1): the wave-per-row form up to this many frames


def _check(tag, got, ref, special=()):
    """got / ref [B, R, D]; ``special``: (b, row) held to their own scale."""
    got = got.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), tag
    mask = np.ones(ref.shape[:2], bool)
    for b, r in special:
        if b < ref.shape[0] and r < ref.shape[1]:
            mask[b, r] = False
            scale = float(np.abs(ref[b, r]).max())
            err = float(np.abs(got[b, r] - ref[b, r]).max())
            record_achieved(f"feature_bwd_ref/{tag}/row{b}_{r}", err / scale if scale > 0 else err)
            print(f"{tag} row ({b}, {r}): err {err:.3e} scale {scale:.3e}")
            assert err <= RTOL * scale, (tag, b, r, err, scale)
    scale = float(np.abs(ref[mask]).max()) if mask.any() else 0.0
    err = float(np.abs(got[mask] - ref[mask]).max()) if mask.any() else 0.0
    record_achieved(f"feature_bwd_ref/{tag}", err / scale if scale > 0 else err)
    print(f"{tag}: err {err:.3e} scale {scale:.3e}")
    assert err <= RTOL * scale, (tag, err, scale)


def _inputs(B, N, M, D, seed):
    r = np.random.default_rng(seed)
    f = np.float32
    tf = r.standard_normal((B, M, D)).astype(f)
    pf = np.maximum(r.standard_normal((B, N, D)), 0).astype(f)
    return dict(tf=tf, pf=pf, dsim=r.standard_normal((B, M, N)).astype(f), gt=(r.random((B, M, N)) > 0.9).astype(f),
                dl=r.random(B).astype(f))


def _run_all(tag, x, w, nv, mv, loss, special_p=(), special_t=(), modes=(0, 1, 2)):
    tf, pf = dev(x["tf"]), dev(x["pf"])
    tn, tnorm = ops.feature_normalize(tf, want_norms=True)
    pn, pnorm = ops.feature_normalize(pf, want_norms=True)
    cos = ops.cosine(tn, pn)
    ref_t, ref_p = bwd_ref.feature_grads(x["tf"], x["pf"], x["dsim"], w, x["gt"] if loss else None, x["dl"] if loss else None,
                                         nv, mv)                       # once, shared by the three kernels
    dnv = None if nv is None else dev(np.asarray(nv, np.int32))
    dmv = None if mv is None else dev(np.asarray(mv, np.int32))
    args = (dev(x["dsim"]), cos if loss else None, dev(x["gt"]) if loss else None, dev(x["dl"]) if loss else None, w, tf, pf,
            tn, pn, tnorm, pnorm, dnv, dmv)
    out = {}
    for mode in modes:
        with _lib.options(FEAT_BWD_FRAME=mode):
            gt_, gp_ = ops.feature_sim_bwd(*args)
        torch.cuda.synchronize()
        _check(f"{tag}/mode{mode}/g_feat_t", gt_, ref_t, special_t)
        _check(f"{tag}/mode{mode}/g_feat_p", gp_, ref_p, special_p)
        out[mode] = (gt_, gp_)
    return out, (ref_t, ref_p)


@pytest.mark.parametrize("B,N,M,D", [(3, 50, 10, 512), (2, 200, 20, 256), (4, 7, 32, 64), (2, 256, 1, 1024), (1, 3, 5, 128),
                                     (4, 61, 33, 512), (1, 1, 1, 64), (2, 65, 8, 192), (9, 50, 5, 256)])
def test_three_feature_backward_kernels_against_float64_autograd(B, N, M, D):
    """FEAT_BWD_FRAME = 0, 1, 2 against the float64 reference: with and without the loss term, dense and ragged with dead
    frames, a zero row (its gradient is ``g_hat / eps``: the value is checked), a row of norm 1e-9 under the clamp and a row
    scaled by 1e4."""
    x = _inputs(B, N, M, D, 500 + N + M)
    x["pf"][0, 0] = 0                                                   # zero row: c = eps, no correction term
    special_p, special_t = [(0, 0)], []
    if N > 2:
        x["pf"][0, 1] *= np.float32(1e-9 / np.linalg.norm(x["pf"][0, 1].astype(np.float64)))
        x["pf"][0, 2] *= np.float32(1e4)
        special_p += [(0, 1), (0, 2)]
    if M > 2:
        x["tf"][0, 1] *= np.float32(1e-9 / np.linalg.norm(x["tf"][0, 1].astype(np.float64)))
        x["tf"][0, 2] *= np.float32(1e4)
        special_t += [(0, 1), (0, 2)]
    for ragged in (False, True):
        nv = mv = None
        if ragged:
            nv, mv = ([N, max(1, N // 2), 0, N] * 3)[:B], ([M, M, M, 0] * 3)[:B]
        for loss in (False, True):
            tag = f"{B}x{N}x{M}x{D}/{'ragged' if ragged else 'dense'}_{'loss' if loss else 'noloss'}"
            out, (ref_t, ref_p) = _run_all(tag, x, 0.3, nv, mv, loss, special_p, special_t)
            if not loss:                                                # the zero row: g_hat / eps, g_hat = dcos^T @ tn
                tn64 = bwd_ref.normalize(torch.from_numpy(x["tf"][0]).double()).numpy()
                w_feat = float(np.float32(1.0 - 0.3))
                want = (x["dsim"][0, :, 0].astype(np.float64) * w_feat) @ tn64 / bwd_ref.EPS
                assert float(np.abs(ref_p[0, 0] - want).max()) <= 1e-12 * float(np.abs(want).max())
            if ragged:
                for mode, (gt_, gp_) in out.items():
                    for b in range(B):
                        dead = nv[b] == 0 or mv[b] == 0
                        assert not gp_[b, (0 if dead else nv[b]):].any() and not gt_[b, (0 if dead else mv[b]):].any(), (mode, b)


@pytest.mark.parametrize("w", [0.3, 0.0, 1.0])
def test_score_weight_ends(w):
    """``score_weight`` 0.3 / 0 / 1; at 1 and without the loss every feature gradient is exactly zero."""
    x = _inputs(3, 50, 10, 512, 77)
    for loss in (False, True):
        out, _ = _run_all(f"3x50x10x512/w{w}_{'loss' if loss else 'noloss'}", x, w, None, None, loss)
        if w == 1.0 and not loss:
            for gt_, gp_ in out.values():
                assert not gt_.any() and not gp_.any()


@pytest.mark.parametrize("B", [WAVE_MAX_B, WAVE_MAX_B + 1])
def test_by_batch_size_choice_on_both_sides_of_its_crossover(B):
    """Option -1 (the default) takes the wave-per-row form up to ``kFeatBwdWaveMaxB`` frames (read from dmm_cosine.hip) and
    the per-frame form past it: one batch on each side, against the same reference."""
    x = _inputs(B, 10, 3, 256, 9)
    _run_all(f"{B}x10x3x256/default", x, 0.3, None, None, True, modes=(-1,))
