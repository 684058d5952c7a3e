"""Scoring a prediction at another size than the annotation's on the GPU (csrc/dmm_measures.hip, include/dmm_match.h
(14b), (14d), then (14): the route that ships; the fused (14c) was measured slower, profiles/r13_davis_resized.md): the index
tables against ``measures.nearest_table``, the counts against tests/measures_ref.py on the numpy-resized prediction
(tests/measures_resize_ref.py: the rule as a plain loop) and against the fixture captured from the reference
(tests/golden/measures_resized.npz), the resize alone against the numpy gather and PIL's map.  Every output is an integer:
np.array_equal everywhere, no tolerance."""
import os
import re

import numpy as np
import pytest
import torch

import measures_ref as R
import measures_resize_ref as RR
from conftest import golden
from dmm_net_amd import _lib, video
from dmm_net_amd import measures as M
from dmm_net_amd.graphs import SafeGraph
from guarded import banded, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL_PAIRS = [((2, 2), (7, 7)), ((1, 1), (3, 5)), ((3, 5), (1, 1)), ((4, 4), (6, 6)), ((12, 12), (23, 23)),
               ((16, 20), (12, 15)), ((24, 40), (45, 76)), ((14, 8), (5, 6))]


def band_rows(radius):
    """DMM_DAVIS_BAND_ROWS of include/dmm_match.h: the rows of one workgroup's band."""
    return min(64, max(16, 3 * radius + 8))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check(pred, gt, n_obj, radius, what=""):
    """clip_counts(resize=True) inside guarded(), the prediction banded with a live label: a load outside the source shows
    in the counts, a store outside ``counts`` or the tables in the bands."""
    with guarded() as g:
        dp = banded(dev(pred), poison=1)
        got = M.clip_counts(dp, dev(gt), n_obj, radius=radius, resize=True)
        torch.cuda.synchronize()
        assert g.check() == [], (what, pred.shape, gt.shape)
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == (pred.shape[0], n_obj, 6)
    r = M.boundary_radius(pred.shape) if radius is None else radius
    want = R.counts(RR.resize(pred, gt.shape[1:]), gt, n_obj, r)
    got = got.cpu().numpy()
    assert np.array_equal(got, want), (what, pred.shape, gt.shape, n_obj, r, np.argwhere(got != want)[:8].tolist())
    return got


def raw_tables(Hs, Ws, H, W, tables):
    return _lib.load().dmm_nearest_index_tables_i32(Hs, Ws, H, W, None if tables is None else tables.data_ptr(),
                                                    torch.cuda.current_stream().cuda_stream)


def raw_resize(src, Hs, Ws, fs_src, dst, H, W, fs_dst, tables, T):
    ptr = lambda x: None if x is None else x.data_ptr()
    return _lib.load().dmm_resize_labels_nearest_u8(ptr(src), Hs, Ws, fs_src, ptr(dst), H, W, fs_dst, ptr(tables), T,
                                                    torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("src,dst", SMALL_PAIRS)
def test_small_pairs_tables_counts_and_resize(src, dst):
    (Hs, Ws), (H, W) = src, dst
    rng = np.random.default_rng(Hs * 1000 + W)
    with guarded() as g:
        tables = M.nearest_tables(src, dst, DEV)
        torch.cuda.synchronize()
        assert g.check() == []
    want = np.concatenate([M.nearest_table(Hs, H), M.nearest_table(Ws, W)])
    assert tables.dtype == torch.int32 and np.array_equal(tables.cpu().numpy(), want)
    assert np.array_equal(want, np.concatenate([RR.table_loop(Hs, H), RR.table_loop(Ws, W)]))
    pred, gt = RR.label_maps(rng, 2, Hs, Ws, 3), RR.label_maps(rng, 2, H, W, 3)
    for radius in (0, 1, 3):
        check(pred, gt, 3, radius, "small pair")
    with guarded() as g:
        out = video.resize_labels(banded(dev(pred), poison=1), dst)
        torch.cuda.synchronize()
        assert g.check() == []
    assert out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), RR.gather(pred, want[:H], want[H:]))
    assert np.array_equal(video.resize_labels(pred, dst), out.cpu().numpy())          # the host form


@pytest.mark.parametrize("name", [str(c) for c in golden("measures_resized")["clips"]])
def test_fixture_clips_equal_the_reference(name):
    g = golden("measures_resized").group(name)
    pred, gt, n_obj, radius = g["pred"], g["gt"], int(g["n_obj"]), int(g["radius"])
    got = M.clip_counts(dev(pred), dev(gt), n_obj, resize=True).cpu().numpy()          # the radius from the prediction's size
    assert np.array_equal(got[:, :, 2:], g["sums"])
    assert np.array_equal(got, R.counts(g["resized"], gt, n_obj, radius))
    J, F = M.scores_from_counts(got)
    assert (J == g["J"]).all() and (F == g["F"]).all()
    assert np.array_equal(video.resize_labels(dev(pred), gt.shape[1:]).cpu().numpy(), g["resized"])   # PIL's map


@pytest.mark.parametrize("W", [63, 64, 65, 129])
def test_destination_widths_around_the_word(W):
    rng = np.random.default_rng(W)
    for Ws in (31, 64, 100):
        check(RR.label_maps(rng, 1, 9, Ws, 2), RR.label_maps(rng, 1, 17, W, 2), 2, 2, "widths")


@pytest.mark.parametrize("radius", [0, 1, 5, 8])
def test_destination_heights_around_the_band(radius):
    rng = np.random.default_rng(40 + radius)
    bh = band_rows(radius)
    for H in (bh - 1, bh, bh + 1):
        Hs = max(1, int(0.53 * H))
        check(RR.label_maps(rng, 1, Hs, 37, 2), RR.label_maps(rng, 1, H, 70, 2), 2, radius, "heights")


def device_tables_equal_the_rule(src, dst):
    """(14b) for one size pair against ``nearest_table`` and the plain loop: the walk itself, not what counts make of it."""
    (Hs, Ws), (H, W) = src, dst
    got = M.nearest_tables(src, dst, DEV).cpu().numpy()
    assert np.array_equal(got, np.concatenate([M.nearest_table(Hs, H), M.nearest_table(Ws, W)])), (src, dst)
    assert np.array_equal(got, np.concatenate([RR.table_loop(Hs, H), RR.table_loop(Ws, W)])), (src, dst)
    return got


def test_column_tiles():
    rng = np.random.default_rng(4096)
    device_tables_equal_the_rule((20, 2000), (40, 4096))
    gt = RR.label_maps(rng, 1, 40, 4096, 3)
    check(RR.label_maps(rng, 1, 20, 2000, 3), gt, 3, 8, "column tiles")


def test_product_sizes_with_the_default_radius():
    rng = np.random.default_rng(255)
    pred = np.kron(RR.label_maps(rng, 2, 37, 64, 3), np.ones((7, 7), dtype=np.uint8))[:, :255, :448]
    gt = RR.resize(np.roll(pred, (3, -4), axis=(1, 2)), (480, 854))
    gt[:, :50] = np.kron(RR.label_maps(rng, 2, 10, 171, 3), np.ones((5, 5), dtype=np.uint8))[:, :50, :854]
    assert M.boundary_radius(pred.shape) == 5 and M.boundary_radius(gt.shape) == 8
    tables = device_tables_equal_the_rule((255, 448), (480, 854))
    assert not np.array_equal(tables[480:], RR.closed_form(448, 854))        # the pair on which the closed form is wrong
    device_tables_equal_the_rule((480, 854), (255, 448))
    check(pred, gt, 3, None, "product")


def test_identity_tables_equal_the_equal_size_entry_bit_for_bit():
    rng = np.random.default_rng(21)
    T, H, W, n_obj, radius = 3, 45, 131, 3, 5
    pred, gt = dev(RR.label_maps(rng, T, H, W, n_obj)), dev(RR.label_maps(rng, T, H, W, n_obj))
    tables = M.nearest_tables((H, W), (H, W), DEV)
    assert tables.cpu().tolist() == list(range(H)) + list(range(W))
    plain = M.clip_counts(pred, gt, n_obj, radius=radius)
    assert torch.equal(M.clip_counts(pred, gt, n_obj, radius=radius, resize=True), plain)
    copy = video.resize_labels(pred, (H, W), tables=tables)                  # (14d) through identity tables, then (14)
    assert copy.data_ptr() != pred.data_ptr() and torch.equal(copy, pred)
    assert torch.equal(M.clip_counts(copy, gt, n_obj, radius=radius), plain)


def test_strided_frames_and_out_of_range_table_entries():
    rng = np.random.default_rng(23)
    T, (Hs, Ws), (H, W), n_obj, radius = 3, (14, 23), (33, 70), 3, 2
    pred, gt = RR.label_maps(rng, T, Hs, Ws, n_obj), RR.label_maps(rng, T, H, W, n_obj)
    pad_p, pad_g = 13, 1000
    bp = torch.full((T, Hs * Ws + pad_p), 1, dtype=torch.uint8, device=DEV)       # the gaps hold a live label
    bg = torch.full((T, H * W + pad_g), 1, dtype=torch.uint8, device=DEV)
    bp[:, :Hs * Ws], bg[:, :H * W] = dev(pred).view(T, -1), dev(gt).view(T, -1)
    vp, vg = bp[:, :Hs * Ws].view(T, Hs, Ws), bg[:, :H * W].view(T, H, W)
    assert vp.stride(0) == Hs * Ws + pad_p and vg.stride(0) == H * W + pad_g
    want = R.counts(RR.resize(pred, (H, W)), gt, n_obj, radius)
    assert np.array_equal(M.clip_counts(vp, vg, n_obj, radius=radius, resize=True).cpu().numpy(), want)
    # the resize alone: strided source, and a strided destination whose frames start at odd addresses
    tables = M.nearest_tables((Hs, Ws), (H, W), DEV)
    assert np.array_equal(video.resize_labels(vp, (H, W), tables=tables).cpu().numpy(), RR.resize(pred, (H, W)))
    fs_dst = H * W + 7
    with guarded() as g:
        whole = torch.full((1 + T * fs_dst,), 9, dtype=torch.uint8, device=DEV)
        assert raw_resize(bp, Hs, Ws, Hs * Ws + pad_p, whole[1:], H, W, fs_dst, tables, T) == _lib.DMM_OK
        torch.cuda.synchronize()
        assert g.check() == []
    host = whole.cpu().numpy()
    frames = host[1:].reshape(T, fs_dst)
    assert host[0] == 9 and (frames[:, H * W:] == 9).all()
    assert np.array_equal(frames[:, :H * W].reshape(T, H, W), RR.resize(pred, (H, W)))
    # table entries outside the source (written here) read as label 0, and (14) counts what (14d) wrote
    t = tables.cpu().numpy().copy()
    t[[0, 5, H - 1]] = [-1, Hs, 1 << 30]
    t[[H + 1, H + 40, H + W - 1]] = [Ws, -7, -(1 << 31)]
    bad = dev(t)
    resized = RR.gather(pred, t[:H], t[H:])
    assert not resized[:, 0].any() and not resized[:, :, 1].any()
    with guarded() as g:
        dp = banded(dev(pred), poison=1)
        out = torch.empty((T, H, W), dtype=torch.uint8, device=DEV)
        assert raw_resize(dp, Hs, Ws, dp.stride(0), out, H, W, H * W, bad, T) == _lib.DMM_OK
        c = M.clip_counts(out, dev(gt), n_obj, radius=radius)
        torch.cuda.synchronize()
        assert g.check() == []
    assert np.array_equal(out.cpu().numpy(), resized)
    assert np.array_equal(c.cpu().numpy(), R.counts(resized, gt, n_obj, radius))


def test_clip_scorer_with_pred_size_equals_one_clip_counts_call():
    rng = np.random.default_rng(27)
    B, T, (Hs, Ws), (H, W), n_obj = 2, 3, (60, 100), (140, 250), 3
    gt = RR.label_maps(rng, B * T, H, W, n_obj).reshape(B, T, H, W)
    pred = RR.label_maps(rng, B * T, Hs, Ws, n_obj).reshape(B, T, Hs, Ws)
    scorer = M.ClipScorer(dev(gt), n_obj, pred_size=(Hs, Ws))
    assert scorer.radius == M.boundary_radius((Hs, Ws)) == 1 and M.boundary_radius((H, W)) == 3
    dp = dev(pred)
    L = _lib.load()
    n0 = L.dmm_launch_count()
    for t in range(T):
        for b in range(B):
            scorer(b, t, dp[b, t])
    assert L.dmm_launch_count() - n0 == 3 * B * T          # resize, clear, counts: the tables were built in the constructor
    whole = M.clip_counts(dp.view(B * T, Hs, Ws), dev(gt).view(B * T, H, W), n_obj, resize=True).view(B, T, n_obj, 6)
    assert torch.equal(scorer.counts, whole)
    assert np.array_equal(whole.cpu().numpy().reshape(B * T, n_obj, 6),
                          R.counts(RR.resize(pred.reshape(-1, Hs, Ws), (H, W)), gt.reshape(-1, H, W), n_obj, 1))
    assert len(scorer.results()) == B
    assert M.ClipScorer(dev(gt), n_obj, pred_size=(Hs, Ws), radius=3).radius == 3
    with pytest.raises(ValueError):
        scorer(0, 0, dev(gt)[0, 0])                        # the annotation's size is not this scorer's
    with pytest.raises(ValueError):
        M.ClipScorer(dev(gt), n_obj)(0, 0, dp[0, 0])       # without pred_size the sizes must agree, as before


def test_statuses_one_by_one():
    L = _lib.load()
    OK, BAD, UNS = _lib.DMM_OK, _lib.DMM_ERR_BAD_ARG, _lib.DMM_ERR_UNSUPPORTED
    T, (Hs, Ws), (H, W) = 2, (5, 6), (8, 9)
    hws, hw = Hs * Ws, H * W
    p = torch.zeros((T, Hs, Ws), dtype=torch.uint8, device=DEV)
    a = torch.zeros((T, H, W), dtype=torch.uint8, device=DEV)
    tab = torch.full((H + W + 4,), -9, dtype=torch.int32, device=DEV)
    cap = int(re.search(r"^#define\s+DMM_NEAREST_MAX_AXIS\s+(\d+)", open(os.path.normpath(_lib.HEADER)).read(), re.M).group(1))
    # (14b)
    n0 = L.dmm_launch_count()
    for bad in [(-1, Ws, H, W), (Hs, -1, H, W), (Hs, Ws, -1, W), (Hs, Ws, H, -1)]:
        assert raw_tables(*bad, tab) == BAD, bad
    assert raw_tables(-1, Ws, H, W, None) == BAD
    assert raw_tables(Hs, Ws, 0, 0, None) == OK
    assert raw_tables(Hs, Ws, H, W, None) == BAD
    for k in range(4):
        sizes = [Hs, Ws, H, W]
        sizes[k] = cap + 1
        assert raw_tables(*sizes, tab) == UNS
    assert raw_tables(cap + 1, Ws, H, W, None) == BAD      # the earlier answer is named
    assert L.dmm_launch_count() == n0
    assert raw_tables(Hs, Ws, H, W, tab) == OK
    assert L.dmm_launch_count() - n0 == 1
    torch.cuda.synchronize()
    host = tab.cpu().numpy()
    assert np.array_equal(host[:H + W], np.concatenate([M.nearest_table(Hs, H), M.nearest_table(Ws, W)])) and (host[H + W:] == -9).all()
    # (14d)
    d = torch.full((T, H, W), 7, dtype=torch.uint8, device=DEV)

    def resize(src=p, dst=d, tables=tab, **kw):
        k = dict(Hs=Hs, Ws=Ws, fs_src=hws, H=H, W=W, fs_dst=hw, T=T)
        k.update(kw)
        return raw_resize(src, k["Hs"], k["Ws"], k["fs_src"], dst, k["H"], k["W"], k["fs_dst"], tables, k["T"])

    n0 = L.dmm_launch_count()
    for bad in [dict(T=-1), dict(Hs=-1), dict(Ws=-1), dict(H=-1), dict(W=-1), dict(fs_src=hws - 1), dict(fs_dst=hw - 1)]:
        assert resize(**bad) == BAD, bad
    assert resize(src=None, dst=None, tables=None, T=0) == OK
    assert resize(src=None, dst=None, tables=None, H=0, fs_dst=0) == OK and resize(src=None, dst=None, tables=None, W=0, fs_dst=0) == OK
    assert resize(src=None) == BAD and resize(dst=None) == BAD and resize(tables=None) == BAD
    assert resize(src=d, Hs=H, Ws=W, fs_src=hw) == BAD     # in place
    # answer 4, clause by clause (nothing is launched, so the pointers are never followed): H * W >= 2^31, Hs * Ws >= 2^31,
    # the workgroup cap at a small frame (one workgroup per frame here) and at 2^31 - 1 frames
    big = 46341                                            # 46341^2 = 2^31 + 4633
    header = open(os.path.normpath(_lib.HEADER)).read()
    max_wg = int(re.search(r"^#define\s+DMM_RESIZE_MAX_WORKGROUPS\s+(\d+)", header, re.M).group(1))
    assert big * big >= 2 ** 31 > (big - 1) ** 2 and max_wg * 256 == 2 ** 32
    assert resize(H=big, W=big, fs_dst=big * big) == UNS
    assert resize(Hs=big, Ws=big, fs_src=big * big) == UNS
    assert resize(T=max_wg) == UNS and resize(T=2 ** 31 - 1) == UNS
    assert resize(H=40, W=40, fs_dst=1600, T=max_wg // 2) == UNS            # two workgroups per frame
    assert resize(H=big, W=big, fs_dst=big * big - 1) == BAD and resize(T=max_wg, fs_src=hws - 1) == BAD   # the earlier answer
    assert resize(T=max_wg, tables=None) == BAD
    assert L.dmm_launch_count() == n0
    torch.cuda.synchronize()
    assert int((d != 7).sum()) == 0
    assert resize() == OK
    assert L.dmm_launch_count() - n0 == 1
    torch.cuda.synchronize()
    assert not d.any()
    # the wrappers: a radius past the limit is the library's answer, differing sizes without resize= are a ValueError
    with pytest.raises(_lib.DmmError):
        M.clip_counts(p, a, 3, radius=64, resize=True)
    with pytest.raises(ValueError):
        M.clip_counts(p, a, 3)


def test_one_capture_replays_the_entries_on_new_inputs():
    rng = np.random.default_rng(29)
    T, (Hs, Ws), (H, W), n_obj, radius = 2, (37, 70), (70, 130), 2, 5
    preds = [RR.label_maps(rng, T, Hs, Ws, n_obj) for _ in range(2)]
    gts = [RR.label_maps(rng, T, H, W, n_obj) for _ in range(2)]
    pred, gt = dev(preds[0]), dev(gts[0])
    M.clip_counts(pred, gt, n_obj, radius=radius, resize=True)          # (loads the library outside the capture)
    g = SafeGraph()
    with g.capture():
        tables = M.nearest_tables((Hs, Ws), (H, W), DEV)
        resized = video.resize_labels(pred, (H, W), tables=tables)
        counts = M.clip_counts(pred, gt, n_obj, radius=radius, resize=True)
    want_t = np.concatenate([M.nearest_table(Hs, H), M.nearest_table(Ws, W)])
    for k in range(2):
        pred.copy_(dev(preds[k]))
        gt.copy_(dev(gts[k]))
        for out in (tables, counts, resized):
            out.fill_(3)
        g.replay()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(tables.cpu().numpy(), want_t)
        assert np.array_equal(resized.cpu().numpy(), RR.resize(preds[k], (H, W)))
        assert np.array_equal(counts.cpu().numpy(), R.counts(RR.resize(preds[k], (H, W)), gts[k], n_obj, radius))
    assert g.left == 0
