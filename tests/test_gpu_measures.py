"""The DAVIS counts on the GPU (csrc/dmm_measures.hip, include/dmm_match.h (14)) against tests/measures_ref.py and the fixture
captured from the reference (tests/golden/measures.npz).  Every output is an integer: np.array_equal everywhere, no tolerance.

The yardstick dilates with the full disk footprint, which costs (pixels x footprint) on the host: radius 63 is held on small
frames only (at most 1500 pixels), the product frames at the reference's own radius for their size."""
import numpy as np
import pytest
import torch

import measures_ref as R
from conftest import golden
from dmm_net_amd import _lib
from dmm_net_amd import measures as M
from dmm_net_amd.graphs import SafeGraph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RADII = [0, 1, 2, 3, 5, 8, 13, 63]
WIDTHS = [1, 2, 63, 64, 65, 127, 128, 129, 257]


def band_rows(radius):
    """DMM_DAVIS_BAND_ROWS of include/dmm_match.h: the rows of one workgroup's band."""
    return min(64, max(16, 3 * radius + 8))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def label_maps(rng, T, H, W, n_labels):
    """Seeded label maps [T,H,W] of random blocks (1, 3 or 7 pixels wide): objects lie against every edge and corner, labels
    0 .. n_labels."""
    out = np.zeros((T, H, W), dtype=np.uint8)
    for t in range(T):
        bs = int(rng.choice([1, 3, 7]))
        coarse = rng.integers(0, n_labels + 1, size=(-(-H // bs), -(-W // bs)))
        coarse[rng.random(coarse.shape) < 0.4] = 0
        out[t] = np.kron(coarse, np.ones((bs, bs), dtype=np.int64))[:H, :W]
    return out


def check(pred, gt, n_obj, radius, what=""):
    got = M.clip_counts(dev(pred), dev(gt), n_obj, radius=radius)
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == (pred.shape[0], n_obj, 6)
    want = R.counts(pred, gt, n_obj, radius)
    got = got.cpu().numpy()
    assert np.array_equal(got, want), (what, pred.shape, n_obj, radius, np.argwhere(got != want)[:8].tolist())
    return got


@pytest.mark.parametrize("radius", RADII)
def test_edge_shapes_against_the_yardstick(radius):
    """W around the 64-pixel word and its multiples, H of 1 to 3 rows and one row below, at and above the band height; the
    radius is larger than H, than W, or than both in many of them."""
    rng = np.random.default_rng(100 + radius)
    bh = band_rows(radius)
    cap = 1500 if radius > 13 else 1 << 30                 # the yardstick's cost at radius 63
    shapes = [(H, W) for H in (1, 2, 3, bh - 1, bh, bh + 1) for W in WIDTHS if H * W <= cap]
    assert len(shapes) >= 30
    for H, W in shapes:
        check(label_maps(rng, 1, H, W, 2), label_maps(rng, 1, H, W, 2), 2, radius, "edge shape")


@pytest.mark.parametrize("name", [str(c) for c in golden("measures")["clips"]])
def test_fixture_clips_equal_the_reference(name):
    g = golden("measures").group(name)
    pred, gt, n_obj, radius = g["pred"], g["gt"], int(g["n_obj"]), int(g["radius"])
    got = M.clip_counts(dev(pred), dev(gt), n_obj).cpu().numpy()          # the radius from the frame size
    assert np.array_equal(got[:, :, 2:], g["sums"])
    assert np.array_equal(got, R.counts(pred, gt, n_obj, radius))
    J, F = M.scores_from_counts(got)
    assert (J == g["J"]).all() and (F == g["F"]).all()


@pytest.mark.parametrize("H,W,radius", [(255, 448, None), (480, 854, None), (48, 1000, 13), (2, 600, 63), (40, 4096, 8)])
def test_product_frames_and_column_tiles(H, W, radius):
    """The two product sizes at the reference's radius (5 and 8), and frames wider than one workgroup's column tile."""
    rng = np.random.default_rng(H + W)
    r = M.boundary_radius((H, W)) if radius is None else radius
    gt = label_maps(rng, 1, H, W, 3)
    pred = np.roll(gt, (2, -3), axis=(1, 2))
    pred[0, : H // 3] = label_maps(rng, 1, H, W, 3)[0, : H // 3]
    check(pred, gt, 3, r, "product / tiles")


@pytest.mark.parametrize("radius", [0, 2, 8])
def test_objects_on_the_edges_and_special_masks(radius):
    H, W = 37, 131
    boxes = {"top": (0, 9, 40, 90), "bottom": (28, 37, 40, 90), "left": (10, 30, 0, 11), "right": (10, 30, 120, 131),
             "tl": (0, 8, 0, 8), "tr": (0, 8, 123, 131), "bl": (29, 37, 0, 8), "br": (29, 37, 123, 131), "pixel_br": (36, 37, 130, 131)}
    gts, preds = [], []
    for y0, y1, x0, x1 in boxes.values():
        a = np.zeros((H, W), dtype=np.uint8)
        a[y0:y1, x0:x1] = 1
        gts.append(a)
        preds.append(np.roll(a, (1, -1), axis=(0, 1)))              # wraps round the image: lies on the opposite edge too
    empty, full = np.zeros((H, W), dtype=np.uint8), np.ones((H, W), dtype=np.uint8)
    some = gts[0]
    for p, a in [(empty, some), (some, empty), (empty, empty), (full, some), (some, full), (full, full), (full, empty)]:
        preds.append(p)
        gts.append(a)
    got = check(np.stack(preds), np.stack(gts), 1, radius, "edges")
    k = len(boxes)
    assert got[k, 0].tolist()[:3] == [0, int(some.sum()), 0] and not got[k + 2].any()
    assert got[k + 5, 0].tolist() == [H * W, H * W, 0, 0, 0, 0]          # a full mask has no boundary at all


def test_absent_labels_and_labels_above_n_obj():
    rng = np.random.default_rng(7)
    H, W = 50, 97
    gt, pred = label_maps(rng, 2, H, W, 6), label_maps(rng, 2, H, W, 6)
    gt[gt == 2] = 0                                        # object 1 (label 2) is in neither map of any frame
    pred[pred == 2] = 0
    pred[0][pred[0] == 3] = 0                              # label 3 only in the annotation of frame 0
    pred[1, :5, :5] = 255
    got = check(pred, gt, 4, 3, "labels")                  # labels 5, 6 and 255 belong to no object
    assert not got[:, 1].any() and got[0, 2, 0] == 0 and got[0, 2, 3] > 0


@pytest.mark.parametrize("n_obj,T", [(1, 1), (3, 5), (255, 1), (255, 5), (1, 5)])
def test_object_and_frame_counts(n_obj, T):
    rng = np.random.default_rng(n_obj * 10 + T)
    H, W = (12, 70) if n_obj == 255 else (40, 70)
    check(label_maps(rng, T, H, W, min(n_obj + 1, 255)), label_maps(rng, T, H, W, min(n_obj + 1, 255)), n_obj, 2, "n_obj / T")


def raw_call(pred, gt, T, n_obj, H, W, fs_pred, fs_gt, radius, counts, ws=None, ws_bytes=0):
    ptr = lambda x: None if x is None else x.data_ptr()
    return _lib.load().dmm_davis_counts_u8(ptr(pred), ptr(gt), T, n_obj, H, W, fs_pred, fs_gt, radius, ptr(counts), ptr(ws),
                                           ws_bytes, torch.cuda.current_stream().cuda_stream)


def test_strided_frames_guard_words_and_repeats():
    rng = np.random.default_rng(11)
    T, H, W, n_obj, radius = 5, 33, 70, 3, 5
    pred, gt = label_maps(rng, T, H, W, n_obj), label_maps(rng, T, H, W, n_obj)
    want = R.counts(pred, gt, n_obj, radius)
    pad_p, pad_g = 13, 1000
    bp = torch.full((T, H * W + pad_p), 1, dtype=torch.uint8, device=DEV)    # the gaps hold a live label
    bg = torch.full((T, H * W + pad_g), 1, dtype=torch.uint8, device=DEV)
    bp[:, :H * W], bg[:, :H * W] = dev(pred).view(T, -1), dev(gt).view(T, -1)
    vp, vg = bp[:, :H * W].view(T, H, W), bg[:, :H * W].view(T, H, W)
    assert vp.stride(0) == H * W + pad_p and not vp.is_contiguous()
    assert np.array_equal(M.clip_counts(vp, vg, n_obj, radius=radius).cpu().numpy(), want)
    # the entry itself, into the middle of a guarded buffer, three times: the same bytes, the guards untouched
    n, guard = T * n_obj * 6, 64
    runs = []
    for rep in range(3):
        buf = torch.full((guard + n + guard,), -12345 - rep, dtype=torch.int32, device=DEV)
        rc = raw_call(bp, bg, T, n_obj, H, W, H * W + pad_p, H * W + pad_g, radius, buf[guard:])
        assert rc == _lib.DMM_OK
        host = buf.cpu().numpy()
        assert (host[:guard] == -12345 - rep).all() and (host[guard + n:] == -12345 - rep).all()
        runs.append(host[guard:guard + n].tobytes())
    assert runs[0] == runs[1] == runs[2] == want.tobytes()


def test_one_capture_replays_on_new_inputs():
    rng = np.random.default_rng(13)
    T, H, W, n_obj, radius = 2, 70, 130, 2, 8
    a = [label_maps(rng, T, H, W, n_obj) for _ in range(4)]
    pred, gt = dev(a[0]), dev(a[1])
    M.clip_counts(pred, gt, n_obj, radius=radius)          # (loads the library outside the capture)
    g = SafeGraph()
    with g.capture():
        out = M.clip_counts(pred, gt, n_obj, radius=radius)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), R.counts(a[0], a[1], n_obj, radius))
    pred.copy_(dev(a[2]))
    gt.copy_(dev(a[3]))
    out.fill_(-7)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), R.counts(a[2], a[3], n_obj, radius))
    assert g.left == 0


def test_statuses():
    L = _lib.load()
    T, H, W = 2, 8, 9
    p = torch.zeros((T, H, W), dtype=torch.uint8, device=DEV)
    c = torch.full((T, 256, 6), 5, dtype=torch.int32, device=DEV)
    hw = H * W
    OK, BAD, UNS = _lib.DMM_OK, _lib.DMM_ERR_BAD_ARG, _lib.DMM_ERR_UNSUPPORTED
    assert L.dmm_davis_counts_workspace_bytes(T, 3, H, W, 8) >= 0
    assert raw_call(p, p, T, 3, H, W, hw, hw, 64, c) == UNS
    assert raw_call(p, p, T, 256, H, W, hw, hw, 3, c) == UNS
    assert raw_call(p, p, T, 255, H, W, hw, hw, 63, c) == OK
    for bad in [dict(T=-1), dict(n_obj=-1), dict(H=-1), dict(W=-1), dict(radius=-1), dict(fs_pred=hw - 1), dict(fs_gt=hw - 1)]:
        a = dict(T=T, n_obj=3, H=H, W=W, fs_pred=hw, fs_gt=hw, radius=2)
        a.update(bad)
        assert raw_call(p, p, a["T"], a["n_obj"], a["H"], a["W"], a["fs_pred"], a["fs_gt"], a["radius"], c) == BAD, bad
    assert raw_call(None, p, T, 3, H, W, hw, hw, 2, c) == BAD
    assert raw_call(p, None, T, 3, H, W, hw, hw, 2, c) == BAD
    assert raw_call(p, p, T, 3, H, W, hw, hw, 2, None) == BAD
    assert raw_call(p, p, T, 3, H, W, hw - 1, hw, 64, c) == BAD           # the earlier answer is named
    # nothing to do: DMM_OK, nothing launched, pointers not looked at
    c.fill_(5)
    n0 = L.dmm_launch_count()
    assert raw_call(None, None, 0, 3, H, W, hw, hw, 2, None) == OK
    assert raw_call(None, None, T, 0, H, W, hw, hw, 2, None) == OK
    assert L.dmm_launch_count() == n0
    torch.cuda.synchronize()
    assert int((c != 5).sum()) == 0
    # an image without pixels: every count is 0
    assert raw_call(p, p, T, 3, 0, W, 0, 0, 2, c) == OK
    torch.cuda.synchronize()
    assert not c.view(-1)[:T * 3 * 6].any() and int((c.view(-1)[T * 3 * 6:] != 5).sum()) == 0
    with pytest.raises(_lib.DmmError):
        M.clip_counts(p, p, 3, radius=64)
    with pytest.raises(ValueError):
        M.clip_counts(p, p[:, :, :8], 3)


def test_clip_scorer_equals_one_clip_counts_call():
    rng = np.random.default_rng(17)
    B, T, H, W, n_obj = 2, 4, 45, 100, 3
    gt = label_maps(rng, B * T, H, W, n_obj).reshape(B, T, H, W)
    pred = label_maps(rng, B * T, H, W, n_obj).reshape(B, T, H, W)
    scorer = M.ClipScorer(dev(gt), n_obj)
    assert scorer.radius == M.boundary_radius((H, W)) == 1
    dp = dev(pred)
    for t in range(T):
        for b in range(B):
            scorer(b, t, dp[b, t])
    whole = M.clip_counts(dp.view(B * T, H, W), dev(gt).view(B * T, H, W), n_obj).view(B, T, n_obj, 6)
    assert torch.equal(scorer.counts, whole)
    assert np.array_equal(whole.cpu().numpy().reshape(B * T, n_obj, 6), R.counts(pred.reshape(-1, H, W), gt.reshape(-1, H, W), n_obj, 1))
    res = scorer.results()
    assert len(res) == B
    for b in range(B):
        J, F = M.scores_from_counts(whole[b])
        assert np.array_equal(res[b]["J"], J) and np.array_equal(res[b]["F"], F)
        assert res[b]["J_seq"]["mean"] == M.sequence_results(J)["mean"] and len(res[b]["F_seq"]["raw"][0]) == T


def _frame_loop_inputs(rng, B, T, O, H, W, n_obj):
    """Frames, first-frame masks and raw proposals the way tests/test_gpu_video.py builds them."""
    from dmm_net_amd import proposals as prop
    frames = torch.randn(B, T, 3, H, W, device=DEV)
    first = torch.zeros(B, O, H, W, device=DEV)
    for b in range(B):
        for o in range(n_obj[b]):
            y0, x0 = int(rng.integers(0, H - 30)), int(rng.integers(0, W - 30))
            first[b, o, y0:y0 + 25, x0:x0 + 28] = 1.0

    def raw_proposals(n):
        x1, y1 = rng.uniform(0, W - 24, n), rng.uniform(0, H - 24, n)
        boxes = np.stack([x1, y1, np.minimum(x1 + rng.uniform(10, 60, n), W - 1), np.minimum(y1 + rng.uniform(10, 50, n), H - 1)], 1)
        bl = prop.SimpleBoxList(torch.from_numpy(boxes.astype(np.float32)), (W, H))
        bl.add_field("scores", torch.from_numpy(rng.random(n).astype(np.float32)))
        bl.add_field("mask", torch.from_numpy((rng.random((n, 1, 28, 28)) * 0.6 + 0.4).astype(np.float32)))
        return bl

    props = [[raw_proposals(30 + 5 * b + t) for t in range(T)] for b in range(B)]
    return frames, first.view(B, O, H * W), props


class _PoolEncoder:
    """Batch-independent toy encoder (pooling only): 4 levels, C channels, strides 4..32."""

    def __init__(self, C=8):
        self.mul = torch.linspace(0.5, 1.5, C, device=DEV).view(1, C, 1, 1)

    def __call__(self, x):
        import torch.nn.functional as F
        g = x.mean(1, keepdim=True)
        lv = tuple(F.avg_pool2d(g, s, ceil_mode=True) * self.mul for s in (4, 8, 16, 32))
        return {"backbone_feature": lv, "refine_input_feat": lv}


def test_frame_loop_scores_its_labels_as_it_goes():
    from dmm_net_amd import video
    from dmm_net_amd.dmm_model import DMM_Model
    from dmm_net_amd.roi_features import FeatureExtractor
    rng = np.random.default_rng(19)
    B, T, O, H, W = 2, 3, 5, 96, 128
    n_obj = [2, 4]
    frames, first, props = _frame_loop_inputs(rng, B, T, O, H, W, n_obj)
    cfgs = {"matching": {"algo": "relax"}, "relax_max_iter": 40, "relax_proj_iter": 5, "relax_learning_rate": 0.1,
            "score_weight": 0.3}
    gt = dev(label_maps(rng, B * T, H, W, 4).reshape(B, T, H, W))
    scorer = M.ClipScorer(gt, 4)
    kept = {}

    def on_labels(b, t, labels):
        scorer(b, t, labels)
        kept[(b, t)] = labels.clone()

    loop = video.FrameLoop(_PoolEncoder(), DMM_Model(cfgs, is_test=1, feature_extractor=FeatureExtractor()), nms_thresh=0.4,
                           max_proposals=20)
    loop.run(frames, first, props, [T] * B, on_labels=on_labels)
    assert sorted(kept) == [(b, t) for b in range(B) for t in range(T)]
    labels = torch.stack([torch.stack([kept[(b, t)] for t in range(T)]) for b in range(B)])
    assert int(labels.max()) >= 1                          # the loop did label something
    whole = M.clip_counts(labels.view(B * T, H, W), gt.view(B * T, H, W), 4).view(B, T, 4, 6)
    assert torch.equal(scorer.counts, whole)
    assert np.array_equal(whole.cpu().numpy().reshape(B * T, 4, 6),
                          R.counts(labels.cpu().numpy().reshape(-1, H, W), gt.cpu().numpy().reshape(-1, H, W), 4, scorer.radius))
    assert len(scorer.results()) == B
