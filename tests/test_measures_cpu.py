"""The DAVIS scores without a GPU: tests/measures_ref.py and the package's host path (dmm_net_amd/measures.py) against the
fixture captured from the reference's jaccard.py / f_boundary.py / statistics.py (tests/golden/measures.npz,
gen_golden_measures.py).  Counts are integers and compared with array_equal; J, F and the statistics are float64 and compared
with ==: the package divides the same integers the same way."""
import numpy as np
import pytest
import torch

import measures_ref as R
from conftest import golden
from dmm_net_amd import measures as M

G = golden("measures")
CLIPS = [str(c) for c in G["clips"]]


def clip(name):
    g = G.group(name)
    pred, gt = g["pred"], g["gt"]
    T, H, W = pred.shape
    n_obj = int(g["n_obj"])
    bm = np.unpackbits(g["bmaps"])[:T * n_obj * 2 * H * W].reshape(T, n_obj, 2, H, W).astype(bool)
    return pred, gt, n_obj, int(g["radius"]), g, bm


def fixture_counts(name):
    """The fixture's sums in the entry's slot order (its S & A and S | A come from the label maps themselves)."""
    pred, gt, n_obj, _, g, _ = clip(name)
    out = np.zeros((pred.shape[0], n_obj, 6), dtype=np.int32)
    for o in range(n_obj):
        S, A = pred == o + 1, gt == o + 1
        out[:, o, 0], out[:, o, 1] = (S & A).sum((1, 2)), (S | A).sum((1, 2))
    out[:, :, 2:] = g["sums"]
    return out


@pytest.mark.parametrize("name", CLIPS)
def test_the_yardstick_equals_the_fixture(name):
    pred, gt, n_obj, radius, g, bm = clip(name)
    for t in range(pred.shape[0]):
        for o in range(n_obj):
            assert np.array_equal(R.bmap(pred[t] == o + 1), bm[t, o, 0]), (name, t, o)
            assert np.array_equal(R.bmap(gt[t] == o + 1), bm[t, o, 1]), (name, t, o)
    assert np.array_equal(R.counts(pred, gt, n_obj, radius), fixture_counts(name))


@pytest.mark.parametrize("name", CLIPS)
def test_the_host_path_equals_the_fixture(name):
    pred, gt, n_obj, radius, g, bm = clip(name)
    counts = M.clip_counts(pred, gt, n_obj)                          # the radius from the frame size, as the reference
    assert counts.dtype == np.int32 and counts.shape == (pred.shape[0], n_obj, 6)
    assert M.boundary_radius(pred.shape) == radius
    assert np.array_equal(counts, fixture_counts(name))
    assert np.array_equal(M.clip_counts(pred, gt, n_obj, radius=radius), counts)
    J, F = M.scores_from_counts(counts)
    assert J.dtype == np.float64 and F.dtype == np.float64
    assert (J == g["J"]).all() and (F == g["F"]).all(), (J - g["J"], F - g["F"])
    for t in range(pred.shape[0]):
        for o in range(n_obj):
            assert np.array_equal(M.seg2bmap(pred[t] == o + 1), bm[t, o, 0])
    if "J_mean" in g:
        res = M.sequence_results(J)
        for stat in ("mean", "recall", "decay"):
            assert (np.array(res[stat]) == g["J_" + stat]).all(), stat


def test_tensors_and_single_frames_take_the_host_path():
    pred, gt, n_obj, radius, g, _ = clip("c96x128")
    want = fixture_counts("c96x128")
    got = M.clip_counts(torch.from_numpy(pred), torch.from_numpy(gt), n_obj)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.int32 and np.array_equal(got.numpy(), want)
    one = M.clip_counts(pred[1], gt[1], n_obj)
    assert one.shape == (1, n_obj, 6) and np.array_equal(one[0], want[1])


def test_statistics_equal_the_reference_on_every_length():
    for L in range(4, 41):
        s = G.group(f"stats/{L}")
        X = list(s["X"])
        assert float(M.mean(X)) == float(s["mean"]) and float(M.recall(X)) == float(s["recall"]), L
        assert float(M.decay(X)) == float(s["decay"]), L
    assert M.std([1.0, 3.0]) == 1.0


def test_radius_follows_the_reference_expression():
    for name in ("c75x100", "c300x400"):                              # the product lands on or next to an integer
        pred, _, _, radius, _, _ = clip(name)
        assert M.boundary_radius(pred.shape) == radius == int(np.ceil(0.008 * np.linalg.norm(pred.shape[1:])))
    assert M.boundary_radius((480, 854)) == 8 and M.boundary_radius((480, 854), bound_th=3) == 3
    assert M.boundary_radius((480, 854), bound_th=1) == 1 and M.boundary_radius((7, 480, 854), 2.0) == 2


def test_a_fractional_bound_th_above_one_is_refused():
    m = np.zeros((8, 8), dtype=np.uint8)
    with pytest.raises(ValueError):
        M.clip_counts(m, m, 1, bound_th=2.5)
    with pytest.raises(ValueError):
        M.db_eval_boundary(m, m, bound_th=1.5)
    with pytest.raises(ValueError):
        M.clip_counts(m, m, 1, radius=2.5)


def test_mismatched_shapes_are_refused():
    a, b = np.zeros((2, 8, 8), dtype=np.uint8), np.zeros((2, 8, 9), dtype=np.uint8)
    with pytest.raises(ValueError):
        M.clip_counts(a, b, 1)
    with pytest.raises(ValueError):
        M.db_eval_iou(a[0], b[0])
    with pytest.raises(ValueError):
        M.db_eval_boundary(a[0], b[0])
    with pytest.raises(ValueError):
        M.clip_counts(a.astype(np.int64), a, 1)


def test_the_drop_in_names_keep_the_reference_argument_orders():
    pred, gt, n_obj, radius, g, _ = clip("c130x257")
    for o in range(n_obj):
        an, sg = gt[0] == o + 1, pred[0] == o + 1
        assert M.db_eval_iou(an, sg) == g["J"][o, 0]
        assert M.db_eval_boundary(sg, an) == g["F"][o, 0]
    # A pair with asymmetric precision and recall.  J and F are both symmetric in their two masks (F = 2 p r / (p + r)), so a
    # swapped call shows in the counts behind them, not in the score: the prediction's whole rim lies on the annotation's,
    # most of the annotation's rim has no prediction near it -> precision (slot 4 / slot 2) is high, recall (5 / 3) low.
    an = np.zeros((40, 60), dtype=bool)
    an[5:35, 5:55] = True
    sg = np.zeros_like(an)
    sg[5:12, 5:12] = True
    c = M.clip_counts(sg.astype(np.uint8), an.astype(np.uint8), 1, radius=1)[0, 0]
    n_fg, n_gt, fg_match, gt_match = (int(v) for v in c[2:])
    precision, recall = fg_match / n_fg, gt_match / n_gt
    assert precision > 2 * recall > 0, (precision, recall)           # most of sg's rim is on an's rim, not the reverse
    assert np.array_equal(c, R.counts(sg[None].astype(np.uint8), an[None].astype(np.uint8), 1, 1)[0, 0])
    assert np.array_equal(M.clip_counts(an.astype(np.uint8), sg.astype(np.uint8), 1, radius=1)[0, 0, [2, 3, 4, 5]],
                          c[[3, 2, 5, 4]])                           # swapping the maps swaps the slots
    assert M.db_eval_boundary(sg, an, bound_th=1) == 2 * precision * recall / (precision + recall)
    # the empty / non-empty cases of both
    empty = np.zeros_like(an)
    assert M.db_eval_iou(empty, empty) == 1 and M.db_eval_iou(an, empty) == 0
    assert M.db_eval_boundary(empty, an) == 0 and M.db_eval_boundary(an, empty) == 0 and M.db_eval_boundary(empty, empty) == 1


def test_scores_follow_the_case_analysis():
    c = np.array([[[0, 0, 0, 0, 0, 0]], [[0, 5, 0, 7, 0, 0]], [[0, 5, 7, 0, 0, 0]], [[2, 5, 4, 4, 0, 0]], [[2, 6, 4, 8, 3, 2]]],
                 dtype=np.int32)
    J, F = M.scores_from_counts(c)
    assert J.shape == (1, 5) and J.tolist() == [[1.0, 0.0, 0.0, np.int64(2) / np.float32(5), np.int64(2) / np.float32(6)]]
    p, r = 3 / 4.0, 2 / 8.0
    assert F.tolist() == [[1.0, 0.0, 0.0, 0.0, 2 * p * r / (p + r)]]
    assert M.scores_from_counts(torch.from_numpy(c))[1].tolist() == F.tolist()


def test_sequence_results_pads_and_trims_like_the_reference():
    raw = np.array([[0.9, 0.8, 0.6, 0.4, 0.2, 0.7, 0.1], [1.0, 0.5, 0.5, 0.5, 0.5, 0.5, 0.0]])
    res = M.sequence_results(raw)
    assert sorted(res) == ["decay", "mean", "raw", "recall", "std"]
    for o in range(2):
        assert len(res["raw"][o]) == 7 and np.isnan(res["raw"][o][0]) and np.isnan(res["raw"][o][-1])
        assert res["raw"][o][1:-1] == raw[o, 1:-1].tolist()
        assert all(type(v) is float for v in res["raw"][o])
    scored = raw[:, 1:-1]                                             # frames 1 .. T-2
    assert res["mean"] == [float(np.nanmean(s)) for s in scored]
    assert res["recall"] == [0.6, 0.0]                                # strictly above 0.5
    assert res["std"] == [float(np.std(s)) for s in scored]
    # decay over 5 scored frames: bins [0:2], .., [3:5] -> first quarter minus last quarter
    assert res["decay"] == [float(np.mean(s[0:2]) - np.mean(s[3:5])) for s in scored]


def test_decay_has_no_8_bit_index():
    X = list(np.linspace(1.0, 0.0, 400))
    assert M.decay(X) == np.mean(X[0:101]) - np.mean(X[299:400])
