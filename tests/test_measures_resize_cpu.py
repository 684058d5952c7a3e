"""Scoring a prediction at another size than the annotation's, without a GPU: the index rule (``measures.nearest_table``,
include/dmm_match.h (14b)) against PIL itself and against tests/measures_resize_ref.py's loop, the host forms of
``clip_counts(resize=True)``, ``db_eval_iou`` and ``db_eval_boundary`` against the fixture captured from the reference
(tests/golden/measures_resized.npz), ``dataset_results``, and the header's new entries against the built library."""
import ctypes
import os
import re

import numpy as np
import pytest

import measures_ref as R
import measures_resize_ref as RR
from conftest import ROOT, golden
from dmm_net_amd import _lib
from dmm_net_amd import measures as M

PRODUCT_PAIRS = [(255, 480), (448, 854), (480, 255), (854, 448)]
NEW_ENTRIES = ["dmm_nearest_index_tables_i32", "dmm_resize_labels_nearest_u8"]


def pil_table(n_in, n_out):
    """What PIL's NEAREST resize reads for each destination sample: the resize of an index ramp."""
    Image = pytest.importorskip("PIL.Image")
    ramp = np.arange(n_in, dtype=np.int32)[None, :]
    return np.array(Image.fromarray(ramp, "I").resize((n_out, 1), Image.NEAREST)).astype(np.int32)[0]


def test_nearest_table_equals_pil_on_every_small_pair_and_the_product_pairs():
    pytest.importorskip("PIL")
    pairs = [(i, o) for i in range(1, 65) for o in range(1, 201)] + PRODUCT_PAIRS
    for n_in, n_out in pairs:
        tab = M.nearest_table(n_in, n_out)
        assert tab.dtype == np.int32 and tab.shape == (n_out,)
        assert np.array_equal(tab, pil_table(n_in, n_out)), (n_in, n_out)
        assert tab.min() >= 0 and tab.max() < n_in, (n_in, n_out)             # no index leaves the source


def test_nearest_table_is_the_sequential_walk_and_not_the_closed_form():
    for n_in, n_out in [(i, o) for i in range(1, 40) for o in range(1, 90)] + PRODUCT_PAIRS:
        assert np.array_equal(M.nearest_table(n_in, n_out), RR.table_loop(n_in, n_out)), (n_in, n_out)
    for n_in, n_out in [(2, 7), (4, 6), (12, 23), (8, 6), (14, 5), (448, 854)]:
        assert not np.array_equal(M.nearest_table(n_in, n_out), RR.closed_form(n_in, n_out)), (n_in, n_out)
    assert M.nearest_table(5, 0).shape == (0,) and M.nearest_table(0, 3).tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        M.nearest_table(-1, 3)


@pytest.mark.parametrize("name", [str(c) for c in golden("measures_resized")["clips"]])
def test_host_forms_equal_the_reference_on_the_fixture(name):
    g = golden("measures_resized").group(name)
    pred, gt, n_obj, radius = g["pred"], g["gt"], int(g["n_obj"]), int(g["radius"])
    assert pred.shape[1:] != gt.shape[1:]
    resized = M.resize_labels_host(pred, gt.shape[1:])
    assert np.array_equal(resized, g["resized"]) and np.array_equal(RR.resize(pred, gt.shape[1:]), g["resized"])
    assert radius == M.boundary_radius(pred.shape)                              # taken BEFORE the resize
    got = M.clip_counts(pred, gt, n_obj, resize=True)                           # the radius from the prediction's size
    assert got.dtype == np.int32 and got.shape == (pred.shape[0], n_obj, 6)
    assert np.array_equal(got[:, :, 2:], g["sums"])
    assert np.array_equal(got, R.counts(g["resized"], gt, n_obj, radius))
    J, F = M.scores_from_counts(got)
    assert (J == g["J"]).all() and (F == g["F"]).all()
    for t in range(pred.shape[0]):
        for o in range(n_obj):
            an, sg = gt[t] == o + 1, pred[t] == o + 1
            assert M.db_eval_iou(an, sg, resize=True) == g["J"][o, t]
            assert M.db_eval_boundary(sg, an, resize=True) == g["F"][o, t]
    # a single frame pair [Hs,Ws] / [H,W] and host tensors take the same route
    assert np.array_equal(M.clip_counts(pred[0], gt[0], n_obj, resize=True), got[:1])
    import torch
    t_got = M.clip_counts(torch.from_numpy(pred), torch.from_numpy(gt), n_obj, resize=True)
    assert isinstance(t_got, torch.Tensor) and np.array_equal(t_got.numpy(), got)


def test_resize_at_equal_shapes_changes_nothing():
    rng = np.random.default_rng(3)
    pred, gt = RR.label_maps(rng, 2, 21, 34, 3), RR.label_maps(rng, 2, 21, 34, 3)
    for radius in (None, 0, 3):
        assert np.array_equal(M.clip_counts(pred, gt, 3, radius=radius, resize=True), M.clip_counts(pred, gt, 3, radius=radius))
    S, A = pred[0] == 1, gt[0] == 1
    assert M.db_eval_iou(A, S, resize=True) == M.db_eval_iou(A, S)
    assert M.db_eval_boundary(S, A, resize=True) == M.db_eval_boundary(S, A)


def test_the_radius_defaults_to_the_predictions():
    """f_boundary.py:30-31 reads foreground_mask.shape before the resize: 5 for 255 x 448 whatever the annotation's size."""
    assert M.boundary_radius((255, 448)) == 5 and M.boundary_radius((480, 854)) == 8
    rng = np.random.default_rng(5)
    pred, gt = RR.label_maps(rng, 1, 60, 100, 2), RR.label_maps(rng, 1, 140, 250, 2)
    r_pred, r_gt = M.boundary_radius(pred.shape), M.boundary_radius(gt.shape)
    assert (r_pred, r_gt) == (1, 3)
    resized = RR.resize(pred, gt.shape[1:])
    got = M.clip_counts(pred, gt, 2, resize=True)
    assert np.array_equal(got, R.counts(resized, gt, 2, r_pred))
    assert not np.array_equal(got, R.counts(resized, gt, 2, r_gt))
    assert np.array_equal(M.clip_counts(pred, gt, 2, radius=r_gt, resize=True), R.counts(resized, gt, 2, r_gt))


def test_mismatched_shapes_without_resize_still_raise():
    a, b = np.zeros((2, 8, 9), dtype=np.uint8), np.zeros((2, 8, 8), dtype=np.uint8)
    with pytest.raises(ValueError):
        M.clip_counts(a, b, 2)
    with pytest.raises(ValueError):
        M.clip_counts(a, b, 2, resize=False)
    with pytest.raises(ValueError):
        M.db_eval_iou(a[0], b[0])
    with pytest.raises(ValueError):
        M.db_eval_boundary(a[0], b[0])
    with pytest.raises(ValueError):                        # another number of frames is no resize
        M.clip_counts(a, b[:1], 2, resize=True)
    with pytest.raises(ValueError):
        M.clip_counts(a, b[0], 2, resize=True)


def test_dataset_results_is_the_mean_over_every_object_of_every_sequence():
    rng = np.random.default_rng(9)
    J = [rng.uniform(0, 1, size=(2, 9)), rng.uniform(0, 1, size=(3, 6))]      # two sequences: 2 and 3 objects
    F = [rng.uniform(0, 1, size=(2, 9)), rng.uniform(0, 1, size=(3, 6))]
    per_video = [{"J": j, "F": f, "J_seq": M.sequence_results(j), "F_seq": M.sequence_results(f)} for j, f in zip(J, F)]
    got = M.dataset_results(per_video)
    assert sorted(got) == ["F", "J"]
    s_eval = {"a": {"J": per_video[0]["J_seq"], "F": per_video[0]["F_seq"]},
              "b": {"J": per_video[1]["J_seq"], "F": per_video[1]["F_seq"]}}
    for measure in ("J", "F"):
        assert sorted(got[measure]) == ["decay", "mean", "recall"]
        for statistic in ("mean", "recall", "decay"):      # evaluation.py:104-108, written out
            raw_data = np.hstack([s_eval[sequence][measure][statistic] for sequence in s_eval.keys()])
            want = float(np.mean(raw_data))
            assert isinstance(got[measure][statistic], float) and got[measure][statistic] == want
    # five objects weigh the same: not the mean of the two sequences' means
    flat = float(np.mean([np.mean(v["J_seq"]["mean"]) for v in per_video]))
    assert got["J"]["mean"] != flat
    assert M.dataset_results({"a": per_video[0], "b": per_video[1]}) == got
    with pytest.raises(ValueError):
        M.dataset_results([])


def test_header_and_symbol_set_agree_on_the_new_entries():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmm_match.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\bDMM_API\s+[^;(]*?\b(dmm_[a-z0-9_]+)\s*\(", txt)))
    assert sorted(_lib.SYMBOLS) == declared
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in declared and hasattr(L, name), name
    B = _lib.load()
    assert len(B.dmm_nearest_index_tables_i32.argtypes) == 6 and B.dmm_nearest_index_tables_i32.argtypes[4] is ctypes.c_void_p
    assert len(B.dmm_resize_labels_nearest_u8.argtypes) == 11 and B.dmm_resize_labels_nearest_u8.argtypes[3] is ctypes.c_int64
    # the answers that need no device: bad arguments and "nothing to do" come before any launch
    OK, BAD, UNS = _lib.DMM_OK, _lib.DMM_ERR_BAD_ARG, _lib.DMM_ERR_UNSUPPORTED
    cap = int(re.search(r"^#define\s+DMM_NEAREST_MAX_AXIS\s+(\d+)", open(os.path.join(ROOT, "include", "dmm_match.h")).read(),
                        re.M).group(1))
    p = ctypes.c_void_p(256)
    n0 = B.dmm_launch_count()
    assert B.dmm_nearest_index_tables_i32(-1, 2, 3, 4, p, None) == BAD
    assert B.dmm_nearest_index_tables_i32(1, 2, 0, 0, None, None) == OK
    assert B.dmm_nearest_index_tables_i32(1, 2, 3, 4, None, None) == BAD
    for k in range(4):
        sizes = [4, 4, 4, 4]
        sizes[k] = cap + 1
        assert B.dmm_nearest_index_tables_i32(*sizes, p, None) == UNS
    assert B.dmm_resize_labels_nearest_u8(p, 2, 2, 4, p, 4, 4, 15, p, 1, None) == BAD
    assert B.dmm_resize_labels_nearest_u8(None, 2, 2, 4, None, 4, 0, 0, None, 1, None) == OK
    q = ctypes.c_void_p(512)
    assert B.dmm_resize_labels_nearest_u8(p, 2, 2, 4, p, 4, 4, 16, p, 1, None) == BAD                      # in place
    # (14d) answer 4, clause by clause, with pointers that are never followed: nothing is launched
    big = 46341                                            # 46341^2 = 2^31 + 4633
    max_wg = int(re.search(r"^#define\s+DMM_RESIZE_MAX_WORKGROUPS\s+(\d+)", open(os.path.join(ROOT, "include", "dmm_match.h")).read(),
                           re.M).group(1))
    assert big * big >= 2 ** 31 > (big - 1) ** 2 and max_wg * 256 == 2 ** 32
    assert B.dmm_resize_labels_nearest_u8(p, 2, 2, 4, q, big, big, big * big, p, 1, None) == UNS
    assert B.dmm_resize_labels_nearest_u8(p, big, big, big * big, q, 4, 4, 16, p, 1, None) == UNS
    assert B.dmm_resize_labels_nearest_u8(p, 2, 2, 4, q, 4, 4, 16, p, max_wg, None) == UNS                # one workgroup per frame
    assert B.dmm_resize_labels_nearest_u8(p, 2, 2, 4, q, 40, 40, 1600, p, max_wg // 2, None) == UNS       # two per frame
    assert B.dmm_resize_labels_nearest_u8(p, 2, 2, 4, q, 4, 4, 16, p, 2 ** 31 - 1, None) == UNS
    assert B.dmm_resize_labels_nearest_u8(p, 2, 2, 4, q, big, big, big * big - 1, p, 1, None) == BAD     # the stride comes first
    assert B.dmm_resize_labels_nearest_u8(p, 2, 2, 3, q, 4, 4, 16, p, max_wg, None) == BAD
    assert B.dmm_resize_labels_nearest_u8(p, 2, 2, 4, q, 4, 4, 16, None, max_wg, None) == BAD              # and the null pointer
    assert B.dmm_launch_count() == n0
