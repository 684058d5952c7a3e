"""The clip augmentation without a GPU: tests/augment_ref.py (the arithmetic of include/dmm_match.h (15) in numpy fp32) against
the fixture captured from the reference's own transforms (tests/golden/augment.npz), and the host-side helpers of
dmm_net_amd/augment.py.

The reference forms its source coordinates with a bmm whose last bit may differ from (15)'s order, so the comparison leaves
out the near-tie pixels (``augment_ref.near_tie``: a clamped coordinate, in float64, within 1e-3 of a half-integer; at most
1.5 % of a fixture frame of 1000 pixels or more, asserted when the fixture is made).  On those the value must still be the
source at one of the two neighbouring rows and columns, for the restatement and the reference alike."""
import random

import numpy as np
import pytest
import torch

import augment_ref as R
from conftest import golden
from dmm_net_amd import augment as A

CLIPS = [str(c) for c in golden("augment")["clips"]]


def clip(name):
    g = golden("augment").group(name)
    g["flip"], g["F"], g["seed"], g["drawn"] = bool(g["flip"]), int(g["F"]), int(g["seed"]), int(g["drawn"])
    return g


def restated(g):
    n = g["labels"].shape[0]
    return R.augment_clip(g["frames"], g["labels"], g["masks"], g["boxes_in"], g["matrices"], [g["flip"]] * n, g["F"])


def candidates(plane, m, flip, H, W):
    """[4,H,W]: the plane at the two neighbouring rows x the two neighbouring columns of every pixel's source."""
    r_lo, r_hi, c_lo, c_hi = R.neighbours(m, flip, H, W)
    return np.stack([plane[r_lo, c_lo], plane[r_lo, c_hi], plane[r_hi, c_lo], plane[r_hi, c_hi]])


def test_fixture_is_what_the_issue_asks_for():
    shapes = {tuple(golden("augment")[c + "/labels"].shape[1:]) for c in CLIPS}
    assert shapes == {(37, 53), (1, 1), (1, 9), (9, 1), (16, 64)}
    assert {golden("augment")[c + "/masks"].shape[1] for c in CLIPS} == {0, 1, 6}
    assert {int(golden("augment")[c + "/F"]) for c in CLIPS} == {1, 5}
    assert {bool(golden("augment")[c + "/flip"]) for c in CLIPS} == {False, True}
    for c in CLIPS:
        g = clip(c)
        n, H, W = g["labels"].shape
        for f in range(n):
            ties = int(R.near_tie(g["matrices"][f], H, W).sum())
            assert ties == int(g["near_tie"][f])
            assert H * W < 1000 or ties <= 0.015 * H * W
        assert (g["out_box_valid"] == 0).any() or g["masks"].shape[1] == 0


@pytest.mark.parametrize("name", CLIPS)
def test_warp_equals_the_reference_outside_near_ties(name):
    g = clip(name)
    got = restated(g)
    n, H, W = g["labels"].shape
    for f in range(n):
        tie = R.near_tie(g["matrices"][f], H, W)
        for key in ("frames", "labels", "masks"):
            mine, ref, src = got[key][f], g["out_" + key][f], g[key][f]
            assert mine.dtype == ref.dtype and mine.shape == ref.shape
            assert np.array_equal(mine[..., ~tie], ref[..., ~tie]), (name, f, key)
            for pl_m, pl_r, pl_s in zip(mine.reshape(-1, H, W), ref.reshape(-1, H, W), src.reshape(-1, H, W)):
                cand = candidates(pl_s, g["matrices"][f], g["flip"], H, W)
                assert ((cand == pl_m[None]).any(axis=0))[tie].all(), (name, f, key)
                assert ((cand == pl_r[None]).any(axis=0))[tie].all(), (name, f, key)


@pytest.mark.parametrize("name", CLIPS)
def test_boxes_targets_and_sizes(name):
    g = clip(name)
    got = restated(g)
    n, H, W = g["labels"].shape
    P, F = g["masks"].shape[1], g["F"]
    ref_rows = np.unpackbits(g["out_rows"])[: n * F * (H * W + 1)].reshape(n, F, H * W + 1).astype(np.float64)
    mine_rows = R.reference_rows(got["targets"], got["sizes"])
    exact = 0
    for f in range(n):
        tie = R.near_tie(g["matrices"][f], H, W)
        # a near-tie pixel lies on an edge when its candidate sources disagree about (mask > 0.5) or about the label
        lab_c = candidates(g["labels"][f], g["matrices"][f], g["flip"], H, W)
        lab_edge = tie & (lab_c != lab_c[0]).any(axis=0)
        if not lab_edge.any():
            assert np.array_equal(mine_rows[f], ref_rows[f]), (name, f)
            exact += 1
        else:                                              # the planes differ on those pixels only; the flag unless one decides it
            diff = (mine_rows[f, :, :-1] != ref_rows[f, :, :-1]).reshape(F, H, W)
            assert not (diff & ~lab_edge[None]).any(), (name, f)
            assert (np.abs(got["sizes"][f] - ref_rows[f, :, :-1].sum(axis=1)) <= lab_edge.sum()).all()
        assert np.array_equal(got["sizes"][f], got["targets"][f].reshape(F, -1).sum(axis=1))
        for p in range(P):
            m_c = candidates(g["masks"][f, p], g["matrices"][f], g["flip"], H, W) > 0.5
            m_edge = tie & (m_c != m_c[0]).any(axis=0)
            if not m_edge.any():
                assert got["box_valid"][f, p] == g["out_box_valid"][f, p], (name, f, p)
                assert np.array_equal(got["boxes"][f, p], g["out_boxes"][f, p]), (name, f, p)
                exact += 1
            elif got["box_valid"][f, p] and g["out_box_valid"][f, p]:
                assert np.abs(got["boxes"][f, p] - g["out_boxes"][f, p]).max() <= 1, (name, f, p)
            if not got["box_valid"][f, p]:
                assert np.array_equal(got["boxes"][f, p], g["boxes_in"][f, p])
    assert exact >= 3                                      # the special frames have no near-tie pixel: the exact branch runs


def test_targets_ignore_255_and_labels_above_F():
    lab = np.array([[0, 1, 2, 255], [6, 5, 1, 0]], dtype=np.uint8)
    planes, sizes = R.targets(lab, 5)
    assert sizes.tolist() == [2, 1, 0, 0, 1] and planes.sum() == 4 and planes[0, 0, 1] == 1 and planes[4, 1, 1] == 1


@pytest.mark.parametrize("name", CLIPS)
def test_affine_matrix_is_bit_equal_to_the_reference_chain(name):
    g = clip(name)
    n, H, W = g["labels"].shape
    for f in range(n):
        deg, dh, dw, sh, zx, zy = (float(v) for v in g["params"][f])
        m = A.affine_matrix(deg, (dh, dw), sh, (zx, zy), H, W)
        assert m.dtype == torch.float32 and tuple(m.shape) == (3, 3) and not m.is_cuda
        assert m.numpy().tobytes() == g["matrices"][f].tobytes(), (name, f)
        # the numpy chain of the restatement: each product entry is three fp32 products summed in order; a BLAS may fuse
        # or reorder them, which moves an entry by at most 2 ulp of the largest term
        mine = R.matrix_chain(deg, (dh, dw), sh, (zx, zy), H, W)
        tol = 2 * np.finfo(np.float32).eps * max(1.0, float(np.abs(g["matrices"][f]).max()))
        assert np.abs(mine.astype(np.float64) - g["matrices"][f]).max() <= tol, (name, f)


class CountingRandom(random.Random):
    def __init__(self, seed):
        super().__init__(seed)
        self.calls = []

    def random(self):
        v = super().random()
        if not getattr(self, "_inside", False):
            self.calls.append(("random",))
        return v

    def uniform(self, a, b):
        self._inside = True
        try:
            v = super().uniform(a, b)
        finally:
            self._inside = False
        self.calls.append(("uniform", a, b))
        return v


@pytest.mark.parametrize("T", [0, 1, 4])
def test_draw_clip_params_draws_in_the_reference_order(T):
    rng = CountingRandom(5)
    flip, mats = A.draw_clip_params(rng, T, H=37, W=53)
    assert isinstance(flip, bool) and tuple(mats.shape) == (T, 3, 3) and mats.dtype == torch.float32
    per_frame = [("uniform", -10, 10), ("uniform", -0.1, 0.1), ("uniform", -0.1, 0.1), ("uniform", -0.1, 0.1),
                 ("uniform", 0.7, 1.4), ("uniform", 0.7, 1.4)]
    assert len(rng.calls) == 1 + 6 * T and rng.calls == [("random",)] + per_frame * T
    # the same stream consumed by hand gives the same matrices
    chk = random.Random(5)
    assert flip == (chk.random() < 0.5)
    for t in range(T):
        d = [chk.uniform(*c[1:]) for c in per_frame]
        assert torch.equal(mats[t], A.affine_matrix(d[0], (d[1], d[2]), d[3], (d[4], d[5]), 37, 53))
    nxt = chk.random()
    assert rng.random() == nxt                             # and not one draw more


@pytest.mark.parametrize("name", CLIPS)
def test_draw_clip_params_equals_the_reference_draws(name):
    """The fixture's drawn frames came from the reference's RandomAffine under ``random.seed(seed)`` after the clip's flip."""
    g = clip(name)
    H, W = g["labels"].shape[1:]
    flip, mats = A.draw_clip_params(random.Random(g["seed"]), g["drawn"], H=H, W=W)
    assert flip == g["flip"]
    assert mats.numpy().tobytes() == g["matrices"][: g["drawn"]].tobytes()


def test_host_tensors_are_refused_and_the_package_exports_lazily():
    import dmm_net_amd
    from dmm_net_amd import _lib
    assert dmm_net_amd.augment_clip is A.augment_clip and dmm_net_amd.affine_matrix is A.affine_matrix
    assert dmm_net_amd.draw_clip_params is A.draw_clip_params and dmm_net_amd.AugmentedClip is A.AugmentedClip
    with pytest.raises(_lib.DmmError):
        A.augment_clip(torch.zeros(1, 3, 4, 5), torch.zeros(1, 4, 5, dtype=torch.uint8), matrices=torch.eye(3)[None], flip=False)
