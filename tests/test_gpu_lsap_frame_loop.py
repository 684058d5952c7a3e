"""FrameLoop with algo 'hun': the fixed-slot frame step (dmm_match_solve_packed_hun inside the captured step) against the
BoxList path on the scipy route."""
import numpy as np
import pytest
import torch

from dmm_net_amd import autograd, video
from dmm_net_amd.dmm_model import DMM_Model
from dmm_net_amd.roi_features import FeatureExtractor
from test_gpu_video import _PoolEncoder, _raw_proposals

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cfg(algo):
    return {"matching": {"algo": algo}, "relax_max_iter": 12, "relax_proj_iter": 3, "relax_learning_rate": 0.1,
            "score_weight": 0.3}


def _clip(seed):
    rng = np.random.default_rng(seed)
    B, T, O, H, W = 3, 4, 4, 64, 96
    frames = torch.randn(B, T, 3, H, W, device=DEV)
    n_frames = [4, 3, 4]
    props = [[_raw_proposals(rng, 24 + 3 * b, H, W) for t in range(n_frames[b])] for b in range(B)]
    first = torch.zeros(B, O, H, W, device=DEV)
    first[0, 0, 5:30, 8:40] = 1.0
    first[0, 1, 30:60, 50:90] = 1.0
    first[0, 3, 2:20, 60:90] = 1.0                       # slot 2 empty: the live templates are not a prefix
    first[2, 0, 10:50, 20:60] = 1.0
    first[2, 1, 40:62, 0:30] = 1.0                        # video 1: no object, skipped
    return frames, first.view(B, O, H * W), props, n_frames


def _loop(algo, slots, graph=False):
    lp = video.FrameLoop(_PoolEncoder(), DMM_Model(_cfg(algo), is_test=1, feature_extractor=FeatureExtractor()),
                         nms_thresh=0.4, max_proposals=10)
    lp.slots, lp.graph = slots, graph
    return lp


def _run(lp, clip):
    frames, first, props, n_frames = clip
    labels = {}
    hist = lp.run(frames, first, props, n_frames, on_labels=lambda b, t, lab: labels.__setitem__((b, t), lab.clone()))
    torch.cuda.synchronize()
    return [h.clone() for h in hist], labels


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and sorted(a[1]) == sorted(b[1]) and \
        all(torch.equal(a[1][k], b[1][k]) for k in a[1])


def test_frame_loop_hun_fixed_slot_step_equals_boxlist_scipy_route():
    clip = _clip(3)
    frames, first, props, _ = clip
    assert _loop("hun", True)._slots_ok(frames, props, first.shape[1])
    old = autograd._DEVICE_LSAP
    autograd._DEVICE_LSAP = False
    try:
        ref = _run(_loop("hun", False), clip)                # the reference's steps, scipy on the host
    finally:
        autograd._DEVICE_LSAP = old
    for graph in (False, True):
        lp = _loop("hun", True, graph)
        got = _run(lp, clip)
        assert lp._plan is not None and lp._plan.cfg[5] == "hun"
        assert _same(got, ref), graph
    rel = _run(_loop("relax", True, True), clip)
    assert not _same(rel, ref)                                # the one-hot assignment really is another result


def test_frame_loop_rebuilds_a_relax_plan_for_hun():
    clip = _clip(4)
    lp = _loop("relax", True, True)
    _run(lp, clip)
    plan = lp._plan
    lp.dmm.match_algo = lp.dmm.match_layer.match_algo = "hun"
    got = _run(lp, clip)
    assert lp._plan is not plan and lp._plan.cfg[5] == "hun"
    assert _same(got, _run(_loop("hun", False), clip))
