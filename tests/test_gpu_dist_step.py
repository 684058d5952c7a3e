"""Two gloo ranks of the ``TrainEncoder`` training step on one device against the one-process eager reference of
``dist_step.py``, bit for bit: graph replays with three plans in flight, the weight-gradient graphs on the side stream, the
one-segment-late hand-over into ``GradBucketer(overlap=True)``, Adam.  Every two-rank run is a child process group of its
own under a time limit; the runs start one after the other, and after one that aborted, faulted or hit its limit nothing
more starts.  At most three processes hold the GPU: this one (the reference) and the two ranks."""
import gc
import math
import shutil

import pytest
import torch

import dist_step as ds

pytestmark = pytest.mark.gpu

# ResNet-34 with 32-channel heads, bf16, a clip of 3 frames of 2 x 3 x 96 x 128 per step (three plans in flight, one
# backward), 4 steps; 87 MB of fp32 gradients in 25 MB buckets: four buckets.
GPU_CFG = ds.config(dtype="bfloat16", device="cuda:0", shape=(2, 3, 96, 128), frames=3, steps=4, bucket_mb=25.0, overlap=True,
                    graphs=True, overlap_wgrad=True, deterministic=True, threads=0)
ENV = {"HSA_ENABLE_IPC_MODE_LEGACY": "0"}       # (as the other two-rank tests on one device)

# Time limits of the children: three times the wall time measured on an MI355X, rounded up (LABLOG.md, "two-rank training
# step"; measured: replay 33 s, one_stream 17 s, keep_grads 42 s, own_all 25 - 37 s, wide_heads 25 s, asym 35 s, cfg4 27 s,
# default_mode 26 s -- most of it process start, the capture of three plans per rank and 170 MB of files per step and rank).
LIMIT_S = {"replay": 100, "one_stream": 60, "keep_grads": 130, "own_all": 110, "wide_heads": 80, "asym": 105, "cfg4": 80,
           "default_mode": 80}

_STOP = []               # why nothing more may start (a child aborted, faulted or hit its limit)


def _record(name, v):
    try:
        from conftest import record_achieved
        record_achieved(name, v)
    except Exception:
        pass


@pytest.fixture(autouse=True)
def _release():
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("dist_step_gpu")
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(scope="module")
def ref(workdir):
    """The eager reference of the symmetric step under ``set_deterministic_conv("library")``: computed once, shared by the
    cases that only change how the ranks replay, overlap or clear (none of which the reference has)."""
    return ds.reference(GPU_CFG, str(workdir / "ref"))


def _run(cfg, workdir, name):
    if _STOP:
        pytest.fail(f"not started: {_STOP[0]}")
    try:
        got, wall = ds.run_ranks(cfg, str(workdir / name), LIMIT_S[name], ENV)
    except ds.ChildFailed as e:
        if e.abnormal:
            _STOP.append(f"the two-rank run '{name}' ended abnormally")
        raise
    metas = [got.meta(r) for r in range(ds.WORLD)]
    n_p, n_b, n_s = ds.counts(got)
    for k, v in (("wall_s", wall), ("buckets", metas[0]["buckets"]), ("parameters", n_p), ("buffers", n_b), ("steps", n_s)):
        _record(f"dist_step_gpu/{name}/{k}", v)
    print(f"dist_step_gpu/{name}: wall {wall:.1f} s, in-rank {[round(m['wall_s'], 1) for m in metas]} s, "
          f"buckets {metas[0]['buckets']}, {n_p} parameters, {n_b} buffers, {n_s} steps")
    assert metas[0]["buckets"] == metas[1]["buckets"] >= 3, metas
    assert n_s == cfg["steps"] and n_p > 100 and n_b > 100
    if cfg["graphs"]:
        assert [m["plans"] for m in metas] == [cfg["frames"]] * 2, metas       # one captured plan per frame in flight
    return got, metas


def _assert_equal(got, ref):
    diff = ds.compare(got, ref)
    assert not diff, {k: (len(v), v[:4]) for k, v in diff.items()}
    assert ds.between_ranks(got, "params") == [[]] * got.steps
    assert ds.between_ranks(got, "grads") == [[]] * got.steps
    assert all(len(names) > 0 for names in ds.between_ranks(got, "buffers"))


# ---- a. the encoder's step in the deterministic mode -----------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", [("replay", {}), ("one_stream", {"overlap_wgrad": False}),
                                     ("keep_grads", {"set_to_none": False})])
def test_two_ranks_of_graph_replays_equal_the_eager_reference(workdir, ref, name, kw):
    """Gradients after ``finish()``, parameters and buffers after ``opt.step()``: bit-equal to the reference on both ranks
    after every one of 4 steps.  ``one_stream``: weight gradients inline, no late hand-over; ``keep_grads``:
    ``zero_grad(set_to_none=False)``, the hand-over accumulates into the bucket views."""
    got, _ = _run(ds.config(GPU_CFG, **kw), workdir, name)
    _assert_equal(got, ref)
    g = got[got.steps - 1][0]["grads"]
    assert sorted(n for n, t in g.items() if t is None) == ["base.fc.bias", "base.fc.weight"]
    shutil.rmtree(workdir / name, ignore_errors=True)


@pytest.mark.parametrize("name,kw", [("own_all", {"det_conv": "own_all"}),
                                     ("wide_heads", {"det_conv": "own", "hidden": 128, "steps": 2})])
def test_two_ranks_equal_the_reference_on_the_own_convolutions(workdir, name, kw):
    """The same with the project's MFMA convolutions on both sides.  ``own_all``: the 3x3 convolutions of the body and the
    32-channel heads of levels 4 and 5 (``dmm_conv3x3_narrow_bf16``).  ``wide_heads``: ``hidden_size=128``, where the heads of
    levels 3 to 5 are wide enough for the routed 3x3 convolution, under ``"own"``.  In both the heads' captured graphs take
    bf16 weight copies from ``_prep_3x3``: a replay must see the optimiser's update of the masters (a plan whose head graphs
    read the copies of the day of the capture equals the reference in step 0 and not in step 1)."""
    cfg = ds.config(GPU_CFG, **kw)
    got, _ = _run(cfg, workdir, name)
    _assert_equal(got, ds.reference(cfg, str(workdir / (name + "_ref"))))
    for d in (name, name + "_ref"):
        shutil.rmtree(workdir / d, ignore_errors=True)


# ---- b. one rank leaves heads out of its loss for a step --------------------------------------------------------------------
def test_a_rank_that_leaves_heads_out_for_one_step(workdir):
    """Rank 1 leaves ``refine_input_feat`` out of its loss in step 1.  Its replayed backward then delivers ZERO gradients for
    the skip heads where the eager reference has ``None`` ("Outputs left out of the loss"); rank 0 still
    produces them, so the mean counts rank 1's share as zeros either way: the same bits, the same ``None`` pattern, no hang."""
    cfg = ds.config(GPU_CFG, skip_refine=(1, 1), steps=3)
    got, _ = _run(cfg, workdir, "asym")
    _assert_equal(got, ds.reference(cfg, str(workdir / "asym_ref")))
    for d in ("asym", "asym_ref"):
        shutil.rmtree(workdir / d, ignore_errors=True)


# ---- c. a config-4 style step through DMM_Model ------------------------------------------------------------------------------
_CFG4_RANK = r"""
import os, sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
torch.backends.cudnn.benchmark = False
torch.backends.cudnn.deterministic = True          # the reference's train.py:46: the mode follows it
import dmm_net_amd
assert dmm_net_amd.is_deterministic()
import test_gpu_deterministic as t
rank = int(os.environ["RANK"])
losses, chk, params = t._cfg4_run(steps=int(sys.argv[4]), data_seed=int(sys.argv[5 + rank]), backend="gloo", world=2)
torch.save({"losses": losses, "chk": chk, "params": [p.cpu() for p in params]}, os.path.join(sys.argv[3], f"r{rank}.pt"))
"""
CFG4_STEPS, CFG4_SEEDS = 3, (4, 14)


def test_config4_style_step_of_two_ranks_equals_one_process(workdir):
    """``test_gpu_deterministic._cfg4_run`` (ResNet-50 ``TrainEncoder`` -> ROI features -> ``DMM_Model`` -> losses,
    ``GradBucketer(overlap=True)``, Adam; 2 videos x clip 2 at 128 x 224, 3 steps) as two gloo ranks with their own data
    against the same step run once per rank's data in this process with the mean taken by hand: losses of every step, the
    parameters and the checksum over parameters and buffers after the last, bit-equal on both ranks."""
    import os
    import test_gpu_deterministic as t
    if _STOP:
        pytest.fail(f"not started: {_STOP[0]}")
    out = workdir / "cfg4"
    out.mkdir()
    (out / "cfg4_rank.py").write_text(_CFG4_RANK)
    try:
        wall = ds.launch([str(out / "cfg4_rank.py"), ds.ROOT, os.path.join(ds.ROOT, "tests"), str(out), str(CFG4_STEPS)]
                         + [str(s) for s in CFG4_SEEDS], str(out), LIMIT_S["cfg4"], ENV)
    except ds.ChildFailed as e:
        if e.abnormal:
            _STOP.append("the two-rank run 'cfg4' ended abnormally")
        raise
    _record("dist_step_gpu/cfg4/wall_s", wall)
    print(f"dist_step_gpu/cfg4: wall {wall:.1f} s")
    got = [torch.load(out / f"r{r}.pt", map_location="cpu") for r in range(ds.WORLD)]
    with ds.mode(ds.config(GPU_CFG)):
        ref = t._cfg4_reference(CFG4_STEPS, CFG4_SEEDS)
    _record("dist_step_gpu/cfg4/parameters", len(got[0]["params"]))
    _record("dist_step_gpu/cfg4/steps", CFG4_STEPS)
    for r, (g, (losses, chk, params)) in enumerate(zip(got, ref)):
        assert len(g["losses"]) == CFG4_STEPS and g["losses"] == losses, (r, g["losses"], losses)
        bad = [k for k, (a, b) in enumerate(zip(g["params"], params)) if not torch.equal(a, b.cpu())]
        assert not bad and len(g["params"]) == len(params) > 100, (r, bad[:8])
        assert g["chk"] == chk, r
    assert all(torch.equal(a, b) for a, b in zip(got[0]["params"], got[1]["params"]))        # the same bits on both ranks
    assert got[0]["losses"] != got[1]["losses"] and got[0]["chk"] != got[1]["chk"]            # their data (and buffers) differ
    shutil.rmtree(out, ignore_errors=True)


# ---- d. the default mode -----------------------------------------------------------------------------------------------------
def test_default_mode_ranks_apply_the_same_reduced_bits(workdir):
    """Without the deterministic mode there is no reference to equal (two eager bf16 runs differ by 0.2 relative), but both
    ranks apply the same reduced bits: parameters and reduced gradients bit-equal BETWEEN the ranks after every step, losses
    finite, buffers different."""
    cfg = ds.config(GPU_CFG, deterministic=False)
    got, metas = _run(cfg, workdir, "default_mode")
    assert ds.between_ranks(got, "params") == [[]] * got.steps
    assert ds.between_ranks(got, "grads") == [[]] * got.steps
    assert all(len(names) > 0 for names in ds.between_ranks(got, "buffers"))
    assert all(math.isfinite(x) for m in metas for x in m["losses"]), metas
    last = got[got.steps - 1][0]["params"]
    assert all(bool(torch.isfinite(t).all()) for t in last.values())
    shutil.rmtree(workdir / "default_mode", ignore_errors=True)
