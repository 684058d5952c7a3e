"""The two-rank step harness (``dist_step.py``) on the CPU: two gloo ranks of a ``TrainEncoder`` step through ``GradBucketer``
equal the one-process reference bit for bit in gradients, ``None`` pattern, parameters and buffers; the comparer reports a
stale segment and a rank that took the other's data; one rank may leave heads out of its loss for a step.

ResNet-34 with 32-channel heads in fp32, two frames of 1 x 3 x 32 x 48 per step, one backward, one thread (a single
thread's fp32 sums have one order, so the CPU step is the same function in every process)."""
import shutil

import pytest

import dist_step as ds

LIMIT_S = 240            # a two-rank run takes 10 - 15 s here (most of it process start and 170 MB of files per step and rank)
LIMIT_ASYM_S = 120       # the asymmetric case, run first and alone: a hang must not cost more than this


def _record(name, v):
    try:
        from conftest import record_achieved
        record_achieved(name, v)
    except Exception:
        pass


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("dist_step_cpu")
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(scope="module")
def ref(workdir):
    """The reference of the symmetric step, computed once and shared (it does not depend on how the ranks bucket or clear
    their gradients: no parameter changes sides between ``None`` and a tensor)."""
    return ds.reference(ds.config(), str(workdir / "ref"))


def _run(cfg, workdir, name, limit=LIMIT_S):
    got, wall = ds.run_ranks(cfg, str(workdir / name), limit)
    _record(f"dist_step_cpu/{name}/wall_s", wall)
    metas = [got.meta(r) for r in range(ds.WORLD)]
    assert metas[0]["buckets"] == metas[1]["buckets"] >= 3, metas
    _record(f"dist_step_cpu/{name}/buckets", metas[0]["buckets"])
    return got, metas


@pytest.fixture(scope="module")
def overlap_run(workdir):
    """The symmetric run with ``GradBucketer(overlap=True)``, shared by its own test and the comparer's."""
    return _run(ds.config(), workdir, "overlap")


def _assert_equal(got, ref):
    diff = ds.compare(got, ref)
    assert not diff, {k: v[:4] for k, v in diff.items()}
    # the same reduced bits are applied on both ranks; their data -- hence their running statistics -- differ
    assert ds.between_ranks(got, "params") == [[]] * got.steps
    assert ds.between_ranks(got, "grads") == [[]] * got.steps
    assert all(len(names) > 0 for names in ds.between_ranks(got, "buffers"))


def test_a_rank_that_leaves_heads_out_for_one_step(workdir, ref):
    """(First in the file, alone under a short limit.)  Rank 1 leaves the ``refine_input_feat`` outputs out of its loss in
    step 1 only: the skip heads' parameters go idle on one rank and wake up again.  Both ranks get the mean with rank 1's
    share counted as zeros, and nobody waits for a collective the other never issues."""
    cfg = ds.config(skip_refine=(1, 1))
    got, metas = _run(cfg, workdir, "asym", LIMIT_ASYM_S)
    _assert_equal(got, ds.reference(cfg, str(workdir / "asym_ref")))
    # the case is what it says: against the symmetric reference step 0 is the same, and in step 1 the skip heads' gradients
    # differ (and the body's under them: the taps miss rank 1's share) while the proposal heads' do not
    diff = ds.compare(got, ref)
    assert not [k for k in diff if k[0] == 0]
    skips = {n for n in got[0][0]["params"] if n.split(".")[0] in ("sk2", "sk3", "sk4", "sk5", "bn2", "bn3", "bn4", "bn5")}
    assert len(skips) == 16 and diff[(1, 0, "gradient")] == diff[(1, 1, "gradient")]
    assert skips <= set(diff[(1, 0, "gradient")]) and not [n for n in diff[(1, 0, "gradient")] if n.startswith("prop")]
    for d in ("asym", "asym_ref"):
        shutil.rmtree(workdir / d, ignore_errors=True)


@pytest.mark.parametrize("name,kw", [("overlap", {}), ("keep_grads", {"set_to_none": False}), ("no_overlap", {"overlap": False})])
def test_two_ranks_equal_the_reference(workdir, ref, request, name, kw):
    """3 steps, at least 3 buckets: ``GradBucketer(overlap=True)`` + ``finish()``; the same with
    ``zero_grad(set_to_none=False)`` (gradients stay bucket views and the hand-over accumulates into them); the same with
    ``overlap=False`` / ``all_reduce_mean()``."""
    got, metas = request.getfixturevalue("overlap_run") if name == "overlap" else _run(ds.config(**kw), workdir, name)
    n_p, n_b, n_s = ds.counts(got)
    _record(f"dist_step_cpu/{name}/parameters", n_p)
    _record(f"dist_step_cpu/{name}/buffers", n_b)
    _record(f"dist_step_cpu/{name}/steps", n_s)
    assert n_s == 3 and n_p > 100 and n_b > 100
    _assert_equal(got, ref)
    # the unused classifier stays None on both sides, everything else has a gradient
    g = got[2][0]["grads"]
    assert sorted(n for n, t in g.items() if t is None) == ["base.fc.bias", "base.fc.weight"]
    if name != "overlap":                                    # (the shared run stays for the comparer's tests)
        shutil.rmtree(workdir / name, ignore_errors=True)


def test_compare_reports_a_stale_segment(workdir, ref, overlap_run):
    """A reference whose ``layer2`` gradients are the previous step's (a static buffer that was not refreshed): clean at
    step 0, and at step 1 exactly that segment's parameters are named, on both ranks."""
    good = overlap_run[0]
    assert not ds.compare(good, ref)
    bad = ds.reference(ds.config(), str(workdir / "stale"), stale_segment="layer2")
    diff = ds.compare(good, bad)
    names = ds.segment_param_names(ds.config(), "layer2")
    assert len(names) > 10 and all(n.startswith("base.layer2.") for n in names)
    assert not [k for k in diff if k[0] == 0]
    for rank in range(ds.WORLD):
        assert diff[(1, rank, "gradient")] == names
        assert set(names) <= set(diff[(1, rank, "parameter")])
        assert (1, rank, "none_pattern") not in diff
    shutil.rmtree(workdir / "stale", ignore_errors=True)


def test_compare_reports_a_rank_that_took_the_other_ranks_data(workdir, overlap_run):
    """A reference built from rank 0's data on both ranks: gradients, parameters and rank 1's buffers are named from step 0 on,
    ``layer2``'s among them."""
    good = overlap_run[0]
    bad = ds.reference(ds.config(steps=1), str(workdir / "same"), same_data=True)
    diff = ds.compare(ds.Saved(good.outdir, 1), bad)
    names = set(ds.segment_param_names(ds.config(), "layer2"))
    for rank in range(ds.WORLD):
        assert names <= set(diff[(0, rank, "gradient")]) and names <= set(diff[(0, rank, "parameter")])
    # rank 0's running statistics are right; rank 1's are rank 0's: every BatchNorm's mean and variance (not its step count)
    stats = sorted(n for n in good[0][1]["buffers"] if not n.endswith("num_batches_tracked"))
    assert (0, 0, "buffer") not in diff and diff[(0, 1, "buffer")] == stats and len(stats) == 96
    shutil.rmtree(workdir / "same", ignore_errors=True)
