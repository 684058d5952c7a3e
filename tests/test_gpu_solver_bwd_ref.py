"""The solver's backward (``dmm_relax_match_bwd_f32`` and the kernels behind it) against the gate-following fp64 replay of
tests/bwd_ref.py -- a reference outside the kernels, at every row count, width class and route the dispatch has.

Bound, for every frame:  max |got - ref| <= 2e-5 * max |ref| + 1e-7  (the backward's stated contract; a correct fp32
evaluation lies about 4e-6 from this reference, tests/test_bwd_ref_cpu.py measures torch's own at 4e-7 on these cases).

Before a gradient is looked at, the device FORWARD of the same inputs must give the oracle's ``R`` and ``iters`` bit for bit:
the replay differentiates through the oracle's branches, so a forward that took others is a finding of its own and fails
the case.  No frame is left out of a comparison; the frames that sit on a kink of the reference itself are counted
(``SolverRecord.near_kink``) and must stay within 2 % (the committed seeds have none: tests/test_bwd_ref_cpu.py).

``(MT, NG, EXACT)`` instantiations of ``DMM_DISPATCH_SOLVER`` (dmm_solve.h) and the case that reaches each:
  (1..16, 1, exact)  exact/M1..16_N40 (and N33 / N55)      (32, 1, guarded)  guarded/M17,20,21,32_N40,N64, padded/M32_N31
  (16, 1, guarded)   ragged/M12_N40                        (8, 1, guarded)   none: a ragged batch of <= 8 rows in one wave
  (8, 2)   waves/M3_N65, M8_N128                                             takes relax_match_bwd_ragged_kernel<8>
  (16, 2)  waves/M12_N100, ragged/M12_N100                 (32, 2)  waves/M20_N128
  (8, 4)   waves/M5_N200                                   (16, 4)  waves/M16_N200, M10_N129 (three waves run as four)
  (20, 4, exact)  waves/M20_N200                           (32, 4)  waves/M32_N256
  relax_match_bwd_ragged_kernel<8>  ragged/M8_N50          launch_relax_match_bwd_wide  general/*
"""
import numpy as np
import pytest
import torch

import bwd_ref
from conftest import record_achieved
from dmm_net_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL, ATOL = 2e-5, 1e-7


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_REFS = {}


def references(case, is_test):
    """The replay of every live frame of a case, once (shared by whatever runs the case again)."""
    key = (case["tag"], is_test)
    if key not in _REFS:
        inp, sim, live, dead = bwd_ref.case_frames(case)
        _REFS[key] = (inp, sim, dead, [(b, m, n) + bwd_ref.frame_reference(case, inp, sim, b, m, n, is_test)
                                       for b, m, n in live])
    return _REFS[key]


def device_forward(case, inp, sim, is_test):
    """``ops.relax_match`` on the case's inputs -> (sim the device formed, R, iters)."""
    B, M, N = sim.shape
    if "cos" in inp:
        cos, inter, ap, at, w = inp["cos"], inp["inter"], inp["area_p"], inp["area_t"], 0.3
    else:                                                     # weight 0: sim = cos * 1 + iou * 0, the table itself
        cos, w = sim, 0.0
        inter, ap, at = np.zeros((B, M, N), np.int32), np.ones((B, N), np.int32), np.ones((B, M), np.int32)
    nv = dev(inp["nv"]) if "nv" in inp else None
    mv = dev(inp["mv"]) if "mv" in inp else None
    out = ops.relax_match(dev(cos), dev(inter), dev(ap), dev(at), dev(inp["score"]), score_weight=w,
                          max_iter=bwd_ref.case_max_iter(case), proj_iter=case["proj_iter"], lr=case["lr"], is_test=is_test,
                          n_valid=nv, m_valid=mv)
    torch.cuda.synchronize()
    return out["sim"].cpu().numpy(), out["R"].cpu().numpy(), out["iters"].cpu().numpy()


def run_case(case):
    """-> the records of the case's frames (both modes), after every assertion on it."""
    recs = []
    for is_test in (0, 1):
        inp, sim, dead, refs = references(case, is_test)
        B, M, N = sim.shape
        nv = dev(inp["nv"]) if "nv" in inp else None
        mv = dev(inp["mv"]) if "mv" in inp else None
        with _lib.options(**case["opts"]):
            # ---- the forward first: same table, same R, same iteration count as the oracle, bit for bit ----
            d_sim, d_R, d_iters = device_forward(case, inp, sim, is_test)
            for b, m, n, rec, _ in refs:
                assert np.array_equal(d_sim[b, :m, :n], sim[b, :m, :n]), (case["tag"], "sim", b)
                assert int(d_iters[b]) == rec.iters, (case["tag"], "iters", b, int(d_iters[b]), rec.iters)
                assert np.array_equal(d_R[b, :m, :rec.Pp], rec.R), \
                    (case["tag"], "forward R", b, float(np.abs(d_R[b, :m, :rec.Pp] - rec.R).max()))
            got = ops.relax_match_bwd(dev(sim), dev(inp["score"]), dev(inp["dRb"]), dev(inp["dms"]), dev(inp["dds"]),
                                      max_iter=bwd_ref.case_max_iter(case), proj_iter=case["proj_iter"], lr=case["lr"],
                                      is_test=is_test, n_valid=nv, m_valid=mv)
            torch.cuda.synchronize()
        got = got.cpu().numpy().astype(np.float64)
        for b, _, _ in dead:
            assert not got[b].any(), (case["tag"], "dead frame", b)
        kinks = 0
        for b, m, n, rec, ref in refs:
            kinks += rec.near_kink()
            scale = float(np.abs(ref).max())
            err = float(np.abs(got[b, :m, :n] - ref).max())
            ratio = err / scale if scale > 0 else 0.0
            record_achieved(f"solver_bwd_ref/{case['tag']}/is_test{is_test}/frame{b}_{m}x{n}_iters{rec.iters}", ratio)
            print(f"{case['tag']} is_test={is_test} frame {b} ({m} x {n}, {rec.iters} iterations): "
                  f"err {err:.3e} scale {scale:.3e} ratio {ratio:.3e}")
            assert np.isfinite(got[b]).all()
            assert err <= RTOL * scale + ATOL, (case["tag"], is_test, b, err, scale)
            assert not got[b, m:].any() and not got[b, :, n:].any(), (case["tag"], "outside the live block", b)
            recs.append(rec)
        assert kinks <= 0.02 * max(len(refs), 1), (case["tag"], kinks)
    return recs


def _cases(*classes):
    cs = [c for c in bwd_ref.SOLVER_CASES if c["cls"] in classes]
    return pytest.mark.parametrize("case", cs, ids=[c["tag"] for c in cs])


@_cases("exact", "guarded", "waves")
def test_register_kernels_against_the_replay(case):
    """``relax_match_bwd_kernel<MT, NG, EXACT>``: every exact-row body (1..16 rows; 9..16 carry two ATen lanes as a packed
    pair), the guarded 17..32-row bodies, and two and four waves of columns."""
    run_case(case)


@_cases("padded")
def test_padded_tables_against_the_replay(case):
    """N <= M: the solver runs on M + 1 columns, the zero columns take part in every projection, and their gradient must
    not leak -- ``dsim`` has N columns and the reference slices likewise."""
    run_case(case)


@_cases("ragged")
def test_ragged_batches_against_the_replay(case):
    """``n_valid`` / ``m_valid``: a full, a half, a one-proposal and two dead frames.  M = 8, N = 50 takes
    ``relax_match_bwd_ragged_kernel<8>``, M = 12 the guarded dense bodies at one and at two waves.  Dead frames and
    everything outside a live block are exactly zero."""
    recs = run_case(case)
    assert {(r.m, r.n) for r in recs} == {(case["M"], case["N"]), (case["M"] // 2, case["N"] // 2), (case["M"], 1)}


@_cases("general")
def test_general_backward_against_the_replay(case):
    """``launch_relax_match_bwd_wide``: tables outside the envelope, option FORCE_WIDE inside it, and one more outer
    iteration than the register kernel's tape index (``kMaxTapeOuter``, read from dmm_solve.hip) holds."""
    if case["max_iter"] == "above_tape":
        assert bwd_ref.case_max_iter(case) == bwd_ref.max_tape_outer() + 1 > 1
    run_case(case)


@_cases("settings")
def test_solver_settings_against_the_replay(case):
    """``proj_iter`` 1 / 5, ``max_iter`` 0 / 1 / 20, ``lr`` 0.5; sim mixed on the device from a cosine and count tables.
    With ``max_iter`` = 0, R is the one-hot start and the gradient flows through ``sim`` in ``match_score`` alone."""
    recs = run_case(case)
    if case["max_iter"] == 0:
        assert all(r.iters == 0 and set(np.unique(r.R)) <= {0.0, 1.0} for r in recs)


def test_tables_on_which_the_solver_exits_early():
    """Both data-dependent exits (40 x 5): ``cost[-2] == cost[-1]`` ends the outer loop, a sweep that moves nothing ends the
    inner one.  That each kind occurs is read off the oracle's own ``iters`` / ``inner`` -- a check on the inputs."""
    recs = []
    for case in [c for c in bwd_ref.SOLVER_CASES if c["cls"] == "exits"]:
        recs += run_case(case)
    assert any(r.outer_exit for r in recs) and any(r.inner_exit for r in recs)
    record_achieved("solver_bwd_ref/exits/frames_with_outer_exit", sum(r.outer_exit for r in recs) / len(recs))
    record_achieved("solver_bwd_ref/exits/frames_with_inner_exit", sum(r.inner_exit for r in recs) / len(recs))


# ---------------------------------------------------------------------------------------------------------------------
# the training call: the walk of the forward's tape, and the re-run into the workspace, against the references chained
# ---------------------------------------------------------------------------------------------------------------------
def _chain_reference(fr, saved, B, N, M, HW, kw, d_full, d_ms, d_ds, d_loss, iters):
    """float64 autograd through cosine -> (1 - w) mix -> solver replay -> mask mix product / scores / matching loss of
    every frame -> (g_feat_t [B, M, D], g_feat_p [B, N, D]).  The IoU part of sim, gt and the solver's branches come from
    the forward's saved block (cos | sim | Rb | gt) and the oracle's record on that very sim."""
    Pp = bwd_ref.padded_width(N, M)
    n_cs, n_rb = B * M * N, B * M * Pp
    sv = saved.cpu().numpy()
    sim32 = sv[n_cs:2 * n_cs].reshape(B, M, N)
    Rb32 = sv[2 * n_cs:2 * n_cs + n_rb].reshape(B, M, Pp)
    gt = torch.from_numpy(sv[2 * n_cs + n_rb:3 * n_cs + n_rb].reshape(B, M, N).copy()).double()
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    tf = t64(np.stack([f.template_feature for f in fr])).requires_grad_(True)
    pf = t64(np.stack([f.proposed_feature for f in fr])).requires_grad_(True)
    cos = bwd_ref.cosine(tf, pf)
    w_feat = float(np.float32(1.0 - kw["score_weight"]))
    sim = w_feat * cos + (t64(sim32) - w_feat * cos.detach())          # the forward's fp32 table in value, d sim = w d cos
    obj = (t64(d_loss) * ((cos - gt) ** 2).mean((1, 2))).sum()
    for b in range(B):
        rec = bwd_ref.SolverRecord(sim32[b], kw["max_iter"], kw["proj_iter"], kw["lr"], kw["is_test"])
        assert rec.iters == int(iters[b]) and np.array_equal(Rb32[b], rec.R * rec.logic), ("forward", b)
        assert not rec.near_kink()
        o, _, Rb, _, _ = bwd_ref.solver_objective(sim[b], rec, fr[b].proposal_score, None, d_ms[b], d_ds[b])
        full = Rb[:, :N] @ t64(fr[b].proposed_mask.reshape(N, HW))
        obj = obj + o + (full * t64(d_full[b].reshape(M, HW))).sum()
    obj.backward()
    return tf.grad.numpy(), pf.grad.numpy()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("M", [1, 5, 9, 16])
def test_training_call_backward_tape_walk_and_rerun_against_the_chained_references(M, B):
    """``dmm_match_train_backward`` both ways -- walking the tape the forward kept, and re-running the solver into the
    workspace -- against float64 autograd through the references chained: the float64 mix product, the solver replay, the
    feature side.  test_gpu_train_fused.py holds the two to each other; this holds each to something else."""
    from dmm_net_amd import synth
    N, H, W, D = 50, 12, 14, 256
    fr = [synth.make_frame(N, M, H, W, D, seed=700 + 31 * M + b, kind="structured", with_targets=True) for b in range(B)]
    st = lambda k: dev(np.stack([getattr(f, k) for f in fr], 0))
    pm, tm, tg, pf, tf, sc = (st(k) for k in ("proposed_mask", "mask_last_occurence", "targets", "proposed_feature",
                                               "template_feature", "proposal_score"))
    r = np.random.default_rng(40 + M + B)
    for is_test in (0, 1):
        kw = dict(score_weight=0.3, max_iter=10, proj_iter=5, lr=0.1, is_test=is_test)
        full, ms, ds, loss, iters, saved, taped = ops.match_train_forward(pm, tm, tg, pf, tf, sc, None, None, **kw)
        assert taped == 1
        d_full, d_ms, d_ds, d_loss = (r.random(t.shape).astype(np.float32) for t in (full, ms, ds, loss))
        args = (pm, pf, tf, sc, saved, True, dev(d_full), dev(d_ms), dev(d_ds), dev(d_loss), None, None, M)
        walked = ops.match_train_backward(*args, iters=iters, taped=taped, **kw)
        rerun = ops.match_train_backward(*args, **kw)
        torch.cuda.synchronize()
        ref = _chain_reference(fr, saved, B, N, M, H * W, kw, d_full, d_ms, d_ds, d_loss, iters.cpu().numpy())
        for how, got in (("tape", walked), ("rerun", rerun)):
            for name, g, e in zip(("g_feat_t", "g_feat_p"), got, ref):
                scale = float(np.abs(e).max())
                err = float(np.abs(g.cpu().numpy().astype(np.float64) - e).max())
                record_achieved(f"solver_bwd_ref/train_call/B{B}_M{M}_N{N}_is_test{is_test}/{how}/{name}", err / scale)
                print(f"train call B={B} M={M} is_test={is_test} {how} {name}: err {err:.3e} scale {scale:.3e}")
                assert scale > 0 and err <= RTOL * scale, (how, name, is_test, err, scale)
