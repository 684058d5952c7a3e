"""The gate record of the oracle's solver and the gate-following fp64 replay built on it (tests/bwd_ref.py) -- no GPU.

The replay is the reference the GPU tests hold the backward kernels to, so it is itself held here: to the oracle's forward
(an fp32 replay along the record reproduces R) and to torch's own fp32 autograd through ``oracle/torch_ref.py``."""
import numpy as np
import pytest
import torch

import bwd_ref
import oracle
from oracle import torch_ref

CLASSES = sorted({c["cls"] for c in bwd_ref.SOLVER_CASES})


@pytest.mark.parametrize("m,n,max_iter,proj_iter,kind", [(5, 50, 10, 5, "uniform"), (1, 4, 40, 5, "dominant0.0"),
                                                         (16, 17, 20, 5, "uniform"), (3, 10, 40, 5, "dominant0.05"),
                                                         (9, 130, 10, 3, "uniform"), (4, 7, 0, 5, "uniform")])
def test_gate_record_leaves_the_results_alone_and_is_complete(m, n, max_iter, proj_iter, kind):
    """With the record requested X, R, cost, iters and inner are the same bits; and an fp32 replay that applies the recorded
    gates, with no comparison of its own, reproduces R to 1e-6: the record is complete and indexed as documented."""
    case = dict(B=2, M=m, N=n, seed=3, kind=kind, nv=None)
    sim = bwd_ref.case_inputs(case)["sim"]
    for b in range(2):
        C = -sim[b]
        plain = oracle.relax(C, max_iter, proj_iter, 0.1)
        gates = oracle.gate_record(m, n, max_iter, proj_iter)
        rec = oracle.relax(C, max_iter, proj_iter, 0.1, gates=gates)
        assert rec["iters"] == plain["iters"]
        for k in ("X", "R", "cost", "inner"):
            assert np.array_equal(plain[k], rec[k]), k
        if n > m:                                            # (SolverRecord pads N <= M itself: the bare table is its input)
            r = bwd_ref.SolverRecord(sim[b], max_iter, proj_iter, 0.1, 0)
            assert np.array_equal(r.R, plain["R"]) and r.iters == plain["iters"]
            assert float(np.abs(bwd_ref.fp32_replay_R(r) - r.R).max()) <= 1e-6
        # slots of sweeps that did not run stay as the caller left them
        for it in range(max_iter):
            ran = int(plain["inner"][it]) if it < plain["iters"] else 0
            assert not gates["relu"][it, ran:].any() and not gates["col"][it, ran:].any()


def _torch_fp32_grad(sim, score, dRb, dms, dds, max_iter, proj_iter, lr, is_test):
    """torch's own fp32 autograd through torch_ref.relax_matching and the layer's head (torch_ref.match_forward)."""
    m, n = sim.shape
    Pp = bwd_ref.padded_width(n, m)
    s = torch.from_numpy(sim.copy()).requires_grad_(True)
    sp = torch.cat([s, s.new_zeros(m, Pp - n)], 1) if Pp > n else s
    sc = torch.zeros(Pp)
    sc[:n] = torch.from_numpy(score)
    _, _, xs = torch_ref.relax_matching(-sp, max_iter, proj_iter, lr)
    R = torch.stack(xs, 0).mean(0)
    logic = (R == R.max(1, keepdim=True)[0]).float() if is_test else (R > 0.01).float()
    Rb = R * logic
    ms = (R.clamp(0, 1) * sp).max(1)[0]
    ds = (sc.view(1, -1) * Rb).sum(1)
    ((Rb * torch.from_numpy(dRb)).sum() + (ms * torch.from_numpy(dms)).sum() + (ds * torch.from_numpy(dds)).sum()).backward()
    return s.grad.double().numpy(), len(xs) - 1


@pytest.mark.parametrize("cls", CLASSES)
def test_replay_agrees_with_torch_fp32_autograd_on_every_solver_case(cls):
    """Guards the reference: on every solver case of the GPU list the fp64 replay lies within 2e-5 of the largest entry of
    torch's fp32 autograd through ``torch_ref.relax_matching`` -- the bound the GPU tests hold the kernels to.  Also the
    checks on the inputs: no committed case sits on a kink of the reference, and the exit cases do exit."""
    kinks = frames = 0
    outer = inner = False
    worst = 0.0
    for case in [c for c in bwd_ref.SOLVER_CASES if c["cls"] == cls]:
        inp, sim, live, _ = bwd_ref.case_frames(case)
        mi = bwd_ref.case_max_iter(case)
        for is_test in (0, 1):
            for b, m, n in live:
                pp = bwd_ref.padded_width(n, m)
                rec = bwd_ref.SolverRecord(sim[b, :m, :n], mi, case["proj_iter"], case["lr"], is_test)
                frames += 1
                kinks += rec.near_kink()
                outer |= rec.outer_exit
                inner |= rec.inner_exit
                if m * pp > 16 * 130 or mi > 100:            # (torch_ref's start is m * Pp Python steps: the large tables
                    continue                                 #  and the 1025-iteration case are left to the GPU tests)
                _, ref = bwd_ref.frame_reference(case, inp, sim, b, m, n, is_test)
                got, iters = _torch_fp32_grad(sim[b, :m, :n], inp["score"][b, :n], inp["dRb"][b, :m, :pp], inp["dms"][b, :m],
                                              inp["dds"][b, :m], mi, case["proj_iter"], case["lr"], is_test)
                assert iters == rec.iters, (case["tag"], b)
                scale = float(np.abs(ref).max())
                err = float(np.abs(got - ref).max())
                worst = max(worst, err / max(scale, 1e-30))
                assert err <= 2e-5 * scale + 1e-7, (case["tag"], is_test, b, err, scale)
    print(f"{cls}: {frames} frames, worst fp32-autograd / replay ratio {worst:.2e}")
    assert kinks == 0, kinks
    if cls == "exits":
        assert outer and inner
