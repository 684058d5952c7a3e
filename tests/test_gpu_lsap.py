"""The device Hungarian solver (algo 'hun'): dmm_lsap_f32 / dmm_hungarian_match_f32 pick exactly scipy's assignment, and
the layer's 'hun' route on the device computes what the host route (scipy on the copied cost table) computes."""
import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment as scipy_lsa

import lsap_model
from dmm_net_amd import _lib, autograd, ops, synth
from dmm_net_amd.match_model import MatchModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def cfg(algo="hun", w=0.3):
    return {"matching": {"algo": algo}, "relax_max_iter": 10, "relax_proj_iter": 5, "relax_learning_rate": 0.1,
            "score_weight": w}


def same_bits(a, b, zero_sign_free=False):
    """Bit identity (torch.equal treats -0.0 == +0.0).  ``zero_sign_free``: a zero may carry either sign -- a
    match_score of a row whose assigned sim is <= 0 is a max over products 0 * sim, and which signed zero torch's max
    reduction keeps is its own order, not the assignment's."""
    a, b = a.detach().float().contiguous(), b.detach().float().contiguous()
    if a.shape != b.shape:
        return False
    same = a.view(torch.int32) == b.view(torch.int32)
    if zero_sign_free:
        same |= (a == 0) & (b == 0)
    return bool(same.all())


def _col_of_row(c):
    r, k = scipy_lsa(c)
    out = np.full(c.shape[0], -1, np.int64)
    out[r] = k
    return out


def _check_batch(C, rv, cv, maximize=False):
    X, col, st = ops.linear_sum_assignment(torch.from_numpy(C).to(DEV),
                                           torch.tensor(rv, dtype=torch.int32, device=DEV),
                                           torch.tensor(cv, dtype=torch.int32, device=DEV), maximize=maximize)
    X, col, st = X.cpu().numpy(), col.cpu().numpy(), st.cpu().numpy()
    B, nr, nc = C.shape
    assert (st == 0).all()
    for b in range(B):
        blk = C[b, :rv[b], :cv[b]]
        exp = np.full(nr, -1, np.int64)
        if rv[b] and cv[b]:
            exp[:rv[b]] = _col_of_row(-blk.astype(np.float64) if maximize else blk)
        np.testing.assert_array_equal(col[b], exp, err_msg=f"frame {b} {blk!r}")
        ex = np.zeros((nr, nc), np.float32)
        ex[np.nonzero(exp >= 0)[0], exp[exp >= 0]] = 1
        np.testing.assert_array_equal(X[b], ex)


@pytest.mark.parametrize("family", lsap_model.FAMILIES)
def test_lsap_matches_scipy_on_ragged_batches(family):
    """Hundreds of ragged frames in one launch, the padding outside each live block filled with NaN (never read);
    frames with more live rows than columns go through the kernel's own transpose."""
    rng = np.random.default_rng(100 + lsap_model.FAMILIES.index(family))
    for nr, nc, B in ((12, 16, 400), (32, 256, 40), (5, 50, 300)):
        C = np.full((B, nr, nc), np.nan, np.float32)
        rv = rng.integers(0, nr + 1, B)
        cv = rng.integers(0, nc + 1, B)
        for b in range(B):
            C[b, :rv[b], :cv[b]] = lsap_model.make_table(rng, family, int(rv[b]), int(cv[b]))
        _check_batch(C, rv, cv)


def test_lsap_tall_tables_and_maximize():
    rng = np.random.default_rng(5)
    B, nr, nc = 200, 40, 12                                  # nr > nc: the wrapper transposes, as scipy does
    C = rng.integers(-3, 4, (B, nr, nc)).astype(np.float32)
    _check_batch(C, np.full(B, nr), np.full(B, nc))
    C = rng.standard_normal((B, 20, 200)).astype(np.float32)
    _check_batch(C, np.full(B, 20), np.full(B, 200), maximize=True)


def test_lsap_status_of_invalid_frames_leaves_neighbours_alone():
    rng = np.random.default_rng(9)
    B, nr, nc = 8, 4, 6
    C = rng.integers(0, 3, (B, nr, nc)).astype(np.float32)
    C[1, 2, 3] = np.nan
    C[3, 0, 0] = -np.inf
    C[5, :, :5] = np.inf                                     # every row needs column 5: infeasible
    C[6, 1, 2] = np.inf                                      # a +inf entry alone is fine
    X, col, st = ops.linear_sum_assignment(torch.from_numpy(C).to(DEV))
    assert st.cpu().tolist() == [0, 1, 0, 1, 0, 2, 0, 0]
    col, X = col.cpu().numpy(), X.cpu().numpy()
    for b in range(B):
        if b in (1, 3, 5):
            assert (col[b] == -1).all() and not X[b].any()
            with pytest.raises(ValueError):
                scipy_lsa(C[b])
        else:
            np.testing.assert_array_equal(col[b], _col_of_row(C[b]))
    with pytest.raises(ValueError, match="invalid numeric entries"):
        ops.check_lsap_status(st)


def test_lsap_entry_refuses_tables_outside_its_envelope():
    L = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    for nr, nc in ((33, 40), (4, 257), (6, 5)):
        C = torch.zeros((2, nr, nc), device=DEV)
        st = torch.zeros((2,), dtype=torch.int32, device=DEV)
        assert L.dmm_lsap_f32(C.data_ptr(), 2, nr, nc, None, None, None, None, st.data_ptr(), s) == \
            _lib.DMM_ERR_UNSUPPORTED
    X, col, st = ops.linear_sum_assignment(torch.randn((3, 40, 300), device=DEV))   # host fallback outside it
    for b in range(3):
        assert int(st[b]) == 0


def _layer_inputs(B, N, M, seed, n_valid=None, m_valid=None, H=24, W=24, D=32):
    g = torch.Generator().manual_seed(seed)
    pm = (torch.rand((B, N, H, W), generator=g) > 0.6).float().to(DEV)
    tm = (torch.rand((B, M, H, W), generator=g) > 0.6).float().to(DEV)
    pf = torch.randn((B, N, D), generator=g).to(DEV)
    tf = torch.randn((B, M, D), generator=g).to(DEV)
    sc = torch.rand((B, N), generator=g).to(DEV)
    nv = None if n_valid is None else torch.tensor(n_valid, dtype=torch.int32, device=DEV)
    mv = None if m_valid is None else torch.tensor(m_valid, dtype=torch.int32, device=DEV)
    inter, ap, at = ops.iou_counts(pm, tm, nv, mv)
    cos = ops.cosine(ops.feature_normalize(tf), ops.feature_normalize(pf), nv, mv)
    return cos, inter, ap, at, sc, nv, mv


@pytest.mark.parametrize("B,N,M,n_valid,m_valid", [
    (6, 10, 5, None, None), (4, 3, 5, None, None),                         # P <= O: padded columns of -0.0
    (5, 12, 6, [12, 3, 0, 7, 6], [6, 6, 2, 0, 4]),                          # ragged, dead frames
    (3, 200, 20, None, None), (3, 50, 10, [50, 9, 31], [10, 10, 1])])
def test_hungarian_match_equals_the_host_route(B, N, M, n_valid, m_valid):
    """dmm_hungarian_match_f32 against the reference's route: sim of the relaxed layer's prologue, padded, negated,
    scipy, and the scores in torch."""
    cos, inter, ap, at, sc, nv, mv = _layer_inputs(B, N, M, seed=B * 1000 + N, n_valid=n_valid, m_valid=m_valid)
    for is_test in (0, 1):
        r = ops.hungarian_match(cos, inter, ap, at, sc, score_weight=0.3, is_test=is_test, n_valid=nv, m_valid=mv)
        ref = ops.relax_match(cos, inter, ap, at, sc, score_weight=0.3, max_iter=0, proj_iter=0, lr=0.0, is_test=is_test,
                              n_valid=nv, m_valid=mv)
        assert same_bits(r["sim"], ref["sim"])
        assert (r["status"] == 0).all()
        PpS = ops.padded_width(N, M)
        for b in range(B):
            Nb = N if n_valid is None else n_valid[b]
            Mb = M if m_valid is None else m_valid[b]
            R = torch.zeros((M, PpS), device=DEV)
            ms = torch.zeros((M,), device=DEV)
            ds = torch.zeros((M,), device=DEV)
            if Nb > 0 and Mb > 0:
                Pp = ops.padded_width(Nb, Mb)
                simp = torch.zeros((Mb, Pp), device=DEV)
                simp[:, :Nb] = ref["sim"][b, :Mb, :Nb]
                Rh = autograd.hungarian_onehot(-simp)
                Rb = Rh * ((Rh == Rh.max(1, keepdim=True)[0]).float() if is_test else (Rh > 0.01).float())
                R[:Mb, :Pp] = Rb
                ms[:Mb] = (Rh.clamp(0, 1) * simp).max(1)[0]
                scp = torch.zeros((Pp,), device=DEV)
                scp[:Nb] = sc[b, :Nb]
                ds[:Mb] = (scp.view(1, -1) * Rb).sum(1)
            assert same_bits(r["R"][b], R) and same_bits(r["Rb"][b], R)
            assert same_bits(r["match_score"][b], ms, zero_sign_free=True) and same_bits(r["det_score"][b], ds)


def test_hungarian_match_without_templates_reports_ok():
    cos, inter, ap, at, sc, nv, mv = _layer_inputs(3, 10, 2, seed=5)
    r = ops.hungarian_match(cos[:, :0].contiguous(), inter[:, :0].contiguous(), ap, at[:, :0].contiguous(), sc,
                            score_weight=0.3, is_test=1)
    assert r["status"].cpu().tolist() == [0, 0, 0] and r["Rb"].shape == (3, 0, 10)


def _packed_inputs(B, N, M, H, W, D, seed):
    g = torch.Generator().manual_seed(seed)
    pm = (torch.rand((B, N, H, W), generator=g) > 0.5).float().to(DEV)
    tm = (torch.rand((B, M, H, W), generator=g) > 0.5).float().to(DEV)
    pf = torch.randn((B, N, D), generator=g).to(DEV)
    tf = torch.randn((B, M, D), generator=g).to(DEV)
    sc = torch.rand((B, N), generator=g).to(DEV)
    return ops.pack_masks(pm), ops.pack_masks(tm), pf, tf, sc


def test_match_solve_packed_hun_equals_the_relaxed_front_and_scipy():
    """dmm_match_solve_packed_hun (the fixed-slot frame step's 'hun' solve): Rb, scores and status against the relaxed
    step's own cosine + counts (its sim output) followed by scipy on -sim padded; a NaN feature sets its frame's
    status only."""
    B, N, M, H, W, D = 5, 20, 6, 40, 40, 32
    nv = torch.tensor([20, 7, 0, 3, 12], dtype=torch.int32, device=DEV)      # a dead frame, a P <= O frame
    mv = torch.tensor([6, 6, 4, 6, 2], dtype=torch.int32, device=DEV)
    pp, pt, pf, tf, sc = _packed_inputs(B, N, M, H, W, D, seed=21)
    pf[4, 1, 3] = float("nan")
    Pp = ops.padded_width(N, M)
    f32 = dict(dtype=torch.float32, device=DEV)
    ws_bytes = int(_lib.load().dmm_workspace_bytes(B, N, M, D))
    for is_test in (0, 1):
        Rb, ms, ds = torch.empty((B, M, Pp), **f32), torch.empty((B, M), **f32), torch.empty((B, M), **f32)
        st = torch.empty((B,), dtype=torch.int32, device=DEV)
        ops.match_solve_packed_hun(pp, pt, pf, tf, sc, nv, mv, H * W, score_weight=0.3, is_test=is_test,
                                   out=(Rb, ms, ds), status=st, workspace=torch.empty((ws_bytes,), dtype=torch.uint8,
                                                                                      device=DEV))
        sim = torch.empty((B, M, N), **f32)
        rr, mr, dr = torch.empty((B, M, Pp), **f32), torch.empty((B, M), **f32), torch.empty((B, M), **f32)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=DEV)
        _lib.call("dmm_match_solve_packed", DEV, pp.data_ptr(), pt.data_ptr(), pf.data_ptr(), tf.data_ptr(), sc.data_ptr(),
                  B, N, M, H * W, D, nv.data_ptr(), mv.data_ptr(), 0.3, 0, 0, 0.0, is_test, rr.data_ptr(), mr.data_ptr(),
                  dr.data_ptr(), sim.data_ptr(), None, None, ws.data_ptr(), ws.numel(),
                  torch.cuda.current_stream().cuda_stream)
        assert st.cpu().tolist() == [0, 0, 0, 0, 1]
        for b in range(4):
            Nb, Mb = int(nv[b]), int(mv[b])
            R = torch.zeros((M, Pp), **f32)
            ms_e, ds_e = torch.zeros((M,), **f32), torch.zeros((M,), **f32)
            if Nb > 0 and Mb > 0:
                Pb = ops.padded_width(Nb, Mb)
                simp = torch.zeros((Mb, Pb), **f32)
                simp[:, :Nb] = sim[b, :Mb, :Nb]
                Rh = autograd.hungarian_onehot(-simp)
                R[:Mb, :Pb] = Rh
                ms_e[:Mb] = (Rh.clamp(0, 1) * simp).max(1)[0]
                scp = torch.zeros((Pb,), **f32)
                scp[:Nb] = sc[b, :Nb]
                ds_e[:Mb] = (scp.view(1, -1) * Rh).sum(1)
            assert same_bits(Rb[b], R), b
            assert same_bits(ms[b], ms_e, zero_sign_free=True) and same_bits(ds[b], ds_e), b
        assert float(Rb[4].abs().sum()) == 0.0                       # the NaN frame: zeros


def _frame(seed, P=10, O=5, H=32, W=32, D=64):
    fr = synth.make_frame(P, O, H, W, D, seed=seed, kind="structured", with_targets=True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return (t(fr.proposed_feature), t(fr.proposed_mask), t(fr.template_feature), t(fr.mask_last_occurence),
            t(fr.proposal_score), t(fr.targets))


def _run_match(device_route, is_test, inputs, det=False):
    old = autograd._DEVICE_LSAP
    autograd._DEVICE_LSAP = device_route
    try:
        pf, pm, tf, tm, sc, tg = inputs
        pf, tf = pf.clone().requires_grad_(True), tf.clone().requires_grad_(True)
        model = MatchModel(cfg(), is_test)
        from dmm_net_amd import deterministic
        with deterministic(det):
            full, ms, ds, _, loss = model(pf, pm, [tf], tm, sc, tg)
            loss["cost_loss"].backward()
        torch.cuda.synchronize()
        return full, ms, ds, loss["cost_loss"].detach(), pf.grad, tf.grad
    finally:
        autograd._DEVICE_LSAP = old


@pytest.mark.parametrize("is_test", [0, 1])
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("P,O", [(10, 5), (4, 6), (50, 10)])
def test_match_model_hun_device_route_equals_scipy_route(is_test, det, P, O):
    inputs = _frame(700 + P + O, P=P, O=O)
    dev_out = _run_match(True, is_test, inputs, det)
    host_out = _run_match(False, is_test, inputs, det)
    for k, (a, b) in enumerate(zip(dev_out[:4], host_out[:4])):     # full, match_score, det_score, cost_loss
        assert same_bits(a, b, zero_sign_free=k == 1)
    for a, b in zip(dev_out[4:], host_out[4:]):
        assert torch.allclose(a, b, rtol=1e-6, atol=0), float((a - b).abs().max())


def test_nan_feature_raises_value_error_on_both_routes():
    pf, pm, tf, tm, sc, tg = _frame(811)
    pf = pf.clone()
    pf[0, 0] = float("nan")
    for route in (True, False):
        old = autograd._DEVICE_LSAP
        autograd._DEVICE_LSAP = route
        try:
            with pytest.raises(ValueError, match="invalid numeric entries"):
                MatchModel(cfg(), 1)(pf, pm, [tf], tm, sc)
        finally:
            autograd._DEVICE_LSAP = old


class _Props:
    def __init__(self, mask, scores):
        self._f = {"mask": mask, "scores": scores}

    def __len__(self):
        return self._f["mask"].shape[0]

    def fields(self):
        return list(self._f.keys())

    def get_field(self, k):
        return self._f[k]


def test_dmm_model_hun_inference_captures_into_a_graph():
    """Eval-mode DMM_Model.inference with 'hun' has no host round trip left: it captures into a CUDA graph and the replay
    equals the eager call (the host route's .cpu() makes the capture fail)."""
    from dmm_net_amd.dmm_model import DMM_Model
    B, F, P, H, W, D = 4, 5, 12, 32, 32, 64
    n_valid = [5, 2, 4, 3]
    frames = [synth.make_frame(P, F, H, W, D, seed=4600 + b, kind="structured") for b in range(B)]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    feats = torch.cat([t(fr.proposed_feature) for fr in frames], 0)
    props = [_Props(t(fr.proposed_mask).unsqueeze(1), t(fr.proposal_score)) for fr in frames]
    valid = torch.zeros((B, F), device=DEV)
    for b, o in enumerate(n_valid):
        valid[b, :o] = 1
    ml = torch.stack([t(fr.mask_last_occurence) for fr in frames], 0)
    tplt = {b: {"feat": [t(frames[b].template_feature)]} for b in range(B)}
    model = DMM_Model(cfg(), is_test=1, feature_extractor=lambda bf, pr: feats)
    infos = {"args": None, "shape": None, "extra_frame": [0] * B, "valid": valid}
    with torch.no_grad():
        eager = model.inference(infos, props, None, ml, tplt)[0].clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            model.inference(infos, props, None, ml, tplt)            # warm-up (the valid layout is read once per clip)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = model.inference(infos, props, None, ml, tplt)[0]
        g.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, eager)
