"""Every branch of the one-call entries' shared front (csrc/dmm_front.hip), through every entry, at the smallest shapes that
reach it: results per frame against the C oracle, and the number of kernels each call enqueues against
tests/golden/entry_launch_counts.json -- the counts of the commit BEFORE the entries shared one front, recorded with
``collect()`` below against a build of that commit.

Branches of the chain (dmm_launchers.h): the small fused launch (default, dense, D = 512), the lanes kernel
(SMALL_FUSED=0, ragged batches, more than 16 rows), the dense tile kernel (COSINE_KERNEL=1, D = 64) and
normalise + cosine (D = 48, ragged fallbacks).  A row may differ from the recorded one only where the packed entries'
fallback now normalises both feature sets with one launch instead of two (``_expected``)."""
import json
import os

import numpy as np
import pytest
import torch

import oracle
from dmm_net_amd import _lib, autograd, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KW = dict(score_weight=0.3, max_iter=10, proj_iter=5, lr=0.1)
# (name, options, D)
BRANCHES = [("default", {}, 512), ("small_fused0", {"SMALL_FUSED": 0}, 512), ("cosine_kernel1", {"COSINE_KERNEL": 1}, 512),
            ("d64", {}, 64), ("d48", {}, 48)]
# B, N, M, H, W: HW = 240 is no multiple of 64 (packed words, chunk tails); M = 17: the targets take their own count pass
SHAPES = {"6x3": (2, 6, 3, 12, 20), "18x17": (2, 18, 17, 12, 20)}
CASES = [(br[0], sh, ragged, is_test, "f32") for br in BRANCHES for sh in SHAPES for ragged in (0, 1) for is_test in (0, 1)]
CASES.append(("default", "6x3", 0, 0, "f16"))
COUNTS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "entry_launch_counts.json")
PACKED_ENTRIES = ("forward_packed", "solve_packed", "solve_packed_hun")
_inputs = {}


def case_id(case):
    br, sh, ragged, is_test, dt = case
    return f"{br}/{sh}/{'ragged' if ragged else 'dense'}/is_test{is_test}/{dt}"


def _case_inputs(sh, D, ragged, is_test, dt):
    """Host inputs and the per-frame oracle results of one case: computed once, shared by every branch, never written."""
    key = (sh, D, ragged, is_test, dt)
    if key in _inputs:
        return _inputs[key]
    B, N, M, H, W = SHAPES[sh]
    rng = np.random.Generator(np.random.PCG64(1000 + 7 * D + N))
    mdt = torch.float16 if dt == "f16" else torch.float32
    soft = lambda k: torch.from_numpy(rng.random((B, k, H, W), dtype=np.float32)).to(mdt).float().numpy()
    d = dict(pm=soft(N), tm=soft(M), tg=soft(M), pf=rng.standard_normal((B, N, D), dtype=np.float32),
             tf=rng.standard_normal((B, M, D), dtype=np.float32), sc=rng.random((B, N), dtype=np.float32),
             nv=np.array([N, N - 2] if ragged else [N, N]), mv=np.array([M, M - 1] if ragged else [M, M]), mdt=mdt)
    d["oracle"] = []
    for b in range(B):
        n, m = int(d["nv"][b]), int(d["mv"][b])
        o = oracle.match_forward(d["pm"][b, :n], d["tm"][b, :m], d["pf"][b, :n], d["tf"][b, :m], d["sc"][b, :n],
                                 is_test=is_test, **KW)
        o["loss"] = float(oracle.matching_loss(d["pm"][b, :n], d["tg"][b, :m], o["cos"])[0])
        # the 'hun' route on the same sim: scipy on -sim padded, scores as the layer's epilogue computes them
        pp = ops.padded_width(n, m)
        simp = torch.zeros((m, pp))
        simp[:, :n] = torch.from_numpy(np.asarray(o["sim"]).reshape(m, n))
        Rh = autograd.hungarian_onehot(-simp)
        scp = torch.zeros((pp,))
        scp[:n] = torch.from_numpy(d["sc"][b, :n])
        o["hun"] = (Rh.numpy(), (Rh.clamp(0, 1) * simp).max(1)[0].numpy(), (scp.view(1, -1) * Rh).sum(1).numpy())
        d["oracle"].append(o)
    _inputs[key] = d
    return d


def _check(d, is_test, tag, *, full=None, ms=None, ds=None, iters=None, sim=None, R=None, Rb=None, loss=None):
    """Device outputs of one call against the oracle, frame by frame on the live block (the bounds of test_gpu_parity.py)."""
    np_ = lambda t: None if t is None else t.detach().float().cpu().numpy()
    full, ms, ds, iters, sim, R, Rb, loss = (np_(x) for x in (full, ms, ds, iters, sim, R, Rb, loss))
    for b, o in enumerate(d["oracle"]):
        n, m = int(d["nv"][b]), int(d["mv"][b])
        pp = ops.padded_width(n, m)
        t = (tag, b)
        assert np.array_equal(ms[b, :m], o["match_score"]), ("match_score", t)
        assert np.array_equal(ds[b, :m], o["det_score"]), ("det_score", t)
        assert int(iters[b]) == o["iters"], ("iters", t)
        assert np.array_equal(Rb[b, :m, :pp], np.asarray(o["Rb"]).reshape(m, pp)), ("Rb", t)
        if sim is not None:
            assert np.array_equal(sim[b, :m, :n], np.asarray(o["sim"]).reshape(m, n)), ("sim", t)
        if R is not None:
            assert np.array_equal(R[b, :m, :pp], np.asarray(o["R"]).reshape(m, pp)), ("R", t)
        if full is not None:
            if is_test:
                assert np.array_equal(full[b, :m], o["full_outmask"]), ("full_outmask", t)
            else:
                assert np.abs(full[b, :m] - o["full_outmask"]).max() <= 1e-5, ("full_outmask", t)
            assert not full[b, m:].any(), ("rows beyond the live templates", t)
        if loss is not None:                                         # the bound of the G21 fixture's test
            assert abs(float(loss[b]) - o["loss"]) <= 2e-7 * max(1.0, abs(o["loss"])), ("cost_loss", t, float(loss[b]), o["loss"])


def _check_hun(d, tag, Rb, ms, ds, status):
    from test_gpu_lsap import same_bits
    assert status.cpu().tolist() == [0] * len(d["oracle"]), tag
    for b, o in enumerate(d["oracle"]):
        n, m = int(d["nv"][b]), int(d["mv"][b])
        pp = ops.padded_width(n, m)
        R = torch.zeros(Rb.shape[1:])
        ms_e, ds_e = torch.zeros(ms.shape[1:]), torch.zeros(ds.shape[1:])
        Rh, mh, dh = (torch.from_numpy(x) for x in o["hun"])
        R[:m, :pp], ms_e[:m], ds_e[:m] = Rh, mh, dh
        assert same_bits(Rb[b].cpu(), R), ("Rb", tag, b)
        assert same_bits(ms[b].cpu(), ms_e, zero_sign_free=True) and same_bits(ds[b].cpu(), ds_e), ("scores", tag, b)


def run_case(case):
    """Every entry once on one case: outputs checked against the oracle; -> {entry: kernels enqueued by its call}."""
    br, sh, ragged, is_test, dt = case
    opts, D = next((o, dd) for name, o, dd in BRANCHES if name == br)
    B, N, M, H, W = SHAPES[sh]
    d = _case_inputs(sh, D, ragged, is_test, dt)
    g = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    pm, tm, tg = (g(d[k]).to(d["mdt"]) for k in ("pm", "tm", "tg"))
    pf, tf, sc = g(d["pf"]), g(d["tf"]), g(d["sc"])
    nv = g(d["nv"].astype(np.int32)) if ragged else None
    mv = g(d["mv"].astype(np.int32)) if ragged else None
    pp_, pt_ = ops.pack_masks(pm), ops.pack_masks(tm)
    L = _lib.load()
    Pp = ops.padded_width(N, M)
    f32 = dict(dtype=torch.float32, device=DEV)
    kw = dict(is_test=is_test, **KW)
    counts = {}
    tag = case_id(case)

    def counted(name, fn):
        torch.cuda.synchronize()
        c0 = L.dmm_launch_count()
        r = fn()
        counts[name] = int(L.dmm_launch_count() - c0)
        return r

    with _lib.options(**opts):
        # dmm_match_forward_ws twice on one workspace: the second call may find the tables the first one left zero
        ops._WS_STATE.clear()
        for name in ("forward", "forward_again"):
            full, ms, ds, iters, tb = counted(name, lambda: ops.match_forward(pm, tm, pf, tf, sc, n_valid=nv, m_valid=mv,
                                                                             return_tables=True, **kw))
            _check(d, is_test, (tag, name), full=full, ms=ms, ds=ds, iters=iters, sim=tb["sim"], R=tb["R"], Rb=tb["Rb"])

        full, ms, ds, iters = counted("forward_packed", lambda: ops.match_forward_packed(pm, pp_, tm, pf, tf, sc, nv, mv, **kw))
        # (this entry's Rb stays in its workspace: the mix it feeds is checked instead)
        for b, o in enumerate(d["oracle"]):
            m = int(d["mv"][b])
            assert np.array_equal(ms[b, :m].cpu().numpy(), o["match_score"]), (tag, "forward_packed", b)
            assert np.array_equal(ds[b, :m].cpu().numpy(), o["det_score"]) and int(iters[b]) == o["iters"]
            fo = full[b, :m].cpu().numpy()
            assert np.array_equal(fo, o["full_outmask"]) if is_test else np.abs(fo - o["full_outmask"]).max() <= 1e-5

        ws = torch.empty((int(L.dmm_workspace_bytes(B, N, M, D)),), dtype=torch.uint8, device=DEV)
        out = (torch.empty((B, M, Pp), **f32), torch.empty((B, M), **f32), torch.empty((B, M), **f32),
               torch.empty((B,), dtype=torch.int32, device=DEV))
        counted("solve_packed", lambda: ops.match_solve_packed(pp_, pt_, pf, tf, sc, nv, mv, H * W, out=out, workspace=ws, **kw))
        _check(d, is_test, (tag, "solve_packed"), ms=out[1], ds=out[2], iters=out[3], Rb=out[0])

        out = (torch.empty((B, M, Pp), **f32), torch.empty((B, M), **f32), torch.empty((B, M), **f32))
        st = torch.empty((B,), dtype=torch.int32, device=DEV)
        counted("solve_packed_hun", lambda: ops.match_solve_packed_hun(pp_, pt_, pf, tf, sc, nv, mv, H * W, score_weight=0.3,
                                                                       is_test=is_test, out=out, status=st, workspace=ws))
        _check_hun(d, (tag, "solve_packed_hun"), out[0], out[1], out[2], st)

        for targets in (tg, None):
            for want_tape in (True, False):
                name = f"train_{'targets' if targets is not None else 'notargets'}_{'tape' if want_tape else 'notape'}"
                r = counted(name, lambda: ops.match_train_forward(pm, tm, targets, pf, tf, sc, nv, mv, want_tape=want_tape, **kw))
                assert r is not None, (tag, name)
                full, ms, ds, loss, iters, saved, taped = r
                n_cs = B * M * N
                sim = saved[n_cs:2 * n_cs].view(B, M, N)
                Rb = saved[2 * n_cs:2 * n_cs + B * M * Pp].view(B, M, Pp)
                _check(d, is_test, (tag, name), full=full, ms=ms, ds=ds, iters=iters, sim=sim, Rb=Rb, loss=loss)
                assert (loss is None) == (targets is None) and (taped in (0, 1)) and (want_tape or not taped)
    return counts


def _expected(entry, case, recorded):
    """Kernels a call may enqueue, given what the commit before the shared front enqueued: the same number, except that
    the packed entries' normalise + cosine fallback went from two normalising launches to one."""
    br, sh, ragged, is_test, dt = case
    return recorded - (1 if entry in PACKED_ENTRIES and br in ("cosine_kernel1", "d64", "d48") else 0)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_entry_on_every_front_branch(case):
    with open(COUNTS_FILE) as f:
        recorded = json.load(f)[case_id(case)]
    counts = run_case(case)
    print(case_id(case), counts)
    assert set(counts) == set(recorded)
    for entry, n in counts.items():
        assert n == _expected(entry, case, recorded[entry]), (entry, n, recorded[entry])


def collect():
    """{case id: {entry: launches}} over all cases -- run against a build of the commit to record (``_lib.use_library``)."""
    return {case_id(c): run_case(c) for c in CASES}
