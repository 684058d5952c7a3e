"""fp64 references for the matching layer's backward kernels -- TEST INFRASTRUCTURE ONLY (no test functions here).

Written from ``oracle/torch_ref.py`` and DESIGN.md's description of the layer; plain torch on the CPU under autograd.

Solver side.  ``relax_matching`` is piecewise linear in ``sim``: relu gates, ``col_sum <= 1`` gates, two data-dependent exits,
the ``logic`` mask, the ``clamp(0, 1)`` branches and an argmax.  A float64 run that decided those for itself could take another
branch than the fp32 forward and then has another gradient altogether.  So the replay here DECIDES NOTHING: it takes

  * the greedy start from ``oracle.greedy_init``,
  * the executed iteration / sweep counts (``iters``, ``inner``) and every relu and column gate from the oracle's gate
    record (``oracle.relax(..., gates=)``),
  * ``logic``, the clamp branches and the argmax column of ``match_score`` from the oracle's fp32 ``R`` and the fp32 ``sim``,

and evaluates the linear pieces between them in float64.  The oracle's forward is what the device reproduces bit for bit
(the GPU tests check that per case before they look at a gradient), so these are exactly the branches the device's backward
differentiates through, whatever the summation order of the torch build that runs the test.

Feature side.  No gates beyond the eps clamp: autograd through ``x / max(||x||, 1e-8)`` with the clamp's VALUE taken as a
constant and its derivative that of ``||x||`` (what ``dmm_net_amd.backward._normalize_backward`` documents), the
``[M, D] x [D, N]`` cosine, ``(1 - w) * cos`` and, with targets, ``d_loss * mean((cos - gt)^2)`` over the live block.
"""
import numpy as np
import torch

import oracle

EPS = 1e-8


def padded_width(n, m):
    return n if n > m else m + 1


def _ulp_near(a, value):
    """Entries of fp32 ``a`` within one ulp of ``value`` (value itself included)."""
    v = np.float32(value)
    lo, hi = np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))
    return (a >= lo) & (a <= hi)


class SolverRecord:
    """The oracle's forward of one frame's table and everything the replay takes from it.

    sim32: the live [m, n] block, fp32.  Holds the padded table ``simp`` [m, Pp], the start ``idx``, ``iters``, ``inner``,
    the gates, ``R`` (fp32, [m, Pp]) and the head's branches for ``is_test``."""

    def __init__(self, sim32, max_iter, proj_iter, lr, is_test):
        sim32 = np.ascontiguousarray(sim32, np.float32)
        self.m, self.n = sim32.shape
        self.Pp = padded_width(self.n, self.m)
        self.simp = np.zeros((self.m, self.Pp), np.float32)
        self.simp[:, :self.n] = sim32
        C = -self.simp
        self.idx = oracle.greedy_init(C).astype(np.int64)
        self.gates = oracle.gate_record(self.m, self.Pp, max_iter, proj_iter)
        o = oracle.relax(C, max_iter, proj_iter, lr, gates=self.gates)
        self.R, self.iters, self.inner = o["R"], int(o["iters"]), [int(v) for v in o["inner"]]
        self.max_iter, self.proj_iter, self.is_test = int(max_iter), int(proj_iter), int(is_test)
        self.lr = float(np.float32(lr))                       # the fp32 scalar the solver multiplies with
        R = self.R
        self.logic = (R == R.max(1, keepdims=True)) if is_test else (R > np.float32(0.01))
        self.clamp_pass = (R >= 0) & (R <= 1)                 # torch.clamp's backward passes on the closed interval
        self.clamp_const = np.clip(R, 0, 1)
        self.argmax = np.argmax(self.clamp_const * self.simp, axis=1)      # first maximal column, fp32 products
        self.outer_exit = self.iters < self.max_iter
        self.inner_exit = any(s < self.proj_iter for s in self.inner)

    def near_kink(self):
        """Does this frame sit on a kink of the reference itself: an ``R`` entry within one ulp of the 0.01 threshold
        (training mode), or the ``match_score`` entry within one ulp of a clamp bound while ``R`` depends on ``sim``."""
        if self.iters == 0:
            return False                                      # R is the constant one-hot start: nothing to differentiate
        k = bool(_ulp_near(self.R, 0.01).any()) if not self.is_test else False
        ra = self.R[np.arange(self.m), self.argmax]
        return k or bool((_ulp_near(ra, 0.0) | _ulp_near(ra, 1.0)).any())


def replay(sim_t, rec):
    """The solver + head on ``sim_t`` ([m, n] torch tensor carrying the graph, any float dtype) along ``rec``'s branches.
    -> R [m, Pp], Rb [m, Pp], match_score [m], det_score needs the scores: see ``solver_objective``."""
    dt = sim_t.dtype
    m, n, Pp = rec.m, rec.n, rec.Pp
    s = torch.cat([sim_t, sim_t.new_zeros((m, Pp - n))], 1) if Pp > n else sim_t
    C = -s
    X = torch.zeros((m, Pp), dtype=dt)
    X[torch.arange(m), torch.from_numpy(rec.idx)] = 1.0
    xs = [X]
    P0 = P1 = P2 = torch.zeros((m, Pp), dtype=dt)
    relu, col = rec.gates["relu"], rec.gates["col"]
    for it in range(rec.iters):
        X = X - rec.lr * C
        xs.append(X)
        for j in range(rec.inner[it]):
            X = X + P0
            Y = X * torch.from_numpy(relu[it, j]).to(dt)
            P0 = X - Y
            X = Y + P1
            cs = X.sum(0, keepdim=True)
            Y = torch.where(torch.from_numpy(col[it, j]).bool()[None, :], X, X - (cs - 1) / m)
            P1 = X - Y
            X = Y + P2
            Y = X - (X.sum(1, keepdim=True) - 1) / Pp
            P2 = X - Y
            X = Y
    R = torch.stack(xs, 0).mean(0)
    Rb = R * torch.from_numpy(rec.logic).to(dt)
    Rc = torch.where(torch.from_numpy(rec.clamp_pass), R, torch.from_numpy(rec.clamp_const).to(dt))
    ms = (Rc * s).gather(1, torch.from_numpy(rec.argmax)[:, None])[:, 0]
    return R, Rb, ms


def solver_objective(sim_t, rec, score, dRb, dms, dds):
    """sum(Rb * dRb) + sum(ms * dms) + sum(ds * dds) along ``rec``; score [n], dRb [m, Pp], dms / dds [m] (numpy or None)."""
    dt = sim_t.dtype
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
    R, Rb, ms = replay(sim_t, rec)
    sc = torch.zeros((rec.Pp,), dtype=dt)
    sc[:rec.n] = t(score)
    ds = (sc[None, :] * Rb).sum(1)
    obj = sim_t.new_zeros(())
    if dRb is not None:
        obj = obj + (Rb * t(dRb)).sum()
    if dms is not None:
        obj = obj + (ms * t(dms)).sum()
    if dds is not None:
        obj = obj + (ds * t(dds)).sum()
    return obj, R, Rb, ms, ds


def solver_grad(rec, score, dRb, dms, dds, dtype=torch.float64):
    """d objective / d sim over the live [m, n] block (numpy float64) -- the padded columns' gradient is dropped, as the
    layer drops it.  ``dtype=torch.float32``: the same replay in fp32, the measure of a correct fp32 evaluation's error."""
    sim_t = torch.from_numpy(rec.simp[:, :rec.n].copy()).to(dtype).requires_grad_(True)
    obj, R, _, _, _ = solver_objective(sim_t, rec, score, dRb, dms, dds)
    if not obj.requires_grad:
        return np.zeros((rec.m, rec.n)), R.detach().numpy()
    obj.backward()
    return sim_t.grad.double().numpy(), R.detach().numpy()


def fp32_replay_R(rec):
    """fp32 NumPy replay of the solver along the record, with no comparison of its own -> R [m, Pp] fp32 (proves that the
    record is complete and indexed correctly: it must reproduce the oracle's R to rounding)."""
    f = np.float32
    m, Pp = rec.m, rec.Pp
    C = -rec.simp
    X = np.zeros((m, Pp), f)
    X[np.arange(m), rec.idx] = 1
    acc = X.copy()
    P0, P1, P2 = np.zeros((m, Pp), f), np.zeros((m, Pp), f), np.zeros((m, Pp), f)
    for it in range(rec.iters):
        X = X - f(rec.lr) * C
        acc = acc + X
        for j in range(rec.inner[it]):
            X = X + P0
            Y = X * rec.gates["relu"][it, j].astype(f)
            P0 = X - Y
            X = Y + P1
            cs = X.sum(0, keepdims=True, dtype=f)
            g = rec.gates["col"][it, j].astype(f)[None, :]
            Y = X * g + (1 - g) * (X - (cs - f(1)) / f(m))
            P1 = X - Y
            X = Y + P2
            Y = X - (X.sum(1, keepdims=True, dtype=f) - f(1)) / f(Pp)
            P2 = X - Y
            X = Y
    return acc / f(rec.iters + 1)


# ---------------------------------------------------------------------------------------------------------------------
# feature side
# ---------------------------------------------------------------------------------------------------------------------
def normalize(x):
    """x [..., D] -> x / c, c = max(||x||, eps) in value and ||x|| in derivative (a zero row: derivative of the norm 0)."""
    n = torch.linalg.vector_norm(x, dim=-1, keepdim=True)
    c = n + (n.clamp_min(EPS) - n).detach()
    return x / c


def cosine(feat_t, feat_p):
    """feat_t [B, M, D], feat_p [B, N, D] -> cos [B, M, N]."""
    return torch.einsum("bmd,bnd->bmn", normalize(feat_t), normalize(feat_p))


def feature_grads(feat_t, feat_p, dsim, score_weight, gt=None, d_loss=None, n_valid=None, m_valid=None):
    """float64 autograd of  sum(dsim * (1 - w) * cos) + sum_b d_loss[b] * mean_live((cos - gt)^2)  over every frame's live
    block -> (g_feat_t [B, M, D], g_feat_p [B, N, D]) numpy float64.  All arguments numpy; w as the layer rounds it."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    ft, fp = t(feat_t).requires_grad_(True), t(feat_p).requires_grad_(True)
    B, M, _ = ft.shape
    N = fp.shape[1]
    nv = np.full(B, N) if n_valid is None else np.asarray(n_valid)
    mv = np.full(B, M) if m_valid is None else np.asarray(m_valid)
    live = torch.zeros((B, M, N), dtype=torch.float64)
    for b in range(B):
        if nv[b] > 0 and mv[b] > 0:
            live[b, :mv[b], :nv[b]] = 1.0
    w_feat = float(np.float32(1.0 - float(score_weight)))
    cos = cosine(ft, fp)
    obj = (t(dsim) * w_feat * cos * live).sum()
    if gt is not None and d_loss is not None:
        cnt = torch.from_numpy(np.maximum(nv * mv, 1).astype(np.float64))
        obj = obj + (t(d_loss) * (((cos - t(gt)) ** 2) * live).sum((1, 2)) / cnt).sum()
    if not obj.requires_grad:
        return np.zeros(ft.shape), np.zeros(fp.shape)
    obj.backward()
    return ft.grad.numpy(), fp.grad.numpy()


# ---------------------------------------------------------------------------------------------------------------------
# the solver cases (shared by the GPU test and the CPU test that guards this reference)
# ---------------------------------------------------------------------------------------------------------------------
def _case(cls, M, N, B=2, max_iter=10, proj_iter=5, lr=0.1, seed=0, kind="uniform", nv=None, mv=None, opts=None):
    tag = f"{cls}/M{M}_N{N}_{max_iter}x{proj_iter}_lr{lr}" + ("_" + "_".join(f"{k}{v}" for k, v in opts.items()) if opts else "")
    return dict(cls=cls, tag=tag, M=M, N=N, B=B, max_iter=max_iter, proj_iter=proj_iter, lr=lr, seed=seed, kind=kind, nv=nv,
                mv=mv, opts=opts or {})


def _ragged(cls, M, N):
    # a full frame, a half frame, a one-proposal frame, a frame without templates, a frame without proposals
    return _case(cls, M, N, B=5, nv=[N, N // 2, 1, N, 0], mv=[M, M // 2, M, 0, M])


def max_tape_outer():
    """``kMaxTapeOuter`` of dmm_solve.hip: more outer iterations than this go to the general backward."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "dmm_net_amd", "csrc", "dmm_solve.hip")) as fh:
        return int(re.search(r"constexpr\s+int\s+kMaxTapeOuter\s*=\s*(\d+)\s*;", fh.read()).group(1))


def case_max_iter(case):
    return max_tape_outer() + 1 if case["max_iter"] == "above_tape" else case["max_iter"]

SOLVER_CASES = (
    # every exact-row instantiation, and the forward's width-class ends
    [_case("exact", M, 40) for M in range(1, 17)]
    + [_case("exact", M, N) for N in (33, 55) for M in (1, 5, 8, 9, 16)]
    # guarded rows
    + [_case("guarded", M, N) for M in (17, 20, 21, 32) for N in (40, 64)]
    # more than one wave of columns: the issue's five, then one shape for each (MT, NG) pair those do not reach
    + [_case("waves", M, N) for M, N in ((3, 65), (8, 128), (16, 200), (32, 256), (10, 129))]
    + [_case("waves", M, N) for M, N in ((12, 100), (20, 128), (5, 200), (20, 200))]
    # N <= M: the table is padded to M + 1 zero columns
    + [_case("padded", M, N) for N, M in ((3, 5), (1, 1), (5, 5), (1, 4), (16, 16), (31, 32))]
    # ragged batches: the ragged kernel (M <= 8, one wave), the guarded dense route at one wave and at two
    + [_ragged("ragged", 8, 50), _ragged("ragged", 12, 40), _ragged("ragged", 12, 100)]
    # the general backward: outside the envelope, forced inside it, more outer iterations than the tape index holds
    + [_case("general", M, N) for N, M in ((257, 3), (64, 33), (130, 40))]
    + [_case("general", M, N, opts={"FORCE_WIDE": 1}) for N, M in ((50, 10), (7, 16))]
    + [_case("general", 5, 50, max_iter="above_tape")]
    # settings; sim mixed from a cosine and integer count tables as relax_match builds it
    + [_case("settings", 5, 40, max_iter=mi, proj_iter=pi, kind="mixed") for pi in (1, 5) for mi in (0, 1, 20)]
    + [_case("settings", M, N, lr=0.5, kind="mixed") for M, N in ((5, 40), (12, 50), (20, 64))]
    # early exits (40 x 5): one dominant entry per row in distinct columns over a background of `kind`'s level
    + [_case("exits", M, N, B=3, max_iter=40, kind=kind) for M, N, kind in
       ((3, 10, "dominant0.05"), (5, 40, "dominant0.0"), (8, 50, "dominant0.0"), (1, 4, "dominant0.0"),
        (1, 40, "dominant0.0"), (2, 5, "dominant0.0"))]
)


def case_inputs(case):
    """-> dict(sim [B, M, N] fp32 or the parts it is mixed from, score [B, N], dRb [B, M, Pp], dms, dds [B, M]) numpy."""
    B, M, N = case["B"], case["M"], case["N"]
    Pp = padded_width(N, M)
    r = np.random.default_rng(1000 + 97 * M + N + 7919 * case["seed"])
    f = np.float32
    out = dict(score=r.random((B, N)).astype(f), dRb=r.standard_normal((B, M, Pp)).astype(f),
               dms=r.standard_normal((B, M)).astype(f), dds=r.standard_normal((B, M)).astype(f))
    kind = case["kind"]
    if case["nv"] is not None:
        out["nv"], out["mv"] = np.asarray(case["nv"], np.int32), np.asarray(case["mv"], np.int32)
    if kind == "uniform":
        out["sim"] = r.random((B, M, N)).astype(f)
    elif kind == "mixed":                                     # cos and IoU counts; the device mixes them (score_weight 0.3)
        out["cos"] = (2 * r.random((B, M, N)) - 1).astype(f)
        ap, at = r.integers(1, 200, (B, N)), r.integers(1, 200, (B, M))
        inter = (r.random((B, M, N)) * np.minimum(ap[:, None, :], at[:, :, None])).astype(np.int32)
        out.update(area_p=ap.astype(np.int32), area_t=at.astype(np.int32), inter=inter)
    else:
        bg = float(kind[len("dominant"):])
        sim = (bg * r.random((B, M, N))).astype(f)
        for b in range(B):
            cols = r.permutation(N)[:M]
            sim[b, np.arange(M), cols] = (0.8 + 0.2 * r.random(M)).astype(f)
        out["sim"] = sim
    return out


def mixed_sim(inp, score_weight=0.3):
    """The fp32 table ``relax_match`` forms from ``case_inputs``' parts: the oracle's IoU, then a = cos * (1 - w),
    b = iou * w, a + b, each rounded once."""
    f = np.float32
    w1, w2 = f(1.0 - float(score_weight)), f(score_weight)
    sim = np.empty(inp["cos"].shape, f)
    for b in range(sim.shape[0]):
        iou = oracle.iou_from_counts(inp["inter"][b], inp["area_p"][b], inp["area_t"][b])
        sim[b] = inp["cos"][b] * w1 + iou * w2
    return sim


def case_frames(case, inp=None):
    """-> (inputs, sim [B, M, N] fp32, [(b, m, n)] of the live frames, [b] of the dead ones)."""
    inp = case_inputs(case) if inp is None else inp
    sim = inp["sim"] if "sim" in inp else mixed_sim(inp)
    B, M, N = sim.shape
    live, dead = [], []
    for b in range(B):
        m, n = (M, N) if case["nv"] is None else (int(case["mv"][b]), int(case["nv"][b]))
        (live if m > 0 and n > 0 else dead).append((b, m, n))
    return inp, sim, live, dead


def frame_reference(case, inp, sim, b, m, n, is_test, dtype=torch.float64):
    """-> (record, d sim [m, n] float64) of frame b's live block."""
    pp = padded_width(n, m)
    rec = SolverRecord(sim[b, :m, :n], case_max_iter(case), case["proj_iter"], case["lr"], is_test)
    g, _ = solver_grad(rec, inp["score"][b, :n], inp["dRb"][b, :m, :pp], inp["dms"][b, :m], inp["dds"][b, :m], dtype)
    return rec, g
