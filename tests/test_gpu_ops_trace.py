"""What every wrapper of dmm_net_amd/ops.py hands to the C ABI: for each wrapper call the ordered list of entries and their
arguments, against tests/golden/ops_call_trace.json -- recorded with ``collect()`` below against the ops.py of the commit
BEFORE its plane, table, workspace and launch code was written once.  Equality cell by cell: no tolerance, no exclusions.

``_lib.call`` is replaced by a recorder that delegates to the real one.  Per call: the entry, whether a device guard was asked
for, and per argument (told apart by the argtypes ``_lib`` parsed from include/dmm_match.h) an integer or float by value, a
pointer as ``null`` or as ``<name>+<byte offset>`` when the address lies inside a tensor the case knows by name (its inputs,
a ``ForwardPlan``'s buffers, the cached workspaces, what the wrapper returned) and ``other`` when not -- a copy made by
``.contiguous()`` shows up as ``other`` -- a ``byref`` note with the value it carried in, and the stream as current or side.
The results themselves are held to the oracle by the suites around this one; nothing here reads them."""
import json
import os
import re

import pytest
import torch

from dmm_net_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, N, M, H, W, D = 2, 6, 3, 12, 20, 64
KW = dict(score_weight=0.3, max_iter=10, proj_iter=5, lr=0.1, is_test=1)
TRACE_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops_call_trace.json")
_INT_TYPES = tuple(t for k, t in _lib._CTYPES.items() if k not in ("float", "dmm_stream_t"))


def _stream_params():
    """{entry: index of its dmm_stream_t parameter}, from the header."""
    with open(_lib.HEADER) as f:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
    text = re.sub(r"^\s*#[^\n]*", "", text, flags=re.M)
    out = {}
    for fn, params in re.findall(r"\bDMM_API\s+[^;(]*?\s*\b(dmm_\w+)\s*\(([^)]*)\)\s*;", text):
        out[fn] = next((i for i, p in enumerate(params.split(",")) if "dmm_stream_t" in p), None)
    return out


_STREAM_AT = _stream_params()


def _extent(t):
    """Bytes from a tensor's first element to one past its last."""
    if t.numel() == 0:
        return 0
    return (sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1) * t.element_size()


def _named(prefix, x, out):
    """Every tensor inside a wrapper's result (tensor, tuple, dict), by a name of its place in it."""
    if torch.is_tensor(x):
        out.setdefault(prefix, x)
    elif isinstance(x, dict):
        for k, v in x.items():
            _named(f"{prefix}.{k}", v, out)
    elif isinstance(x, (tuple, list)):
        for i, v in enumerate(x):
            _named(f"{prefix}[{i}]", v, out)


class Recorder:
    """``_lib.call`` that notes what it is given, then makes the call."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __call__(self, name, device, *args, allow=()):
        argtypes = _lib._DECLS[name][1]
        assert len(args) == len(argtypes), (name, len(args), len(argtypes))
        current = torch.cuda.current_stream(DEV).cuda_stream
        cells = []
        for i, (a, ty) in enumerate(zip(args, argtypes)):
            if i == _STREAM_AT[name]:
                cells.append("stream:current" if (a or 0) == current else "stream:side")
            elif ty in _INT_TYPES:
                cells.append(int(a))
            elif ty is _lib._CTYPES["float"]:
                cells.append(float(a))
            elif a is None:
                cells.append("null")
            elif isinstance(a, int):
                cells.append(("ptr", a))                             # named once the wrapper has returned
            else:                                                    # ctypes.byref(c_int): the note, with what it says now
                cells.append(f"byref({a._obj.value})")
        self.calls.append({"entry": name, "guard": device is not None, "args": cells})
        return self.real(name, device, *args, allow=allow)

    def take(self, env):
        """The calls since the last ``take``, their pointers named from ``env`` ({name: tensor}, first match wins)."""
        spans = [(k, t.data_ptr(), _extent(t)) for k, t in env.items()]

        def label(addr):
            return next((f"{k}+{addr - p}" for k, p, n in spans if p <= addr < p + n), "other")
        calls, self.calls = self.calls, []
        for c in calls:
            c["args"] = [label(a[1]) if isinstance(a, tuple) else a for a in c["args"]]
        return calls


def _inputs(ragged, B=B, N=N, M=M, D=D, dtype=torch.float32, layout="tensor"):
    """The named device tensors of one case.  ``layout`` of the plane tensors: "tensor" (contiguous), "alloc"
    (``alloc_planes``: plane stride rounded up, passed as it is), "slice" (a slice along the batch and plane axes of a larger
    tensor, passed as it is), "wT" (a W-transposed view: copied)."""
    g = torch.Generator().manual_seed(100 * N + M)
    r = lambda *s: torch.rand(s, generator=g)

    def planes(K):
        x = r(B, K, H, W).to(dtype)
        if layout == "alloc":
            y = ops.alloc_planes(B, K, H, W, dtype, DEV)
            y.copy_(x)
            return y
        if layout == "wT":
            return x.transpose(2, 3).contiguous().to(DEV).transpose(2, 3)
        if layout == "slice":
            big = torch.zeros((B + 1, K + 2, H, W), dtype=dtype, device=DEV)
            big[1:, 1:K + 1] = x.to(DEV)
            return big[1:, 1:K + 1]
        return x.to(DEV)
    env = dict(pm=planes(N), tm=planes(M), tg=planes(M))
    env.update(pf=(r(B, N, D) - 0.5).to(DEV), tf=(r(B, M, D) - 0.5).to(DEV), sc=r(B, N).to(DEV))
    Pp = ops.padded_width(N, M)
    env.update(Rb=r(B, M, Pp).to(DEV), cos=r(B, M, N).to(DEV), dout=r(B, M, H, W).to(DEV), dRb=r(B, M, Pp).to(DEV),
               dms=r(B, M).to(DEV), dds=r(B, M).to(DEV), gt=r(B, M, N).to(DEV), dloss=r(B).to(DEV))
    env["nv"] = torch.tensor([N - 2 * (b % 2) for b in range(B)], dtype=torch.int32, device=DEV) if ragged else None
    env["mv"] = torch.tensor([M - (b % 2) for b in range(B)], dtype=torch.int32, device=DEV) if ragged else None
    return env


def _frames(env):
    """The proposal planes as a ``FramePlanes`` of 6 and 4 planes (its counts are the case's n_valid)."""
    env["frame0"], env["frame1"] = env["pm"][0].clone(), env["pm"][1, :4].clone()
    fp = ops.FramePlanes([env["frame0"], env["frame1"]])
    env["fp.table"], env["nv"] = fp.table, fp.n_valid()
    return fp


def _one(env):
    """Frame 0 of every input without the batch axis (the ``one_frame`` forms), layout kept."""
    for k, v in list(env.items()):
        if v is not None:
            env[k] = v[0] if k in ("pm", "tm", "tg") else (v[:1] if k in ("nv", "mv") else v[0].contiguous())
    return env


# ---- the cases: name -> function(ragged) -> (env, [(step name, function(env) -> result)]) ------------------------------
CASES = {}


def case(name, **kw):
    def deco(fn):
        CASES[name] = (fn, kw)
        return fn
    return deco


def _vm(e):
    return dict(n_valid=e["nv"], m_valid=e["mv"])


def _plane_cases(name, layouts, steps):
    """One case per layout of the plane inputs; ``steps(p)`` with p(env) -> the proposal planes argument."""
    for layout in layouts:
        def build(ragged, layout=layout):
            env = _inputs(ragged, layout="tensor" if layout == "frames" else layout)
            fp = _frames(env) if layout == "frames" else None
            return env, steps((lambda e: fp) if fp is not None else (lambda e: e["pm"]))
        CASES[f"{name}/{layout}"] = (build, {})


TENSORS = ("tensor", "alloc", "slice", "wT")
ALL = TENSORS + ("frames",)
_plane_cases("iou_counts", ALL, lambda p: [("r", lambda e: ops.iou_counts(p(e), e["tm"], e["nv"], e["mv"]))])
_plane_cases("iou_counts_dual", ALL, lambda p: [("r", lambda e: ops.iou_counts_dual(p(e), e["tm"], e["tg"], e["nv"], e["mv"]))])
_plane_cases("mask_mix", ALL, lambda p: [
    ("r", lambda e: ops.mask_mix(e["Rb"], p(e), e["nv"], e["mv"])),
    ("shared", lambda e: ops.mask_mix(e["Rb"], p(e), e["nv"], e["mv"], shared=True)),
    ("no_n_valid", lambda e: ops.mask_mix(e["Rb"], p(e), None, e["mv"]))])
_plane_cases("mask_mix_bwd", ALL, lambda p: [
    ("r", lambda e: ops.mask_mix_bwd(e["Rb"], p(e), e["dout"], e["nv"], e["mv"], det=False)),
    ("det", lambda e: ops.mask_mix_bwd(e["Rb"], p(e), e["dout"], e["nv"], e["mv"], det=True)),
    ("no_n_valid", lambda e: ops.mask_mix_bwd(e["Rb"], p(e), e["dout"], None, e["mv"], det=False))])


def _train_steps(p, one_frame=False, targets=True, **more):
    kw = dict(KW, is_test=0, one_frame=one_frame)

    def fwd(e):
        r = ops.match_train_forward(p(e), e["tm"], e["tg"] if targets else None, e["pf"], e["tf"], e["sc"], e["nv"], e["mv"],
                                    **kw, **more)
        e["_taped"] = r[6]
        return r

    def bwd(e, det=False):
        return ops.match_train_backward(p(e), e["pf"], e["tf"], e["sc"], e["fwd[5]"], targets, e["dout"], e["dms"], e["dds"],
                                        e["dloss"] if targets else None, e["nv"], e["mv"], e["tm"].shape[-3], **kw,
                                        iters=e["fwd[4]"], taped=e["_taped"], det=det)
    return [("fwd", fwd), ("bwd", bwd), ("bwd_det", lambda e: bwd(e, det=True)),
            ("bwd_untaped", lambda e: ops.match_train_backward(p(e), e["pf"], e["tf"], e["sc"], e["fwd[5]"], targets, e["dout"], None,
                                                               None, None, e["nv"], e["mv"], e["tm"].shape[-3], **kw, det=False))]


_plane_cases("match_train", ALL, _train_steps)
_plane_cases("match_train_notargets_notape", ("tensor",), lambda p: _train_steps(p, targets=False, want_tape=False)[:2])
for _layout in TENSORS:
    for _tg in (True, False):
        CASES[f"match_train_one_frame/{'targets' if _tg else 'notargets'}/{_layout}"] = (
            lambda ragged, l=_layout, t=_tg: (_one(_inputs(ragged, layout=l)), _train_steps(lambda e: e["pm"], True, t)), {})

_fwd_args = lambda e: (e["pm"], e["tm"], e["pf"], e["tf"], e["sc"])
_plane_cases("match_forward", TENSORS, lambda p: [
    ("r", lambda e: ops.match_forward(*_fwd_args(e), **KW, **_vm(e))),
    ("tables", lambda e: ops.match_forward(*_fwd_args(e), **KW, **_vm(e), return_tables=True))])
for _layout in TENSORS:
    CASES[f"match_forward_frame/{_layout}"] = (lambda ragged, l=_layout: (_one(_inputs(False, layout=l)), [
        ("r", lambda e: ops.match_forward_frame(*_fwd_args(e), **KW)),
        ("again", lambda e: ops.match_forward_frame(*_fwd_args(e), **KW))]), {"dense_only": True})


@case("match_forward/note_kept_then_reset")
def _(ragged):
    env = _inputs(ragged, D=512)                 # (D = 512: dense frames take the launch that leaves the note at "tables zero")
    other = {k + "2": v for k, v in _inputs(ragged, N=5, M=2, D=512).items()}
    env.update(other)
    second = lambda e: ops.match_forward(e["pm2"], e["tm2"], e["pf2"], e["tf2"], e["sc2"], **KW, n_valid=e["nv2"], m_valid=e["mv2"])
    first = lambda e: ops.match_forward(*_fwd_args(e), **KW, **_vm(e))
    return env, [("first", first), ("again", first), ("other_shape", second), ("back", first)]


@case("match_forward/capture_latches")
def _(ragged):
    side = torch.cuda.Stream(DEV)

    def on_side(fn, capture=False):
        def run(e):
            side.wait_stream(torch.cuda.current_stream(DEV))
            with torch.cuda.stream(side):
                if capture:
                    e["_graph"] = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(e["_graph"], stream=side):
                        r = fn(e)
                else:
                    r = fn(e)
            torch.cuda.current_stream(DEV).wait_stream(side)
            return r
        return run
    first = lambda e: ops.match_forward(*_fwd_args(e), **KW, **_vm(e))
    frame = lambda e: ops.match_forward_frame(e["pm"][0], e["tm"][0], e["pf"][0], e["tf"][0], e["sc"][0], **KW)
    return _inputs(ragged, D=512), [("warm", on_side(first)), ("captured", on_side(first, True)), ("after", on_side(first)),
                             ("frame_after", on_side(frame))]


def _packed(e):
    e["pp"], e["pt"] = ops.pack_masks(e["pm"]), ops.pack_masks(e["tm"])
    return e


_plane_cases("pack_masks", TENSORS, lambda p: [
    ("r", lambda e: ops.pack_masks(e["pm"])), ("plane_slice", lambda e: ops.pack_masks(e["pm"][:, 1:]))])
_plane_cases("match_forward_packed", ("tensor", "alloc", "wT"),  # (the entry wants one template plane stride over the batch)
             lambda p: [
    ("pack", lambda e: ops.pack_masks(e["pm"])),
    ("r", lambda e: ops.match_forward_packed(e["pm"], e["pack"], e["tm"], e["pf"], e["tf"], e["sc"], e["nv"], e["mv"], **KW)),
    ("again", lambda e: ops.match_forward_packed(e["pm"], e["pack"], e["tm"], e["pf"], e["tf"], e["sc"], e["nv"], e["mv"], **KW)),
    ("own", lambda e: ops.match_forward_packed(e["pm"], e["pack"], e["tm"], e["pf"], e["tf"], e["sc"], e["nv"], e["mv"], **KW,
                                               out=tuple(e[f"r[{i}]"] for i in range(4)), workspace=e["ws"]))])


@case("iou_counts_packed")
def _(ragged):
    return _packed(_inputs(ragged)), [("r", lambda e: ops.iou_counts_packed(e["pp"], e["pt"], H * W, e["nv"], e["mv"]))]


@case("match_solve_packed")
def _(ragged):
    e = _packed(_inputs(ragged))
    f32 = dict(dtype=torch.float32, device=DEV)
    e["o0"], e["o1"], e["o2"] = torch.empty((B, M, ops.padded_width(N, M)), **f32), torch.empty((B, M), **f32), torch.empty((B, M), **f32)
    e["o3"], e["st"] = torch.empty((B,), dtype=torch.int32, device=DEV), torch.empty((B,), dtype=torch.int32, device=DEV)
    args = lambda e: (e["pp"], e["pt"], e["pf"], e["tf"], e["sc"], e["nv"], e["mv"], H * W)
    return e, [("relax", lambda e: ops.match_solve_packed(*args(e), **KW, out=(e["o0"], e["o1"], e["o2"], e["o3"]), workspace=e["ws"])),
               ("hun", lambda e: ops.match_solve_packed_hun(*args(e), score_weight=0.3, is_test=1, out=(e["o0"], e["o1"], e["o2"]),
                                                            status=e["st"], workspace=e["ws"]))]


@case("ragged_pad")
def _(ragged):
    e = _inputs(ragged)
    e["b0"], e["b1"], e["cnt"] = e["pf"][0, :4].clone(), e["pf"][1, :3].clone(), torch.tensor([4, 3], dtype=torch.int32, device=DEV)
    e["b1T"] = e["pf"][1, :3].t().contiguous().t()                       # a block that has to be copied

    def with_table(e):
        blocks, addrs = ops.ragged_blocks([e["b0"], e["b1"]])
        e["tab"] = _lib.small_to_device(addrs, torch.int64, DEV)
        return ops.ragged_pad(blocks, 5, e["cnt"], e["tab"])
    return e, [("r", lambda e: ops.ragged_pad([e["b0"], e["b1"]], 5, e["cnt"])),
               ("copied", lambda e: ops.ragged_pad([e["b0"], e["b1T"]], 5, e["cnt"])), ("table", with_table)]


@case("features")
def _(ragged):
    e = _inputs(ragged)
    e.update({k + "48": v for k, v in _inputs(ragged, D=48).items() if k in ("pf", "tf")})
    return e, [("normalize", lambda e: ops.feature_normalize(e["pf"])),
               ("norms_t", lambda e: ops.feature_normalize(e["tf"], want_norms=True)),
               ("norms_p", lambda e: ops.feature_normalize(e["pf"], want_norms=True)),
               ("normalize_copy", lambda e: ops.feature_normalize(e["pf"].transpose(0, 1))),
               ("cosine", lambda e: ops.cosine(e["norms_t[0]"], e["norms_p[0]"], e["nv"], e["mv"])),
               ("cosine_features", lambda e: ops.cosine_features(e["tf"], e["pf"])),
               ("cosine_features_d48", lambda e: ops.cosine_features(e["tf48"], e["pf48"])),
               ("sim_bwd", lambda e: ops.feature_sim_bwd(e["dRb"][:, :, :N], e["cosine"], e["gt"], e["dloss"], 0.3, e["tf"], e["pf"],
                                                          e["norms_t[0]"], e["norms_p[0]"], e["norms_t[1]"], e["norms_p[1]"],
                                                          e["nv"], e["mv"])),
               ("sim_bwd_noloss", lambda e: ops.feature_sim_bwd(e["gt"], e["cosine"], None, None, 0.3, e["tf"], e["pf"],
                                                                 e["norms_t[0]"], e["norms_p[0]"], e["norms_t[1]"], e["norms_p[1]"],
                                                                 e["nv"], e["mv"]))]


def _solver_steps(e_):
    counts = lambda e: (e["cos"], e["counts[0]"], e["counts[1]"], e["counts[2]"], e["sc"])
    kw = {k: v for k, v in KW.items() if k != "score_weight"}
    return [("counts", lambda e: ops.iou_counts(e["pm"], e["tm"], e["nv"], e["mv"])),
            ("relax", lambda e: ops.relax_match(*counts(e), **KW, **_vm(e))),
            ("relax_x", lambda e: ops.relax_match(*counts(e), **KW, **_vm(e), want_x=True)),
            ("relax_f16", lambda e: ops.relax_match(*counts(e), **KW, **_vm(e), state="f16")),
            ("relax_bwd", lambda e: ops.relax_match_bwd(e["relax.sim"], e["sc"], e["dRb"], e["dms"], e["dds"], **kw, **_vm(e))),
            ("relax_bwd_dRb_only", lambda e: ops.relax_match_bwd(e["relax.sim"], e["sc"], e["dRb"], None, None, **kw, **_vm(e))),
            ("hungarian", lambda e: ops.hungarian_match(*counts(e), score_weight=0.3, is_test=1, **_vm(e))),
            ("solve", lambda e: ops.relax_solve(e["cos"], 10, 5, 0.1, e["mv"], e["nv"])),
            ("lsap", lambda e: ops.linear_sum_assignment(e["cos"], e["mv"], e["nv"])),
            ("lsap_tall_max", lambda e: ops.linear_sum_assignment(e["cos"].transpose(1, 2), e["nv"], e["mv"], maximize=True))]


@case("solvers")
def _(ragged):
    e = _inputs(ragged)
    return e, _solver_steps(e)


@case("relax_match/wide_40x33")
def _(ragged):
    e = _inputs(ragged, N=40, M=33)
    return e, _solver_steps(e)[:2]


# ---- ForwardPlan ---------------------------------------------------------------------------------------------------
_PLAN_BUFFERS = ("full_outmask", "match_score", "det_score", "iters", "sim", "R", "Rb", "workspace", "pn", "tn", "cos")


def _plan_case(name, calls=1, B=B, D=D, dtype=torch.float32, layouts=("tensor",), **plan_kw):
    for layout in layouts:
        def build(ragged, layout=layout):
            e = _inputs(ragged, B=B, D=D, dtype=dtype, layout=layout)
            plan = ops.ForwardPlan(B, N, M, H, W, D, DEV, mask_dtype=dtype, **plan_kw)
            for k in _PLAN_BUFFERS:
                if getattr(plan, k, None) is not None:
                    e["plan." + k] = getattr(plan, k)
            for i, c in enumerate(getattr(plan, "counts", [])):
                e[f"plan.counts[{i}]"] = c
            run = lambda e: plan.run(*_fwd_args(e), **KW, **_vm(e))
            return e, [(f"call{i + 1}", run) for i in range(calls)]
        CASES[f"plan/{name}" + (f"/{layout}" if len(layouts) > 1 else "")] = (build, {})


_plan_case("single", calls=2, layouts=TENSORS, pipeline=False)
_plan_case("single_tables", pipeline=False, want_tables=True)
_plan_case("time_kernels", pipeline=False, time_kernels=True)
_plan_case("f16_solver", pipeline=False, solver_state="f16")
_plan_case("out_f16_aligned", dtype=torch.float16, pipeline=False, out_dtype=torch.float16, out_plane_align=128)
_plan_case("pipeline_2_parts", B=5, layouts=("tensor", "alloc"), pipeline=True, parts=2, split=0.5, want_tables=True)
_plan_case("pipeline_3_parts", B=5, pipeline=True, parts=3)
_plan_case("graph", calls=3, pipeline=False, graph=True)
_plan_case("graph_fork", calls=3, pipeline=False, graph=True, graph_fork=True)
_plan_case("single_d512", calls=3, D=512, pipeline=False)              # (D = 512: the plan's note moves, see above)
_plan_case("graph_d512", calls=4, D=512, pipeline=False, graph=True)

CASE_IDS = [f"{name}/{'ragged' if r else 'dense'}" for name, (_, kw) in CASES.items() for r in (0, 1)
            if not (r and kw.get("dense_only"))]


def run_case(case_id):
    """One case from empty caches -> {step: [calls]}."""
    name, _, kind = case_id.rpartition("/")
    saved = [(d, dict(d)) for d in (ops._WORKSPACES, ops._WS_STATE, ops._WS_NEED)]
    rec = Recorder(_lib.call)
    for d, _ in saved:
        d.clear()
    _lib.call = rec
    try:
        env, steps = CASES[name][0](kind == "ragged")
        env["ws"] = torch.empty((1 << 20,), dtype=torch.uint8, device=DEV)   # a caller-owned workspace, for the entries that take one
        rec.take({})                                                          # (what building the inputs called is not the case)
        trace = {}
        for step, fn in steps:
            result = fn(env)
            _named(step, result, env)
            known = {k: t for k, t in env.items() if torch.is_tensor(t)}
            for key, ws in ops._WORKSPACES.items():
                known[".".join(("workspace",) + tuple(str(k) for k in key[2:]))] = ws
            trace[step] = rec.take(known)
        torch.cuda.synchronize()
        return trace
    finally:
        _lib.call = rec.real
        for d, old in saved:
            d.clear()
            d.update(old)


@pytest.fixture(scope="module")
def golden():
    with open(TRACE_FILE) as f:
        return json.load(f)


def test_the_golden_holds_exactly_these_cases(golden):
    assert sorted(golden) == sorted(CASE_IDS)


@pytest.mark.parametrize("case_id", CASE_IDS)
def test_wrapper_calls_equal_the_recorded_trace(case_id, golden):
    want, got = golden[case_id], json.loads(json.dumps(run_case(case_id)))
    assert list(got) == list(want), "steps"
    for step in want:
        assert [c["entry"] for c in got[step]] == [c["entry"] for c in want[step]], (step, "entries")
        for i, (g, w) in enumerate(zip(got[step], want[step])):
            assert g["guard"] == w["guard"], (step, i, g["entry"], "device guard")
            assert len(g["args"]) == len(w["args"]), (step, i, g["entry"])
            for j, (ga, wa) in enumerate(zip(g["args"], w["args"])):
                assert ga == wa and type(ga) is type(wa), (step, i, g["entry"], "argument", j, ga, wa)


def collect():
    """{case id: {step: [calls]}} over all cases -- run against the ops.py to record."""
    return {c: run_case(c) for c in CASE_IDS}


def write(trace, path):
    """The trace as JSON with one call per line."""
    cases = []
    for cid, steps in trace.items():
        body = ",\n".join(f' {json.dumps(step)}: [\n' + ",\n".join("  " + json.dumps(c) for c in calls) + "\n ]"
                          for step, calls in steps.items())
        cases.append(f"{json.dumps(cid)}: {{\n{body}\n}}")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(cases) + "\n}\n")


if __name__ == "__main__":
    import sys
    write(collect(), sys.argv[1] if len(sys.argv) > 1 else TRACE_FILE)
