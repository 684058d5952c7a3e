"""Every mask-mix entry (csrc/dmm_mix.hip) through every kernel kind, at the smallest shapes that reach it: the number of
kernels each call enqueues against tests/golden/mix_launch_counts.json -- the counts of the commit BEFORE the entries
shared one argument bundle, one dtype dispatch and one kernel choice (7c7ab6b), recorded with ``collect()`` below against
a build of that commit -- and each call's result against the fp64 product.

Kinds: the row kernel, the union kernel (rows that share planes) and the general kernel; option MIX_SHARED 0 / 1 pins
the first two, FORCE_WIDE = 1 the third, the default leaves the choice to the entry (forward) or to the table (backward).
What this file can and cannot see of the choice: every forward kernel is one launch and the fast ones agree bit for bit, so
the FORWARD kind is not observable here -- the cells pin that whichever kernel an option picks gives that one result, not
which kernel ran.  The backward kind shows in the deterministic slab (tests/test_cabi.py pins its size either side of the
union / rows switch) and in which non-deterministic results are bit-equal.
The pre-zeroed backward is reached through ``ops.match_train_backward``: its dRb lies in that call's workspace."""
import json
import os

import pytest
import torch

from dmm_net_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# B, N, M, H, W.  HW = 240 is no multiple of 256; M = 3 / 16 / 17 take the union kernels of 8 / 16 / 32 rows; 112 x 32 is
# the widest table of the union backward (4 * N * 32 floats of LDS <= 56 KB), 113 x 32 takes the row kernel
SHAPES = {"6x3": (2, 6, 3, 12, 20), "18x17": (2, 18, 17, 12, 20), "12x16": (1, 12, 16, 12, 20), "112x32": (1, 112, 32, 8, 8),
          "113x32": (1, 113, 32, 8, 8)}
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
OPTIONS = [("default", {}), ("mix_shared0", {"MIX_SHARED": 0}), ("mix_shared1", {"MIX_SHARED": 1}), ("force_wide", {"FORCE_WIDE": 1})]
CASES = [(sh, dt) for sh in SHAPES for dt in DTYPES]
COUNTS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mix_launch_counts.json")
D = 64                                           # feature width of the training call that carries the pre-zeroed backward
SOLVER = dict(score_weight=0.3, max_iter=2, proj_iter=2, lr=0.1, is_test=0)
_inputs = {}


def case_id(case):
    return "/".join(case)


def _case_inputs(sh, dt):
    """Device inputs and the fp64 references of one case, dense and ragged: computed once, never written."""
    if (sh, dt) in _inputs:
        return _inputs[(sh, dt)]
    B, N, M, H, W = SHAPES[sh]
    g = torch.Generator(device=DEV).manual_seed(7000 + 31 * N + M)
    Pp = ops.padded_width(N, M)
    pm = torch.rand((B, N, H, W), generator=g, device=DEV).to(DTYPES[dt])
    Rb = torch.rand((B, M, Pp), generator=g, device=DEV)
    Rb = torch.where(torch.rand((B, M, Pp), generator=g, device=DEV) < 0.3, Rb, torch.zeros_like(Rb))       # ~30 % kept
    Rb[:, :, N:] = 0
    Rb[0, M - 1] = 0                                                       # a row that selects nothing
    d = dict(pm=pm, Rb=Rb, dout=torch.randn((B, M, H, W), generator=g, device=DEV), Pp=Pp,
             sim=torch.rand((B, M, N), generator=g, device=DEV), pf=torch.randn((B, N, D), generator=g, device=DEV),
             tf=torch.randn((B, M, D), generator=g, device=DEV), sc=torch.rand((B, N), generator=g, device=DEV))
    for ragged in (0, 1):
        nv_l, mv_l = ([N, N - 2][:B], [M, M - 1][:B]) if B > 1 else ([N - 2], [M - 1])
        Rl = Rb.clone()
        if ragged:
            for b in range(B):
                Rl[b, :, nv_l[b]:] = 0
                Rl[b, mv_l[b]:] = 0
        planes = pm.double().flatten(2)
        ref = torch.bmm(Rl[:, :, :N].double(), planes).view(B, M, H, W)
        dref = torch.bmm(d["dout"].double().flatten(2), planes.transpose(1, 2)) * (Rl[:, :, :N] != 0)
        d[ragged] = dict(nv=torch.tensor(nv_l, dtype=torch.int32, device=DEV) if ragged else None,
                         mv=torch.tensor(mv_l, dtype=torch.int32, device=DEV) if ragged else None,
                         frames=ops.FramePlanes([pm[b] for b in range(B)]), ref=ref, dref=dref)
    _inputs[(sh, dt)] = d
    return d


def _train_bwd_drb(d, r, B, N, M, det):
    """The mix backward inside dmm_match_train_backward(_det), which clears dRb with the launch in front of it: -> dRb, read
    out of the call's workspace (featn_p | featn_t | norm_p | norm_t | dRb, each 256-byte aligned: carve_train_bwd)."""
    Pp = d["Pp"]
    saved = torch.cat([torch.zeros(B * M * N, device=DEV), d["sim"].flatten(), d["Rb"].flatten()])      # cos | sim | Rb
    ops.match_train_backward(d["pm"], d["pf"], d["tf"], d["sc"], saved, False, d["dout"], None, None, None, r["nv"], r["mv"], M,
                             det=det, **SOLVER)
    a256 = lambda n: (n + 255) // 256 * 256
    off = a256(4 * B * N * D) + a256(4 * B * M * D) + a256(4 * B * N) + a256(4 * B * M)
    dev = d["pm"].device
    ws = ops._WORKSPACES[(dev.index, torch.cuda.current_stream(dev).cuda_stream, "train_bwd")]
    return ws[off:off + 4 * B * M * Pp].view(torch.float32).view(B, M, Pp).clone()


def run_case(case):
    """Every entry once per (option set, batch form) of one case, results checked; -> {cell: {entry: kernels enqueued}}."""
    sh, dt = case
    B, N, M, H, W = SHAPES[sh]
    d = _case_inputs(sh, dt)
    pm, Rb, dout, Pp, tdt = d["pm"], d["Rb"], d["dout"], d["Pp"], DTYPES[dt]
    L = _lib.load()
    HW = H * W
    out = {}
    fwd_bits = {}                                                          # ragged -> the fp32 forward every fast form must equal
    for opt_name, opts in OPTIONS:
        wide = "FORCE_WIDE" in opts
        for ragged in (0, 1):
            r = d[ragged]
            nv, mv, fp, ref, dref = r["nv"], r["mv"], r["frames"], r["ref"], r["dref"]
            counts = {}
            tag = (case_id(case), opt_name, "ragged" if ragged else "dense")

            def counted(name, fn):
                torch.cuda.synchronize()
                c0 = L.dmm_launch_count()
                res = fn()
                counts[name] = int(L.dmm_launch_count() - c0)
                return res

            def plain_mix():                                               # dmm_mask_mix itself (ops goes through dmm_mask_mix_to)
                o = torch.empty((B, M, H, W), dtype=torch.float32, device=DEV)
                _lib.call("dmm_mask_mix", Rb.device, Rb.data_ptr(), pm.data_ptr(), ops._DT[tdt], B, N, M, Pp, HW, N * HW, HW,
                          ops._ptr(nv), ops._ptr(mv), o.data_ptr(), M * HW, HW, ops._stream(Rb))
                return o

            ops._WS_NEED.clear()                                           # (workspace sizes follow the options: no stale ones)
            with _lib.options(**opts):
                f = {"mix_to": counted("mix_to", lambda: ops.mask_mix(Rb, pm, nv, mv)),
                     "mix_shared_to": counted("mix_shared_to", lambda: ops.mask_mix(Rb, pm, nv, mv, shared=True)),
                     "mix": counted("mix", plain_mix),
                     "mix_frames": counted("mix_frames", lambda: ops.mask_mix(Rb, fp, nv, mv)),
                     "mix_shared_frames": counted("mix_shared_frames", lambda: ops.mask_mix(Rb, fp, nv, mv, shared=True))}
                own = {"mix_to": counted("mix_to_own", lambda: ops.mask_mix(Rb, pm, nv, mv, out_dtype=tdt)),
                       "mix_shared_to": counted("mix_shared_to_own", lambda: ops.mask_mix(Rb, pm, nv, mv, out_dtype=tdt, shared=True))}
                bwd = {"bwd": counted("bwd", lambda: ops.mask_mix_bwd(Rb, pm, dout, nv, mv, det=False)),
                       "bwd_frames": counted("bwd_frames", lambda: ops.mask_mix_bwd(Rb, fp, dout, nv, mv, det=False)),
                       "bwd_det": counted("bwd_det", lambda: ops.mask_mix_bwd(Rb, pm, dout, nv, mv, det=True)),
                       "bwd_frames_det": counted("bwd_frames_det", lambda: ops.mask_mix_bwd(Rb, fp, dout, nv, mv, det=True)),
                       "train_bwd": counted("train_bwd", lambda: _train_bwd_drb(d, r, B, N, M, False)),
                       "train_bwd_det": counted("train_bwd_det", lambda: _train_bwd_drb(d, r, B, N, M, True))}
                again = {"bwd_det": ops.mask_mix_bwd(Rb, pm, dout, nv, mv, det=True),
                         "bwd_frames_det": ops.mask_mix_bwd(Rb, fp, dout, nv, mv, det=True)}
            # forward: one result whatever the entry, the batch form and (inside the fast envelope) the kernel
            base = f["mix_to"] if wide else fwd_bits.setdefault(ragged, f["mix_to"])
            fscale = max(1.0, float(ref.abs().max()))
            for name, o in f.items():
                assert o.dtype == torch.float32 and torch.equal(o, base), (name, tag)
                err = float((o.double() - ref).abs().max())
                assert err <= 1e-5 * fscale, (name, tag, err)
            for name, o in own.items():                                    # the planes' own type: the fp32 result rounded once
                assert o.dtype == tdt and torch.equal(o, f[name].to(tdt)), (name, tag)
            # backward: the fp64 product on the support of the live block, exact zeros in the padded columns
            bscale = float(dref.abs().max())
            for name, o in bwd.items():
                err = float((o[:, :, :N].double() - dref).abs().max())
                assert err <= 2e-5 * bscale, (name, tag, err, bscale)
                assert float(o[:, :, N:].abs().sum()) == 0.0, (name, tag)
            for name, o in again.items():
                assert torch.equal(o, bwd[name]), (name, tag)
            assert torch.equal(bwd["bwd_frames_det"], bwd["bwd_det"]) and torch.equal(bwd["train_bwd_det"], bwd["bwd_det"]), tag
            if wide:                                                       # the general kernel sums in a fixed order as it is
                assert torch.equal(bwd["train_bwd"], bwd["bwd"]) and torch.equal(bwd["bwd_frames"], bwd["bwd"]), tag
            out["/".join(tag[1:])] = counts
    ops._WS_NEED.clear()
    return out


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_mix_entry_on_every_kernel_kind(case):
    with open(COUNTS_FILE) as fh:
        recorded = json.load(fh)[case_id(case)]
    counts = run_case(case)
    print(case_id(case), counts)
    assert counts == recorded


def collect():
    """{case id: {cell: {entry: launches}}} over all cases -- run against a build of the commit to record (``_lib.use_library``)."""
    return {case_id(c): run_case(c) for c in CASES}
