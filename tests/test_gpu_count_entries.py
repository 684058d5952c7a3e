"""Every IoU count entry (csrc/dmm_cost.hip) through every kernel form, at the smallest shapes that reach it: each call's tables
against the integer reference computed with torch on the device -- bit for bit -- and the number of kernels each call
enqueues against tests/golden/count_launch_counts.json: the counts of the commit BEFORE the entries shared one argument
bundle, one dtype dispatch, one sub-tile rule and one batch slice (ebfc1cf), recorded with ``collect()`` below against a build
of that commit.

Entries: dmm_iou_counts, dmm_iou_counts_dual, dmm_iou_counts_frames, dmm_iou_counts_dual_frames, and dmm_iou_counts on
DMM_PACKED1 words -- each dense and ragged, once on one contiguous inter | area_p | area_t block (one clearing launch) and
once on tables that lie apart (three); the dual tables always lie apart (two more).  The entries are called through
``_lib.call``: ``ops`` always allocates its tables separately.
Reference: (x > 0.5) of the values the kernel received; a frame's tables are zero outside its live block (and altogether when
it has no live proposal or no live template).  Every table is filled with -7 before the call, so a clear that went missing
shows.

Forms (options): by shape; COST_KERNEL = 0 pins the register tiles -- their ladder of MT 8 / 16 / 24 / 32 rows x NG 1 / 2 / 4
proposal groups, a second template set doubling the rows; with COST_TINY_FRAMES = 0 also at B <= 8, where a handful of frames
otherwise takes the short-chunk instantiation; COST_KERNEL = 1 pins the template-lane kernel.  Every launch here is far below
COST_SMALL_WGS workgroups, so every register-tile launch is cut into sub-tiles of proposals."""
import json
import os

import pytest
import torch

from dmm_net_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# B, N, M, H, W.  12 x 20 planes: HW = 240 is no multiple of a chunk (the tail instantiations run).  N = 6 / 70 / 130: one,
# two, four proposal groups; M = 3 / 12 / 20 / 28: 8 / 16 / 24 / 32 rows; 130 x 20: more than 16 rows run as 128-proposal
# tiles; 257 x 33: two n-tiles and two m-tiles.  Dual: M = 3 / 8 / 12 / 16 share one tile with their targets, 17 takes two
# m-tiles of 16.
SHAPES = {f"{n}x{m}": (4, n, m, 12, 20) for n, m in ((6, 3), (6, 8), (6, 12), (6, 16), (6, 17), (6, 20), (6, 28), (70, 3),
                                                     (70, 12), (70, 20), (70, 28), (130, 3), (130, 12), (130, 20), (257, 33))}
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
CASES = [(sh, dt) for sh in SHAPES for dt in DTYPES]
# one case each: more than one 1024-pixel chunk; two frames; more frames than COST_TINY_FRAMES (and one whole group of 8 for
# the XCD mapping); views strided in frame and in plane
SHAPES.update({"6x3@33x40": (4, 6, 3, 33, 40), "B2": (2, 6, 3, 12, 20), "B9": (9, 6, 12, 12, 20), "strided": (4, 6, 12, 12, 20)})
CASES += [("6x3@33x40", "f32"), ("B2", "f16"), ("B9", "f16"), ("strided", "bf16")]
OPTIONS = [("default", {}), ("tiles", {"COST_KERNEL": 0}), ("tiles_no_tiny", {"COST_KERNEL": 0, "COST_TINY_FRAMES": 0}),
           ("lanes", {"COST_KERNEL": 1})]
ENTRIES = ("counts", "dual", "frames", "dual_frames", "packed")
FORMS = ("block", "apart")
COUNTS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "count_launch_counts.json")
GAP = 16                                         # words between tables that lie apart
_inputs = {}


def case_id(case):
    return "/".join(case)


def _rand_planes(B, K, H, W, dtype, g, strided):
    """[B, K, H, W] planes of uniform values, a few of them exactly 0.5 (not above the threshold)."""
    HW = H * W
    x = torch.rand((B, K, HW), generator=g, device=DEV)
    x[:, :, ::7] = 0.5
    x = x.to(dtype)
    if strided:                                  # one plane of room behind every frame, 8 elements behind every plane
        buf = torch.zeros((B, K + 1, HW + 8), dtype=dtype, device=DEV)
        buf[:, :K, :HW] = x
        return torch.as_strided(buf, (B, K, H, W), ((K + 1) * (HW + 8), HW + 8, W, 1))
    return x.view(B, K, H, W)


def _reference(pm, tm, nv, mv):
    """-> inter [B, M, N], area_p [B, N], area_t [B, M] as int32: exact (fp32 sums of at most HW < 2^24 ones).  nv / mv: the
    live counts per frame as int32 tensors (None: every plane is live)."""
    bp, bt = (pm > 0.5).flatten(2).float(), (tm > 0.5).flatten(2).float()
    inter, ap, at = torch.bmm(bt, bp.transpose(1, 2)), bp.sum(2), bt.sum(2)
    if nv is not None or mv is not None:
        B, N, M = pm.shape[0], pm.shape[1], tm.shape[1]
        nv = torch.full((B,), N, device=DEV) if nv is None else nv.long()
        mv = torch.full((B,), M, device=DEV) if mv is None else mv.long()
        live = (nv > 0) & (mv > 0)
        cols = (torch.arange(N, device=DEV)[None, :] < (nv * live)[:, None]).float()
        rows = (torch.arange(M, device=DEV)[None, :] < (mv * live)[:, None]).float()
        inter, ap, at = inter * rows[:, :, None] * cols[:, None, :], ap * cols, at * rows
    return inter.to(torch.int32), ap.to(torch.int32), at.to(torch.int32)


def _case_inputs(sh, dt):
    """Device inputs and the integer references of one case, dense and ragged: computed once, never written."""
    if (sh, dt) in _inputs:
        return _inputs[(sh, dt)]
    B, N, M, H, W = SHAPES[sh]
    g = torch.Generator(device=DEV).manual_seed(9000 + 31 * N + M + B)
    pm, tm, t2 = (_rand_planes(B, K, H, W, DTYPES[dt], g, sh == "strided") for K in (N, M, M))
    d = dict(pm=pm, tm=tm, t2=t2, pk_p=ops.pack_masks(pm), pk_t=ops.pack_masks(tm),
             table=torch.tensor([pm[b].data_ptr() for b in range(B)], dtype=torch.int64, device=DEV))
    # ragged: a live block, a frame without proposals, a frame without templates, another live block, ...
    nv_l = [(N - 2, 0, N, N - 1)[b % 4] for b in range(B)]
    mv_l = [(M - 1, M, 0, M)[b % 4] for b in range(B)]
    for ragged in (0, 1):
        nv = torch.tensor(nv_l, dtype=torch.int32, device=DEV) if ragged else None
        mv = torch.tensor(mv_l, dtype=torch.int32, device=DEV) if ragged else None
        d[ragged] = dict(nv=nv, mv=mv, ref=_reference(pm, tm, nv, mv), ref2=_reference(pm, t2, nv, mv))
    _inputs[(sh, dt)] = d
    return d


def _tables(B, N, M, form):
    """inter, area_p, area_t (one block, or GAP words apart), inter2, area_t2 (always apart), every word -7."""
    gap = 0 if form == "block" else GAP
    sizes, gaps = (B * M * N, B * N, B * M, B * M * N, B * M), (0, gap, gap, GAP, GAP)
    buf = torch.full((sum(sizes) + sum(gaps),), -7, dtype=torch.int32, device=DEV)
    out, off = [], 0
    for n, g in zip(sizes, gaps):
        off += g
        out.append(buf[off:off + n])
        off += n
    return [t.view(s) for t, s in zip(out, ((B, M, N), (B, N), (B, M), (B, M, N), (B, M)))]


def call_entry(entry, form, shape, planes, table, packed, nv, mv):
    """One C entry on fresh tables -> (the tables it owes, kernels it enqueued).  planes = (pm, tm, t2) as [B, K, H, W] views
    with contiguous pixels, table = the device array of the frames' first planes, packed = (words_p, words_t)."""
    B, N, M, H, W = shape
    HW = H * W
    pm, tm, t2 = planes
    inter, ap, at, inter2, at2 = _tables(B, N, M, form)
    p = ops._ptr
    dual, frames = entry.startswith("dual"), entry.endswith("frames")
    name = "dmm_iou_counts" + ("_dual" if dual else "") + ("_frames" if frames else "")
    if entry == "packed":
        wd = ops.pack_words(HW)
        first = (p(packed[0]), p(packed[1]), _lib.DTYPE_PACKED1, B, N, M, HW, N * wd, wd, M * wd, wd)
    else:
        first = (p(table) if frames else p(pm), p(tm)) + ((p(t2),) if dual else ()) + (ops._DT[pm.dtype], B, N, M, HW)
        first += (() if frames else (pm.stride(0),)) + (pm.stride(1), tm.stride(0), tm.stride(1))
        first += (t2.stride(0), t2.stride(1)) if dual else ()
    L = _lib.load()
    torch.cuda.synchronize()
    c0 = L.dmm_launch_count()
    _lib.call(name, DEV, *first, p(nv), p(mv), p(inter), p(ap), p(at), *((p(inter2), p(at2)) if dual else ()), ops._stream(tm))
    launches = int(L.dmm_launch_count() - c0)
    return ((inter, ap, at, inter2, at2) if dual else (inter, ap, at)), launches


def run_case(case):
    """Every entry once per (option set, batch form, table form) of one case, results checked; -> {cell: {entry/form: kernels}}."""
    sh, dt = case
    d = _case_inputs(sh, dt)
    out = {}
    for opt_name, opts in OPTIONS:
        for ragged in (0, 1):
            r = d[ragged]
            counts = {}
            with _lib.options(**opts):
                for entry in ENTRIES:
                    for form in FORMS:
                        tag = (case_id(case), opt_name, "ragged" if ragged else "dense", entry, form)
                        got, counts[entry + "/" + form] = call_entry(entry, form, SHAPES[sh], (d["pm"], d["tm"], d["t2"]),
                                                                     d["table"], (d["pk_p"], d["pk_t"]), r["nv"], r["mv"])
                        want = r["ref"] + ((r["ref2"][0], r["ref2"][2]) if entry.startswith("dual") else ())
                        for name, g, w in zip(("inter", "area_p", "area_t", "inter2", "area_t2"), got, want):
                            assert torch.equal(g, w), (tag, name)
            out[opt_name + "/" + ("ragged" if ragged else "dense")] = counts
    return out


def run_many_frames():
    """B = 65537 (grid.y stops at 65535: two batch slices), N = 2, M = 1, 4 x 4 planes in f16: the dense single-set entry, and
    the dual pointer-table entry with n_valid, its table built as base + arange * stride.  -> {cell: kernels}."""
    B, N, M, H, W = shape = (65537, 2, 1, 4, 4)
    g = torch.Generator(device=DEV).manual_seed(65537)
    pm, tm, t2 = (_rand_planes(B, K, H, W, torch.float16, g, False) for K in (N, M, M))
    table = pm.data_ptr() + torch.arange(B, dtype=torch.int64, device=DEV) * (pm.stride(0) * pm.element_size())
    nv = (torch.arange(B, device=DEV) % 3).to(torch.int32)
    out = {}
    for form in FORMS:
        got, out["counts/dense/" + form] = call_entry("counts", form, shape, (pm, tm, t2), table, None, None, None)
        for name, gt, w in zip(("inter", "area_p", "area_t"), got, _reference(pm, tm, None, None)):
            assert torch.equal(gt, w), ("counts", form, name)
        got, out["dual_frames/n_valid/" + form] = call_entry("dual_frames", form, shape, (pm, tm, t2), table, None, nv, None)
        ref, ref2 = _reference(pm, tm, nv, None), _reference(pm, t2, nv, None)
        for name, gt, w in zip(("inter", "area_p", "area_t", "inter2", "area_t2"), got, ref + (ref2[0], ref2[2])):
            assert torch.equal(gt, w), ("dual_frames", form, name)
    return out


def run_no_pixels():
    """HW = 0 on valid pointers: the tables are cleared, nothing else is enqueued.  -> {entry/form: kernels}."""
    sh = "6x3"
    d = _case_inputs(sh, "f32")
    B, N, M, H, W = SHAPES[sh]
    out = {}
    for entry in ENTRIES:
        for form in FORMS:
            got, out[entry + "/" + form] = call_entry(entry, form, (B, N, M, 0, 0), (d["pm"], d["tm"], d["t2"]), d["table"],
                                                      (d["pk_p"], d["pk_t"]), None, None)
            for t in got:
                assert int(t.abs().sum()) == 0, (entry, form)
    return out


def _recorded(key):
    with open(COUNTS_FILE) as fh:
        return json.load(fh)[key]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_count_entry_on_every_kernel_form(case):
    counts = run_case(case)
    print(case_id(case), counts)
    assert counts == _recorded(case_id(case))


def test_more_frames_than_one_grid_holds():
    counts = run_many_frames()
    print(counts)
    assert counts == _recorded("B65537")


def test_planes_without_pixels_only_clear_the_tables():
    counts = run_no_pixels()
    print(counts)
    assert counts == _recorded("HW0")


def collect():
    """{case id: {cell: {entry/form: launches}}} over all cases -- run against a build of the commit to record (``_lib.use_library``)."""
    out = {case_id(c): run_case(c) for c in CASES}
    out["B65537"] = run_many_frames()
    out["HW0"] = run_no_pixels()
    return out
