"""The C-ABI library builds for gfx950, loads without a GPU and exports every symbol include/dmm_match.h declares.
(No compute calls here: those are the -m gpu tests.)"""
import ctypes
import os
import re

from conftest import ROOT
from dmm_net_amd import _lib


def header_symbols():
    txt = open(os.path.join(ROOT, "include", "dmm_match.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(dmm_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    syms = header_symbols()
    assert len(syms) >= 10
    for s in syms:
        assert hasattr(L, s), f"{s} declared in include/dmm_match.h but not exported"
    assert sorted(_lib.SYMBOLS) == syms, "dmm_net_amd/_lib.py binds a different symbol set than the header declares"



def test_bindings_follow_the_header_declarations():
    """_lib reads every argtypes / restype from include/dmm_match.h: one parameter bound per declared parameter, and one real
    entry of each type class bound as its C type says."""
    L = _lib.load()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmm_match.h")).read(), flags=re.S)
    decls = re.findall(r"\bDMM_API\s+[^;(]*?\b(dmm_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt)
    assert sorted(name for name, _ in decls) == header_symbols()
    for name, params in decls:
        n = 0 if params.strip() in ("", "void") else len(params.split(","))
        assert len(getattr(L, name).argtypes) == n, name
    assert L.dmm_iou_counts.argtypes[7] is ctypes.c_int64                       # int64_t sp_b
    assert L.dmm_relax_match_f32.argtypes[13] is ctypes.c_float                 # float lr
    assert L.dmm_relax_match_f32.argtypes[0] is ctypes.c_void_p                 # const float *
    assert L.dmm_relax_match_f32.argtypes[-1] is ctypes.c_void_p                # dmm_stream_t
    assert L.dmm_workspace_bytes.restype is ctypes.c_size_t
    assert L.dmm_pack_words.restype is ctypes.c_int64
    assert L.dmm_launch_count.restype is ctypes.c_longlong
    assert L.dmm_status_string.restype is ctypes.c_char_p
    assert L.dmm_iou_counts.restype is ctypes.c_int and L.dmm_abi_version.argtypes == []
    assert L.dmm_match_forward_ws.argtypes[31] is ctypes.c_void_p              # int *ws_state: a host out-parameter
    assert L.dmm_match_forward_ws.argtypes[30] is ctypes.c_size_t
    assert L.dmm_pack_words(256) == 4 and L.dmm_pack_words(257) == 8
    assert (_lib.DMM_OK, _lib.DMM_ERR_BAD_ARG, _lib.DMM_ERR_UNSUPPORTED, _lib.DMM_ERR_LAUNCH, _lib.DMM_ERR_WORKSPACE) == \
        (0, 1, 2, 3, 4)
    assert (_lib.DTYPE_F32, _lib.DTYPE_F16, _lib.DTYPE_BF16, _lib.DTYPE_PACKED1) == (0, 1, 2, 3)


def test_header_parser_rejects_unmapped_types():
    import pytest
    decls, enums = _lib.parse_header("typedef enum dmm_x { DMM_A = 2, DMM_B } dmm_x;\n"
                                     "DMM_API size_t dmm_ok(int64_t rows, const int H[4], void *p); /* (unsigned x) */\n"
                                     "DMM_API void dmm_none(void);\n")
    assert decls == {"dmm_ok": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]), "dmm_none": (None, [])}
    assert enums == {"dmm_x": {"DMM_A": 2, "DMM_B": 3}}
    for bad in ("DMM_API int dmm_bad(unsigned x, int y);", "DMM_API double dmm_bad(int y);", "DMM_API int dmm_bad(int);"):
        with pytest.raises(_lib.DmmError, match="dmm_bad"):
            _lib.parse_header(bad)
    with pytest.raises(_lib.DmmError, match="'unsigned'"):
        _lib.parse_header("DMM_API int dmm_bad(unsigned x);")


def test_checked_call_names_the_entry_without_gpu():
    """_lib.call raises DmmError naming the entry for a bad argument, and hands back a status listed in ``allow``."""
    import pytest
    with pytest.raises(_lib.DmmError, match=r"^dmm_iou_counts: bad argument"):
        _lib.call("dmm_iou_counts", None, None, None, 0, 1, 4, 2, 16, 64, 16, 32, 16, None, None, None, None, None, None)
    assert _lib.call("dmm_iou_counts", None, None, None, 0, 0, 4, 2, 16, 64, 16, 32, 16, None, None, None, None, None,
                     None) == _lib.DMM_OK
    one = ctypes.c_void_p(8)
    args = (one, 1, 33, 40, None, None, 1, 1, 0.1, one, one, None, one, None)      # M beyond the solver envelope
    with pytest.raises(_lib.DmmError, match=r"^dmm_relax_solve_f32: shape outside"):
        _lib.call("dmm_relax_solve_f32", None, *args)
    assert _lib.call("dmm_relax_solve_f32", None, *args, allow=(_lib.DMM_ERR_UNSUPPORTED,)) == 2
    with pytest.raises(_lib.DmmError, match="dmm_relax_solve_f32"):               # allow lists only what it lists
        _lib.call("dmm_relax_solve_f32", None, None, *args[1:], allow=(_lib.DMM_ERR_UNSUPPORTED,))

def test_load_and_status_strings():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.load()
    assert L.dmm_abi_version() == 2
    assert L.dmm_status_string(0) == b"ok"
    assert b"gfx950" in L.dmm_build_info() and L.dmm_build_info().endswith(b"abi %d" % L.dmm_abi_version())
    assert L.dmm_workspace_bytes(4, 50, 10, 512) > 4 * (50 + 10) * 512 * 4
    assert L.dmm_workspace_bytes(0, 50, 10, 512) == 0


def test_argument_validation_without_gpu():
    """Bad arguments are rejected before anything touches the device."""
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.load()
    assert L.dmm_iou_counts(None, None, 0, 1, 4, 2, 16, 64, 16, 32, 16, None, None, None, None, None, None) == 1
    assert L.dmm_iou_counts(None, None, 0, -1, 4, 2, 16, 64, 16, 32, 16, None, None, None, None, None, None) == 1
    assert L.dmm_iou_counts(None, None, 0, 0, 4, 2, 16, 64, 16, 32, 16, None, None, None, None, None, None) == 0
    # M beyond the compiled solver envelope
    one = ctypes.c_void_p(8)
    assert L.dmm_relax_solve_f32(one, 1, 33, 40, None, None, 1, 1, 0.1, one, one, None, one, None) == 2
    assert L.dmm_relax_solve_f32(one, 1, 3, 257, None, None, 1, 1, 0.1, one, one, None, one, None) == 2


MIX_FORWARD = ("dmm_mask_mix_to", "dmm_mask_mix_shared_to", "dmm_mask_mix", "dmm_mask_mix_frames", "dmm_mask_mix_shared_frames")
MIX_BACKWARD = ("dmm_mask_mix_bwd", "dmm_mask_mix_bwd_frames", "dmm_mask_mix_bwd_det", "dmm_mask_mix_bwd_frames_det")


def _mix_status(L, entry, *, B=1, N=4, M=2, Pp=4, HW=16, sp_n=16, so_m=16, dtype=0, out_dtype=0, Rb=True, planes=True,
                out=True, dout=True, dRb=True, ws=True, ws_bytes=1 << 30):
    """One mix entry's status for a call that must be answered before the device is touched (every pointer is the
    address 8).  ``out`` / ``out_dtype`` / ``so_m`` go to the entries that take them, ``ws`` to the deterministic ones."""
    p = lambda have: ctypes.c_void_p(8) if have else None
    frames, det = "_frames" in entry, entry.endswith("_det")
    sp = (sp_n,) if frames else (N * sp_n, sp_n)
    if entry in MIX_FORWARD:
        odt = (out_dtype,) if entry.endswith("_to") else ()
        return getattr(L, entry)(p(Rb), p(planes), dtype, B, N, M, Pp, HW, *sp, None, None, p(out), *odt, M * so_m, so_m, None)
    tail = (p(ws), ws_bytes) if det else ()
    return getattr(L, entry)(p(Rb), p(planes), dtype, p(dout), B, N, M, Pp, HW, *sp, None, None, p(dRb), *tail, None)


def test_mix_entries_validate_their_arguments_without_gpu():
    """Every mix entry's answer to arguments it rejects, or has nothing to do for, before any launch.  The expected statuses are
    those of the entries as they stood when each spelled its own checks out (commit 7c7ab6b), read off that code; the
    deterministic workspace sizes were recorded from a build of it."""
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.load()
    OK, BAD, UNSUPPORTED, WORKSPACE = 0, 1, 2, 4
    null = dict(Rb=False, planes=False, out=False, dout=False, dRb=False, ws=False)
    for entry in MIX_FORWARD + MIX_BACKWARD:
        fwd, det = entry in MIX_FORWARD, entry.endswith("_det")
        st = lambda **kw: _mix_status(L, entry, **kw)
        for kw in (dict(B=-1), dict(N=-1), dict(M=-1), dict(HW=-1), dict(Pp=3), dict(sp_n=15), dict(Rb=False),
                   dict(planes=False), dict(dtype=7), dict(dtype=_lib.DTYPE_PACKED1)):
            assert st(**kw) == BAD, (entry, kw)
        assert st(B=0, **null) == OK and st(M=0, **null) == OK, entry                   # nothing to do, whatever the pointers
        assert st(HW=0, **null) == (OK if fwd else BAD), entry                           # (the backward still owes dRb its zeros)
        assert st(B=0, Pp=3, **null) == BAD and st(M=0, HW=-1, **null) == BAD, entry     # sizes before "nothing to do"
        assert st(M=65536) == UNSUPPORTED and st(B=65536) == UNSUPPORTED, entry
        assert st(B=65536, Rb=False) == BAD and st(M=65536, sp_n=15) == UNSUPPORTED, entry    # pointers, grid limits, strides
        if fwd:
            assert st(out=False) == BAD and st(so_m=15) == BAD and st(M=65536, so_m=15) == UNSUPPORTED, entry
        else:
            assert st(dout=False) == BAD and st(dRb=False) == BAD, entry
        if entry.endswith("_to"):
            for kw in (dict(out_dtype=_lib.DTYPE_F16), dict(out_dtype=7), dict(dtype=_lib.DTYPE_F16, out_dtype=_lib.DTYPE_BF16),
                       dict(dtype=7, out_dtype=7)):
                assert st(**kw) == BAD, (entry, kw)
            assert st(M=65536, out_dtype=7) == UNSUPPORTED, entry
        if det:
            need = L.dmm_mask_mix_bwd_det_workspace_bytes(1, 4, 2, 4, 16)
            assert need == 32
            assert st(ws_bytes=need - 4) == WORKSPACE and st(ws=False) == BAD and st(ws=False, ws_bytes=0) == BAD, entry
            assert st(dtype=7, ws_bytes=0) == BAD and st(sp_n=15, ws_bytes=0) == BAD, entry   # before the workspace is looked at
            assert st(M=65536, ws=False) == UNSUPPORTED, entry
    # deterministic slab: pixel splits of the kernel that fills it x B x M x Pp floats.  112 x 32 and 224 x 16 are the widest
    # tables of the union kernel (4 * N * mt floats of LDS <= 56 KB), one proposal more takes the row kernel; at HW = 240 both
    # have one split, at 300 steps of 1024 pixels they differ
    size = L.dmm_mask_mix_bwd_det_workspace_bytes
    for (B, N, M), at240, at300 in (((2, 6, 3), 144, 57600), ((1, 112, 32), 14336, 8601600), ((1, 113, 32), 14464, 3471360),
                                    ((1, 224, 16), 14336, 8601600), ((1, 225, 16), 14400, 5760000)):
        assert size(B, N, M, N, 240) == at240 and size(B, N, M, N, 300 * 4096) == at300, (B, N, M)
    assert size(1, 112, 32, 115, 240) == 14720 and size(1, 225, 16, 228, 240) == 14592
    assert size(1, 300, 16, 300, 300 * 4096) == 0 and size(1, 20, 40, 20, 300 * 4096) == 0     # the wide kernel: no slab
    with _lib.options(MIX_SHARED=0):
        assert size(1, 112, 32, 112, 300 * 4096) == 3440640                                   # the row kernel
    with _lib.options(FORCE_WIDE=1):
        assert size(1, 112, 32, 112, 300 * 4096) == 0
    assert size(0, 4, 2, 4, 16) == 0 and size(1, 4, 0, 4, 16) == 0 and size(1, 4, 2, 3, 16) == 0 and size(1, 4, 2, 4, -1) == 0


COUNT_ENTRIES = ("dmm_iou_counts", "dmm_iou_counts_dual", "dmm_iou_counts_frames", "dmm_iou_counts_dual_frames")


def _count_status(L, entry, *, B=1, N=4, M=2, HW=16, sp_n=16, st_m=16, st2_m=16, dtype=0, planes_p=True, planes_t=True,
                  planes_t2=True, inter=True, area_p=True, area_t=True, inter2=True, area_t2=True):
    """One count entry's status for a call that must be answered before the device is touched (every pointer is the
    address 8).  ``planes_t2`` / ``st2_m`` / ``inter2`` / ``area_t2`` go to the dual entries only."""
    p = lambda have: ctypes.c_void_p(8) if have else None
    dual, frames = "_dual" in entry, "_frames" in entry
    args = (p(planes_p), p(planes_t)) + ((p(planes_t2),) if dual else ()) + (dtype, B, N, M, HW)
    args += (() if frames else (N * sp_n,)) + (sp_n, M * st_m, st_m) + ((M * st2_m, st2_m) if dual else ())
    args += (None, None, p(inter), p(area_p), p(area_t)) + ((p(inter2), p(area_t2)) if dual else ())
    return getattr(L, entry)(*args, None)


def test_count_entries_validate_their_arguments_without_gpu():
    """Every count entry's answer to arguments it rejects, or has nothing to do for, before any launch.  The expected statuses
    are those of the one dispatch behind the four entries as it stood when it took every argument by name (commit ebfc1cf),
    read off that code and confirmed against a build of it."""
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.load()
    OK, BAD = 0, 1
    null = dict(planes_p=False, planes_t=False, inter=False, area_p=False, area_t=False, inter2=False, area_t2=False)
    for entry in COUNT_ENTRIES:
        dual = "_dual" in entry
        st = lambda **kw: _count_status(L, entry, **kw)
        for kw in (dict(B=-1), dict(N=-1), dict(M=-1), dict(HW=-1), dict(planes_p=False), dict(planes_t=False), dict(inter=False),
                   dict(area_p=False), dict(area_t=False), dict(sp_n=15), dict(st_m=15), dict(dtype=7), dict(dtype=-1),
                   dict(dtype=_lib.DTYPE_PACKED1, sp_n=3), dict(dtype=_lib.DTYPE_PACKED1, st_m=3),
                   dict(dtype=_lib.DTYPE_PACKED1, HW=257, sp_n=7)):                  # 1-bit planes: 4 * ceil(HW / 256) words
            assert st(**kw) == BAD, (entry, kw)
        for kw in (dict(B=0), dict(N=0), dict(M=0)):                                 # nothing to do, whatever the pointers
            assert st(**kw) == OK and st(**kw, **null) == OK and st(**kw, dtype=7, sp_n=0) == OK, (entry, kw)
        for kw in (dict(B=0, HW=-1), dict(N=0, M=-1), dict(M=0, B=-1)):              # sizes before "nothing to do"
            assert st(**kw, **null) == BAD, (entry, kw)
        if dual:
            for kw in (dict(inter2=False), dict(area_t2=False), dict(st2_m=15), dict(dtype=_lib.DTYPE_PACKED1, st2_m=3)):
                assert st(**kw) == BAD, (entry, kw)
            # a second template set is what the entry is for: asked before anything else
            for kw in (dict(), dict(B=0), dict(N=0), dict(M=0), dict(B=0, **null)):
                assert st(planes_t2=False, **kw) == BAD, (entry, kw)


# the training BatchNorm entries of include/dmm_match.h (10), (10a) by kind, and the pointers each kind cannot do without at
# relu = 0 (`stats` / `sums` are the `workspace` of the deterministic forms)
BN_KINDS = {"stats": "x stats", "apply": "x stats weight bias y saved", "bwd_reduce": "dy x saved sums",
            "bwd_dx": "dy x saved weight sums dx dweight dbias", "fold": "workspace out"}
BN_SCALARS = dict(rows=64, C=32, groups=1, relu=0, momentum=0.1, eps=1e-5, workspace_bytes=1 << 20, stream=None)
STATUS_NAMES = ("DMM_OK", "DMM_ERR_BAD_ARG", "DMM_ERR_UNSUPPORTED", "DMM_ERR_LAUNCH", "DMM_ERR_WORKSPACE")


def bn_entries():
    """{entry: (kind, parameter names in prototype order)} of the 13 BatchNorm entries that answer with a status, read from
    the header."""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmm_match.h")).read(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\bDMM_API\s+int\s+(dmm_bn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt):
        kind = next(k for k in sorted(BN_KINDS, key=len, reverse=True) if name.startswith("dmm_bn_" + k))
        out[name] = (kind, [re.findall(r"\w+", p)[-1] for p in params.split(",")])
    return out


def bn_fault_rows(kind, params):
    """{label: overrides} -- every call of one entry that must be answered before a launch: each row carries a fault, or has
    no rows.  An override of None is a null pointer; every other pointer is the address 8."""
    det = "workspace" in params
    have = lambda *names: all(n in params for n in names)
    slot = {"stats": "workspace", "sums": "workspace"} if det else {}
    required = [slot.get(p, p) for p in BN_KINDS[kind].split()]
    pointers = [p for p in params if p not in BN_SCALARS]
    rows = [dict(rows=-1), dict(rows=0, **dict.fromkeys(pointers)), dict(C=0), dict(C=-8), dict(C=12), dict(C=24), dict(C=4096),
            dict(rows=0, C=0), dict(rows=0, C=12), dict(rows=-1, C=24)]
    rows += [{p: None} for p in required] + [{p: None, "C": 24} for p in required]          # a null pointer, alone and with an
    if have("groups"):                                                                      # unsupported width
        rows += [dict(groups=0), dict(rows=130, groups=65), dict(groups=3), dict(rows=0, groups=65), dict(groups=3, C=24)]
    if have("running_mean"):
        rows += [dict(running_mean=None), dict(running_var=None), dict(relu=3, C=12), dict(relu=-1, C=12)]
    if kind in ("bwd_reduce", "bwd_dx"):
        rows += [dict(relu=-1), dict(relu=3), dict(rows=0, relu=3), dict(relu=3, C=24), dict(relu=1, y=None), dict(relu=2, bias=None),
                 dict(relu=2, weight=None), dict(relu=1, y=None, C=24)]
    if have("dres"):
        rows += [dict(relu=2), dict(relu=2, C=24)]                                          # (dres is given)
    if det:
        first = [p for p in required if p != "workspace"][-1]                              # an output where the entry has one
        rows += [dict(workspace_bytes=255), dict(workspace_bytes=0), dict(workspace=None, workspace_bytes=0),
                 dict(workspace_bytes=255, C=24), {"workspace_bytes": 255, first: None}, {"workspace": None, first: None}]
    return {",".join(f"{k}={'null' if v is None else v}" for k, v in sorted(r.items())): r for r in rows}


def bn_status(L, entry, params, overrides):
    vals = {p: BN_SCALARS[p] if p in BN_SCALARS else ctypes.c_void_p(8) for p in params}
    vals.update(overrides)
    return STATUS_NAMES[getattr(L, entry)(*(vals[p] for p in params))]


BN_GRID_TABLE = [(n * g, C, g) for C in (8, 32, 64, 256, 512, 1024, 2048) for g in (1, 3, 64)
                 for n in (1, 63, 64, 65, 641, 4097, 100000)]
BN_GRID_REFUSED = [(0, 32, 1), (-64, 32, 1), (64, 32, 0), (130, 32, 65), (64, 32, 3), (64, 0, 1), (64, 12, 1), (64, 24, 1),
                   (64, 4096, 1)]


def bn_entry_golden(L):
    """What tests/golden/bn_entry_status.json holds, of the library ``L``."""
    status = {e: {label: bn_status(L, e, params, r) for label, r in bn_fault_rows(kind, params).items()}
              for e, (kind, params) in sorted(bn_entries().items())}
    size = {f"{rows},{C},{g}": int(L.dmm_bn_det_workspace_bytes(rows, C, g)) for rows, C, g in BN_GRID_TABLE + BN_GRID_REFUSED}
    return {"status_values": {n: i for i, n in enumerate(STATUS_NAMES)}, "status": status, "det_workspace_bytes": size}


def test_bn_entries_keep_their_statuses_and_grids_without_gpu():
    """The 13 training-BatchNorm entries' answers to every call they refuse or have nothing to do for -- which status, and
    which of two coinciding faults is named --, and ``dmm_bn_det_workspace_bytes`` = groups x row groups x 2 C x 4 over a
    table that pins the statistics grid (its row-group count, the 65536 / C cap, the / groups clamp and its floor at 1).
    Expected: tests/golden/bn_entry_status.json, recorded with ``bn_entry_golden`` from a build of commit bf10b8c, where
    each entry spelled its own checks out."""
    import json
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.load()
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "bn_entry_status.json")))
    assert want["status_values"] == {n: getattr(_lib, n) for n in STATUS_NAMES}
    entries = bn_entries()
    assert len(entries) == 13 and sorted(want["status"]) == sorted(entries)
    for e, (kind, params) in entries.items():
        rows = bn_fault_rows(kind, params)
        assert sorted(rows) == sorted(want["status"][e]), e
        for label, r in rows.items():
            # nothing here may launch: an accepted call has no rows, and the pointers are not memory
            assert want["status"][e][label] in ("DMM_ERR_BAD_ARG", "DMM_ERR_UNSUPPORTED", "DMM_ERR_WORKSPACE") or \
                (want["status"][e][label] == "DMM_OK" and r.get("rows") == 0), (e, label)
            assert bn_status(L, e, params, r) == want["status"][e][label], (e, label)
    size = want["det_workspace_bytes"]
    assert len(size) == len(BN_GRID_TABLE) + len(BN_GRID_REFUSED) == 156
    for rows, C, g in BN_GRID_TABLE + BN_GRID_REFUSED:
        assert int(L.dmm_bn_det_workspace_bytes(rows, C, g)) == size[f"{rows},{C},{g}"], (rows, C, g)
    for rows, C, g in BN_GRID_TABLE:                                                # (what the size is made of)
        parts = size[f"{rows},{C},{g}"] // (g * 2 * C * 4)
        rpp = 256 // min(C // 8, 32)
        assert parts == max(min(-(-(rows // g) // (8 * rpp)), max(min(65536 // C, 256) // g, 1)), 1), (rows, C, g)
    assert all(size[f"{rows},{C},{g}"] == 0 for rows, C, g in BN_GRID_REFUSED)


def test_training_entries_validate_their_arguments_without_gpu():
    """(5d) / (5e) / (1e): workspace sizes are positive and grow with the batch, null pointers / negative sizes answer
    DMM_ERR_BAD_ARG, tables outside the fast kernels' envelope answer DMM_ERR_UNSUPPORTED (the caller then takes the granular
    entries) -- all before anything touches the device."""
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.load()
    assert 0 < L.dmm_match_train_forward_workspace_bytes(1, 50, 5, 512) < L.dmm_match_train_forward_workspace_bytes(4, 50, 5, 512)
    assert L.dmm_match_train_forward_workspace_bytes(0, 50, 5, 512) == 0
    assert L.dmm_match_train_backward_workspace_bytes(1, 50, 5, 512, 10, 5) > 4 * (50 + 5) * 512
    # the solver's tape: R + 10 x 5 sweep records of 64 x 8 bytes + 10 sweep counts per frame; none for tables wider than a wave
    assert L.dmm_match_train_tape_bytes(1, 50, 5, 10, 5) >= 4 * 5 * 50 + 50 * 512 + 40
    assert L.dmm_match_train_tape_bytes(4, 50, 5, 10, 5) > 3 * L.dmm_match_train_tape_bytes(1, 50, 5, 10, 5)
    assert L.dmm_match_train_tape_bytes(1, 200, 20, 10, 5) == 0 and L.dmm_match_train_tape_bytes(1, 50, 5, 0, 5) == 0
    one = ctypes.c_void_p(8)
    base = lambda B, N, M: (one, one, one, 0, one, one, one, B, N, M, 64, 512, 3200, 64, 320, 64, 320, 64, None, None, 0.3,
                            10, 5, 0.1, 0, one, one, one, one, one, one, one, one, one, one, 1 << 30, None, 0, None, None)
    assert L.dmm_match_train_forward(*base(-1, 50, 5)) == 1
    assert L.dmm_match_train_forward(*base(0, 50, 5)) == 0                       # nothing to do
    assert L.dmm_match_train_forward(*base(1, 0, 5)) == 1
    assert L.dmm_match_train_forward(*base(1, 50, 33)) == 2                      # more than 32 templates
    assert L.dmm_match_train_forward(*base(1, 300, 5)) == 2                      # more than 256 solver columns
    args = list(base(1, 50, 5))
    args[0] = None
    assert L.dmm_match_train_forward(*args) == 1
    args = list(base(1, 50, 5))
    args[28] = None                                                              # cost_loss missing although targets are given
    assert L.dmm_match_train_forward(*args) == 1
    assert L.dmm_matching_loss_f32(None, None, None, None, 2, 50, 5, None, None, None, None, None) == 1
    assert L.dmm_matching_loss_f32(one, one, one, one, 2, 9000, 5, None, None, one, one, None) == 2
    assert L.dmm_launch_count() >= 0


def test_frame_step_entries_validate_their_arguments_without_gpu():
    """The five fixed-slot entries of the frame step (include/dmm_match.h (7b), (8c)) answer before any launch: DMM_ERR_BAD_ARG
    for a null pointer, a negative size, K <= 0, planes and packed both null and plane_stride < H W; DMM_OK where there is
    nothing to do; DMM_ERR_UNSUPPORTED from the first mask size past the limit (Mm + 2 padding = 65 for the preparation
    entries, 33 for dmm_step_finish_f32), R above 1024, more than 8 rows, Pp above 256, K above Pp.  (The largest legal sizes
    launch: tests/test_gpu_step_ref.py.)"""
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.load()
    p = ctypes.c_void_p(8)
    OK, BAD, UNS = 0, 1, 2

    def boxes(prob=p, bx=p, tight=p, images=1, R=4, M=28, H=8, W=8, pad=1):
        return L.dmm_proposal_boxes_f32(prob, bx, None, images, R, M, H, W, 0.4, pad, None, tight, None)
    for kw in (dict(prob=None), dict(bx=None), dict(tight=None), dict(images=-1), dict(R=-1), dict(M=0), dict(H=-1), dict(W=-1),
               dict(pad=-1)):
        assert boxes(**kw) == BAD, kw
    assert boxes(images=0) == OK and boxes(R=0) == OK and boxes(images=0, prob=None) == OK
    assert boxes(M=63) == UNS and boxes(M=65, pad=0) == UNS and boxes(images=1 << 16, R=1 << 15) == UNS

    def nms(tight=p, scores=p, keep=p, cnt=p, images=1, R=4, K=2):
        return L.dmm_nms_slots_f32(tight, scores, None, images, R, 0.5, K, None, keep, cnt, None)
    for kw in (dict(tight=None), dict(scores=None), dict(keep=None), dict(cnt=None), dict(images=-1), dict(R=-1), dict(K=0),
               dict(K=-1)):
        assert nms(**kw) == BAD, kw
    assert nms(images=0) == OK and nms(R=1025) == UNS

    def paste(prob=p, bx=p, scores=p, tight=p, keep=p, cnt=p, images=1, R=4, M=28, K=2, H=8, W=8, pad=1, planes=p, stride=64,
              packed=p):
        return L.dmm_paste_kept_f32(prob, bx, scores, tight, keep, cnt, images, R, M, K, H, W, pad, None, None, planes, stride,
                                    packed, None, None, None, None)
    for kw in (dict(prob=None), dict(bx=None), dict(scores=None), dict(tight=None), dict(keep=None), dict(cnt=None),
               dict(planes=None, packed=None), dict(stride=63), dict(stride=63, packed=None), dict(images=-1), dict(R=-1),
               dict(M=0), dict(K=0), dict(K=-3), dict(H=-1), dict(W=-1), dict(pad=-1)):
        assert paste(**kw) == BAD, kw
    assert paste(images=0) == OK
    assert paste(M=63) == UNS and paste(M=63, planes=None) == UNS and paste(images=1024, K=64) == UNS

    def finish(Rb=p, Pp=6, prob=p, bx=p, keep=p, cnt=p, B=1, R=4, Mm=28, K=4, M=5, H=8, W=8, pad=1, full=p, hist=p):
        return L.dmm_step_finish_f32(Rb, Pp, prob, bx, keep, cnt, B, R, Mm, K, M, H, W, pad, None, None, None, None, full, hist,
                                     None, None, None)
    for kw in (dict(Rb=None), dict(prob=None), dict(bx=None), dict(keep=None), dict(cnt=None), dict(full=None), dict(hist=None),
               dict(B=-1), dict(R=-1), dict(Mm=0), dict(K=0), dict(K=-1), dict(M=-1), dict(H=-1), dict(W=-1), dict(pad=-1)):
        assert finish(**kw) == BAD, kw
    assert finish(B=0) == OK and finish(M=0) == OK and finish(H=0) == OK and finish(W=0, Rb=None) == OK
    assert finish(Mm=31) == UNS and finish(Mm=33, pad=0) == UNS and finish(M=9, Pp=10) == UNS
    assert finish(Pp=257, K=50) == UNS and finish(K=7) == UNS and finish(B=65536) == UNS


def test_product_does_not_import_oracle():
    """The product package must never reach into oracle/ (CPU fallback would void parity)."""
    pkg = os.path.join(ROOT, "dmm_net_amd")
    for dp, _, fns in os.walk(pkg):
        for fn in fns:
            if fn.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dp, fn)).read()
                assert not re.search(r"^\s*(import|from)\s+oracle\b", src, flags=re.M), fn
                assert not re.search(r"#\s*include\s*[<\"][^>\"]*oracle", src), fn
                assert "libdmm_oracle" not in src and "dmmo_" not in src.replace("dmmo_check_div_by_const", ""), fn


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    """No HIP library -> DmmError with build instructions; nothing falls back to a CPU path."""
    import pytest
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "libdmm_match.so"))
    with pytest.raises(_lib.DmmError, match="no CPU fallback"):
        _lib.load()
    # and the tensor-level ops refuse CPU tensors outright
    import torch
    from dmm_net_amd import ops
    monkeypatch.undo()
    with pytest.raises(_lib.DmmError, match="no CPU fallback"):
        ops.iou_counts(torch.zeros(1, 2, 4, 4), torch.zeros(1, 1, 4, 4))
    from dmm_net_amd.match_model import MatchModel
    m = MatchModel({"matching": {"algo": "relax"}, "relax_max_iter": 2, "relax_proj_iter": 2,
                    "relax_learning_rate": 0.1, "score_weight": 0.3}, 1)
    with pytest.raises(_lib.DmmError):
        m(torch.zeros(2, 8), torch.zeros(2, 4, 4), [torch.zeros(1, 8)], torch.zeros(1, 4, 4), torch.zeros(2))


def test_workspace_sizes_cover_the_general_solver_outside_the_envelope():
    """Host-side size functions (no GPU): beyond 32 templates / 256 solver columns the fused forward's workspace also holds
    the general solver's state -- 9 tables of M x Pp floats per frame -- and dmm_relax_any_scratch_bytes says what the
    granular any-size entry needs."""
    L = _lib.load()
    B, D = 3, 64
    inside, wide_n, wide_m = L.dmm_workspace_bytes(B, 200, 20, D), L.dmm_workspace_bytes(B, 300, 20, D), \
        L.dmm_workspace_bytes(B, 20, 40, D)
    assert wide_n - inside > 9 * B * 20 * 300 * 4 and wide_m > 9 * B * 40 * 41 * 4
    for (N, M) in [(300, 40), (20, 50), (50, 10)]:
        Pp = max(N, M + 1)
        need = L.dmm_relax_any_scratch_bytes(B, N, M)
        assert 9 * B * M * Pp * 4 <= need <= 10 * B * M * Pp * 4 + B * 4096
    assert L.dmm_relax_any_scratch_bytes(0, 300, 40) == 0
    # argument validation of the any-size entry happens before any launch
    assert L.dmm_relax_match_any_f32(None, None, None, None, None, -1, 300, 40, None, None, 0.3, 2, 2, 0.1, 1, None, None, None,
                                     None, None, None, None, None, 0, None) == 1


def test_dispatch_options_go_through_the_abi_and_not_through_the_environment(monkeypatch):
    """VERDICT r3 hygiene: kernel choices / tuning values are integers set with dmm_set_option (include/dmm_match.h (0));
    the library contains no getenv call, so a stray variable cannot change what production dispatches."""
    L = _lib.load()
    names = re.findall(r"\b(DMM_OPT_[A-Z0-9_]+)\s*=\s*(\d+)", open(os.path.join(ROOT, "include", "dmm_match.h")).read())
    count = dict(names).pop("DMM_OPT_COUNT")
    assert int(count) == len(_lib.OPTIONS) == len(names) - 1
    for name, k in names:
        if name != "DMM_OPT_COUNT":
            assert _lib.OPTIONS[name[len("DMM_OPT_"):]] == int(k), name
    defaults = {k: _lib.get_option(k) for k in _lib.OPTIONS}
    assert defaults["COST_KERNEL"] == -1 and defaults["COST_TINY_FRAMES"] == 8 and defaults["FORCE_WIDE"] == 0
    monkeypatch.setenv("DMM_WIDE", "1")                           # what used to flip the dispatch
    monkeypatch.setenv("DMM_COST_KERNEL", "1")
    assert {k: _lib.get_option(k) for k in _lib.OPTIONS} == defaults
    inside = L.dmm_workspace_bytes(3, 200, 20, 64)
    with _lib.options(FORCE_WIDE=1, COST_KERNEL=1):
        assert _lib.get_option("FORCE_WIDE") == 1 and _lib.get_option("COST_KERNEL") == 1
        assert L.dmm_workspace_bytes(3, 200, 20, 64) > inside     # sizes and dispatch use ONE test
    assert {k: _lib.get_option(k) for k in _lib.OPTIONS} == defaults
    assert L.dmm_set_option(99, 1) == 1 and L.dmm_set_option(_lib.OPTIONS["COST_KERNEL"], 7) == 1
    assert L.dmm_set_option(_lib.OPTIONS["MIX_ALIGN"], 48) == 1 and L.dmm_get_option(99) == -2 ** 31
    _lib.set_option("MIX_WGS", 1000)
    assert L.dmm_reset_options() == 0 and _lib.get_option("MIX_WGS") == defaults["MIX_WGS"]
    for fn in os.listdir(_lib.CSRC):
        if fn.endswith((".hip", ".h")):
            assert "getenv" not in open(os.path.join(_lib.CSRC, fn)).read(), fn


def test_small_tables_share_one_staging_buffer():
    """``_lib.small_to_device_many``: several short host lists -> views of ONE buffer (one pinned copy on a GPU), each
    8-byte aligned, dtypes and values kept."""
    import torch
    specs = [([3, 1, 2], torch.int32), ([], torch.int32), ([2 ** 40 + 8, 7], torch.int64), ([0.5, -2.0, 1e-8], torch.float32)]
    got = _lib.small_to_device_many(specs, "cpu")
    assert [t.dtype for t in got] == [s[1] for s in specs]
    assert got[0].tolist() == [3, 1, 2] and got[1].numel() == 0 and got[2].tolist() == [2 ** 40 + 8, 7]
    assert got[3].tolist() == torch.tensor([0.5, -2.0, 1e-8]).tolist()
    base = got[0].untyped_storage().data_ptr()
    assert all(t.untyped_storage().data_ptr() == base for t in got if t.numel())
    assert all(t.data_ptr() % 8 == 0 for t in got if t.numel())
