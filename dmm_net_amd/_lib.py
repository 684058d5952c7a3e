"""Loader for libdmm_match.so (the gfx950 HIP library) through its C ABI (include/dmm_match.h).

The library is built in-tree by ``__graft_entry__.build()`` (or ``make -C dmm_net_amd/csrc``) and
loaded with ctypes.  There is NO fallback: if the library is missing or a call fails, the product
raises -- nothing here ever routes to a CPU path.

The ctypes signatures and the enum values are read from the header itself (``parse_header``): it is the
one description of the ABI, and a binding cannot drift from it.
"""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdmm_match.so")        # no environment override: see use_library()
CSRC = os.path.join(_HERE, "csrc")
HEADER = os.path.join(_HERE, os.pardir, "include", "dmm_match.h")

MAX_TEMPLATES = 32
MAX_PROPOSALS = 256
FRAME_TABLE = -(1 << 63)          # DMM_FRAME_TABLE: sp_b sentinel, masks_p = device table of per-frame base pointers


class DmmError(RuntimeError):
    pass


# the closed map of the header's non-pointer types (every pointer, and dmm_stream_t, is passed as c_void_p)
_CTYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t,
           "float": ctypes.c_float, "dmm_stream_t": ctypes.c_void_p}


def _ctype(decl: str, fn: str, is_return: bool):
    """One C type (a parameter with its name, or a return type) -> its ctypes type."""
    if "*" in decl or "[" in decl:                        # pointers and arrays; a returned string is read by ctypes
        string = decl.replace("*", " ").split() == ["const", "char"]
        return ctypes.c_char_p if is_return and string else ctypes.c_void_p
    words = [w for w in decl.split() if w != "const"]
    if is_return and words == ["void"]:
        return None
    t = " ".join(words if is_return else words[:-1])
    if t not in _CTYPES:
        raise DmmError(f"include/dmm_match.h: {fn} uses type '{t or decl.strip()}', which the ctypes binding does not map")
    return _CTYPES[t]


def parse_header(text: str):
    """include/dmm_match.h -> ({function: (restype, argtypes)} in declaration order, {enum tag: {enumerator: value}})."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^\s*#[^\n]*", "", text, flags=re.M)
    decls = {}
    for ret, fn, params in re.findall(r"\bDMM_API\s+([^;(]*?)\s*\b(dmm_\w+)\s*\(([^)]*)\)\s*;", text):
        params = params.strip()
        args = [] if params in ("", "void") else [_ctype(p, fn, False) for p in params.split(",")]
        decls[fn] = (_ctype(ret, fn, True), args)
    enums = {}
    for tag, body in re.findall(r"\benum\s+(\w+)\s*\{([^}]*)\}", text):
        values, v = {}, -1
        for item in filter(None, (s.strip() for s in body.split(","))):
            name, _, val = (s.strip() for s in item.partition("="))
            v = int(val, 0) if val else v + 1
            values[name] = v
        enums[tag] = values
    return decls, enums


try:
    with open(HEADER) as _f:
        _TEXT = _f.read()
    _DECLS, _ENUMS = parse_header(_TEXT)
    MASK_LOSS_CHUNK = int(re.search(r"^#define\s+DMM_MASK_LOSS_CHUNK\s+(\d+)", _TEXT, re.M).group(1))   # (13): pixels per workgroup
    del _TEXT
except OSError as _e:
    raise DmmError(f"{os.path.normpath(HEADER)} is missing: the C ABI's bindings are read from it ({_e})") from None

SYMBOLS = tuple(_DECLS)                                   # every function include/dmm_match.h declares
DMM_OK, DMM_ERR_BAD_ARG, DMM_ERR_UNSUPPORTED, DMM_ERR_LAUNCH, DMM_ERR_WORKSPACE = (_ENUMS["dmm_status"][k] for k in (
    "DMM_OK", "DMM_ERR_BAD_ARG", "DMM_ERR_UNSUPPORTED", "DMM_ERR_LAUNCH", "DMM_ERR_WORKSPACE"))
DTYPE_F32, DTYPE_F16, DTYPE_BF16, DTYPE_PACKED1 = (_ENUMS["dmm_dtype"]["DMM_" + k] for k in ("F32", "F16", "BF16", "PACKED1"))
# include/dmm_match.h (0): dispatch options, set through the ABI (the library reads no environment variable)
OPTIONS = {k[len("DMM_OPT_"):]: v for k, v in _ENUMS["dmm_option"].items() if k != "DMM_OPT_COUNT"}

_lib = None


def build(verbose: bool = False) -> str:
    """Compile every HIP source for gfx950 into dmm_net_amd/libdmm_match.so (hipcc cross-compiles)."""
    cmd = ["make", "-C", CSRC, "-j", str(min(8, os.cpu_count() or 1))]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)
    if not os.path.exists(LIB_PATH):
        raise DmmError("build did not produce " + LIB_PATH)
    return LIB_PATH


def use_library(path: str) -> None:
    """Load ANOTHER build of the library instead of the in-tree one (A/B builds in tools/: cached instead of non-temporal
    plane loads, other tile sizes).  An explicit call BEFORE the first ``load()``: no environment variable can change which
    library production loads."""
    global LIB_PATH
    if _lib is not None:
        raise DmmError("use_library() after the library has been loaded")
    LIB_PATH = os.path.abspath(path)


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DmmError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(the HIP extension is mandatory; there is no CPU fallback)")
    import torch  # noqa: F401  -- load torch's HIP runtime first so both share one libamdhip64
    L = ctypes.CDLL(LIB_PATH)
    for name, sig in _DECLS.items():
        if not hasattr(L, name):
            raise DmmError(f"{LIB_PATH} does not export {name}")
        fn = getattr(L, name)
        (fn.restype, fn.argtypes) = sig
    if L.dmm_abi_version() != 2:
        raise DmmError("libdmm_match.so ABI version mismatch")
    # libdmm_match.so needs libhipblaslt.so.1 / libamdhip64.so.7 by SONAME; torch (imported above) has already mapped its
    # bundled copies under the same sonames, so the loader binds to those -- ONE HIP runtime and ONE hipBLASLt per process.
    try:
        with open("/proc/self/maps") as f:
            lt = {ln.split()[-1] for ln in f if "libhipblaslt.so" in ln}
        if len(lt) > 1:
            import warnings
            warnings.warn(f"two hipBLASLt copies are mapped ({sorted(lt)}): import torch before loading {LIB_PATH}")
    except OSError:
        pass
    _lib = L
    return L


def check(rc: int, what: str):
    if rc != DMM_OK:
        L = load()
        msg = L.dmm_status_string(rc).decode()
        extra = f" (hipError {L.dmm_last_hip_error()})" if rc == DMM_ERR_LAUNCH else ""
        raise DmmError(f"{what}: {msg}{extra}")


def call(name: str, device, *args, allow=()):
    """``load().<name>(*args)`` under ``device_guard(device)`` (no guard for ``device=None``), checked: a status other than
    DMM_OK raises -- unless ``allow`` lists it (an "outside the envelope" answer the caller handles).  Returns the status."""
    if device is None:
        rc = getattr(load(), name)(*args)
    else:
        with device_guard(device):
            rc = getattr(load(), name)(*args)
    if rc != DMM_OK and rc not in allow:
        check(rc, name)
    return rc


def set_option(name: str, value: int):
    check(load().dmm_set_option(OPTIONS[name], int(value)), f"dmm_set_option({name}, {value})")


def get_option(name: str) -> int:
    return int(load().dmm_get_option(OPTIONS[name]))


_OPTIONS_LOCK = None


class options:
    """``with _lib.options(COST_KERNEL=1, COST_TINY_FRAMES=0): ...`` -- pin dispatch options for a block (tests, A/B
    timing) and put the previous values back.  The options are PROCESS-WIDE: the block holds a re-entrant lock, so two
    threads pinning different values run their blocks one after the other instead of seeing each other's settings
    (ADVICE r4); threads that do not pin anything are not held up -- and see whatever is pinned at the moment."""

    def __init__(self, **kw):
        self.kw, self.old = kw, {}

    def __enter__(self):
        global _OPTIONS_LOCK
        if _OPTIONS_LOCK is None:
            import threading
            _OPTIONS_LOCK = threading.RLock()
        _OPTIONS_LOCK.acquire()
        for k, v in self.kw.items():
            self.old[k] = get_option(k)
            set_option(k, v)
        return self

    def __exit__(self, *exc):
        try:
            for k, v in self.old.items():
                set_option(k, v)
        finally:
            _OPTIONS_LOCK.release()
        return False


def small_to_device(values, dtype, device):
    """A short host list as a device tensor WITHOUT stalling the host: ``torch.tensor(values, device=cuda)`` copies
    from pageable memory, which the HIP runtime completes synchronously -- the host waits until the stream has drained
    to the copy (0.2 ms per call in the frame loop, 6 calls per frame step: the host could not run ahead of the GPU).
    Pinned staging + non_blocking: the caching host allocator keeps the pinned block until the copy's event has passed."""
    import torch
    t = torch.tensor(values, dtype=dtype)
    if torch.device(device).type != "cuda":
        return t.to(device)
    return t.pin_memory().to(device, non_blocking=True)


def small_to_device_many(specs, device, memo=None):
    """Several short host lists in ONE pinned staging buffer and ONE copy: ``specs`` = [(values, torch dtype), ...] ->
    one device tensor per entry (views of one allocation, each 8-byte aligned).  The per-video driver hands five such
    tables to the layer per call (proposal / template counts, three pointer tables): five pinned allocations and five
    copies were ~70 us of host time per call (round 5, ``tools/dropin_trace.py model cprofile``).
    ``memo`` (a dict the caller keeps): when the VALUES are the same as in the caller's previous call -- the frames of a clip
    keep their counts, and the caching allocator hands the same addresses to same-sized tensors step after step -- the
    previous device tables are returned as they are (read-only by contract): no staging, no copy (~35 us of host time)."""
    import numpy as np
    import torch
    if memo is not None:
        key = (str(device), tuple((tuple(v), d) for v, d in specs))
        if memo.get("key") == key:
            return memo["out"]
    np_of = {torch.int32: np.int32, torch.int64: np.int64, torch.float32: np.float32}
    parts, spans, off = [], [], 0
    for values, dtype in specs:
        a = np.asarray(values, dtype=np_of[dtype])
        nbytes = a.size * a.itemsize
        pad = (-nbytes) % 8
        parts.append(a.view(np.uint8))
        if pad:
            parts.append(np.zeros(pad, dtype=np.uint8))
        spans.append((off, nbytes, dtype))
        off += nbytes + pad
    host = torch.from_numpy(np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8))
    if torch.device(device).type == "cuda":
        buf = host.pin_memory().to(device, non_blocking=True)
    else:
        buf = host.to(device)
    out = [buf[o:o + n].view(dt) for (o, n, dt) in spans]
    if memo is not None:
        memo["key"], memo["out"] = key, out
    return out


_NULL_CTX = None


def device_guard(device):
    """``torch.cuda.device(device)`` only when ``device`` is not already the current one: the launchers run under a
    device guard so that the HIP runtime targets the tensors' GPU, but pushing and popping the guard costs several
    microseconds per op -- with ~20 ops per frame step in a host-bound loop -- and almost every call is on the
    current device already."""
    global _NULL_CTX
    import contextlib
    import torch
    if _NULL_CTX is None:
        _NULL_CTX = contextlib.nullcontext()
    dev = torch.device(device) if not isinstance(device, torch.device) else device
    if dev.index is None or dev.index == torch.cuda.current_device():
        return _NULL_CTX
    return torch.cuda.device(dev)
