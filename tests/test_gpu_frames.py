"""The frame preparation on the device (dmm_net_amd/frames.py, include/dmm_match.h (16)) against tests/golden/frames_resized.npz:
Pillow's bytes for every size pair and filter, and torch's ``ToTensor`` + ``Normalize`` of them on the CPU, bit for bit.  No
comparison here has a tolerance."""
import numpy as np
import pytest
import torch

import frames_ref as fr
from dmm_net_amd import _lib, frames as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN2, STD2 = (0.5, 0.25, 0.125), (1.0, 0.5, 0.3)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _launches():
    return int(_lib.load().dmm_launch_count())


def _want_launches(c, f):
    (Hs, Ws), (H, W) = c.src_size, c.size
    return 1 if f == "nearest" else max(1, int(Hs != H) + int(Ws != W))


@pytest.mark.parametrize("pattern", fr.PATTERNS)
@pytest.mark.parametrize("pair", fr.pair_ids())
def test_prepare_frames_equals_pillow_and_torch(pair, pattern):
    """Every pair and filter: the uint8 result is the fixture's, the fp32 result torch's normalisation of it; one launch per pass
    that runs."""
    c = fr.case(pair, pattern)
    src = torch.from_numpy(np.array(c.src)).to(DEV)[None]
    for f in fr.FILTERS:
        mean, std = (F.MEAN, F.STD) if f != "bilinear" else (MEAN2, STD2)
        l0 = _launches()
        tables = F.FrameTables(c.src_size, c.size, f, mean, std, DEV)
        l1 = _launches()
        got, u8 = F.prepare_frames(src, c.size, tables=tables, return_u8=True)
        assert _launches() - l1 == _want_launches(c, f), (c.name, f)
        assert l1 - l0 == (1 if f == "nearest" else 0)                          # (only the nearest tables are made on the device)
        assert u8.dtype == torch.uint8 and tuple(u8.shape) == (1,) + c.size + (3,)
        assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3) + c.size
        assert np.array_equal(u8[0].cpu().numpy(), c.want[f]), (c.name, f, int((u8[0].cpu().numpy() != c.want[f]).sum()))
        assert np.array_equal(c.want[f], F.resize_frames_host(c.src, c.size, f))                 # the second witness
        want = fr.normalised(c.want[f], mean, std)
        assert torch.equal(_bits(got[0].cpu()), _bits(want)), (c.name, f)
        only = F.prepare_frames(src, c.size, filter=f, mean=mean, std=std)                      # without the uint8 output, own tables
        assert torch.equal(_bits(only), _bits(got))


@pytest.mark.parametrize("n", [0, 1, 3])
def test_frame_counts_strided_sources_and_output_slices(n):
    """n frames that differ; the source a view whose row stride is above 3 Ws and whose frame stride is above a frame; the
    output a channel-and-batch slice of a larger tensor whose other elements stay as they were."""
    c = fr.case("37x53_19x23", "noise")
    (Hs, Ws), (H, W) = c.src_size, c.size
    frames = np.stack([np.roll(np.array(c.src), 7 * i, axis=1) for i in range(n)]) if n else np.zeros((0, Hs, Ws, 3), np.uint8)
    big = torch.full((n + 1, Hs + 2, 3 * Ws + 5), 201, dtype=torch.uint8, device=DEV)
    view = big[:n, 1:Hs + 1, 2:3 * Ws + 2].unflatten(2, (Ws, 3))
    view.copy_(torch.from_numpy(frames).to(DEV))
    assert n == 0 or (view.stride(1) > 3 * Ws and not view.is_contiguous())     # (torch makes up the strides of an empty view)
    assert n < 2 or view.stride(0) > Hs * view.stride(1)
    for f in fr.FILTERS:
        want_u8 = F.resize_frames_host(frames, c.size, f)
        want = fr.normalised(want_u8, F.MEAN, F.STD) if n else torch.zeros((0, 3, H, W))
        tables = F.FrameTables(c.src_size, c.size, f, device=DEV)
        whole = torch.full((n + 2, 5, H, W), -7.0, device=DEV)
        out = whole[1:n + 1, 1:4]
        got, u8 = F.prepare_frames(view, c.size, tables=tables, out=out, return_u8=True)
        assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (n, 3, H, W)
        assert np.array_equal(u8.cpu().numpy(), want_u8), (n, f)
        assert torch.equal(_bits(got.cpu()), _bits(want)), (n, f)
        rest = whole.clone()
        rest[1:n + 1, 1:4] = -7.0
        assert bool((rest == -7.0).all()), (n, f)
        # a view the ABI cannot address (the RGB of RGBA pixels: a pixel stride of 4) is copied, not refused
        rgba = torch.full((n, Hs, Ws, 4), 9, dtype=torch.uint8, device=DEV)
        rgba[..., :3] = torch.from_numpy(frames).to(DEV)
        assert torch.equal(_bits(F.prepare_frames(rgba[..., :3], c.size, tables=tables).cpu()), _bits(want)), (n, f)
    assert bool((big[:n, 0] == 201).all()) and bool((big[n:] == 201).all())                     # the source is never written


@pytest.mark.parametrize("pair", fr.pair_ids())
def test_clip_preparer_frames_and_labels(pair):
    """``ClipPreparer``: frames as ``prepare_frames`` gives them, labels equal to the fixture's nearest resize."""
    c = fr.case(pair, "ramp")
    n = 2
    src = torch.from_numpy(np.stack([np.array(c.src)] * n)).to(DEV)
    lab = torch.from_numpy(np.stack([np.array(c.label_src)] * n)).to(DEV)
    for f in ("bicubic", "nearest"):
        prep = F.ClipPreparer(c.src_size, c.size, f, device=DEV)
        frames, labels = prep(src, lab)
        assert labels.dtype == torch.uint8 and tuple(labels.shape) == (n,) + c.size
        for i in range(n):
            assert np.array_equal(labels[i].cpu().numpy(), c.label), (c.name, f)
            assert torch.equal(_bits(frames[i].cpu()), _bits(fr.normalised(c.want[f], F.MEAN, F.STD))), (c.name, f)
        need = int(_lib.load().dmm_prepare_frames_workspace_bytes(n, *c.src_size, *c.size)) if f != "nearest" else 0
        assert (prep.workspace.numel() if prep.workspace is not None else 0) == need
        assert (need > 0) == (f != "nearest" and c.src_size[0] != c.size[0] and c.src_size[1] != c.size[1])
        frames2, none = prep(src)
        assert none is None and torch.equal(_bits(frames2), _bits(frames))


def test_replay_under_a_captured_graph():
    """A second call into ``out=`` under ``torch.cuda.graph`` replays to the same bytes, for new source bytes as well."""
    c = fr.case("90x160_32x56", "noise")
    src = torch.from_numpy(np.stack([np.array(c.src), np.array(c.src)[::-1].copy()])).to(DEV)
    prep = F.ClipPreparer(c.src_size, c.size, "bicubic", device=DEV)
    first, _ = prep(src)
    want = first.clone()
    out = torch.zeros_like(first)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        prep(src, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(want))
    src.copy_(src.flip(0))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(want.flip(0)))


def _entry_args(Hs, Ws, H, W, kx, ky, n=1):
    """Dense device buffers for a direct entry call with tables of the given widths (zeros: never read where the entry refuses)."""
    z = lambda m, dt: torch.zeros((max(m, 1),), dtype=dt, device=DEV)
    return dict(src=z(n * Hs * Ws * 3, torch.uint8), bx=z(2 * W, torch.int32), cx=z(W * kx, torch.int32), by=z(2 * H, torch.int32),
                cy=z(H * ky, torch.int32), lut=z(768, torch.float32), f32=z(n * 3 * H * W, torch.float32), u8=z(n * H * W * 3, torch.uint8))


def _entry(a, Hs, Ws, H, W, kx, ky, n=1, C=3, ws=None, ws_bytes=0, **over):
    p = {k: v.data_ptr() for k, v in a.items()}
    p.update(over)
    return _lib.load().dmm_prepare_frames_u8(p["src"], Hs * Ws * 3, Ws * 3, n, C, Hs, Ws, H, W, p["bx"], p["cx"], kx, p["by"], p["cy"], ky,
                                             p["lut"], p["f32"], 3 * H * W, H * W, p["u8"], H * W * 3, ws, ws_bytes,
                                             torch.cuda.current_stream().cuda_stream)


def test_the_entry_answers_in_the_documented_order():
    """include/dmm_match.h (16): the tap cap answers DMM_ERR_UNSUPPORTED without launching; so do the other answers before a
    launch; where two faults coincide the earlier one is named."""
    L = _lib.load()
    import re
    with open(_lib.HEADER) as fh:
        cap = int(re.search(r"^#define\s+DMM_RESAMPLE_MAX_TAPS\s+(\d+)", fh.read(), re.M).group(1))
    big_b, big_c = F.resample_tables(130, 1, "bicubic")
    assert big_c.shape[1] > cap
    a = _entry_args(1, 130, 1, 1, big_c.shape[1], 0)
    l0 = _launches()
    assert _entry(a, 1, 130, 1, 1, big_c.shape[1], 0) == _lib.DMM_ERR_UNSUPPORTED            # the tap cap, horizontal
    a = _entry_args(130, 1, 1, 1, 0, big_c.shape[1])
    assert _entry(a, 130, 1, 1, 1, 0, big_c.shape[1]) == _lib.DMM_ERR_UNSUPPORTED            # vertical
    with pytest.raises(_lib.DmmError, match="outside the compiled kernel envelope"):
        F.prepare_frames(torch.zeros((1, 1, 130, 3), dtype=torch.uint8, device=DEV), (1, 1))
    a = _entry_args(8, 8, 3, 5, 7, 9)
    assert _entry(a, 8, 8, 3, 5, 7, 9, n=-1) == _lib.DMM_ERR_BAD_ARG                          # 1. negative
    assert _entry(a, 8, 8, 3, 5, 7, 9, n=0, src=None) == _lib.DMM_OK                          # 2. nothing to do: pointers not looked at
    assert _entry(a, 8, 8, 0, 5, 7, 9, src=None) == _lib.DMM_OK
    assert _entry(a, 8, 8, 3, 5, 7, 9, src=None) == _lib.DMM_ERR_BAD_ARG                      # 3. required pointers
    assert _entry(a, 8, 8, 3, 5, 7, 9, f32=None, u8=None) == _lib.DMM_ERR_BAD_ARG
    assert _entry(a, 8, 8, 3, 5, 7, 9, cx=None) == _lib.DMM_ERR_BAD_ARG
    assert _entry(a, 8, 8, 3, 5, 7, 9, by=None) == _lib.DMM_ERR_BAD_ARG
    assert _entry(a, 8, 8, 3, 5, 7, 9, lut=None) == _lib.DMM_ERR_BAD_ARG
    assert _entry(a, 8, 8, 3, 5, 7, 9, C=4) == _lib.DMM_ERR_UNSUPPORTED                       # 4. the envelope
    assert _entry(a, 8, 8, 3, 5, cap + 1, 9, C=4, cx=None) == _lib.DMM_ERR_BAD_ARG            # (3 before 4)
    assert _entry(a, 8, 8, 3, 5, 7, 9) == _lib.DMM_ERR_WORKSPACE                              # 5. the workspace: null
    need = int(L.dmm_prepare_frames_workspace_bytes(1, 8, 8, 3, 5))
    assert need == 8 * 16
    ws = torch.zeros((need + 16,), dtype=torch.uint8, device=DEV)
    assert _entry(a, 8, 8, 3, 5, 7, 9, ws=ws.data_ptr(), ws_bytes=need - 1) == _lib.DMM_ERR_WORKSPACE
    assert _entry(a, 8, 8, 3, 5, 7, 9, ws=ws.data_ptr() + 4, ws_bytes=need) == _lib.DMM_ERR_WORKSPACE
    assert _entry(a, 8, 8, 3, 5, cap + 1, 9, ws=None) == _lib.DMM_ERR_UNSUPPORTED             # (4 before 5)
    assert _launches() == l0                                                                  # nothing was launched
    assert int(L.dmm_prepare_frames_workspace_bytes(1, 8, 8, 8, 5)) == 0 and int(L.dmm_prepare_frames_workspace_bytes(0, 8, 8, 3, 5)) == 0


def test_tables_with_any_values_read_inside_the_source():
    """The tables are read as they stand: bounds far outside the source are clamped into it (include/dmm_match.h (16)), so the
    result is that of the clamped tables -- computed here in numpy."""
    Hs, Ws, H, W, k = 6, 9, 4, 5, 3
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)
    bx = np.array([[8, 7], [2, 3], [-5, 9], [100, 2], [3, -1]], dtype=np.int32)      # (column 0 sets the staged window: 1 pixel)
    by = np.array([[5, 3], [-1, 2], [0, 0], [2, 50]], dtype=np.int32)
    cx = rng.integers(0, 1 << 21, (W, k), dtype=np.int32)
    cy = rng.integers(0, 1 << 21, (H, k), dtype=np.int32)

    def one_pass(x, axis, b, c, n_in):
        x = np.moveaxis(x.astype(np.int64), axis, 0)
        out = np.zeros((b.shape[0],) + x.shape[1:], dtype=np.int64)
        for i, (lo, cnt) in enumerate(b):
            lo = min(max(int(lo), 0), n_in)
            cnt = min(max(int(cnt), 0), min(k, n_in - lo))
            acc = (1 << 21) + sum(int(c[i, j]) * x[lo + j] for j in range(cnt))
            out[i] = np.clip(acc >> 22, 0, 255)
        return np.moveaxis(out, 0, axis).astype(np.uint8)
    want = one_pass(one_pass(src[0], 1, bx, cx, Ws), 0, by, cy, Hs)
    t = lambda a: torch.from_numpy(a).to(DEV)
    a = dict(src=t(src), bx=t(bx), cx=t(cx), by=t(by), cy=t(cy), lut=F.normalise_lut().to(DEV), f32=torch.zeros((3, H, W), device=DEV),
             u8=torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV))
    need = int(_lib.load().dmm_prepare_frames_workspace_bytes(1, Hs, Ws, H, W))
    ws = torch.zeros((need,), dtype=torch.uint8, device=DEV)
    assert _entry(a, Hs, Ws, H, W, k, k, ws=ws.data_ptr(), ws_bytes=need) == _lib.DMM_OK
    torch.cuda.synchronize()
    assert np.array_equal(a["u8"].cpu().numpy(), want)
    assert torch.equal(_bits(a["f32"].cpu()), _bits(fr.normalised(want, F.MEAN, F.STD)))


def test_wrapper_argument_errors_on_the_device():
    x = torch.zeros((2, 4, 5, 3), dtype=torch.uint8, device=DEV)
    tables = F.FrameTables((4, 5), (2, 3), device=DEV)
    with pytest.raises(ValueError):
        F.prepare_frames(x, (3, 3), tables=tables)                             # tables of another size
    with pytest.raises(ValueError):
        F.prepare_frames(x[:, :3], (2, 3), tables=tables)
    with pytest.raises(ValueError):
        F.prepare_frames(x, (2, 3), tables=tables, out=torch.zeros((2, 3, 2, 4), device=DEV))
    with pytest.raises(ValueError):
        F.prepare_frames(x, (2, 3), tables=tables, out=torch.zeros((2, 3, 3, 2), device=DEV).transpose(2, 3))
    with pytest.raises(ValueError):
        F.prepare_frames(torch.zeros((1, 0, 5, 3), dtype=torch.uint8, device=DEV), (2, 3))
    prep = F.ClipPreparer((4, 5), (2, 3), device=DEV)
    with pytest.raises(ValueError):
        prep(x, torch.zeros((2, 4, 4), dtype=torch.uint8, device=DEV))
    with pytest.raises(_lib.DmmError, match="no CPU fallback"):
        prep(x, torch.zeros((2, 4, 5), dtype=torch.uint8))
    assert tuple(F.prepare_frames(x, (0, 3)).shape) == (2, 3, 0, 3)


def test_clip_preparer_feeds_augment_clip():
    """``ClipPreparer -> augment_clip`` with an identity matrix and no flip returns the prepared frames and labels unchanged."""
    from dmm_net_amd import augment as A
    c = fr.case("90x160_32x56", "noise")
    n = 3
    src = torch.from_numpy(np.stack([np.roll(np.array(c.src), i, axis=0) for i in range(n)])).to(DEV)
    lab = torch.from_numpy(np.stack([np.roll(np.array(c.label_src), i, axis=0) for i in range(n)])).to(DEV)
    frames, labels = F.ClipPreparer(c.src_size, c.size, "bicubic", device=DEV)(src, lab)
    got = A.augment_clip(frames, labels, matrices=torch.eye(3).repeat(n, 1, 1), flip=False, max_obj=5)
    assert torch.equal(_bits(got.frames), _bits(frames)) and torch.equal(got.labels, labels)
    assert torch.equal(got.targets[:, 0], (labels == 1).float())
