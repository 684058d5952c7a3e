"""The host side of the frame preparation (dmm_net_amd/frames.py, include/dmm_match.h (16)): the numpy restatement of PIL's 8-bit
resize against tests/golden/frames_resized.npz (and against Pillow itself where it imports), the coefficient tables, the
normalisation table and the wrappers' argument errors.  Every comparison is an integer or bit equality."""
import numpy as np
import pytest
import torch

import frames_ref as fr
from dmm_net_amd import _lib, frames as F


@pytest.mark.parametrize("pattern", fr.PATTERNS)
@pytest.mark.parametrize("pair", fr.pair_ids())
def test_resize_frames_host_equals_the_fixture(pair, pattern):
    c = fr.case(pair, pattern)
    for f in fr.FILTERS:
        got = F.resize_frames_host(c.src, c.size, f)
        assert got.dtype == np.uint8 and got.shape == c.want[f].shape
        assert np.array_equal(got, c.want[f]), (c.name, f, int((got != c.want[f]).sum()))
    both = F.resize_frames_host(np.stack([c.src, c.src[::-1, ::-1]]), c.size, "bicubic")       # leading dimensions
    assert np.array_equal(both[0], c.want["bicubic"])
    assert np.array_equal(both[1], F.resize_frames_host(np.ascontiguousarray(c.src[::-1, ::-1]), c.size, "bicubic"))


@pytest.mark.parametrize("pair", fr.pair_ids())
def test_the_fixture_and_the_rule_equal_pillow(pair):
    Image = pytest.importorskip("PIL.Image")
    flt = {"nearest": Image.NEAREST, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}
    for pattern in fr.PATTERNS:
        c = fr.case(pair, pattern)
        H, W = c.size
        for f in fr.FILTERS:
            pil = np.array(Image.fromarray(np.array(c.src)).resize((W, H), flt[f]))
            assert np.array_equal(pil, c.want[f]), (c.name, f)
            assert np.array_equal(pil, F.resize_frames_host(c.src, c.size, f)), (c.name, f)
    c = fr.case(pair, "noise")
    lab = np.array(Image.fromarray(np.array(c.label_src)).resize(c.size[::-1], Image.NEAREST))
    assert np.array_equal(lab, c.label)


def test_the_fixture_holds_the_cases():
    z = fr.golden("frames_resized")
    want_pairs = ["37x53_19x23", "19x23_37x53", "31x45_31x20", "31x45_12x45", "8x8_3x5", "5x3_9x7", "64x64_1x1", "2x3_64x67",
                  "90x160_32x56", "20x24_20x24"]
    assert fr.pair_ids() == want_pairs
    keys = set(z.keys())
    for pair, ((Hs, Ws), (H, W)) in zip(want_pairs, fr.PAIRS):
        for pattern in ("noise", "ramp"):
            for f in ("nearest", "bilinear", "bicubic"):
                a = z[f"{pattern}_{pair}_{f}"]
                assert a.dtype == np.uint8 and a.shape == (H, W, 3)
            assert fr.case(pair, pattern).src.shape == (Hs, Ws, 3)
        assert z[f"label_{pair}_src"].shape == (Hs, Ws) and z[f"label_{pair}"].shape == (H, W)
        assert f"label_{pair}" in keys
    # what the shapes are there for: widths on both sides of a 4-pixel store and of a 64-lane row, clamped and cut taps, tap
    # counts from 3 to the cap, the skipped passes
    widths = {W for _, (_, W) in fr.PAIRS}
    assert {1, 5, 7} & widths and any(W % 4 for W in widths) and any(W < 64 for W in widths) and any(W > 64 for W in widths)
    ks = {F.resample_tables(s, d, f)[1].shape[1] for (Hs, Ws), (H, W) in fr.PAIRS for s, d in ((Hs, H), (Ws, W)) for f in ("bilinear", "bicubic")}
    assert min(ks) == 3 and max(ks) == _header_cap() == 257


def _header_cap():
    import re
    with open(_lib.HEADER) as f:
        return int(re.search(r"^#define\s+DMM_RESAMPLE_MAX_TAPS\s+(\d+)", f.read(), re.M).group(1))


@pytest.mark.parametrize("filter,support", [("bilinear", 1.0), ("bicubic", 2.0)])
@pytest.mark.parametrize("n_in,n_out", [(53, 23), (23, 53), (64, 1), (3, 67), (160, 56), (1280, 448), (720, 255), (24, 24), (1, 1), (1, 9)])
def test_resample_tables(n_in, n_out, filter, support):
    bounds, coef = F.resample_tables(n_in, n_out, filter)
    ksize = int(np.ceil(support * max(n_in / n_out, 1.0))) * 2 + 1
    assert bounds.dtype == np.int32 and coef.dtype == np.int32
    assert bounds.shape == (n_out, 2) and coef.shape == (n_out, ksize)
    lo, cnt = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
    assert (lo >= 0).all() and (cnt >= 1).all() and (cnt <= ksize).all() and (lo + cnt <= n_in).all()
    assert (np.diff(lo) >= 0).all() and (np.diff(lo + cnt) >= 0).all()
    assert lo[0] == 0 and lo[-1] + cnt[-1] == n_in                      # clamped at 0, cut at n_in
    k = np.arange(ksize)[None, :]
    assert (coef[k >= cnt[:, None]] == 0).all()
    # every weight is rounded to 2^-22 once: a row sums to 2^22 within half a unit per tap
    assert (np.abs(coef.astype(np.int64).sum(1) - (1 << 22)) <= cnt).all()
    if filter == "bilinear":
        assert (coef >= 0).all()
    # the worst accumulator stays inside int32
    assert 255 * int(np.abs(coef.astype(np.int64)).sum(1).max()) + (1 << 21) < (1 << 31)


def test_resample_tables_argument_errors():
    for bad in ((0, 4, "bicubic"), (4, 0, "bicubic"), (-1, 4, "bilinear"), (4, 4, "nearest"), (4, 4, "lanczos")):
        with pytest.raises(ValueError):
            F.resample_tables(*bad)


def test_normalise_lut_equals_the_torch_formula():
    for mean, std in ((F.MEAN, F.STD), ((0.5, 0.25, 0.125), (1.0, 0.5, 0.3))):
        lut = F.normalise_lut(mean, std)
        assert lut.dtype == torch.float32 and tuple(lut.shape) == (3, 256) and lut.is_contiguous()
        u8 = torch.arange(256, dtype=torch.uint8).view(256, 1, 1).repeat(1, 1, 3).numpy()              # [256,1,3]: one column image
        want = fr.normalised(u8, mean, std)                                                            # [3,256,1]
        assert torch.equal(lut.view(torch.int32), want[:, :, 0].contiguous().view(torch.int32))        # all 768 values, bit for bit
    with pytest.raises(ValueError):
        F.normalise_lut((0.5, 0.5), (1.0, 1.0))


def test_host_resize_argument_errors():
    x = np.zeros((4, 5, 3), dtype=np.uint8)
    with pytest.raises(ValueError):
        F.resize_frames_host(x.astype(np.float32), (2, 2))
    with pytest.raises(ValueError):
        F.resize_frames_host(x[..., :2], (2, 2))
    with pytest.raises(ValueError):
        F.resize_frames_host(x, (2, 2), "box")
    with pytest.raises(ValueError):
        F.resize_frames_host(x, (-1, 2))
    with pytest.raises(ValueError):
        F.resize_frames_host(np.zeros((0, 5, 3), dtype=np.uint8), (2, 2), "bilinear")
    assert F.resize_frames_host(x, (0, 7)).shape == (0, 7, 3)
    assert F.resize_frames_host(np.zeros((0, 4, 5, 3), dtype=np.uint8), (2, 2)).shape == (0, 2, 2, 3)
    assert F.resize_frames_host(np.zeros((0, 5, 3), dtype=np.uint8), (2, 2), "nearest").sum() == 0


def test_wrapper_argument_errors_without_a_device():
    """What the wrappers refuse before they touch the device: host tensors (no CPU fallback), wrong dtypes and shapes, an
    unknown filter."""
    x = torch.zeros((2, 4, 5, 3), dtype=torch.uint8)
    with pytest.raises(_lib.DmmError, match="no CPU fallback"):
        F.prepare_frames(x, (2, 2))
    with pytest.raises(_lib.DmmError, match="no CPU fallback"):
        F.ClipPreparer((4, 5), (2, 2), device="cpu")
    for bad in (torch.zeros((2, 4, 5, 3), dtype=torch.float32), torch.zeros((2, 4, 5, 4), dtype=torch.uint8),
                torch.zeros((4, 5, 3), dtype=torch.uint8), np.zeros((2, 4, 5, 3), dtype=np.uint8)):
        with pytest.raises(ValueError):
            F.prepare_frames(bad, (2, 2))
    with pytest.raises(ValueError):
        F.prepare_frames(x, (2, 2), filter="lanczos")
    import dmm_net_amd
    for name in ("resample_tables", "normalise_lut", "resize_frames_host", "prepare_frames", "ClipPreparer"):
        assert getattr(dmm_net_amd, name) is getattr(F, name)


def test_the_header_declares_the_entries():
    assert {"dmm_prepare_frames_workspace_bytes", "dmm_prepare_frames_u8", "dmm_prepare_frames_nearest_u8"} <= set(_lib.SYMBOLS)
    assert _header_cap() >= 65
