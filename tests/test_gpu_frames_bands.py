"""The frame preparation between guard bands (tests/guarded.py): one row per size pair of tests/golden/frames_resized.npz and
filter, run through ``run_row`` of test_gpu_guard_bands.  The two outputs of ``prepare_frames`` (fp32 planes and the uint8
image), the frames and labels of ``ClipPreparer`` and its workspace -- exactly ``dmm_prepare_frames_workspace_bytes`` -- sit
between poisoned bands, the sources between bands of live values (255: a tap or a gather past a row would show in the bytes)."""
import numpy as np
import pytest
import torch

import frames_ref as fr
import test_gpu_guard_bands as tgb
from dmm_net_amd import _lib, frames as F

pytestmark = pytest.mark.gpu
DEV = tgb.DEV


@pytest.mark.parametrize("f", fr.FILTERS)
@pytest.mark.parametrize("pair", fr.pair_ids())
def test_prepare_frames_between_bands(pair, f):
    c = fr.case(pair, "noise")
    n = 2
    src = torch.from_numpy(np.stack([np.array(c.src), np.array(c.src)[::-1, ::-1].copy()])).to(DEV)
    lab = torch.from_numpy(np.stack([np.array(c.label_src)] * n)).to(DEV)
    need = int(_lib.load().dmm_prepare_frames_workspace_bytes(n, *c.src_size, *c.size)) if f != "nearest" else 0

    def call(frames_u8, labels_u8):
        prep = F.ClipPreparer(c.src_size, c.size, f, device=DEV)
        frames, labels = prep(frames_u8, labels_u8)
        assert (prep.workspace.numel() if prep.workspace is not None else 0) == need
        planes, u8 = F.prepare_frames(frames_u8, c.size, tables=prep.tables, return_u8=True)
        return {"out": [frames, labels, planes, u8], "ws": [prep.workspace] if need else []}
    A, B = tgb.run_row(f"frames/{pair}/{f}", lambda w: (w(src, 255), w(lab, 255)), call)
    for got in (A, B):
        assert np.array_equal(got[3][0].cpu().numpy(), c.want[f]), (pair, f)
        assert np.array_equal(got[1][0].cpu().numpy(), c.label), (pair, f)
        assert tgb.same_bits(got[0], got[2])
