"""The cases of tests/golden/frames_resized.npz for the frame-preparation tests (no test functions here): each size pair and
pattern with its source (from the generator's own ``source``: the fixture holds Pillow's results only), Pillow's three
results, and the pair's label map with its nearest resize.  Loaded once and shared; nothing in it is written."""
import importlib.util
import os
from collections import namedtuple

import numpy as np

from conftest import GOLDEN, golden

_spec = importlib.util.spec_from_file_location("gen_golden_frames", os.path.join(GOLDEN, "gen_golden_frames.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

PAIRS, FILTERS, PATTERNS = gen.PAIRS, gen.FILTERS, gen.PATTERNS
Case = namedtuple("Case", "name pattern src_size size src want label_src label")     # want: {filter: uint8 [H,W,3]}
_CASES = {}


def pair_ids():
    return [gen.pair_name(s, d) for s, d in PAIRS]


def case(pair, pattern):
    """The case of one pair name and pattern (arrays read-only)."""
    key = (pair, pattern)
    if key not in _CASES:
        z = golden("frames_resized")
        i = pair_ids().index(pair)
        (Hs, Ws), (H, W) = PAIRS[i]
        arrays = [gen.source(pattern, Hs, Ws, gen.seed_of(i, PATTERNS.index(pattern))), z[f"label_{pair}_src"], z[f"label_{pair}"]]
        want = {f: z[f"{pattern}_{pair}_{f}"] for f in FILTERS}
        for a in arrays + list(want.values()):
            a.setflags(write=False)
        _CASES[key] = Case(f"{pattern}_{pair}", pattern, (Hs, Ws), (H, W), arrays[0], want, arrays[1], arrays[2])
    return _CASES[key]


def normalised(u8, mean, std):
    """``ToTensor`` + ``Normalize`` of uint8 [..,H,W,3] by torch on the CPU, the reference's operations in its order:
    fp32 [..,3,H,W]."""
    import torch
    t = torch.from_numpy(np.array(u8))                         # (a copy: the fixture's arrays are read-only)
    t = t.permute(*range(t.dim() - 3), -1, -3, -2).contiguous().float().div(255)
    m, s = (torch.tensor(v, dtype=torch.float32).view(3, 1, 1) for v in (mean, std))
    return t.sub(m).div(s)
