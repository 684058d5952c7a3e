"""Writes tests/golden/frames_resized.npz: what Pillow's ``Image.resize`` returns for the size pairs of include/dmm_match.h (16)'s
tests.  Run it where Pillow imports (``python tests/golden/gen_golden_frames.py``); the tests read the file and need no Pillow.

Per size pair ``{Hs}x{Ws}_{H}x{W}`` and pattern (``noise``: seeded bytes; ``ramp``: a smooth gradient per channel):
  ``{pattern}_{pair}_{nearest|bilinear|bicubic}``  uint8 [H,W,3] = np.array(Image.fromarray(src).resize((W, H), filter))
with src = ``source(pattern, Hs, Ws, seed_of(i, j))``, uint8 [Hs,Ws,3]: the sources are integer and exact IEEE arithmetic, the same
bytes everywhere, so the tests import ``source`` from here and the file holds the results only (noise does not compress).
Per pair a label map ``label_{pair}_src`` uint8 [Hs,Ws] with ``label_{pair}`` = its NEAREST resize, as the reference resizes an
annotation (dmm/dataloader/dataset.py:213-215).  ``pillow_version`` records what produced the file."""
import os

import numpy as np

PAIRS = [((37, 53), (19, 23)), ((19, 23), (37, 53)), ((31, 45), (31, 20)), ((31, 45), (12, 45)), ((8, 8), (3, 5)),
         ((5, 3), (9, 7)), ((64, 64), (1, 1)), ((2, 3), (64, 67)), ((90, 160), (32, 56)), ((20, 24), (20, 24))]
FILTERS = ("nearest", "bilinear", "bicubic")
PATTERNS = ("noise", "ramp")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "frames_resized.npz")


def pair_name(src, dst):
    return "%dx%d_%dx%d" % (src + dst)


def seed_of(i, j):
    """The seed of pair ``i`` of PAIRS and pattern ``j`` of PATTERNS."""
    return 1600 + 10 * i + j


def source(pattern, Hs, Ws, seed):
    if pattern == "noise":                                  # a 64-bit mix of the byte's index: wrapping integer arithmetic only
        v = np.arange(Hs * Ws * 3, dtype=np.uint64) + np.uint64(seed * 1000003)
        v = v * np.uint64(6364136223846793005) + np.uint64(1442695040888963407)
        v ^= v >> np.uint64(33)
        v *= np.uint64(0xff51afd7ed558ccd)
        v ^= v >> np.uint64(33)
        return ((v >> np.uint64(24)) & np.uint64(255)).astype(np.uint8).reshape(Hs, Ws, 3)
    y, x = np.mgrid[0:Hs, 0:Ws].astype(np.float64)
    ch = [255.0 * x / max(Ws - 1, 1), 255.0 * y / max(Hs - 1, 1), 255.0 * (x + y) / max(Hs + Ws - 2, 1)]
    return np.floor(np.stack(ch, -1) + 0.5).astype(np.uint8)


def labels(Hs, Ws, seed):
    """Blocks of object ids 0 .. 5 with a few 255 ("ignore") pixels."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 6, ((Hs + 3) // 4, (Ws + 4) // 5), dtype=np.uint8)
    lab = np.repeat(np.repeat(coarse, 4, 0), 5, 1)[:Hs, :Ws].copy()
    lab[rng.random((Hs, Ws)) < 0.02] = 255
    return lab


def main():
    import PIL
    from PIL import Image
    flt = {"nearest": Image.NEAREST, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}
    data = {"pillow_version": np.array(PIL.__version__)}
    for i, ((Hs, Ws), (H, W)) in enumerate(PAIRS):
        pair = pair_name((Hs, Ws), (H, W))
        for j, pattern in enumerate(PATTERNS):
            src = source(pattern, Hs, Ws, seed_of(i, j))
            for name, f in flt.items():
                data[f"{pattern}_{pair}_{name}"] = np.array(Image.fromarray(src).resize((W, H), f))
        lab = labels(Hs, Ws, 1700 + i)
        data[f"label_{pair}_src"] = lab
        data[f"label_{pair}"] = np.array(Image.fromarray(lab).resize((W, H), Image.NEAREST))
    np.savez_compressed(OUT, **data)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
