"""Helpers of the resized-measures tests (no test functions here): the index rule of include/dmm_match.h (14b) as a plain
Python loop -- written from the header's three lines, sharing nothing with ``dmm_net_amd.measures.nearest_table`` --, the
closed form it must NOT be mistaken for, the table gather in numpy, and seeded label maps."""
import numpy as np


def table_loop(n_in, n_out):
    """a = n_in / n_out in double; o = a * 0.5; tab[i] = int(o); o += a -- Python floats are C doubles."""
    tab = np.zeros(n_out, dtype=np.int32)
    if n_out == 0:
        return tab
    a = float(n_in) / float(n_out)
    o = a * 0.5
    for i in range(n_out):
        tab[i] = -1 if o < 0 else int(o)
        o += a
    return tab


def closed_form(n_in, n_out):
    """floor((i + 0.5) * n_in / n_out): the textbook nearest rule, which PIL's walk is not."""
    i = np.arange(n_out, dtype=np.float64)
    return np.floor((i + 0.5) * n_in / n_out).astype(np.int32)


def gather(labels, ty, tx):
    """[..,Hs,Ws] -> [..,len(ty),len(tx)] through two index tables; an index outside the source reads as 0."""
    labels = np.asarray(labels)
    Hs, Ws = labels.shape[-2:]
    ty, tx = np.asarray(ty, dtype=np.int64), np.asarray(tx, dtype=np.int64)
    out = np.zeros(labels.shape[:-2] + (len(ty), len(tx)), dtype=labels.dtype)
    oky, okx = (ty >= 0) & (ty < Hs), (tx >= 0) & (tx < Ws)
    ys, xs = np.nonzero(oky)[0], np.nonzero(okx)[0]
    if len(ys) and len(xs):
        out[..., ys[:, None], xs[None, :]] = labels[..., ty[ys][:, None], tx[xs][None, :]]
    return out


def resize(labels, size):
    """The yardstick's resize: the loop's tables, then the gather."""
    Hs, Ws = np.asarray(labels).shape[-2:]
    return gather(labels, table_loop(Hs, size[0]), table_loop(Ws, size[1]))


def label_maps(rng, T, H, W, n_labels):
    """Seeded label maps [T,H,W] of random blocks (1, 2 or 5 pixels wide), labels 0 .. n_labels, objects against every edge."""
    out = np.zeros((T, H, W), dtype=np.uint8)
    for t in range(T):
        bs = int(rng.choice([1, 2, 5]))
        coarse = rng.integers(0, n_labels + 1, size=(-(-H // bs), -(-W // bs)))
        coarse[rng.random(coarse.shape) < 0.3] = 0
        out[t] = np.kron(coarse, np.ones((bs, bs), dtype=np.int64))[:H, :W]
    return out
