"""NumPy restatement of the device LSAP kernel (dmm_net_amd/csrc/dmm_lsap.hip) in its PARALLEL form.

scipy's ``linear_sum_assignment`` is Crouse's shortest augmenting path (rectangular_lsap.cpp) in fp64.  Its column
choice is a sequential scan over ``remaining``: ``spc[j] < lowest || (spc[j] == lowest && row4col[j] == -1)``.  The
kernel replaces the scan by an order-free reduction over the columns, each of which knows its position in
``remaining``: the smallest ``spc`` wins; at equal ``spc`` an unassigned column beats an assigned one; among unassigned
columns the LARGEST position wins, among assigned ones the SMALLEST.  This module runs exactly that reduction (whole-
vector steps, no scan), so the CPU test pins the tie rule the kernel relies on against scipy itself.
"""
from __future__ import annotations

import numpy as np

OK, INVALID, INFEASIBLE = 0, 1, 2


def _rank(spc, lowest, assigned, pos, alive):
    """Per-column rank of the scan rule among the live candidates with spc == lowest (-1 = not a candidate).
    Unassigned: 512 + pos (largest position first); assigned: 511 - pos (smallest position first)."""
    cand = alive & (spc == lowest)
    r = np.where(assigned, 511 - pos, 512 + pos)
    return np.where(cand, r, -1)


def solve_wide(c: np.ndarray):
    """One table c [nr, nc] with nr <= nc, float64 -> (col4row [nr] int, status)."""
    nr, nc = c.shape
    if np.isnan(c).any() or (c == -np.inf).any():
        return np.full(nr, -1, np.int64), INVALID
    u = np.zeros(nr)
    v = np.zeros(nc)
    col4row = np.full(nr, -1, np.int64)
    row4col = np.full(nc, -1, np.int64)
    path = np.full(nc, -1, np.int64)
    for cur in range(nr):
        pos = nc - 1 - np.arange(nc)                 # remaining[it] = nc-1-it  <=>  column j sits at position nc-1-j
        num = nc
        SR = np.zeros(nr, bool)
        spc = np.full(nc, np.inf)
        min_val = 0.0
        i = cur
        sink = -1
        while sink == -1:
            SR[i] = True
            alive = pos >= 0
            r = ((min_val + c[i]) - u[i]) - v         # scipy's evaluation order
            upd = alive & (r < spc)
            path = np.where(upd, i, path)
            spc = np.where(upd, r, spc)
            lowest = np.min(np.where(alive, spc, np.inf))
            min_val = lowest
            if lowest == np.inf:
                return np.full(nr, -1, np.int64), INFEASIBLE
            rank = _rank(spc, lowest, row4col >= 0, pos, alive)
            j = int(np.argmax(rank))                  # unique: the rank encodes the position
            p = pos[j]
            num -= 1
            pos = np.where(pos == num, p, pos)        # remaining[index] = remaining[--num]
            pos[j] = -1                               # (j leaves remaining: SC[j])
            if row4col[j] == -1:
                sink = j
            else:
                i = int(row4col[j])
        SC = pos < 0
        u[cur] += min_val
        others = SR.copy()
        others[cur] = False
        idx = np.nonzero(others)[0]
        u[idx] += min_val - spc[col4row[idx]]
        v[SC] -= min_val - spc[SC]
        j = sink
        while True:
            i = int(path[j])
            row4col[j] = i
            col4row[i], j = j, int(col4row[i])
            if i == cur:
                break
    return col4row, OK


def linear_sum_assignment(c: np.ndarray):
    """float32/float64 [nr, nc] -> (col_of_row [nr], -1 where a row stays unassigned; status).  nr > nc solves the
    transposed table, as scipy does."""
    c = np.asarray(c).astype(np.float64)
    nr, nc = c.shape
    if nr == 0 or nc == 0:
        return np.full(nr, -1, np.int64), OK
    if nr <= nc:
        return solve_wide(c)
    c4r_t, st = solve_wide(c.T.copy())
    out = np.full(nr, -1, np.int64)
    if st == OK:
        out[c4r_t] = np.arange(nc)
    return out, st


FAMILIES = ("random", "small_int", "constant", "zero", "signed_zero", "huge", "denormal")


def make_table(rng: np.random.Generator, family: str, nr: int, nc: int) -> np.ndarray:
    """One float32 [nr, nc] cost table of a family the device solver must get exactly right (ties included)."""
    if family == "random":
        return rng.standard_normal((nr, nc)).astype(np.float32)
    if family == "small_int":                              # tie-heavy: few distinct integer values
        return rng.integers(-2, 3, (nr, nc)).astype(np.float32)
    if family == "constant":
        return np.full((nr, nc), rng.integers(-3, 4), np.float32)
    if family == "zero":
        return np.zeros((nr, nc), np.float32)
    if family == "signed_zero":                            # -0.0 / +0.0 mixtures, some small values (padded columns)
        c = np.where(rng.random((nr, nc)) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        k = rng.random((nr, nc)) < 0.2
        c[k] = rng.integers(-1, 2, int(k.sum())).astype(np.float32)
        return c
    if family == "huge":
        return (rng.standard_normal((nr, nc)) * 1e30).astype(np.float32)
    if family == "denormal":
        return (rng.integers(-4, 5, (nr, nc)) * np.float32(1e-45) +
                (rng.random((nr, nc)) < 0.3) * rng.integers(1, 9, (nr, nc)) * np.float32(1e-40)).astype(np.float32)
    raise ValueError(family)
