"""The parallel form of the device LSAP solver (tests/lsap_model.py: the scan rule as an order-free rank reduction)
picks exactly what scipy.optimize.linear_sum_assignment picks, ties included.  Host only."""
import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import lsap_model


def _scipy_col_of_row(c):
    r, col = linear_sum_assignment(c)
    out = np.full(c.shape[0], -1, np.int64)
    out[r] = col
    return out


@pytest.mark.parametrize("family", lsap_model.FAMILIES)
def test_model_matches_scipy(family):
    rng = np.random.default_rng(lsap_model.FAMILIES.index(family) + 7)
    n = 0
    for _ in range(1500):
        nc = int(rng.integers(1, 12))
        nr = int(rng.integers(1, nc + 1)) if rng.random() < 0.8 else int(rng.integers(nc + 1, nc + 5))  # nr > nc: T
        c = lsap_model.make_table(rng, family, nr, nc)
        got, st = lsap_model.linear_sum_assignment(c)
        assert st == lsap_model.OK
        np.testing.assert_array_equal(got, _scipy_col_of_row(c), err_msg=f"{family} {c!r}")
        n += 1
    assert n == 1500


def test_model_wide_tables_match_scipy():
    """The kernel's envelope reaches 32 x 256: a few wide, tie-heavy tables."""
    rng = np.random.default_rng(3)
    for k in range(60):
        nc = int(rng.integers(20, 257))
        nr = int(rng.integers(1, min(nc, 32) + 1))
        c = lsap_model.make_table(rng, ("random", "small_int", "signed_zero")[k % 3], nr, nc)
        got, st = lsap_model.linear_sum_assignment(c)
        assert st == lsap_model.OK
        np.testing.assert_array_equal(got, _scipy_col_of_row(c))


def test_model_invalid_and_infeasible_follow_scipy():
    c = np.zeros((3, 4), np.float32)
    for bad in (np.nan, -np.inf):
        d = c.copy()
        d[1, 2] = bad
        assert lsap_model.linear_sum_assignment(d)[1] == lsap_model.INVALID
        with pytest.raises(ValueError):
            linear_sum_assignment(d)
    d = c.copy()
    d[:, :3] = np.inf
    d[:2, 3] = 0                                        # rows 0 and 1 both need column 3
    d[2, 3] = np.inf
    assert lsap_model.linear_sum_assignment(d)[1] == lsap_model.INFEASIBLE
    with pytest.raises(ValueError):
        linear_sum_assignment(d)
