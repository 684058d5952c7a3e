"""tests/wgrad_ref.py held on the host, no GPU: the nine-slice reference against float64 ``F.conv2d`` autograd, the precondition of
the exact family, every table literal against the library's host planner, the coverage of the tables, and the derived bound
against an fp32 host product."""
import os

import pytest
import torch

import wgrad_ref as R
from dmm_net_amd import _lib

ROWS = R.ALL_1X1 + R.ALL_3X3
CASES = [row[0] for row in ROWS]


def _L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


@pytest.mark.parametrize("case", [(2, 17, 23, 64, 64, 1), (2, 17, 23, 64, 64, 2), (2, 16, 24, 64, 64, 1), (2, 16, 24, 64, 64, 2),
                                  (3, 1, 1, 64, 64, 1), (1, 1, 5, 64, 64, 2), (2, 2, 3, 64, 128, 2), (9, 3, 2, 128, 64, 2)], ids=R.case_id)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_nine_slices_are_conv2d_autograd(case, family):
    """The reference shares no code with a convolution; float64 ``F.conv2d`` autograd agrees to 1e-12 of max|ref| at both strides,
    odd and even sizes (even sizes at stride 2: the right and bottom padding unused)."""
    ref, A = R.reference(case, family)
    auto = R.conv2d_autograd(case, family)
    assert ref.shape == auto.shape == (case[4], case[3], 3, 3)
    assert float((ref - auto).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert bool((A >= ref.abs()).all())


@pytest.mark.parametrize("case", CASES, ids=R.case_id)
def test_int_family_is_exact_in_fp32(case):
    """The precondition of the exact test: the inputs are bf16 values (``inputs`` asserts the rounding changed nothing), the float64
    reference is representable in fp32, and an fp32 product in the host's order gives it bit for bit.  The outputs span the
    magnitudes the scales promise."""
    ref, A = R.reference(case, "int")
    assert torch.equal(ref.float().double(), ref)
    assert torch.equal(R.host_fp32(case, "int").double(), ref)
    n = R.dims(case)[0]
    assert float(A.max()) <= 9 * n * 2.0 ** 12 and 9 * n < 2 ** 24
    nz = ref[ref != 0].abs()
    if n >= 30:
        assert float(nz.max() / nz.min()) >= 2.0 ** 20


@pytest.mark.parametrize("row", ROWS, ids=lambda row: R.case_id(row[0]))
def test_table_literals_are_the_planners(row):
    case, groups, S = row
    rows, co, cv = R.dims(case)
    assert _L().dmm_wgrad_workspace_bytes(rows, co, cv) == 4 * groups * co * cv
    assert R.reduce_form(case, groups) == S
    table = R.CASES_3X3 if R.is_3x3(case) else R.CASES_1X1
    assert row in table[R.form(case)]


def test_tables_cover_every_cell():
    assert set(R.CASES_1X1) == {"wave", "lds", "tile64x128", "tile128x64"}
    assert set(R.CASES_3X3) == {"wave_patch", "lds_patch", "tile_patch"}
    for name, rows in R.CASES_1X1.items():                         # every plain form: the direct store and every S
        assert {S for _, _, S in rows} == {None, 1, 2, 4, 8, 16}, name
    for name, rows in R.CASES_3X3.items():                         # every patch form: every S of the 9-tap layout, never direct
        assert {S for _, _, S in rows} == {1, 2, 4, 8, 16}, name
    assert len(set(CASES)) == len(CASES)
    for case in R.STRIDED_1X1:
        assert case in CASES
    assert {R.form(c) for c in R.STRIDED_1X1} == set(R.CASES_1X1)
    # the mechanisms the shapes were chosen for
    stage = 64                                                     # output pixels of one stage of the staged kernels (32 rows x 2 slices)
    small = [c for c, _, _ in R.CASES_3X3["lds_patch"] if R.out_hw(c[1], c[2], c[5])[0] * R.out_hw(c[1], c[2], c[5])[1] < stage]
    assert any(R.out_hw(c[1], c[2], c[5]) == (1, 1) for c in small)
    assert any(R.out_hw(c[1], c[2], c[5])[1] == 1 and R.out_hw(c[1], c[2], c[5])[0] > 1 for c in small)
    assert any(R.out_hw(c[1], c[2], c[5])[0] == 1 and R.out_hw(c[1], c[2], c[5])[1] > 1 for c in small)
    assert any(c[0] < 32 for c, _, _ in R.CASES_1X1["lds"]) and any(c[0] < 256 for c, _, _ in R.CASES_1X1["tile128x64"])


def test_fp32_host_product_stays_inside_the_derived_bound():
    """``bound_worst`` is derived; this shows it is not violated by an fp32 evaluation in another order, and how far below it
    such an evaluation stays (the figure in the module's docstring)."""
    worst = []
    for case in CASES:
        ref, A = R.reference(case, "relu")
        q = R.scaled(R.host_fp32(case, "relu"), ref, A)
        b = R.bound_worst(R.dims(case)[0])
        assert q <= b, (case, q, b)
        worst.append((q / b, R.case_id(case)))
    worst.sort(reverse=True)
    print("wgrad_ref: largest scaled() / bound_worst of the host fp32 product:", worst[:3])


def test_scaled_sees_a_small_output_and_leaves_empty_sums_out():
    ref = torch.tensor([1.0, 1e-6, 0.0])
    A = torch.tensor([2.0, 2e-6, 0.0])
    assert R.scaled(ref, ref, A) == 0.0
    assert R.scaled(ref + torch.tensor([0.0, 1e-6, 0.0]), ref, A) == pytest.approx(0.5)      # invisible to max|err| / max|ref|
    assert R.scaled(torch.tensor([1.0, 1e-6, 5.0]), ref, A) == 0.0                             # (A == 0: compared exactly elsewhere)
    assert R.bound_worst(9000) == 9000 * 2.0 ** -23 and R.yardstick(0.0) == 2.0 ** -23
