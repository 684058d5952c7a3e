"""``dmm_wgrad_bf16`` / ``dmm_wgrad3x3_bf16`` (csrc/dmm_wgrad.hip) on the GPU against the float64 reference of tests/wgrad_ref.py, on
every route of the host planner: the four product kernels in their plain and implicit-patch forms, the direct store and all ten
``wgrad_reduce_kernel<S, T9>`` instantiations.  Everything is driven through the C entries, dw and the workspace (exactly
``dmm_wgrad_workspace_bytes`` of it) hold NaN before every call.  The ``"int"`` family must come back bit for bit (it carries the
indexing), the ``"relu"`` family within the derived worst-case bound and within the project's yardstick rule against torch's fp32
product of the same values on the same device."""
import pytest
import torch

import conv_narrow_ref
import wgrad_ref as R
from dmm_net_amd import _lib, ops
from dmm_net_amd import train_encoder as te

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
ROWS = R.ALL_1X1 + R.ALL_3X3
CASES = [row[0] for row in ROWS]
ROW_IDS = [R.case_id(row[0]) for row in ROWS]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _need(case):
    return int(_lib.load().dmm_wgrad_workspace_bytes(*R.dims(case)))


def _operands(case, family, strided=False):
    """-> (dy, x, ldy, ldx) on the device: dy [rows, co] and x [rows, ci], or NHWC for a 3x3 case.  ``strided``: dy the first co
    columns of rows of co + 64, x 64 elements into rows of ci + 128, everything around them NaN."""
    dy, x = R.inputs(case, family)
    if R.is_3x3(case):
        return dy.permute(0, 2, 3, 1).contiguous().to(DEV), x.permute(0, 2, 3, 1).contiguous().to(DEV), case[4], case[3]
    rows, co, ci = case
    if not strided:
        return dy.to(DEV), x.to(DEV), co, ci
    dyb = torch.full((rows, co + 64), NAN, dtype=torch.bfloat16, device=DEV)
    xb = torch.full((rows, ci + 128), NAN, dtype=torch.bfloat16, device=DEV)
    dyb[:, :co] = dy.to(DEV)
    xb[:, 64:64 + ci] = x.to(DEV)
    return dyb[:, :co], xb[:, 64:64 + ci], co + 64, ci + 128


def _entry(case, dy, x, ldy, ldx, short=0, dy_ptr=None):
    """One call of the case's C entry into a NaN-filled dw with a NaN-filled workspace of exactly the bytes the library asks for
    (``short`` fewer are declared) -> (status, dw, launches counted)."""
    L = _lib.load()
    need = _need(case)
    assert need > 0 and need % 4 == 0
    ws = torch.full((need // 4,), NAN, device=DEV)
    dy_ptr = dy.data_ptr() if dy_ptr is None else dy_ptr
    before = L.dmm_launch_count()
    if R.is_3x3(case):
        B, H, W, ci, co, stride = case
        dw = torch.full((co, ci, 3, 3), NAN, device=DEV)
        rc = L.dmm_wgrad3x3_bf16(dy_ptr, x.data_ptr(), B, H, W, ci, co, stride, dw.data_ptr(), ws.data_ptr(), need - short, _stream())
    else:
        rows, co, ci = case
        dw = torch.full((co, ci), NAN, device=DEV)
        rc = L.dmm_wgrad_bf16(dy_ptr, x.data_ptr(), rows, co, ci, ldy, ldx, dw.data_ptr(), ws.data_ptr(), need - short, _stream())
    launches = L.dmm_launch_count() - before
    torch.cuda.synchronize()
    return rc, dw, launches


def _run(case, family, strided=False):
    rc, dw, launches = _entry(case, *_operands(case, family, strided))
    assert rc == _lib.DMM_OK, rc
    return dw, launches


def _same_bits(got, ref64):
    """Every element of ``got`` (fp32, device) is the float64 reference: no NaN left, no element compared by a tolerance."""
    got = got.detach().cpu()
    assert got.dtype == torch.float32 and got.shape == ref64.shape
    bad = got.double() != ref64                                    # (NaN != anything: an element left unwritten is counted)
    assert not bool(bad.any()), (int(bad.sum()), "of", bad.numel(), "first at", tuple(bad.nonzero()[0].tolist()))


# ---- exact: the indexing -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=ROW_IDS)
def test_int_family_is_bit_exact(case):
    dw, _ = _run(case, "int")
    _same_bits(dw, R.reference(case, "int")[0])


@pytest.mark.parametrize("case", R.STRIDED_1X1, ids=R.case_id)
def test_int_family_is_bit_exact_on_strided_operands(case):
    dw, _ = _run(case, "int", strided=True)
    _same_bits(dw, R.reference(case, "int")[0])


# ---- precision -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=ROW_IDS)
def test_relu_family_within_the_derived_bound_and_the_yardstick(case):
    from conftest import record_achieved
    dw, _ = _run(case, "relu")
    ref, A = R.reference(case, "relu")
    dyd, xd = R.inputs(case, "relu")
    stock = R.product(dyd.to(DEV), xd.to(DEV), case, torch.float32)      # torch's fp32 product of the same values, same device
    n = R.dims(case)[0]
    q, q_stock = R.scaled(dw, ref, A), R.scaled(stock, ref, A)
    print(f"wgrad_ref {R.form(case)} {R.case_id(case)}: got {q:.3e}  stock {q_stock:.3e}  worst-case bound {R.bound_worst(n):.3e}  "
          f"yardstick {R.yardstick(q_stock):.3e}")
    record_achieved(f"wgrad_ref/{R.form(case)}/{R.case_id(case)}/got", q)
    record_achieved(f"wgrad_ref/{R.form(case)}/{R.case_id(case)}/stock", q_stock)
    assert bool((dw.cpu()[A == 0] == 0).all())                          # a sum of zeros is zero (scaled() leaves these out)
    assert bool(torch.isfinite(dw).all())
    assert q <= R.bound_worst(n), (q, R.bound_worst(n))
    assert q <= R.yardstick(q_stock), (q, q_stock)


# ---- route -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_launches_and_repeatability(row):
    """One launch where the table says the product is stored straight into dw, the product and the reduce otherwise; a second
    call gives the same bits (no atomics on any route, 3x3 included)."""
    case, groups, S = row
    assert _need(case) == 4 * groups * R.dims(case)[1] * R.dims(case)[2]
    a, launches = _run(case, "relu")
    b, again = _run(case, "relu")
    assert launches == again == (1 if S is None else 2), (launches, again, S)
    assert torch.equal(a, b) and not bool(torch.isnan(a).any())


# ---- the entries' edges ------------------------------------------------------------------------------------------------------------
def test_no_rows_and_no_images_give_zeros():
    L = _lib.load()
    dw = torch.full((64, 128), NAN, device=DEV)
    assert L.dmm_wgrad_bf16(None, None, 0, 64, 128, 64, 128, dw.data_ptr(), None, 0, _stream()) == _lib.DMM_OK
    torch.cuda.synchronize()
    assert bool((dw == 0).all())
    dw = torch.full((128, 64, 3, 3), NAN, device=DEV)
    assert L.dmm_wgrad3x3_bf16(None, None, 0, 5, 7, 64, 128, 2, dw.data_ptr(), None, 0, _stream()) == _lib.DMM_OK
    torch.cuda.synchronize()
    assert bool((dw == 0).all())


@pytest.mark.parametrize("case", [(130, 128, 128), (300, 64, 128), (300, 384, 64)], ids=R.case_id)
def test_staged_forms_refuse_rows_that_are_not_16_byte_aligned(case):
    """The kernels that fetch 16-byte pieces (128-multiples, and the 64 x 128 / 128 x 64 tile forms beside them): a row stride
    that is no multiple of 8 elements, or a base that is only 2-byte aligned, answers DMM_ERR_UNSUPPORTED before anything is
    launched -- the NaNs in dw stay."""
    rows, co, ci = case
    dy, x = (t.to(DEV) for t in R.inputs(case, "int"))
    wide_dy = torch.zeros((rows, co + 2), dtype=torch.bfloat16, device=DEV)
    wide_x = torch.zeros((rows, ci + 2), dtype=torch.bfloat16, device=DEV)
    shifted = torch.zeros((rows * co + 8,), dtype=torch.bfloat16, device=DEV)
    for args in ((wide_dy, x, co + 2, ci, None), (dy, wide_x, co, ci + 2, None), (dy, x, co, ci, shifted.data_ptr() + 2)):
        rc, dw, launches = _entry(case, *args[:4], dy_ptr=args[4])
        assert rc == _lib.DMM_ERR_UNSUPPORTED and launches == 0
        assert bool(torch.isnan(dw).all())


@pytest.mark.parametrize("case", [(37, 64, 64), (130, 128, 128)], ids=R.case_id)
def test_an_odd_row_stride_is_refused(case):
    rows, co, ci = case
    dyb = torch.zeros((rows, co + 1), dtype=torch.bfloat16, device=DEV)
    xb = torch.zeros((rows, ci + 1), dtype=torch.bfloat16, device=DEV)
    dy, x = (t.to(DEV) for t in R.inputs(case, "int"))
    for args in ((dyb, x, co + 1, ci), (dy, xb, co, ci + 1)):
        rc, dw, launches = _entry(case, *args)
        assert rc == _lib.DMM_ERR_UNSUPPORTED and launches == 0
        assert bool(torch.isnan(dw).all())


@pytest.mark.parametrize("case", [(600, 64, 64), (130, 128, 128), (3, 9, 13, 64, 64, 1), (70, 1, 1, 128, 128, 1)], ids=R.case_id)
def test_a_workspace_one_byte_short_is_refused(case):
    rc, dw, launches = _entry(case, *_operands(case, "int"), short=1)
    assert rc == _lib.DMM_ERR_WORKSPACE and launches == 0
    assert bool(torch.isnan(dw).all())


# ---- the callers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("case", [(2100, 192, 64), (2, 17, 23, 128, 128, 2)], ids=R.case_id)
def test_train_encoder_launches_the_same_bits(case, family):
    """``train_encoder._wgrad_launch`` (its own workspace, the entries through ``_lib.call``) gives the bits of the direct entry,
    which the tests above hold to the reference."""
    direct, _ = _run(case, family)
    dy, x, _, _ = _operands(case, family)
    dw = torch.full(direct.shape, NAN, device=DEV)
    if R.is_3x3(case):
        B, H, W, ci, co, stride = case
        te._wgrad_launch(("3x3", dy, x, (B, H, W, ci, co, stride) + R.out_hw(H, W, stride), dw))
    else:
        te._wgrad_launch(("1x1", dy, x, case, dw))
    torch.cuda.synchronize()
    assert torch.equal(dw, direct)


# ---- the reduce kernel's other user ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("narrow", conv_narrow_ref.CASES, ids=conv_narrow_ref.case_id)
def test_narrow_wgrad_int_family_is_bit_exact(narrow):
    """``ops.wgrad3x3_narrow_bf16`` folds its slabs with ``wgrad_reduce_kernel<S, true>`` too: the same exact family on
    tests/conv_narrow_ref.py's shapes (widths that are multiples of 32, stride 1)."""
    ci, co, B, H, W = narrow
    case = (B, H, W, ci, co, 1)
    dy, x = R.inputs(case, "int")
    dw = torch.full((co, ci, 3, 3), NAN, device=DEV)
    got = ops.wgrad3x3_narrow_bf16(dy.to(DEV), x.to(DEV), out=dw)
    torch.cuda.synchronize()
    assert got.data_ptr() == dw.data_ptr()
    _same_bits(dw, R.reference(case, "int")[0])
