"""The refine decoder without a GPU (dmm_net_amd/decoder.py): the stock form against the reference's own outputs (G23,
tests/golden/gen_golden_decoder.py), the algebra of the fused form -- one shared pre-activation + a one-channel stencil per
mask plane -- restated in torch against the reference's fp64 evaluation, the clipped-window model of the mask pyramid,
and ``RefineStep`` over the recorded object chain."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from dmm_net_amd.decoder import RSISMask, RefineStep, pyramid_sizes

CASES = {"nn": (False, False), "sn": (True, False), "nt": (False, True), "st": (True, True)}
FILES = {"concat": "g23_refine_decoder", "sum": "g23_refine_decoder_sum"}


def make_args(skip_mode, hidden=32, kernel_size=3, dropout=0.0):
    return types.SimpleNamespace(hidden_size=hidden, kernel_size=kernel_size, dropout=dropout, skip_mode=skip_mode,
                                 prev_mask_d=1, use_gpu=False)


def load_decoder(mode, device="cpu"):
    """RSISMask with G23's parameters, loaded by the reference's names with strict=True."""
    g = golden(FILES[mode])
    dec = RSISMask(make_args(mode)).eval()
    sd = {k: torch.from_numpy(v.astype(np.float32)) for k, v in g.group(f"{mode}/param").items()}
    dec.load_state_dict(sd, strict=True)
    return dec.to(device), g


def case_inputs(g, mode, case, device="cpu", dtype=torch.float32):
    T = lambda k: torch.from_numpy(g[f"{mode}/{k}"]).to(device=device, dtype=dtype)
    sp, tm = CASES[case]
    feats = [T(f"skip{i}") for i in range(4)]
    masks = [T(f"mask{i}") for i in range(4)]
    spatial = [[T(f"sp{i}_h"), T(f"sp{i}_c")] for i in range(4)] if sp else None
    temporal = [T(f"tm{i}") for i in range(4)] if tm else None
    return feats, masks, spatial, temporal


def flat_outputs(res):
    out_mask, hidden_list = res
    d = {"out_mask": out_mask}
    for i, (h, c) in enumerate(hidden_list):
        d[f"h{i}"], d[f"c{i}"] = h, c
    return d


def split_forward(dec, feats, masks, spatial, temporal):
    """The fused form's arithmetic in torch ops: the same weight slices (``RSISMask.weight_slices``), the same addends in
    the same order ((skip term + temporal term) + chain term, then + the mask plane's stencil), planes in the order 0, 2, 1,
    (a + b + c) / 3.  What csrc/dmm_decoder.hip + the library convolutions compute, minus the device."""
    sl = dec.weight_slices()
    conv = lambda x, w, b=None: F.conv2d(x, w, b, padding=1)
    hidden_list, up = [], None
    for i, d in enumerate(sl):
        Hd = dec.skip_dims_out[i]
        skip_term = None if d["skip"] is None else conv(feats[i], d["skip"], d["bias"])
        temporal_term = None if temporal is None else conv(temporal[i], d["ht"])
        bias = None if skip_term is not None else d["bias"]
        chain = None
        if i == 0:
            if spatial is not None:
                chain = conv(spatial[0][0], d["hs"])
        else:
            x = F.interpolate(up, size=tuple(feats[i].shape[-2:]), mode="bilinear", align_corners=True)
            if dec.skip_mode == "mul":
                x = feats[i] * x
            if spatial is None:
                chain = conv(x, d["up"], bias)
            else:
                chain = conv(torch.cat([x, spatial[i][0]], 1), d["cat"], bias)
        pre = None
        for term in (skip_term, temporal_term, chain):
            if term is not None:
                pre = term if pre is None else pre + term
        c_prev = 0.0 if spatial is None else spatial[i][1]
        hs, cs = [], []
        for k in (0, 2, 1):
            g = pre + F.conv2d(masks[i][:, k:k + 1], d["m"].view(4 * Hd, 1, 3, 3), padding=1)
            gi, gr, go, gc = g.chunk(4, 1)
            cell = torch.sigmoid(gr) * c_prev + torch.sigmoid(gi) * torch.tanh(gc)
            hs.append(torch.sigmoid(go) * torch.tanh(cell))
            cs.append(cell)
        hidden, cell = (hs[0] + hs[1] + hs[2]) / 3, (cs[0] + cs[1] + cs[2]) / 3
        hidden_list.append([hidden, cell])
        up = hidden
    top = F.interpolate(up, size=(up.shape[-2] * 2, up.shape[-1] * 2), mode="bilinear", align_corners=True)
    return conv(top, dec.conv_out.weight, dec.conv_out.bias), hidden_list


@pytest.mark.parametrize("mode", ["concat", "sum"])
@pytest.mark.parametrize("case", list(CASES))
def test_stock_form_reproduces_the_reference(mode, case):
    """Same ops in the same order on the same torch build as the capture: every output EQUAL to the reference's fp32."""
    dec, g = load_decoder(mode)
    assert sorted(dec.state_dict()) == sorted(g.group(f"{mode}/param"))
    torch.set_num_threads(8)
    with torch.no_grad():
        got = flat_outputs(dec(*case_inputs(g, mode, case)))
    for k, v in got.items():
        want = g[f"{mode}/{case}/{k}"]
        assert v.shape == want.shape, k
        assert np.array_equal(v.numpy(), want), (k, float(np.abs(v.numpy() - want).max()))


@pytest.mark.parametrize("mode", ["concat", "sum"])
@pytest.mark.parametrize("case", list(CASES))
def test_split_form_is_a_reordering_of_the_reference_sums(mode, case):
    """The split against the reference's fp64 outputs: <= 2 * e_ref (e_ref = the reference's own fp32 error against the same
    fp64 result; both are fp32 roundings of the same sums in another order -- a wrong slice, plane or gate order is off by
    1e-3 and more)."""
    dec, g = load_decoder(mode)
    with torch.no_grad():
        got = flat_outputs(split_forward(dec, *case_inputs(g, mode, case)))
    for k, v in got.items():
        err = float(np.abs(v.double().numpy() - g[f"{mode}/{case}/f64/{k}"]).max())
        e_ref = float(g[f"{mode}/{case}/e_ref/{k}"])
        print(f"{mode}/{case}/{k}: split {err:.3e}  e_ref {e_ref:.3e}")
        assert err <= 2 * e_ref, (k, err, e_ref)


@pytest.mark.parametrize("mode", ["concat", "sum", "mul", "none"])
def test_split_form_equals_stock_in_fp64_for_every_skip_mode(mode):
    """In fp64 the reordering leaves 1e-15: the slices and the term placement (bias, skip share) of every skip mode."""
    torch.manual_seed(5)
    dec = RSISMask(make_args(mode, hidden=16)).eval().double()
    sizes = pyramid_sizes(61, 45)
    ch, dims = [16, 16, 8, 4], [16, 8, 4, 2]
    feats = [torch.randn((2, c) + s, dtype=torch.float64) for c, s in zip(ch, sizes)]
    masks = [torch.rand((2, 3) + s, dtype=torch.float64) for s in sizes]
    spatial = [[torch.randn((2, d) + s, dtype=torch.float64) for _ in range(2)] for d, s in zip(dims, sizes)]
    temporal = [torch.randn((2, d) + s, dtype=torch.float64) for d, s in zip(dims, sizes)]
    with torch.no_grad():
        for sp in (None, spatial):
            for tm in (None, temporal):
                a, b = flat_outputs(dec(feats, masks, sp, tm)), flat_outputs(split_forward(dec, feats, masks, sp, tm))
                for k in a:
                    assert float((a[k] - b[k]).abs().max()) < 1e-13, (mode, k)


def pyramid_model(x, k):
    """dmm_mask_pyramid's statement: k nested ceil-mode 2x2 pools = max over the clipped 2^k x 2^k window."""
    H, W = x.shape[-2:]
    s = 1 << k
    h, w = -(-H // s), -(-W // s)
    pad = x.new_full(x.shape[:-2] + (h * s, w * s), -np.inf)
    pad[..., :H, :W] = x
    return pad.view(*x.shape[:-2], h, s, w, s).amax((-3, -1))


@pytest.mark.parametrize("size", [(95, 130), (255, 448), (33, 17), (7, 9), (1, 1)])
def test_pyramid_model_equals_nested_ceil_mode_pools(size):
    torch.manual_seed(0)
    x = torch.randn(2, 3, *size)
    y = x
    for k in range(1, 6):
        y = F.max_pool2d(y, (2, 2), ceil_mode=True)
        assert torch.equal(pyramid_model(x, k), y), (size, k)
        if k >= 2:
            assert tuple(y.shape[-2:]) == pyramid_sizes(*size)[5 - k]


def chain_inputs(g, t, device="cpu"):
    T = lambda k: torch.from_numpy(g[f"chain/t{t}/{k}"].astype(np.float32)).to(device)
    H, W = (int(v) for v in g["chain/size"])
    feats = {"refine_input_feat": tuple(T(f"skip{i}") for i in range(4))}
    return feats, T("prev_mask"), T("y_mask"), T("init_pred"), T("mask_hist"), H, W


def test_refine_step_stock_reproduces_the_recorded_chain():
    """evaluator.py:179-212 over 3 objects and 2 time steps: ``outs`` (zero row beyond n_obj), ``mask_hist_new`` including
    the untouched invalid (video, object) pair, and the temporal state's length."""
    dec, _ = load_decoder("concat")
    g = golden("g23_refine_decoder_chain")
    valid = torch.from_numpy(g["chain/valid"])
    step = RefineStep(dec)
    state = None
    torch.set_num_threads(8)
    with torch.no_grad():
        for t in range(2):
            feats, prev_mask, y_mask, init_pred, hist, H, W = chain_inputs(g, t)
            hist_in = hist.clone()
            outs, hist_new, state = step(feats, prev_mask, y_mask, init_pred, hist, valid, state)
            assert np.array_equal(outs.numpy(), g[f"chain/t{t}/outs"])
            assert np.array_equal(hist_new.numpy(), g[f"chain/t{t}/mask_hist_new"])
            assert torch.equal(hist_new[1, 1], hist_in[1, 1]) and torch.equal(hist_new[:, 3], hist_in[:, 3])
            assert float(outs[:, 3].abs().max()) == 0.0
            assert state.n_obj == 3 and len(state) == int(g["chain/n_thid"]) == 3 and len(state[0]) == 4


def test_refine_step_state_modes_and_dispatch():
    """only_spatial keeps the temporal state None; the stock form is what runs on the CPU, under autograd, for 1x1 kernels."""
    dec, _ = load_decoder("concat")
    g = golden("g23_refine_decoder_chain")
    valid = torch.from_numpy(g["chain/valid"])
    feats, prev_mask, y_mask, init_pred, hist, H, W = chain_inputs(g, 0)
    with torch.no_grad():
        _, _, st = RefineStep(dec, only_spatial=True)(feats, prev_mask, y_mask, init_pred, hist.clone(), valid, None)
        assert st.thid is None and st.n_obj == 3
        _, _, st = RefineStep(dec, only_temporal=True)(feats, prev_mask, y_mask, init_pred, hist.clone(), valid, None)
        assert len(st) == 3
    assert not dec.fused_ok([init_pred])                             # CPU tensors
    assert not RSISMask(make_args("concat", kernel_size=1)).fused_ok([init_pred])
    x = [f.clone().requires_grad_(True) for f in feats["refine_input_feat"]]
    masks = [torch.rand((2, 3) + s) for s in pyramid_sizes(H, W)]
    out_mask, _ = dec(x, masks, None, None)                         # autograd through the stock form
    out_mask.sum().backward()
    assert all(v.grad is not None and torch.isfinite(v.grad).all() for v in x)
    assert dec.clstm_list[0].Gates.weight.grad is not None


def test_package_exports():
    import dmm_net_amd
    assert dmm_net_amd.RSISMask is RSISMask and dmm_net_amd.RefineStep is RefineStep
