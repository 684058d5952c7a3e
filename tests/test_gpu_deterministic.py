"""Deterministic mode on the GPU (dmm_net_amd.set_deterministic): every `_det` kernel gives bit-identical results call after
call and agrees with fp64 / the atomic kernels to rounding; the bf16 TrainEncoder step is bit-reproducible eagerly, in graph
replay, and across processes; a graph captured in one mode is never replayed in the other."""
import copy
import gc
import os
import subprocess
import sys

import pytest
import torch

import dmm_net_amd
from dmm_net_amd import _lib, ops
from dmm_net_amd.roi_features import _RoiAlign4Mean
from dmm_net_amd.train_encoder import TrainEncoder, _BNActFn, _channel_sums

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _release_plans():
    """The captured plans of a test (TrainEncoder <-> plan reference cycles) are freed HERE, by a collection between tests --
    not by a garbage collection that happens to run inside a later test's stream capture, where destroying a graph would
    touch the runtime mid-capture."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def _record(name, v):
    try:
        from conftest import record_achieved
        record_achieved(name, v)
    except Exception:
        pass


# ---- kernels -----------------------------------------------------------------------------------------------------------
BN_SHAPES = [(6, 64, 64, 112), (6, 256, 32, 56), (6, 512, 16, 28), (6, 2048, 4, 7), (12, 64, 32, 56)]


def _bn_inputs(B, C, H, W, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    cl = torch.channels_last
    x = (torch.randn((B, C, H, W), generator=g, device=DEV) * 1.7 + 0.4).to(torch.bfloat16).contiguous(memory_format=cl)
    res = torch.randn((B, C, H, W), generator=g, device=DEV).to(torch.bfloat16).contiguous(memory_format=cl)
    dy = torch.randn((B, C, H, W), generator=g, device=DEV).to(torch.bfloat16).contiguous(memory_format=cl)
    dy2 = torch.randn((B, C, H, W), generator=g, device=DEV).to(torch.bfloat16).contiguous(memory_format=cl)
    w = torch.rand(C, generator=g, device=DEV) + 0.5
    b = torch.randn(C, generator=g, device=DEV) * 0.3
    return x, res, dy, dy2, w, b


@pytest.mark.parametrize("B,C,H,W", BN_SHAPES)
@pytest.mark.parametrize("groups", [1, 3])
def test_bn_det_statistics_fold_matches_fp64_and_atomics(B, C, H, W, groups):
    x = _bn_inputs(B, C, H, W, C + H)[0]
    L = _lib.load()
    R = B * H * W
    s = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(int(L.dmm_bn_det_workspace_bytes(R, C, groups)), dtype=torch.uint8, device=DEV)
    outs = []
    for _ in range(3):
        out = torch.empty((groups, 2, C), device=DEV)
        _lib.check(L.dmm_bn_stats_det_grouped_bf16(x.data_ptr(), R, C, groups, ws.data_ptr(), ws.numel(), s), "stats_det")
        _lib.check(L.dmm_bn_fold_det(ws.data_ptr(), ws.numel(), R, C, groups, out.data_ptr(), s), "fold_det")
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    atom = torch.zeros((groups, 2, C), device=DEV)
    _lib.check(L.dmm_bn_stats_grouped_bf16(x.data_ptr(), R, C, groups, atom.data_ptr(), s), "stats")
    xg = x.permute(0, 2, 3, 1).reshape(groups, R // groups, C).double()
    ref = torch.stack([xg.sum(1), (xg * xg).sum(1)], 1)
    for k in range(2):
        e64, ea = _rel(outs[0][:, k], ref[:, k]), _rel(outs[0][:, k], atom[:, k])
        _record(f"bn_det_stats[{B},{C},{H},{W},g{groups},{k}]_vs_fp64", e64)
        assert e64 <= 1e-5 and ea <= 1e-5, (k, e64, ea)


@pytest.mark.parametrize("B,C,H,W", BN_SHAPES[1:4])
@pytest.mark.parametrize("relu,has_res", [(False, False), (True, False), (True, True), (False, True)])
@pytest.mark.parametrize("groups", [1, 3])
def test_bn_det_layer_repeatable_and_close_to_atomics(B, C, H, W, relu, has_res, groups):
    x, res, dy, dy2, w, b = _bn_inputs(B, C, H, W, 7 * C + W)

    def run(det):
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        xg = x.clone().requires_grad_(True)
        wg, bg = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        rg = res.clone().requires_grad_(True) if has_res else None
        with dmm_net_amd.deterministic(det):
            y1, y2 = _BNActFn.apply(xg, wg, bg, rm, rv, 0.1, 1e-5, relu, rg, groups, True)
            torch.autograd.backward([y1, y2], [dy, dy2])           # the forked output: the dy2 second gradient
        return [y1.detach(), xg.grad, wg.grad, bg.grad, rm, rv] + ([rg.grad] if has_res else [])

    d = [run(True) for _ in range(3)]
    for k in range(len(d[0])):
        assert torch.equal(d[0][k], d[1][k]) and torch.equal(d[0][k], d[2][k]), k
    a = run(False)
    # fp32 quantities: the statistics and the parameters' gradients (without a ReLU mask, which one rounding of y can flip)
    for k in (4, 5):
        assert _rel(d[0][k], a[k]) <= 1e-5, (k, _rel(d[0][k], a[k]))
    if not relu:
        for k in (2, 3):
            e = _rel(d[0][k], a[k])
            _record(f"bn_det_param_grad[{C},{relu},{has_res},g{groups},{k}]_vs_atomic", e)
            assert e <= 1e-5, (k, e)
    # bf16 outputs: within a rounding of the atomic kernels'
    assert float((d[0][0].float() - a[0].float()).abs().max()) <= 2 ** -7 * float(a[0].float().abs().max())


def test_channel_sums_det():
    dy = _bn_inputs(6, 128, 32, 56, 3)[2]
    a = [_channel_sums(dy, True) for _ in range(3)]
    assert torch.equal(a[0], a[1]) and torch.equal(a[0], a[2])
    ref = dy.double().sum((0, 2, 3))
    assert _rel(a[0], ref) <= 1e-5 and _rel(a[0], _channel_sums(dy, False)) <= 1e-5


def _mix_inputs(B, N, M, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    H = W = 255
    masks = torch.rand((B, N, H, W), generator=g, device=DEV).to(dtype)
    R = torch.rand((B, M, N), generator=g, device=DEV)
    Rb = torch.zeros((B, M, ops.padded_width(N, M)), device=DEV)
    Rb[:, :, :N] = torch.where(R > 0.75, R, torch.zeros_like(R))          # train-mode support: ~25 % of the pairs
    dout = torch.randn((B, M, H, W), generator=g, device=DEV)
    return Rb, masks, dout


@pytest.mark.parametrize("B,N,M", [(4, 50, 10), (2, 200, 20)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("shared", [1, 0])
def test_mask_mix_bwd_det(B, N, M, dtype, shared):
    Rb, masks, dout = _mix_inputs(B, N, M, dtype, N + M)
    with _lib.options(MIX_SHARED=shared):
        with dmm_net_amd.deterministic():
            d = [ops.mask_mix_bwd(Rb, masks, dout) for _ in range(3)]
        a = ops.mask_mix_bwd(Rb, masks, dout)
    assert torch.equal(d[0], d[1]) and torch.equal(d[0], d[2])
    ref = torch.einsum("bmx,bnx->bmn", dout.double().flatten(2), masks.double().flatten(2))
    Pp = Rb.shape[2]
    ref = torch.nn.functional.pad(ref, (0, Pp - N)) * (Rb != 0)
    with _lib.options(FORCE_WIDE=1):
        wide = ops.mask_mix_bwd(Rb, masks, dout)
    e64, ea, ew = _rel(d[0], ref), _rel(d[0], a), _rel(d[0], wide)
    _record(f"mix_bwd_det[{B},{N},{M},{dtype},{shared}]_vs_wide", ew)
    assert e64 <= 1e-5 and ea <= 1e-5 and ew <= 1e-6, (e64, ea, ew)
    assert bool((d[0][Rb == 0] == 0).all())


def _roi_inputs(B, C, R_per, seed, H=128, W=224):
    g = torch.Generator(device=DEV).manual_seed(seed)
    Hs, Ws = [-(-H // s) for s in (4, 8, 16, 32)], [-(-W // s) for s in (4, 8, 16, 32)]
    feats = [torch.randn((B, C, h, w), generator=g, device=DEV).requires_grad_(True) for h, w in zip(Hs, Ws)]
    xy = torch.rand((B * R_per, 2), generator=g, device=DEV) * torch.tensor([W - 24.0, H - 18.0], device=DEV)
    wh = torch.rand((B * R_per, 2), generator=g, device=DEV) * torch.tensor([W * 0.55, H * 0.7], device=DEV) + 2
    ids = torch.arange(B, device=DEV).repeat_interleave(R_per).float()
    rois = torch.cat([ids[:, None], xy, xy + wh], 1).contiguous()
    dout = torch.randn((B * R_per, 4 * C), generator=g, device=DEV)
    return feats, rois, dout


@pytest.mark.parametrize("B,C,R_per,H,W", [(12, 128, 50, 255, 448), (4, 256, 50, 128, 224), (2, 64, 100, 128, 224)])
def test_roialign_bwd_det(B, C, R_per, H, W):
    """Config-4 frames (12 x 255 x 448, 50 rois each) and smaller ones: three calls bit-equal, the atomic kernel to 1e-5, and
    the fp64 adjoint identity <g, A f> = <A^T g, f> of the forward kernel."""
    feats, rois, dout = _roi_inputs(B, C, R_per, C + R_per, H, W)

    def grads(det):
        with dmm_net_amd.deterministic(det):
            out = _RoiAlign4Mean.apply(rois, *feats)
            return torch.autograd.grad(out, feats, dout)

    d = [grads(True) for _ in range(3)]
    a = grads(False)
    for l in range(4):
        assert torch.equal(d[0][l], d[1][l]) and torch.equal(d[0][l], d[2][l]), l
        e = _rel(d[0][l], a[l])
        _record(f"roi_bwd_det[{B},{C},{R_per},L{l}]_vs_atomic", e)
        assert e <= 1e-5, (l, e)
    out = _RoiAlign4Mean.apply(rois, *[f.detach() for f in feats])
    lhs = float((out.double() * dout.double()).sum())
    rhs = float(sum((gl.double() * f.detach().double()).sum() for gl, f in zip(d[0], feats)))
    assert abs(lhs - rhs) <= 1e-5 * max(1.0, abs(lhs)), (lhs, rhs)


def test_roialign_bwd_det_matches_g12_fixture():
    """G12 (tests/golden: an independent differentiable fp64-built formulation of legacy ROIAlign + mean): d feat_l of the
    deterministic gather <= 1e-5 relative, boxes sub-pixel, clipped, outside and whole-frame."""
    import numpy as np
    from conftest import golden
    g = golden("g12_roialign")
    for k in range(int(g["n"])):
        c = g.group(f"c{k}")
        feats = [torch.from_numpy(c[f"feat{l}"]).to(DEV).requires_grad_(True) for l in range(4)]
        rois = torch.from_numpy(c["rois"]).to(DEV).float().contiguous()
        with dmm_net_amd.deterministic():
            out = _RoiAlign4Mean.apply(rois, *feats)
            grads = torch.autograd.grad(out, feats, torch.from_numpy(c["wgt"]).to(DEV))
        for l in range(4):
            ge = c[f"grad{l}"]
            gerr = float(np.abs(grads[l].cpu().numpy() - ge).max())
            _record(f"g12_roialign/c{k}/grad{l}_det_rel_err", gerr / max(1.0, float(np.abs(ge).max())))
            assert gerr <= 1e-5 * max(1.0, float(np.abs(ge).max())), (k, l, gerr)


# ---- the fused training backward (5e) and the per-frame-table mix ------------------------------------------------------
def _arr_equal(a, b):
    import numpy as np
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("B,N,M,H,W,dtype", [(4, 50, 10, 255, 255, torch.float32), (2, 50, 5, 255, 448, torch.float16),
                                             (3, 130, 6, 40, 56, torch.float32)])
def test_fused_training_backward_det(B, N, M, H, W, dtype):
    """dmm_match_train_backward_det through the layer's autograd function: three calls bit-equal; the granular chain in the
    same mode (dmm_mask_mix_bwd_det and the same solver / similarity kernels) bit-equal; the atomic entry to 1e-5; and the
    per-frame plane tables (dmm_mask_mix_bwd_frames_det inside the fused entry) bit-equal to the stacked planes."""
    import numpy as np
    from test_gpu_train_fused import batch, granular, run_layer
    d = batch(B, N, M, H, W, 512, seed=B + N, dtype=dtype)
    with dmm_net_amd.deterministic():
        runs = [run_layer(d) for _ in range(3)]
        with granular():
            gran = run_layer(d)
        planes = run_layer(d, pm=[d["pm"][b].clone() for b in range(B)])
    atom = run_layer(d)
    assert _arr_equal(runs[0], runs[1]) and _arr_equal(runs[0], runs[2])
    for q in (5, 6):                                                  # d proposed_feature, d template_feature
        assert np.array_equal(runs[0][q], gran[q]), q
        assert np.array_equal(runs[0][q], planes[q]), q
        scale = float(np.abs(atom[q]).max()) or 1.0
        e = float(np.abs(runs[0][q].astype(np.float64) - atom[q].astype(np.float64)).max()) / scale
        _record(f"fused_bwd_det[{B},{N},{M},{H},{W},{dtype}]_d{q}_vs_atomic", e)
        assert e <= 1e-5, (q, e)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_mask_mix_bwd_frames_det(dtype):
    """dmm_mask_mix_bwd_frames_det (per-frame plane tensors, ragged counts): three calls bit-equal, equal to the stacked
    deterministic entry, to fp64 and the atomic frames entry within 1e-5."""
    B, N, M = 4, 50, 10
    Rb, masks, dout = _mix_inputs(B, N, M, dtype, 77)
    counts = [50, 17, 33, 1]
    for b, n in enumerate(counts):
        Rb[b, :, n:] = 0
    nv = torch.tensor(counts, dtype=torch.int32, device=DEV)
    fp = ops.FramePlanes([masks[b, :counts[b]].contiguous() for b in range(B)])
    with dmm_net_amd.deterministic():
        d = [ops.mask_mix_bwd(Rb, fp, dout, nv) for _ in range(3)]
        stacked = ops.mask_mix_bwd(Rb, masks, dout, nv)
    a = ops.mask_mix_bwd(Rb, fp, dout, nv)
    assert torch.equal(d[0], d[1]) and torch.equal(d[0], d[2]) and torch.equal(d[0], stacked)
    ref = torch.einsum("bmx,bnx->bmn", dout.double().flatten(2), masks.double().flatten(2))
    ref = torch.nn.functional.pad(ref, (0, Rb.shape[2] - N)) * (Rb != 0)
    assert _rel(d[0], ref) <= 1e-5 and _rel(d[0], a) <= 1e-5


# ---- the TrainEncoder step ---------------------------------------------------------------------------------------------
def _step(te, enc, img, cot):
    enc.zero_grad(set_to_none=True)
    out = te(img)
    feats = list(out["backbone_feature"]) + list(out["refine_input_feat"])
    loss = sum((f.float() * c).sum() for f, c in zip(feats, cot))
    loss.backward()
    torch.cuda.synchronize()
    return ([f.detach().clone() for f in feats],
            {n: p.grad.clone() for n, p in enc.named_parameters() if p.grad is not None},
            {n: t.clone() for n, t in enc.named_buffers()})


def _same(r1, r2):
    f1, g1, b1 = r1
    f2, g2, b2 = r2
    assert len(f1) == len(f2) and all(torch.equal(a, b) for a, b in zip(f1, f2)), "features"
    assert g1.keys() == g2.keys() and len(g1) > 0
    bad = [k for k in g1 if not torch.equal(g1[k], g2[k])]
    assert not bad, ("grads", bad[:5])
    bad = [k for k in b1 if not torch.equal(b1[k], b2[k])]
    assert not bad, ("buffers", bad[:5])


def test_train_encoder_bit_reproducible_eager_and_graph():
    from dmm_net_amd.encoder import FeatureEncoder
    torch.manual_seed(31)
    ref = FeatureEncoder("resnet50").to(DEV).train()                     # untamed weights
    g = torch.Generator(device=DEV).manual_seed(3)
    imgs = [torch.randn((6, 3, 128, 224), generator=g, device=DEV) for _ in range(2)]
    with torch.no_grad():
        probe = ref(imgs[0])
    cot = [torch.randn(f.shape, generator=g, device=DEV) for f in list(probe["backbone_feature"]) + list(probe["refine_input_feat"])]
    del probe
    encs = [copy.deepcopy(ref) for _ in range(4)]
    e1, e2 = TrainEncoder(encs[0], graphs=False), TrainEncoder(encs[1], graphs=False)
    g1, g2 = TrainEncoder(encs[2]), TrainEncoder(encs[3])
    with dmm_net_amd.deterministic():
        for img in imgs:                                                 # two steps: running statistics carry over
            r_e1, r_e2 = _step(e1, encs[0], img, cot), _step(e2, encs[1], img, cot)
            r_g1, r_g2 = _step(g1, encs[2], img, cot), _step(g2, encs[3], img, cot)
            _same(r_e1, r_e2)                                            # two eager runs
            _same(r_g1, r_g2)                                            # two replays (two plans)
            _same(r_g1, r_e1)                                            # graph replay == eager, every p.grad
        r_g1b = _step(g1, encs[2], imgs[1], cot)                         # a later replay of the same plan
        _same(r_g1b, _step(g2, encs[3], imgs[1], cot))
    assert len(g1._plans) == 1
    # the same shape in the default mode: a plan of its own
    _step(g1, encs[2], imgs[0], cot)
    assert len(g1._plans) == 2 and sorted(k[-1] for k in g1._plans) == [False, True]


_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
torch.backends.cudnn.benchmark = False
torch.backends.cudnn.deterministic = True          # the reference's train.py:46: the mode follows it
import dmm_net_amd
from dmm_net_amd.encoder import FeatureEncoder
from dmm_net_amd.train_encoder import TrainEncoder
assert dmm_net_amd.is_deterministic()
torch.manual_seed(31)
enc = FeatureEncoder("resnet50").to("cuda:0").train()
te = TrainEncoder(enc)
opt = torch.optim.Adam(enc.parameters(), lr=1e-4)
g = torch.Generator(device="cuda:0").manual_seed(5)
for _ in range(3):
    img = torch.randn((6, 3, 128, 224), generator=g, device="cuda:0")
    opt.zero_grad(set_to_none=True)
    out = te(img)
    loss = sum(f.float().square().mean() for f in list(out["backbone_feature"]) + list(out["refine_input_feat"]))
    loss.backward()
    opt.step()
torch.cuda.synchronize()
s = torch.stack([p.detach().double().sum() for p in enc.parameters()] + [b.double().sum() for b in enc.buffers()])
print("CHECKSUM", float(loss), s.cpu().numpy().tobytes().hex())
"""


def test_train_encoder_same_checksum_in_two_processes():
    outs = []
    for _ in range(2):
        p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        outs.append([ln for ln in p.stdout.splitlines() if ln.startswith("CHECKSUM")][-1])
    assert outs[0] == outs[1], outs


# ---- a config-4 style step through DMM_Model ---------------------------------------------------------------------------
def _cfg4_run(steps=3, data_seed=4, backend="nccl", world=1):
    """ResNet-50 TrainEncoder, 2 videos x clip 2 at 128 x 224 -> ROI features -> DMM_Model with targets -> soft IoU + match
    loss; GradBucketer; Adam.  -> (losses, parameter checksum bytes as hex, parameters).  Run under the deterministic mode.
    ``world`` = 1: a process group of one RCCL rank, made here unless there is one.  ``world`` > 1: this process is one rank of
    a launcher's group (``backend``: gloo when the ranks share a device); ``data_seed`` is the rank's own."""
    import socket
    import torch.distributed as dist
    from dmm_net_amd.distributed import init_from_env
    own_pg = not dist.is_initialized()
    if own_pg:
        torch.cuda.set_device(0)
        if world == 1:
            sk = socket.socket()
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
            sk.close()
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
        init_from_env(backend, torch.device(DEV))
    assert dist.get_world_size() == world, (dist.get_world_size(), world)
    try:
        gen = _cfg4_steps(steps, data_seed, True)
        try:
            while True:
                next(gen)
        except StopIteration as done:
            return done.value
    finally:
        if own_pg:
            dist.destroy_process_group()


def _cfg4_reference(steps, data_seeds):
    """The step of ``_cfg4_run`` for ``len(data_seeds)`` ranks in ONE process without a process group: one copy per rank on its
    own data, in lockstep; after every backward the gradients are replaced by their mean under GradBucketer's contract
    (``dist_step.mean_of``: None everywhere stays None, None somewhere counts as zeros, (g0 + g1) / 2 in fp32), then every
    copy takes its Adam step.  Every copy keeps a random-number state of its own.  -> [``_cfg4_run``'s result per rank]."""
    from dist_step import mean_of
    gens = [_cfg4_steps(steps, seed, False) for seed in data_seeds]
    rng, results = [None] * len(gens), [None] * len(gens)
    while any(r is None for r in results):
        waiting = []
        for k, gen in enumerate(gens):
            if rng[k] is not None:
                torch.set_rng_state(rng[k][0]), torch.cuda.set_rng_state(rng[k][1], DEV)
            try:
                waiting.append(next(gen))
            except StopIteration as done:
                results[k] = done.value
            rng[k] = (torch.get_rng_state(), torch.cuda.get_rng_state(DEV))
        assert len(waiting) in (0, len(gens))
        for ps in zip(*waiting):
            mean = mean_of([p.grad for p in ps])
            for p in ps:
                p.grad = None if mean is None else mean.clone()
    return results


def _cfg4_steps(steps, data_seed, bucketer):
    """The step itself, as a generator.  ``bucketer``: the gradients go through ``GradBucketer(overlap=True)`` + ``finish()`` and
    nothing is yielded; otherwise the parameter list is yielded after every backward and the caller puts the reduced gradients
    into ``p.grad`` before the Adam step.  Returns ``_cfg4_run``'s result."""
    from dmm_net_amd.distributed import GradBucketer
    from dmm_net_amd.dmm_model import DMM_Model
    from dmm_net_amd.encoder import FeatureEncoder
    from dmm_net_amd.proposals import SimpleBoxList
    from dmm_net_amd.roi_features import FeatureExtractor
    NV, T, F, P, H, W = 2, 2, 4, 30, 128, 224
    torch.manual_seed(31)
    g = torch.Generator(device=DEV).manual_seed(data_seed)
    enc = FeatureEncoder("resnet50").to(DEV).train()
    run_enc = TrainEncoder(enc, skips_need_grad=False)
    cfgs = {"matching": {"algo": "relax"}, "relax_max_iter": 10, "relax_proj_iter": 5, "relax_learning_rate": 0.1,
            "score_weight": 0.3}
    model = DMM_Model(cfgs, is_test=0, feature_extractor=FeatureExtractor())
    params = list(enc.get_skip_params()) + list(enc.get_backbone_para())
    opt = torch.optim.Adam(params, lr=1e-4)
    gb = GradBucketer(params, bucket_mb=64.0, overlap=True) if bucketer else None
    frames = torch.randn(NV, T, 3, H, W, generator=g, device=DEV)
    valid = torch.zeros(NV, F, device=DEV)
    valid[0, :3], valid[1, :2] = 1, 1
    targets = (torch.rand((NV, T, F, H, W), generator=g, device=DEV) > 0.6).float() * valid[:, None, :, None, None]

    def boxes(n):
        x1 = torch.rand(n, generator=g, device=DEV) * (W - 40)
        y1 = torch.rand(n, generator=g, device=DEV) * (H - 30)
        return torch.stack([x1, y1, x1 + 8 + torch.rand(n, generator=g, device=DEV) * 80,
                            y1 + 8 + torch.rand(n, generator=g, device=DEV) * 60], 1).clamp(max=W - 1)

    per_frame = []
    for _ in range(T):
        props = []
        for b in range(NV):
            bl = SimpleBoxList(boxes(P), (W, H))
            bl.add_field("mask", torch.rand((P, 1, H, W), generator=g, device=DEV))
            bl.add_field("scores", torch.rand(P, generator=g, device=DEV))
            props.append(bl)
        per_frame.append((props, [SimpleBoxList(boxes(F), (W, H)) for _ in range(NV)]))
    losses = []
    try:
        for _ in range(steps):
            opt.zero_grad(set_to_none=True)
            total, tplt, mask_last = 0.0, None, targets[:, 0]
            for t in range(T):
                props, tboxes = per_frame[t]
                feats = run_enc(frames[:, t])
                if t == 0:
                    tplt = model.fill_template_dict(None, tboxes, feats, None, valid)
                out, _, match_loss, last = model(None, props, feats["backbone_feature"], mask_last, tplt, valid, targets[:, t])
                tg = targets[:, t]
                inter = (out * tg).flatten(2).sum(2)
                union = (out + tg - out * tg).flatten(2).sum(2)
                total = total + ((1.0 - inter / (union + 1e-6)) * valid).sum() / valid.sum() + sum(match_loss) / NV
                mask_last = last.detach()
            loss = total / T
            loss.backward()
            if gb is not None:
                gb.finish()
            else:
                yield params
            opt.step()
            losses.append(float(loss))
        torch.cuda.synchronize()
        chk = torch.stack([p.detach().double().sum() for p in enc.parameters()] + [b.double().sum() for b in enc.buffers()])
        return losses, chk.cpu().numpy().tobytes().hex(), [p.detach().clone() for p in enc.parameters()]
    finally:
        if gb is not None:
            gb.remove_hooks()


_CHILD_CFG4 = r"""
import sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
torch.backends.cudnn.benchmark = False
torch.backends.cudnn.deterministic = True          # the reference's train.py:46: the mode follows it
import dmm_net_amd
assert dmm_net_amd.is_deterministic()
import test_gpu_deterministic as t
losses, chk, params = t._cfg4_run()
if len(sys.argv) > 3:                               # a second copy from the same seed in the same process
    l2, c2, p2 = t._cfg4_run()
    assert losses == l2 and chk == c2 and all(torch.equal(a, b) for a, b in zip(params, p2)), (losses, l2)
    print("TWO_COPIES_EQUAL")
print("CHECKSUM", losses, chk)
"""


def _cfg4_child(*extra):
    # (a process of its own: the step initialises an RCCL process group and captures graphs -- none of that stays behind in
    # the test process)
    p = subprocess.run([sys.executable, "-c", _CHILD_CFG4, ROOT, os.path.join(ROOT, "tests"), *extra], capture_output=True,
                       text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    return p.stdout.splitlines()


def test_config4_style_step_two_copies_equal():
    """Two copies of the step from the same seed, 3 Adam steps each: equal losses and parameters, bit for bit."""
    out = _cfg4_child("twice")
    assert "TWO_COPIES_EQUAL" in out, out[-5:]


def test_config4_style_step_same_checksum_in_two_processes():
    """Two fresh processes with cudnn.benchmark=False (cudnn.deterministic=True turns the mode on): the same losses and
    parameter checksum."""
    outs = [[ln for ln in _cfg4_child() if ln.startswith("CHECKSUM")][-1] for _ in range(2)]
    assert outs[0] == outs[1], outs
