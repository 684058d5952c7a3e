"""The clip augmentation on the GPU (csrc/dmm_augment.hip, include/dmm_match.h (15), dmm_net_amd/augment.py) against
tests/augment_ref.py, the same arithmetic in numpy fp32: np.array_equal on every output, no tolerance.  (tests/test_augment_cpu.py
holds augment_ref.py to the fixture captured from the reference.)"""
import random

import numpy as np
import pytest
import torch

import augment_ref as R
from conftest import golden
from dmm_net_amd import _lib
from dmm_net_amd import augment as A
from dmm_net_amd.graphs import SafeGraph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("frames", "labels", "masks", "boxes", "box_valid", "targets", "sizes")
IDENTITY = np.eye(3, dtype=np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def inputs(rng, n, C, H, W, P, n_labels=6):
    """Seeded inputs: image planes that number their pixels, a block annotation with 255 and labels above any F in it, soft
    masks on a 1/8 grid (0.5 among the values) of which the last never passes the threshold, and boxes to fall back on."""
    y, x = np.mgrid[0:H, 0:W]
    frames = np.stack([np.stack([(y * W + x + 1000 * ch + f).astype(np.float32) for ch in range(C)]) for f in range(n)]) \
        if C else np.zeros((n, 0, H, W), dtype=np.float32)
    labels = np.zeros((n, H, W), dtype=np.uint8)
    for f in range(n):
        bs = int(rng.choice([1, 2, 5]))
        coarse = rng.integers(0, n_labels + 1, size=(-(-H // bs), -(-W // bs)))
        coarse[rng.random(coarse.shape) < 0.3] = 0
        coarse[rng.random(coarse.shape) < 0.05] = 255
        labels[f] = np.kron(coarse, np.ones((bs, bs), dtype=np.int64))[:H, :W]
    masks = np.zeros((n, P, H, W), dtype=np.float32)
    for f in range(n):
        for p in range(P):
            cy, cx = rng.uniform(0, H), rng.uniform(0, W)
            ry, rx = max(1.0, H * rng.uniform(0.1, 0.5)), max(1.0, W * rng.uniform(0.1, 0.5))
            masks[f, p] = np.round(np.clip(1.25 - ((y - cy) / ry) ** 2 - ((x - cx) / rx) ** 2, 0, 1) * 8) / 8
        if P > 1:
            masks[f, P - 1] = np.minimum(masks[f, P - 1], 0.5)
    boxes = rng.uniform(0, 50, size=(n, P, 4)).astype(np.float32)
    return frames, labels, masks, boxes


def drawn(seed, n, H, W):
    flip, mats = A.draw_clip_params(random.Random(seed), n, H=H, W=W)
    return flip, mats.numpy()


def check(frames, labels, masks, boxes, mats, flips, F, what="", flip_arg=None, **kw):
    """Runs the device on uploads of the arrays and compares every output with the restatement."""
    n = labels.shape[0]
    flips = [bool(flips)] * n if isinstance(flips, (bool, np.bool_)) else [bool(v) for v in flips]
    want = R.augment_clip(frames, labels, masks, boxes, mats, flips, F)
    P = masks.shape[1]
    d_masks, d_boxes = (dev(masks), dev(boxes)) if P else (None, None)
    got = A.augment_clip(dev(frames), dev(labels), d_masks, d_boxes, matrices=torch.from_numpy(np.asarray(mats, dtype=np.float32)),
                         flip=flips if flip_arg is None else flip_arg, max_obj=F, **kw)
    compare(got, want, what)
    return got, want


def compare(got, want, what=""):
    for k in KEYS:
        g = getattr(got, k).cpu().numpy()
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (what, k, g.dtype, g.shape, want[k].shape)
        assert np.array_equal(g, want[k]), (what, k, np.argwhere(g != want[k])[:6].tolist())


@pytest.mark.parametrize("name", [str(c) for c in golden("augment")["clips"]])
def test_fixture_clips(name):
    g = golden("augment").group(name)
    n, H, W = g["labels"].shape
    F = int(g["F"])
    got, want = check(g["frames"], g["labels"], g["masks"], g["boxes_in"], g["matrices"], bool(g["flip"]), F, name)
    # ... and the reference's own planes wherever no near-tie pixel is (the CPU test's rule), its rows for the tie-free frames
    rows = np.unpackbits(g["out_rows"])[: n * F * (H * W + 1)].reshape(n, F, H * W + 1)
    mine = got.reference_targets()
    assert tuple(mine.shape) == (n, F, H * W + 1) and mine.dtype == torch.float32
    mine = mine.cpu().numpy()
    assert np.array_equal(mine, R.reference_rows(want["targets"], want["sizes"]).astype(np.float32))
    assert np.array_equal(got.sw.cpu().numpy(), (want["sizes"] > 0).astype(np.float32))
    for f in range(n):
        tie = R.near_tie(g["matrices"][f], H, W)
        for k in ("frames", "labels", "masks"):
            assert np.array_equal(getattr(got, k)[f].cpu().numpy()[..., ~tie], g["out_" + k][f][..., ~tie]), (name, f, k)
        if not tie.any():
            assert np.array_equal(mine[f], rows[f].astype(np.float32)), (name, f)
            assert np.array_equal(got.boxes[f].cpu().numpy(), g["out_boxes"][f])
            assert np.array_equal(got.box_valid[f].cpu().numpy(), g["out_box_valid"][f])


@pytest.mark.parametrize("H", [1, 2, 17])
def test_edge_widths(H):
    """Widths around the 64-column tile and the wave, one, two and several tile rows; several workgroups per frame."""
    rng = np.random.default_rng(300 + H)
    for W in (1, 2, 63, 64, 65, 129):
        n = 3
        frames, labels, masks, boxes = inputs(rng, n, 3, H, W, 2)
        flip, mats = drawn(1000 * H + W, n, H, W)
        mats[2] = IDENTITY
        check(frames, labels, masks, boxes, mats, [flip, not flip, True], 2, f"{H}x{W}")


@pytest.mark.parametrize("P", [0, 1, 50])
@pytest.mark.parametrize("F", [1, 5])
def test_proposal_and_target_counts(P, F):
    rng = np.random.default_rng(10 * P + F)
    n, H, W = 12, 37, 53
    frames, labels, masks, boxes = inputs(rng, n, 3, H, W, P)
    flip, mats = drawn(P + F, n, H, W)
    check(frames, labels, masks, boxes, mats, flip, F, f"P={P} F={F}", flip_arg=flip)


def test_flip_on_off_mixed_and_identity():
    rng = np.random.default_rng(5)
    n, H, W = 4, 19, 70
    frames, labels, masks, boxes = inputs(rng, n, 3, H, W, 3)
    _, mats = drawn(77, n, H, W)
    for flips, arg in ((False, False), (True, True), ([True, False, False, True], None),
                       ([0, 1, 1, 0], torch.tensor([0, 1, 1, 0], device=DEV))):
        check(frames, labels, masks, boxes, mats, flips, 5, f"flips {flips}", flip_arg=arg)
    ident = np.stack([IDENTITY] * n)
    got, _ = check(frames, labels, masks, boxes, ident, False, 5, "identity")
    assert np.array_equal(got.frames.cpu().numpy(), frames) and np.array_equal(got.labels.cpu().numpy(), labels)
    assert np.array_equal(got.masks.cpu().numpy(), masks)
    got, _ = check(frames, labels, masks, boxes, ident, True, 5, "identity + flip")
    assert np.array_equal(got.frames.cpu().numpy(), frames[..., ::-1]) and np.array_equal(got.labels.cpu().numpy(), labels[..., ::-1])
    assert np.array_equal(got.masks.cpu().numpy(), masks[..., ::-1])


def test_all_clamped_translation_replicates_an_edge():
    rng = np.random.default_rng(6)
    n, H, W = 3, 20, 66
    frames, labels, masks, boxes = inputs(rng, n, 3, H, W, 2)
    masks[:, 0, :, W - 1] = 1.0                            # mask 0 is on along the right edge
    masks[:, 0, H - 1, W - 1] = 0.0                        # ... but for the corner
    mats = np.stack([IDENTITY] * n)
    mats[0, 0, 2] = H                                      # every source row past the bottom: row H - 1 everywhere
    mats[1, 1, 2] = -W                                     # every source column before the left: column 0 everywhere
    mats[2, 0, 2], mats[2, 1, 2] = H, W                    # both: one corner pixel everywhere
    got, _ = check(frames, labels, masks, boxes, mats, False, 5, "clamped")
    fr, lb = got.frames.cpu().numpy(), got.labels.cpu().numpy()
    assert np.array_equal(fr[0], np.broadcast_to(frames[0][:, H - 1:H, :], frames[0].shape))
    assert np.array_equal(fr[1], np.broadcast_to(frames[1][:, :, 0:1], frames[1].shape))
    assert np.array_equal(lb[2], np.full((H, W), labels[2, H - 1, W - 1]))
    # frame 2: mask 0 reads its corner (0.0) everywhere -> empty: the input box stays; frame 0 is the bottom row repeated
    assert got.box_valid[2, 0].item() == 0 and np.array_equal(got.boxes[2, 0].cpu().numpy(), boxes[2, 0])


def test_empty_masks_threshold_and_stray_labels():
    H, W, F = 9, 70, 3
    frames = np.zeros((1, 1, H, W), dtype=np.float32)
    labels = np.zeros((1, H, W), dtype=np.uint8)
    labels[0, 0, :5], labels[0, 1, :7], labels[0, 2, :9], labels[0, 3, :4] = 255, F + 1, F, 1
    masks = np.zeros((1, 4, H, W), dtype=np.float32)
    masks[0, 0, 2:5, 64:69] = 0.5                          # exactly the threshold: strict >, so empty
    masks[0, 1, 2:5, 64:69] = np.nextafter(np.float32(0.5), np.float32(1))
    masks[0, 3, H - 1, W - 1] = 1.0                        # (mask 2 stays zero)
    boxes = np.arange(16, dtype=np.float32).reshape(1, 4, 4) + 100
    got, want = check(frames, labels, masks, boxes, IDENTITY[None], False, F, "threshold")
    assert got.box_valid.cpu().numpy().tolist() == [[0, 1, 0, 1]]
    b = got.boxes.cpu().numpy()[0]
    assert np.array_equal(b[0], boxes[0, 0]) and np.array_equal(b[2], boxes[0, 2])
    assert b[1].tolist() == [64, 2, 68, 4] and b[3].tolist() == [W - 1, H - 1, W - 1, H - 1]
    assert got.sizes.cpu().numpy().tolist() == [[4, 0, 9]]              # 255 and F + 1 are in no plane and no size
    assert got.targets.sum().item() == 13 and got.sw.cpu().numpy().tolist() == [[1.0, 0.0, 1.0]]


def test_strided_inputs_are_not_copied_and_not_written():
    rng = np.random.default_rng(8)
    n, H, W, P, F = 3, 21, 67, 4, 5
    frames, labels, masks, boxes = inputs(rng, n, 3, H, W, P)
    flip, mats = drawn(8, n, H, W)
    want = R.augment_clip(frames, labels, masks, boxes, mats, [flip] * n, F)
    big_f = torch.full((n, 5, H, W), -3.0, device=DEV)     # frame stride above the dense size: channels 1 .. 3 of 5
    big_f[:, 1:4] = dev(frames)
    big_l = torch.full((n, 2, H, W), 9, dtype=torch.uint8, device=DEV)
    big_l[:, 1] = dev(labels)
    m5 = dev(masks).unsqueeze(2)                           # [n,P,1,H,W], as the proposals' mask field comes
    vf, vl, vm = big_f[:, 1:4], big_l[:, 1], m5.squeeze(2)
    assert not vf.is_contiguous() and not vl.is_contiguous()
    assert A._strided(vf, 2) is vf and A._strided(vl, 1) is vl and A._strided(vm, 2) is vm
    keep = [t.clone() for t in (big_f, big_l, m5)]
    got = A.augment_clip(vf, vl, vm, dev(boxes), matrices=torch.from_numpy(mats), flip=flip, max_obj=F)
    compare(got, want, "strided")
    assert all(torch.equal(a, b) for a, b in zip(keep, (big_f, big_l, m5)))
    # views the ABI cannot address are copied: every other column, and a transposed frame
    wide = torch.zeros((n, 3, H, 2 * W), device=DEV)
    wide[..., ::2] = dev(frames)
    compare(A.augment_clip(wide[..., ::2], vl, vm, dev(boxes), matrices=torch.from_numpy(mats), flip=flip, max_obj=F), want, "copied")


def test_out_reuse_and_graph_replay():
    rng = np.random.default_rng(9)
    n, H, W, P, F = 4, 30, 65, 5, 5
    a = [inputs(rng, n, 3, H, W, P) for _ in range(2)]
    m = [drawn(90 + i, n, H, W) for i in range(2)]
    want = [R.augment_clip(*a[i], m[i][1], [m[i][0]] * n, F) for i in range(2)]
    frames, labels, masks, boxes = (dev(x) for x in a[0])
    mats = dev(m[0][1])
    flips = torch.full((n,), int(m[0][0]), dtype=torch.int32, device=DEV)
    out = A.augment_clip(frames, labels, masks, boxes, matrices=mats, flip=flips, max_obj=F)
    compare(out, want[0], "first")
    ptrs = [getattr(out, k).data_ptr() for k in KEYS]
    for k in KEYS:
        getattr(out, k).fill_(77)
    again = A.augment_clip(frames, labels, masks, boxes, matrices=mats, flip=flips, max_obj=F, out=out)
    assert again is out and ptrs == [getattr(out, k).data_ptr() for k in KEYS]
    compare(out, want[0], "out= reuse")
    g = SafeGraph()
    # (a capture stream of the test's own: this file runs early, and the process-wide capture stream -- with its place in
    # torch's stream pool -- stays for the first test that asks for it, as it was before this file existed)
    with g.capture(stream=torch.cuda.Stream()):
        A.augment_clip(frames, labels, masks, boxes, matrices=mats, flip=flips, max_obj=F, out=out)
    for x, src in zip((frames, labels, masks, boxes), a[1]):
        x.copy_(dev(src))
    mats.copy_(dev(m[1][1]))
    flips.fill_(int(m[1][0]))
    for k in KEYS:
        getattr(out, k).fill_(55)
    g.replay()
    torch.cuda.synchronize()
    compare(out, want[1], "replay 1")
    first = [getattr(out, k).cpu().numpy().tobytes() for k in KEYS]
    g.replay()
    torch.cuda.synchronize()
    assert first == [getattr(out, k).cpu().numpy().tobytes() for k in KEYS]
    assert g.left == 0
    with pytest.raises(ValueError):
        A.augment_clip(frames, labels, masks, boxes, matrices=mats, flip=flips, max_obj=F + 1, out=out)


def test_statuses_in_their_documented_order():
    """Argument checks only: nothing here launches."""
    L = _lib.load()
    n, C, P, F, H, W = 2, 3, 2, 5, 8, 9
    hw = H * W
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=DEV)
    t = dict(frames_in=z(n, C, H, W), frames_out=z(n, C, H, W), labels_in=z(n, H, W, dt=torch.uint8),
             labels_out=z(n, H, W, dt=torch.uint8), masks_in=z(n, P, H, W), masks_out=z(n, P, H, W), boxes_in=z(n, P, 4),
             boxes_out=z(n, P, 4), box_valid=z(n, P, dt=torch.int32), targets=z(n, F, H, W), sizes=z(n, F, dt=torch.int32),
             matrices=z(n, 9), flips=z(n, dt=torch.int32))
    base = dict(fs_fi=C * hw, ps_fi=hw, fs_fo=C * hw, ps_fo=hw, fs_li=hw, fs_lo=hw, fs_mi=P * hw, ps_mi=hw, fs_mo=P * hw, ps_mo=hw,
                n=n, C=C, P=P, F=F, H=H, W=W)
    OK, BAD, UNS = _lib.DMM_OK, _lib.DMM_ERR_BAD_ARG, _lib.DMM_ERR_UNSUPPORTED

    def call(**kw):
        a, p = dict(base), {k: v.data_ptr() for k, v in t.items()}
        for k, v in kw.items():
            if k in a:
                a[k] = v
            else:
                p[k] = None if v is None else v.data_ptr()
        return L.dmm_augment_clip_f32(p["frames_in"], a["fs_fi"], a["ps_fi"], p["frames_out"], a["fs_fo"], a["ps_fo"], p["labels_in"],
                                      a["fs_li"], p["labels_out"], a["fs_lo"], p["masks_in"], a["fs_mi"], a["ps_mi"], p["masks_out"],
                                      a["fs_mo"], a["ps_mo"], p["boxes_in"], p["boxes_out"], p["box_valid"], p["targets"], p["sizes"],
                                      p["matrices"], p["flips"], a["n"], a["C"], a["P"], a["F"], a["H"], a["W"], None, 0,
                                      torch.cuda.current_stream().cuda_stream)

    n0 = L.dmm_launch_count()
    assert L.dmm_augment_clip_workspace_bytes(n, C, P, F, H, W) == 0
    # 1. sizes and strides
    for bad in [dict(n=-1), dict(C=-1), dict(P=-1), dict(F=-1), dict(H=-1), dict(W=-1), dict(ps_fi=hw - 1), dict(ps_fo=hw - 1),
                dict(fs_fi=hw - 1), dict(fs_fo=hw - 1), dict(fs_li=hw - 1), dict(fs_lo=hw - 1), dict(ps_mi=hw - 1),
                dict(ps_mo=hw - 1), dict(fs_mi=hw - 1), dict(fs_mo=hw - 1)]:
        assert call(**bad) == BAD, bad
    assert call(ps_fi=hw - 1, n=0) == BAD and call(ps_mo=hw - 1, F=255) == BAD      # the earlier answer is named
    # 2. nothing to do: pointers not looked at
    none = {k: None for k in t}
    assert call(n=0, **none) == OK and call(H=0, fs_li=0, fs_lo=0, **none) == OK and call(W=0, **none) == OK
    # 3. null pointers; in place
    for k in t:
        if k != "flips":
            assert call(**{k: None}) == BAD, k
    assert call(targets=None, sizes=None, F=255) == BAD
    for a, b in (("frames_in", "frames_out"), ("labels_in", "labels_out"), ("masks_in", "masks_out"), ("boxes_in", "boxes_out")):
        assert call(**{b: t[a]}) == BAD, a
    assert call(frames_out=t["frames_in"], F=255) == BAD
    # 4. the envelope
    assert call(F=255) == UNS
    assert call(H=1 << 16, W=1 << 15, **{k: 1 << 31 for k in ("fs_fi", "ps_fi", "fs_fo", "ps_fo", "fs_li", "fs_lo", "fs_mi", "ps_mi",
                                                               "fs_mo", "ps_mo")}) == UNS
    assert call(n=(1 << 31) - 1, H=1, W=1025, fs_li=1025, fs_lo=1025, C=0, P=0, F=0) == UNS    # several tiles a frame: the grid
    assert L.dmm_launch_count() == n0
    with pytest.raises(_lib.DmmError):
        A.augment_clip(t["frames_in"], t["labels_in"], matrices=t["matrices"].view(n, 3, 3), flip=False, max_obj=255)
    assert L.dmm_launch_count() == n0
