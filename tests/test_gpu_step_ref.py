"""The frame step's fixed-slot chain (``dmm_proposals.hip``: ``proposal_boxes_kernel``, ``nms_slots_kernel``,
``nms_slots_small_kernel``, ``paste_kept_kernel``, ``pack_kept_kernel``, ``step_finish_kernel``) against tests/step_ref.py, the
five C entries driven directly.  EVERY output is a view into a larger tensor with ``step_ref.GUARD`` sentinel elements on both
sides (and sentinels between planes where plane_stride > H W); what an entry must leave alone -- dead slots, ``keep`` past the
count, an uncommitted video's history -- holds sentinels too, and the whole buffer is compared: a stray store stays inside
memory the test owns and is a failed assertion.  Preparation entries: bit for bit.  ``dmm_step_finish_f32``: ``full`` / ``hist``
inside the derived bound on every element (one-hot rows exact), bits and labels equal where the reference decides, and bit for
bit against the unfused composition on the device.  Worst error / bound per case: profiles/step_ref_achieved.jsonl."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import step_ref as sr
from dmm_net_amd import _lib, ops
from dmm_net_amd import proposals as prop

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _record(name, v):
    from conftest import record_achieved
    record_achieved("step_ref/" + name, v)


def _s():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.array(a), dtype=dtype).to(DEV)      # (a copy: the cases' arrays are read-only)


def _p(t):
    return None if t is None else (t.ptr() if isinstance(t, Buf) else t.data_ptr())


class Buf:
    """An output buffer between two guard bands, everything filled with ``sent``."""

    def __init__(self, shape, dtype, sent):
        n = int(np.prod(shape))
        self.sent = int(sent) if dtype != torch.float32 else float(sent)
        self.all = torch.full((n + 2 * sr.GUARD,), self.sent, dtype=dtype, device=DEV)
        self.t = self.all[sr.GUARD:sr.GUARD + n].view(shape)

    def ptr(self):
        return self.t.data_ptr()

    def np(self):
        return self.t.cpu().numpy()

    def guards_intact(self):
        return bool((self.all[:sr.GUARD] == self.sent).all()) and bool((self.all[-sr.GUARD:] == self.sent).all())

    def untouched(self):
        return bool((self.all == self.sent).all())


def _guards(bufs):
    bad = [k for k, b in bufs.items() if b is not None and not b.guards_intact()]
    assert not bad, f"guard bands written: {bad}"


# ---- dmm_nms_slots_f32 ------------------------------------------------------------------------------------------------------
def _nms(tight, scores, counts, R, K, step=None, images=None):
    """One call -> (keep [images, K], keep_count [images]) as numpy, guards checked."""
    images = tight.shape[0] if images is None else images
    keep, cnt = Buf((images, K), torch.int32, sr.SENT_I), Buf((images,), torch.int32, sr.SENT_I)
    _lib.call("dmm_nms_slots_f32", DEV, tight.data_ptr(), scores.data_ptr(), _p(counts), images, R, float(sr.NMS_T), K, _p(step),
              keep.ptr(), cnt.ptr(), _s())
    _guards({"keep": keep, "keep_count": cnt})
    return keep.np(), cnt.np()


@pytest.mark.parametrize("wave", [1, 0], ids=["small", "general"])
@pytest.mark.parametrize("n", sr.NMS_SIZES)
def test_nms_slots_sizes_at_r64(n, wave):
    """n boxes in R = 64 slots through the one-workgroup kernel (its four 16-column wave slices, both halves of the 64-bit
    mask) and the same inputs through the general kernel: duplicates, score ties, a pair at IoU exactly 0.5, a chain, and from
    n = 49 a lowest box that only the highest suppresses (column n - 1); K in {1, n - 1, n, n + 5}; ``keep`` past the count
    keeps its sentinel; the slots past n hold boxes with higher scores that must not be read."""
    tight, scores, counts = sr.nms_inputs(n)
    dt, ds, dc = _dev(tight), _dev(scores), _dev(counts)
    with _lib.options(NMS_WAVE=wave):
        for K in sr.nms_ks(n):
            ek, ec = sr.nms_expected(tight, scores, counts, 64, sr.NMS_T, K)
            gk, gc = _nms(dt, ds, dc, 64, K)
            assert np.array_equal(gc, ec) and np.array_equal(gk, ek), (n, K, gc, ec)


@pytest.mark.parametrize("n", [65, 1024])
def test_nms_slots_general_kernel_at_its_edges(n):
    """n = R = 65 (the first size past the routing edge) and n = R = 1024 (the largest), counts == NULL."""
    tight, scores, _ = sr.nms_inputs(n, R=n)
    dt, ds = _dev(tight), _dev(scores)
    for K in sr.nms_ks(n):
        ek, ec = sr.nms_expected(tight, scores, None, n, sr.NMS_T, K)
        gk, gc = _nms(dt, ds, None, n, K)
        assert np.array_equal(gc, ec) and np.array_equal(gk, ek), (n, K)
    rc = _lib.call("dmm_nms_slots_f32", DEV, dt.data_ptr(), ds.data_ptr(), None, 1, 1025, 0.5, 4, None, dt.data_ptr(),
                   dt.data_ptr(), _s(), allow=(_lib.DMM_ERR_UNSUPPORTED,))
    assert rc == _lib.DMM_ERR_UNSUPPORTED


@pytest.mark.parametrize("wave", [1, 0], ids=["small", "general"])
def test_nms_slots_counts_clamped_null_and_clip_resident(wave):
    """counts above R (clamped to R), negative (no box), NULL (R boxes); scores / counts clip resident with T = 3 and the
    device ``step`` at 0 and 2."""
    R, K = 64, 40
    tight, scores, _ = sr.nms_inputs(64, images=3)
    dt, ds = _dev(tight), _dev(scores)
    with _lib.options(NMS_WAVE=wave):
        for counts in (np.asarray([70, -3, 64], np.int32), np.asarray([1 << 30, 0, 17], np.int32), None):
            ek, ec = sr.nms_expected(tight, scores, counts, R, sr.NMS_T, K)
            gk, gc = _nms(dt, ds, _dev(counts), R, K)
            assert np.array_equal(gc, ec) and np.array_equal(gk, ek), counts
            if counts is not None:
                assert gc[1] == 0
        gen = np.random.default_rng(3)
        clip_s = np.stack([scores, gen.permuted(scores, axis=1), gen.permuted(scores, axis=1)])
        clip_c = np.asarray([[64, 30, 5], [1, 1, 1], [49, 64, 0]], np.int32)
        dcs, dcc = _dev(clip_s), _dev(clip_c)
        for t in (0, 2):
            ek, ec = sr.nms_expected(tight, clip_s[t], clip_c[t], R, sr.NMS_T, K)
            gk, gc = _nms(dt, dcs, dcc, R, K, step=_dev(np.asarray([t], np.int32)), images=3)
            assert np.array_equal(gc, ec) and np.array_equal(gk, ek), t


# ---- the three preparation entries on every plane size ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _prep_dev(name):
    c, d = sr.PREP_BY_NAME[name], sr.prep_inputs(name)
    out = {k: _dev(v) for k, v in d.items()}
    out["step"] = None if c.step is None else _dev(np.asarray([c.step], np.int32))
    out["base"] = None if c.base is None else _dev(np.asarray([c.base + t for t in range(c.T)], np.int32))
    return out


def _run_prep(name, form, null=()):
    """proposal_boxes -> nms_slots -> paste_kept in one of its forms -> (Prep of numpy arrays, None where not asked for)."""
    c, dv = sr.PREP_BY_NAME[name], _prep_dev(name)
    HW, words = c.H * c.W, sr.pack_words(c.H * c.W)
    stride = HW + c.stride_extra
    f32, i32 = torch.float32, torch.int32
    b = {"tight": Buf((c.images, c.R, 4), f32, sr.SENT_F), "keep": Buf((c.images, c.K), i32, sr.SENT_I),
         "count": Buf((c.images,), i32, sr.SENT_I),
         "planes": Buf((c.images * c.K, stride), f32, sr.SENT_F) if form != "packed" else None,
         "packed": Buf((c.images, c.K, words), torch.int64, sr.SENT_W) if form != "planes" else None,
         "kept_boxes": None if "kept_boxes" in null else Buf((c.images, c.K, 4), f32, sr.SENT_F),
         "kept_scores": None if "kept_scores" in null else Buf((c.images, c.K), f32, sr.SENT_F),
         "rois": None if "rois" in null else Buf((c.images * c.K, 5), f32, sr.SENT_F)}
    b["keep"].t.copy_(_dev(sr.keep_before(c.images, c.K, c.R)))
    s = _s()
    _lib.call("dmm_proposal_boxes_f32", DEV, _p(dv["prob"]), _p(dv["boxes"]), _p(dv["counts"]), c.images, c.R, c.Mm, c.H, c.W,
              float(sr.MASK_T), c.pad, _p(dv["step"]), b["tight"].ptr(), s)
    _lib.call("dmm_nms_slots_f32", DEV, b["tight"].ptr(), _p(dv["scores"]), _p(dv["counts"]), c.images, c.R, float(sr.NMS_T),
              c.K, _p(dv["step"]), b["keep"].ptr(), b["count"].ptr(), s)
    _lib.call("dmm_paste_kept_f32", DEV, _p(dv["prob"]), _p(dv["boxes"]), _p(dv["scores"]), b["tight"].ptr(), b["keep"].ptr(),
              b["count"].ptr(), c.images, c.R, c.Mm, c.K, c.H, c.W, c.pad, _p(dv["step"]), _p(dv["base"]), _p(b["planes"]),
              stride, _p(b["packed"]), _p(b["kept_boxes"]), _p(b["kept_scores"]), _p(b["rois"]), s)
    _guards(b)
    planes = None
    if b["planes"] is not None:
        pl = b["planes"].np().reshape(c.images, c.K, stride)
        assert bool((pl[:, :, HW:] == np.float32(sr.SENT_F)).all()), "the gap between two planes was written"
        planes = pl[:, :, :HW]
    g = lambda k: None if b[k] is None else b[k].np()
    return sr.Prep(g("tight"), g("keep"), g("count"), planes, g("kept_boxes"), g("kept_scores"), g("rois"), g("packed"))


@pytest.mark.parametrize("form", ["both", "planes", "packed"])
@pytest.mark.parametrize("name", [c.name for c in sr.PREP_CASES])
def test_preparation_entries_bit_for_bit(name, form):
    """Tight boxes, keep / count, kept planes, 1-bit planes, boxes, scores and roi rows equal paste-everything + NMS + top-K +
    gather of the oracle on every plane size of the list (1 x 1 to three paste bands; a width below 4; tails of 1, 3 and 4
    pixels), with boxes inside, cut by each side, wholly outside, degenerate, sub-pixel, larger than the frame, over
    probabilities all below the threshold, all one and all exactly 0.5; an image without a kept proposal and dead slots (plane
    and words keep their sentinels, score 0, box 0, roi image index -1); plane_stride above H W; mask sizes 1, 32 and 64.
    ``packed``: planes == NULL, the product's form (``pack_kept_kernel``)."""
    fails = sr.compare_prep(sr.prep_expected(name), _run_prep(name, form))
    assert not fails, fails


@pytest.mark.parametrize("form", ["both", "packed"])
def test_paste_kept_optional_outputs_null_in_turn(form):
    name = "33x40"
    exp = sr.prep_expected(name)
    for null in ("kept_boxes", "kept_scores", "rois"):
        fails = sr.compare_prep(exp, _run_prep(name, form, null=(null,)))
        assert not fails, (null, fails)


def test_mask_size_limits_of_the_preparation_entries():
    """Mp = 64 is served (case mp64_33x40 above); Mp = 65 is DMM_ERR_UNSUPPORTED at all three and nothing is written."""
    one = torch.zeros(65 * 65 * 4, device=DEV)
    out = Buf((64,), torch.float32, sr.SENT_F)
    U = _lib.DMM_ERR_UNSUPPORTED
    assert _lib.call("dmm_proposal_boxes_f32", DEV, one.data_ptr(), one.data_ptr(), None, 1, 1, 63, 8, 8, 0.4, 1, None, out.ptr(),
                     _s(), allow=(U,)) == U
    assert _lib.call("dmm_paste_kept_f32", DEV, *[one.data_ptr()] * 6, 1, 1, 63, 1, 8, 8, 1, None, None, out.ptr(), 64, None,
                     None, None, None, _s(), allow=(U,)) == U
    assert _lib.call("dmm_paste_kept_f32", DEV, *[one.data_ptr()] * 6, 1, 1, 63, 1, 8, 8, 1, None, None, None, 64, out.ptr(),
                     None, None, None, _s(), allow=(U,)) == U
    torch.cuda.synchronize()
    assert out.untouched()


# ---- dmm_step_finish_f32 ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _finish_dev(name):
    c, d = sr.FINISH_BY_NAME[name], sr.finish_inputs(name)
    i32 = lambda v: None if v is None else _dev(np.asarray(v, np.int32))
    return dict(Rb=_dev(d["Rb"]), prob=_dev(d["prob"]), boxes=_dev(d["boxes"]), scores=_dev(d["scores"]), keep=_dev(d["keep"]),
                count=_dev(d["count"]), m_valid=i32(c.m_valid), o_valid=i32(c.o_valid), commit=i32(c.commit),
                step=None if c.step is None else i32([c.step]))


def _run_finish(name, Mm=None, allow=()):
    c, d, dv = sr.FINISH_BY_NAME[name], sr.finish_inputs(name), _finish_dev(name)
    HW = c.H * c.W
    b = {"full": Buf((c.B, c.M, HW), torch.float32, sr.SENT_F), "hist": Buf((c.B, c.M, HW), torch.float32, sr.SENT_F),
         "packed": Buf((c.B, c.M, sr.pack_words(HW)), torch.int64, sr.SENT_W) if c.packed else None,
         "labels": Buf((c.B, HW), torch.uint8, sr.SENT_L) if c.labels else None}
    rc = _lib.call("dmm_step_finish_f32", DEV, _p(dv["Rb"]), d["Pp"], _p(dv["prob"]), _p(dv["boxes"]), _p(dv["keep"]),
                   _p(dv["count"]), c.B, c.R, c.Mm if Mm is None else Mm, c.K, c.M, c.H, c.W, c.pad, _p(dv["step"]),
                   _p(dv["m_valid"]), _p(dv["commit"]), _p(dv["o_valid"]), b["full"].ptr(), b["hist"].ptr(), _p(b["packed"]),
                   _p(b["labels"]), _s(), allow=allow)
    return rc, b


def _unfused(name):
    """dmm_paste_kept_f32 (planes) -> ops.mask_mix -> dmm_commit_masks_f32 -> ops.pack_masks -> dmm_merge_labels_f32."""
    c, dv = sr.FINISH_BY_NAME[name], _finish_dev(name)
    HW = c.H * c.W
    planes = torch.zeros((c.B, c.K, c.H, c.W), device=DEV)
    tight = torch.zeros((c.B, c.R, 4), device=DEV)
    s = _s()
    _lib.call("dmm_paste_kept_f32", DEV, _p(dv["prob"]), _p(dv["boxes"]), _p(dv["scores"]), tight.data_ptr(), _p(dv["keep"]),
              _p(dv["count"]), c.B, c.R, c.Mm, c.K, c.H, c.W, c.pad, _p(dv["step"]), None, planes.data_ptr(), HW, None, None,
              None, None, s)
    full = ops.mask_mix(dv["Rb"], planes, n_valid=dv["count"], m_valid=dv["m_valid"])
    hist = torch.full((c.B, c.M, c.H, c.W), sr.SENT_F, device=DEV)
    if dv["commit"] is not None:
        _lib.call("dmm_commit_masks_f32", DEV, full.data_ptr(), hist.data_ptr(), _p(dv["commit"]), c.B, c.M * HW, s)
    labels = torch.empty((c.B, HW), dtype=torch.uint8, device=DEV)
    _lib.call("dmm_merge_labels_f32", DEV, full.data_ptr(), c.B, c.M, HW, c.M * HW, HW, _p(dv["o_valid"]), labels.data_ptr(), s)
    return full.view(c.B, c.M, HW), hist.view(c.B, c.M, HW), ops.pack_masks(hist), labels


@pytest.mark.parametrize("name", [c.name for c in sr.FINISH_CASES])
def test_step_finish_against_reference_and_unfused_composition(name):
    """Every case of step_ref.FINISH_CASES: one-hot rows (exact; a label tie of two identical rows, a row at most 0.5, a
    negative row, values exactly 0.5), dense rows with 0, 1, 15, 16, 17 and 33 used columns (the second and third chunk of
    16), weights in rows >= m_valid and columns >= keep_count that must not count, m_valid / o_valid below M, 0 and NULL,
    commit NULL and mixed -- the uncommitted video after a committed one holds sentinels in ``hist`` and ``packed_hist`` and
    must keep them -- packed_hist / labels NULL, keep_count 0, the plane sizes whose last workgroup has waves past the plane
    (25 x 41, 33 x 40, 57 x 83), planes below one block, Mp of 1 and 32, a clip-resident frame."""
    c = sr.FINISH_BY_NAME[name]
    ref = sr.finish_expected(name)
    rc, b = _run_finish(name)
    full, hist = b["full"].np(), b["hist"].np()
    flat = b["packed"].all.cpu().numpy() if c.packed else None
    labels = b["labels"].np() if c.labels else None
    fails, ratio = sr.compare_finish(ref, full, hist, flat, labels, has_packed=c.packed, has_labels=c.labels)
    _record(f"finish/{name}", ratio)
    fails += [f"guard band of {k} written" for k, v in b.items() if v is not None and not v.guards_intact()]
    # the unfused composition on the device: bit for bit
    f2, h2, p2, l2 = _unfused(name)
    if not torch.equal(b["full"].t, f2):
        fails.append("full differs from paste + mask_mix")
    if not torch.equal(b["hist"].t, h2):
        fails.append("hist differs from paste + mask_mix + commit")
    if c.labels and not torch.equal(b["labels"].t, l2):
        fails.append("labels differ from merge_labels")
    if c.packed:
        for v in range(c.B):
            if ref.hist_written[v] and not torch.equal(b["packed"].t[v], p2[v]):
                fails.append(f"packed_hist[{v}] differs from pack_masks(hist)")
    assert not fails, fails


def test_step_finish_refuses_mp33_and_touches_nothing():
    """Mp = 32 is served (case mp32); Mm = 31 with padding 1 is DMM_ERR_UNSUPPORTED and no output is written."""
    rc, b = _run_finish("mp32", Mm=31, allow=(_lib.DMM_ERR_UNSUPPORTED,))
    assert rc == _lib.DMM_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(v.untouched() for v in b.values())


# ---- routes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [64, 65])
def test_prepare_slots_on_both_sides_of_the_routing_edge(R):
    """``proposals.prepare_slots`` with 64 raw proposals in R = 64 (one-workgroup NMS) and R = 65 slots (general kernel)."""
    H, W, K, images = 33, 40, 12, 2
    prob, boxes, scores = sr.raw_proposals(H, W, 1, images, 64, 28, 9064)
    counts = np.asarray([64, 50], np.int32)
    exp = sr.prepare_expected(prob[0], boxes[0], scores[0], counts, H, W, sr.MASK_T, 1, sr.NMS_T, K)

    def padded(a, fill):
        out = np.full(a.shape[:2] + (R,) + a.shape[3:], fill, dtype=a.dtype)
        out[:, :, :64] = a
        return out
    clip = prop.ClipProposals(_dev(padded(prob, 0.9)), _dev(padded(boxes, 3.0)), _dev(padded(scores, 5.0)), _dev(counts[None]))
    slots = prop.ProposalSlots(images, K, H, W, R, DEV)
    slots.planes.fill_(sr.SENT_F)
    slots.packed.fill_(int(sr.SENT_W))
    prop.prepare_slots(clip, slots, sr.NMS_T, sr.MASK_T, 1)
    got = sr.Prep(slots.tight.cpu().numpy()[:, :64], None, slots.count.cpu().numpy(), slots.planes.view(images, K, H * W).cpu().numpy(),
                  slots.boxes.cpu().numpy(), slots.scores.cpu().numpy(), slots.rois.cpu().numpy(), slots.packed.cpu().numpy())
    fails = sr.compare_prep(exp, got)
    keep = slots.keep.cpu().numpy()
    for i in range(images):
        if not np.array_equal(keep[i, :exp.count[i]], exp.keep[i, :exp.count[i]]):
            fails.append(f"keep[{i}]")
    assert not fails, fails


def test_frame_loop_33x40_three_routes_and_the_packed_history():
    """One clip of three frames at 33 x 40 (H W rounds to 1536: two waves of the last workgroup lie past the plane): the
    two templates and two of the three proposal groups lie in the plane's first rows, so words 0..3 of history planes that
    follow another plane in the buffer hold real bits (asserted).  Fused graph, fused direct, unfused and BoxList paths give equal histories and label maps;
    the fused paths' ``packed_hist`` equals ``ops.pack_masks(hist)`` after every frame."""
    from dmm_net_amd import video
    from dmm_net_amd.dmm_model import DMM_Model
    from dmm_net_amd.roi_features import FeatureExtractor
    from test_gpu_video import _PoolEncoder
    rng = np.random.default_rng(3340)
    B, T, O, H, W = 3, 3, 2, 33, 40
    cfgs = {"matching": {"algo": "relax"}, "relax_max_iter": 40, "relax_proj_iter": 5, "relax_learning_rate": 0.1,
            "score_weight": 0.3}
    frames = torch.randn(B, T, 3, H, W, generator=torch.Generator().manual_seed(3340)).to(DEV)

    def raw(n):
        # three groups of near-duplicates: the left and the right half of the first rows (one per template) and the bottom
        g = np.arange(n) % 3
        x0 = np.where(g == 1, 20.0, 0.0) + rng.uniform(0, 2, n)
        y0 = np.where(g == 2, 20.0, 0.0) + rng.uniform(0, 2, n)
        bx = np.stack([x0, y0, x0 + np.where(g == 2, 30.0, 17.0) + rng.uniform(0, 1.5, n), y0 + rng.uniform(9, 11, n)], 1)
        bl = prop.SimpleBoxList(torch.from_numpy(bx.astype(np.float32)), (W, H))
        bl.add_field("scores", torch.from_numpy(rng.random(n).astype(np.float32)))
        bl.add_field("mask", torch.from_numpy((rng.random((n, 1, 28, 28)) * 0.4 + 0.6).astype(np.float32)))
        return bl
    props = [[raw(18 + 3 * b + t) for t in range(T)] for b in range(B)]
    first = torch.zeros(B, O, H, W, device=DEV)
    first[:, 0, 0:11, 0:19] = 1.0
    first[:, 1, 0:11, 20:39] = 1.0
    first = first.view(B, O, H * W)

    def run(slots, graph, **kn):
        lp = video.FrameLoop(_PoolEncoder(), DMM_Model(cfgs, is_test=1, feature_extractor=FeatureExtractor()), refine=None,
                             nms_thresh=0.4, max_proposals=10)
        lp.slots, lp.graph = slots, graph
        for k, v in kn.items():
            setattr(lp, k, v)
        labs, packs = {}, []

        def on_labels(b, t, lab):
            labs[(b, t)] = lab.clone()
            if b == 0 and lp._plan is not None and lp._plan.fused:
                packs.append((lp._plan.packed_hist.clone(), ops.pack_masks(lp._plan.hist)))
        h = [x.clone() for x in lp.run(frames, first, props, [T] * B, on_labels=on_labels)]
        return h, labs, packs
    ref_h, ref_l, _ = run(False, False)
    for h in ref_h:                # a plane that has a predecessor in the buffer holds bits in its first block, in every frame
        assert bool((h.view(B * O, H * W)[1:, :256] > 0.5).any())
    seen = []
    for slots, graph, kn in [(True, True, {}), (True, False, {}), (True, True, dict(fuse_epilogue=False))]:
        h, l, packs = run(slots, graph, **kn)
        assert all(torch.equal(a, c) for a, c in zip(ref_h, h)), (slots, graph, kn)
        assert sorted(l) == sorted(ref_l) and all(torch.equal(ref_l[k], l[k]) for k in ref_l), (slots, graph, kn)
        if kn == {}:
            assert len(packs) == T
            for t, (got, exp) in enumerate(packs):
                assert torch.equal(got, exp), (graph, t, int((got != exp).sum()))
            seen.append([p[0] for p in packs])
    assert all(torch.equal(a, c) for a, c in zip(*seen))
