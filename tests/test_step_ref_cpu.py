"""tests/step_ref.py held to what it can be held to without a GPU: the reference's goldens, the 1-bit layout's identities, an
fp32 emulation of the kernel's fma chain against the derived bound, every mutant red through the SAME comparison the GPU tests
use, and the 1 % condition on the undecided bits and labels -- a condition on the inputs, met by the reference alone."""
import numpy as np
import pytest

import oracle
import step_ref as sr
from conftest import golden


def test_reference_reproduces_the_paste_and_nms_goldens():
    g = golden("g9_paste")
    for k in range(int(g["n"])):
        c = g.group(f"c{k}")
        h, w = [int(v) for v in c["size"]]
        P = len(c["boxes"])
        scores = np.linspace(0.9, 0.1, P).astype(np.float32)[None]
        e = sr.prepare_expected(c["prob"].reshape(1, P, c["prob"].shape[-1], -1), c["boxes"][None], scores, None, h, w,
                                float(c["thresh"]), int(c["padding"]), 2.0, P)                 # IoU <= 1: nothing suppressed
        assert list(e.keep[0]) == list(range(P)) and int(e.count[0]) == P
        assert float(np.abs(e.planes[0].reshape(P, h, w) - c["masks"].reshape(P, h, w)).max()) <= 2.4e-7
        assert np.array_equal(e.tight[0], c["new_boxes"]) and np.array_equal(e.kept_boxes[0], c["new_boxes"])
        assert np.array_equal(e.packed[0], sr.pack_bits(e.planes[0]))
    g = golden("g13_nms")
    for k in range(int(g["n"])):
        c = g.group(f"c{k}")
        n, K = len(c["scores"]), int(c["max_keep"]) or max(len(c["scores"]), 1)
        keep, cnt = sr.nms_expected(c["boxes"].reshape(1, n, 4), c["scores"].reshape(1, n), None, n, float(c["thresh"]), K)
        assert np.array_equal(keep[0, :cnt[0]], c["keep"]) and bool((keep[0, cnt[0]:] == sr.SENT_I).all()), k
        assert np.array_equal(sr.nms_np(c["boxes"], c["scores"], float(c["thresh"]), int(c["max_keep"])), c["keep"]), k


@pytest.mark.parametrize("HW", [1, 15, 255, 256, 257, 259, 1025, 1320, 4731])
def test_pack_layout_identities(HW):
    gen = np.random.default_rng(HW)
    planes = gen.uniform(0, 1, (3, HW)).astype(np.float32)
    planes[0, : min(HW, 7)] = 0.5                              # exactly at the threshold: not set
    w = sr.pack_bits(planes)
    assert w.shape == (3, 4 * ((HW + 255) // 256)) and w.dtype == np.int64
    pop = np.array([sum(bin(int(x)).count("1") for x in row.view(np.uint64)) for row in w])
    assert np.array_equal(pop, (planes > 0.5).sum(axis=1))     # popcount == area: no pad bit is set
    assert np.array_equal(sr.unpack_bits(w, HW), planes > 0.5)
    p = HW - 1                                                 # one pixel -> word 4 (p / 256) + p % 4, bit (p % 256) / 4
    one = np.zeros(HW, np.float32)
    one[p] = 1.0
    w1 = sr.pack_bits(one).view(np.uint64)
    assert int(w1[4 * (p // 256) + p % 4]) == 1 << ((p % 256) // 4) and int((w1 != 0).sum()) == 1


@pytest.mark.parametrize("n", sr.NMS_SIZES + (65, 1024))
def test_numpy_nms_is_the_oracle(n):
    R = max(n, 64)
    tight, scores, _ = sr.nms_inputs(n, R)
    for i in range(tight.shape[0]):
        for K in sr.nms_ks(n) + [0]:
            assert np.array_equal(sr.nms_np(tight[i, :n], scores[i, :n], sr.NMS_T, K), oracle.nms(tight[i, :n], scores[i, :n], sr.NMS_T, K))
    if n >= 8:                                                 # what the generator promises
        b, s = sr.nms_boxes(n)
        keep = list(oracle.nms(b, s, sr.NMS_T))
        at = lambda box: int(np.nonzero((b == np.asarray(box, np.float32)).all(axis=1))[0][0])
        assert at((6, 0, 15, 9)) in keep and at((3, 0, 12, 9)) not in keep                      # the chain
        assert at((100, 0, 109, 4)) in keep                    # IoU exactly 0.5 does not suppress
        assert at((1, 0, 10, 9)) not in keep
        rank = list(np.argsort(-s, kind="stable"))
        assert rank.index(at((1, 0, 10, 9))) - rank.index(at((0, 0, 9, 9))) == n - 1


def _as_device(fin):
    """A reference (or mutant) result in the form the device hands back: full rounded to float32, hist, words, labels."""
    full = fin.full.astype(np.float32)
    hist = np.where(fin.hist_written[:, None, None], full, fin.hist)
    return full, hist, fin.packed_flat, fin.labels


@pytest.mark.parametrize("name", [c.name for c in sr.FINISH_CASES])
def test_fp32_emulation_inside_the_bound_and_one_percent_condition(name):
    c, d = sr.FINISH_BY_NAME[name], sr.finish_inputs(name)
    ref = sr.finish_expected(name)
    emu = sr.emulate_finish32(d["Rb"], d["planes"], d["count"], c.m_valid)
    err = np.abs(emu.astype(np.float64) - ref.full)
    assert bool((err <= ref.bound).all()), float((err - ref.bound).max())
    assert np.array_equal(emu[ref.exact], ref.full[ref.exact].astype(np.float32))              # one-hot rows: exact
    # the emulation's bits and labels agree with the reference on every decided element
    assert not ((emu > 0.5) != ref.bits)[ref.bits_decided].any()
    fails, _ = sr.compare_finish(ref, *_as_device(ref), has_packed=c.packed, has_labels=c.labels)
    assert not fails, fails
    ub, ul = sr.undecided_share(ref)
    assert ub <= 0.01 and ul <= 0.01, (ub, ul)
    # the case forms are what the list says
    for b in range(c.B):
        Nb = int(d["count"][b])
        Mb = c.M if c.m_valid is None else c.m_valid[b]
        used = int((d["Rb"][b, :Mb, :Nb] != 0).any(axis=0).sum()) if Nb else 0
        if c.weights == "dense":
            assert used == c.U[b], (b, used)
        else:
            assert bool(ref.exact[b].all())


def test_exact_ties_are_present_and_decided():
    ref = sr.finish_expected("onehot_33x40")
    assert bool((ref.full[0] == 0.5).any()), "no value exactly at the 1-bit threshold"
    assert bool(((ref.full[0, 0] == ref.full[0, 1]) & (ref.full[0, 0] > 0.5) & (ref.labels[0] == 1)).any()), "no label tie"
    assert bool(ref.labels_decided.all() and ref.bits_decided.all())
    e = sr.prep_expected("33x40")
    assert bool((e.planes[e.planes != sr.SENT_F] == 0.5).any())


def _finish_applies(mut, c):
    if mut == "unbounded_store":
        return c.packed and c.commit is not None and any(c.commit) and (-(-(c.H * c.W) // 256) * 256) % 1024 != 0
    if mut == "chunk16":
        return c.weights == "dense" and max(c.U) > 16
    if mut == "no_mb":
        return c.m_valid is not None and any(m < c.M for m in c.m_valid)
    return True


@pytest.mark.parametrize("mut", [m for m, (_, fam) in sr.MUTANTS.items() if "finish" in fam])
def test_finish_mutants_are_red(mut):
    red = []
    for c in sr.FINISH_CASES:
        if not _finish_applies(mut, c):
            continue
        fails, _ = sr.compare_finish(sr.finish_expected(c.name), *_as_device(sr.finish_expected(c.name, mut)),
                                     has_packed=c.packed, has_labels=c.labels)
        if fails:
            red.append(c.name)
    assert red, f"mutant '{sr.MUTANTS[mut][0]}' passes every case"
    if mut == "unbounded_store":                               # the three sizes with out-of-range waves all show it
        assert {"onehot_33x40", "onehot_57x83", "onehot_25x41"} <= set(red), red


@pytest.mark.parametrize("mut", [m for m, (_, fam) in sr.MUTANTS.items() if "prep" in fam or fam == "nms"])
def test_preparation_mutants_are_red(mut):
    red = []
    if sr.MUTANTS[mut][1] != "nms":
        for c in sr.PREP_CASES:
            if sr.compare_prep(sr.prep_expected(c.name), sr.prep_expected(c.name, mut)):
                red.append(c.name)
    else:
        for n in sr.NMS_SIZES:
            tight, scores, counts = sr.nms_inputs(n)
            cnts = np.asarray([70, 64]) if mut == "no_clamp" else counts
            for K in sr.nms_ks(n):
                a = sr.nms_expected(tight, scores, cnts, 64, sr.NMS_T, K)
                m = sr.nms_expected(tight, scores, cnts, 64, sr.NMS_T, K, mut=mut)
                if not (np.array_equal(a[0], m[0]) and np.array_equal(a[1], m[1])):
                    red.append((n, K))
        if mut == "cols48":
            assert {n for n, _ in red} == {49, 63, 64}, red    # every size that has columns 48..63
    assert red, f"mutant '{sr.MUTANTS[mut][0]}' passes every case"


def test_preparation_cases_hold_what_they_promise():
    """Dead slots, an image without a kept proposal, a truncated image (more survivors than K), the [0, 0, H, W] rule, the
    empty rule and a tight box equal to the clipped box, in every sized case."""
    for c in sr.PREP_CASES[:len(sr.SIZES)]:
        d, e = sr.prep_inputs(c.name), sr.prep_expected(c.name)
        t = c.step or 0
        assert 0 in e.count and int(e.count.max()) > 0 and bool((e.count < c.K).any()), (c.name, e.count)
        full_n = [i for i in range(c.images) if d["counts"][t][i] >= 14]
        assert full_n
        for i in full_n:
            whole = np.asarray([0, 0, c.H, c.W], np.float32)
            for r in (5, 6, sr.ALL_LOW):                       # wholly outside twice, all below the threshold
                assert np.array_equal(e.tight[i, r], whole), (c.name, r, e.tight[i, r])
    e = sr.prep_expected("57x83")
    assert int(e.count.max()) == sr.PREP_BY_NAME["57x83"].K    # truncated by K
