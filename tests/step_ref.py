"""Reference of the frame-step proposal kernels (``csrc/dmm_proposals.hip``: ``proposal_boxes_kernel``, ``nms_slots_kernel``,
``nms_slots_small_kernel``, ``paste_kept_kernel``, ``pack_kept_kernel``, ``step_finish_kernel``), the expected contents of
every output BUFFER (what the entry must write and what it must leave alone), the shared comparison, the seeded case builders
and the mutants -- TEST INFRASTRUCTURE ONLY (no test functions here).  Plain numpy and the project's C oracle on the host.

Paste, tight boxes and NMS are the oracle's (``oracle.paste_masks``, ``oracle.nms``: the device is held to them bit for bit by
the existing tests), composed the way the evaluator does: paste every raw proposal, NMS + top-K on the tight boxes, gather.
The 1-bit layout is written here from the header's statement: in a block of 256 pixels word e (0..3), bit l holds pixel
256 q + 4 l + e for value > 0.5, pad bits zero, 4 ceil(HW / 256) words per plane.

``finish_ref`` is float64: full[m] = sum_n Rb[m, n] plane_n over the live block m < Mb, n < Nb.  The kernel does ONE fma per
non-zero weight of the row (zeros are skipped), so a row with k non-zero weights carries k roundings and
|device - reference| <= gamma(k) sum_n |Rb[m, n] plane_n| with gamma(k) = k u / (1 - k u), u = 2^-24 (Higham) -- derived from
the operation count, not measured.  A row with ONE non-zero weight is exact: fma(w, v, 0) is the one rounding of w v, which
float32(w) * float32(v) reproduces; a row without any is zero.  Bits (full > 0.5) and labels are compared where the reference
DECIDES: the margin to 0.5 / between the two best rows / of the best row to 0.5 is larger than the bounds of the rows
involved (an exact row has bound 0 and always decides, ties included: the first maximum wins).  The share left undecided is
asserted to stay at or below 1 % of every case (tests/test_step_ref_cpu.py).
"""
import collections
import functools

import numpy as np

import oracle

U = 2.0 ** -24
F = np.float32
SENT_F = -777.25                                               # finite, never a pasted value or a mix of the cases' weights
SENT_W = np.int64(0x5AA53CC35AA53CC3)                          # no ballot of the cases' planes gives it
SENT_I = -12345
SENT_L = 0xEE
GUARD = 64                                                     # sentinel elements in front of and behind every output


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


def pack_words(HW):
    return 4 * ((HW + 255) // 256)


def pack_bits(planes, ge=False):
    """[..., HW] values -> [..., words] int64: word 4 q + e, bit l = (pixel 256 q + 4 l + e > 0.5); pad bits zero."""
    planes = np.asarray(planes)
    HW = planes.shape[-1]
    nblk = (HW + 255) // 256
    bits = np.zeros(planes.shape[:-1] + (nblk * 256,), dtype=bool)
    bits[..., :HW] = (planes >= 0.5) if ge else (planes > 0.5)
    bits = bits.reshape(planes.shape[:-1] + (nblk, 64, 4))     # [q, l, e]
    sh = np.arange(64, dtype=np.uint64)[:, None]
    words = (bits.astype(np.uint64) << sh).sum(axis=-2, dtype=np.uint64)             # distinct bits: the sum is the or
    return words.reshape(planes.shape[:-1] + (nblk * 4,)).view(np.int64)


def unpack_bits(words, HW):
    """The inverse (tests of the layout): [..., words] int64 -> [..., HW] bool."""
    w = np.asarray(words).view(np.uint64)
    nblk = w.shape[-1] // 4
    w = w.reshape(w.shape[:-1] + (nblk, 1, 4))
    bits = (w >> np.arange(64, dtype=np.uint64)[:, None]) & np.uint64(1)
    return bits.reshape(w.shape[:-3] + (nblk * 256,)).astype(bool)[..., :HW]


# ---- NMS ----------------------------------------------------------------------------------------------------------------
def nms_np(boxes, scores, thresh, max_keep=0, mut=None):
    """``oracle.nms`` again in numpy float32 (descending score, the lower index first among equals, +1 areas, IoU > thresh
    suppresses) -- held to the oracle on every case; it exists to carry the mutants."""
    boxes, scores = np.asarray(boxes, dtype=np.float32).reshape(-1, 4), np.asarray(scores, dtype=np.float32)
    n = len(scores)
    order = np.argsort(-scores, kind="stable")
    b = boxes[order]
    one = F(1)
    area = (b[:, 2] - b[:, 0] + one) * (b[:, 3] - b[:, 1] + one)
    l, r = np.maximum(b[:, None, 0], b[None, :, 0]), np.minimum(b[:, None, 2], b[None, :, 2])
    t, d = np.maximum(b[:, None, 1], b[None, :, 1]), np.minimum(b[:, None, 3], b[None, :, 3])
    inter = np.maximum(r - l + one, F(0)) * np.maximum(d - t + one, F(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter / (area[:, None] + area[None, :] - inter)
    supp = (iou >= F(thresh)) if mut == "nms_ge" else (iou > F(thresh))
    if mut == "cols48" and n <= 64:
        supp[:, 48:] = False
    dead = np.zeros(n, dtype=bool)
    keep = []
    for a in range(n):
        if dead[a]:
            continue
        keep.append(int(order[a]))
        if max_keep > 0 and len(keep) >= max_keep:
            break
        dead[a + 1:] |= supp[a, a + 1:]
    return np.asarray(keep, dtype=np.int32)


def nms_boxes(n, seed=0):
    """n integer-valued boxes + scores with a chain (A kills B so C survives), a pair at IoU exactly 0.5 (50 / 100: not
    suppressed at thresh 0.5), a duplicate with a score tie, clustered boxes with tied scores, and -- from n = 8 on -- a lowest
    box that only the highest one suppresses (their ranks are n - 1 apart: >= 48 from n = 49).  Shuffled, so index != rank."""
    gen = np.random.default_rng(4000 + 131 * n + seed)
    bx, sc = [], []
    special = [((0, 0, 9, 9), 0.99), ((3, 0, 12, 9), 0.9), ((6, 0, 15, 9), 0.8),              # the chain
               ((100, 0, 109, 9), 0.7), ((100, 0, 109, 4), 0.6),                               # IoU = 50 / 100 exactly
               ((200, 0, 209, 9), 0.5), ((200, 0, 209, 9), 0.5)]                               # duplicate, equal scores
    for b, s in special[:n]:
        bx.append(b)
        sc.append(s)
    far = n >= 8
    clusters = max(1, n // 6)
    while len(bx) < n - (1 if far else 0):
        c = int(gen.integers(0, clusters))
        x0, y0 = 30 * (c % 40) + int(gen.integers(0, 6)), 50 + 30 * (c // 40) + int(gen.integers(0, 6))
        bx.append((x0, y0, x0 + int(gen.integers(8, 16)), y0 + int(gen.integers(8, 16))))
        sc.append(float(gen.integers(2, 15)) / 32.0)                                           # 13 values: many ties
    if far:
        bx.append((1, 0, 10, 9))                               # IoU 90 / 110 with (0, 0, 9, 9); 50 / 150 with the chain's C
        sc.append(0.01)
    perm = gen.permutation(n)
    boxes = np.asarray(bx, dtype=np.float32).reshape(-1, 4)[perm]
    scores = np.asarray(sc, dtype=np.float32)[perm]
    return np.ascontiguousarray(boxes), np.ascontiguousarray(scores)


def nms_expected(tight, scores, counts, R, thresh, K, mut=None, init_keep=None):
    """keep [images, K] (``SENT_I`` past the count: the entry leaves it alone) and keep_count [images] of dmm_nms_slots_f32
    for one frame: tight [images, R, 4], scores [images, R], counts [images] or None."""
    images = tight.shape[0]
    keep = np.full((images, K), SENT_I, dtype=np.int32) if init_keep is None else init_keep.copy()
    cnt = np.zeros(images, dtype=np.int32)
    flat_b = np.concatenate([tight.reshape(-1, 4), np.zeros((1024, 4), np.float32)])
    flat_s = np.concatenate([scores.reshape(-1), np.zeros(1024, np.float32)])
    for i in range(images):
        n = R if counts is None else int(counts[i])
        n = max(n, 0)
        if mut != "no_clamp":
            n = min(n, R)
        bb, ss = flat_b[i * R:i * R + n], flat_s[i * R:i * R + n]
        k = nms_np(bb, ss, thresh, K, mut) if mut else oracle.nms(bb, ss, thresh, K)
        cnt[i] = len(k)
        keep[i, :len(k)] = k
    return keep, cnt


# ---- proposals of a frame: the evaluator's composition --------------------------------------------------------------------
def box_kinds(H, W):
    """The raw boxes every sized case mixes (xyxy, image coordinates)."""
    h, w = float(H), float(W)
    return [(0.2 * w, 0.2 * h, 0.7 * w, 0.8 * h),                                  # inside
            (-0.4 * w - 2, 0.1 * h, 0.5 * w, 0.6 * h), (0.1 * w, -0.5 * h - 2, 0.6 * w, 0.5 * h),      # cut left / top
            (0.5 * w, 0.3 * h, 1.4 * w + 2, 0.9 * h), (0.3 * w, 0.5 * h, 0.8 * w, 1.5 * h + 2),        # cut right / bottom
            (-3 * w - 20, -3 * h - 20, -2 * w - 9, -2 * h - 9), (2 * w + 9, 0.0, 3 * w + 9, h),        # wholly outside
            (0.6 * w, 0.2 * h, 0.6 * w - 3.0, 0.7 * h),                            # degenerate: x2 < x1
            (0.3 * w + 0.2, 0.3 * h + 0.1, 0.3 * w + 0.5, 0.3 * h + 0.4),          # sub-pixel
            (-0.5 * w - 3, -0.5 * h - 3, 1.5 * w + 3, 1.5 * h + 3),                # larger than the frame
            (0.1 * w, 0.1 * h, 0.9 * w, 0.9 * h),                                  # (probabilities all below the threshold)
            (0.05 * w, 0.3 * h, 0.95 * w, 0.75 * h),                               # (probabilities all one)
            (0.0, 0.0, w - 1.0, h - 1.0), (0.25 * w, 0.0, 0.5 * w, h)]
ALL_LOW, ALL_ONE, ALL_HALF = 10, 11, 12                        # rows of box_kinds with constant probabilities


def raw_proposals(H, W, T, images, R, Mm, seed, extra_random=True):
    """Seeded clip-resident raw proposals: prob [T, images, R, Mm, Mm], boxes [T, images, R, 4], scores [T, images, R].
    Slot r carries box kind r % 14 (jittered from the second round on); kinds 10 / 11 / 12 carry probabilities all 0.3 / all
    1 / all 0.5 (pasted values exactly at the 1-bit threshold)."""
    gen = np.random.default_rng(seed)
    kinds = box_kinds(H, W)
    prob = gen.uniform(0.0, 1.0, (T, images, R, Mm, Mm)).astype(np.float32)
    prob[..., : (Mm + 1) // 2, :] = np.maximum(prob[..., : (Mm + 1) // 2, :], F(0.55))          # a solid upper half
    boxes = np.zeros((T, images, R, 4), dtype=np.float32)
    for r in range(R):
        k = r % len(kinds)
        jit = gen.uniform(-0.15, 0.15, (T, images, 4)) * np.asarray([W, H, W, H]) if r >= len(kinds) else 0.0
        boxes[:, :, r] = np.asarray(kinds[k], dtype=np.float64) + jit
        if k == ALL_LOW:
            prob[:, :, r] = F(0.3)
        if k == ALL_ONE:
            prob[:, :, r] = F(1.0)
        if k == ALL_HALF:
            prob[:, :, r] = F(0.5)
    scores = (gen.permutation(T * images * R).reshape(T, images, R).astype(np.float32) + F(1)) / F(T * images * R + 1)
    return prob, boxes, scores


Prep = collections.namedtuple("Prep", "tight keep count planes kept_boxes kept_scores rois packed")


def keep_before(images, K, R):
    """What ``keep`` holds before the chain runs in the tests: a pattern of raw indices in [0, R), so that the table stays a
    legal input of dmm_paste_kept_f32 in every slot; the entries past keep_count must still hold it afterwards."""
    return ((3 + 5 * np.arange(K)[None, :] + np.arange(images)[:, None]) % max(R, 1)).astype(np.int32)


def prepare_expected(prob, boxes, scores, counts, H, W, mask_thresh, padding, nms_thresh, K, base=0, mut=None):
    """One frame (prob [images, R, Mm, Mm], ...; counts [images] or None) -> the buffers the three preparation entries leave
    behind when every output started as its sentinel (``keep`` as ``keep_before``): tight [images, R, 4] (zeros for empty raw slots), keep / count,
    planes [images, K, HW] and packed [images, K, words] (dead slots keep their sentinels), kept boxes / scores (0 on dead
    slots), rois [images K, 5] (image index -1 on dead slots)."""
    images, R = scores.shape
    HW = H * W
    tight = np.zeros((images, R, 4), dtype=np.float32)
    all_planes = []
    for i in range(images):
        n = R if counts is None else min(max(int(counts[i]), 0), R)
        pl, tb = oracle.paste_masks(prob[i, :n], boxes[i, :n], H, W, mask_thresh, padding) if n else \
            (np.zeros((0, H, W), np.float32), np.zeros((0, 4), np.float32))
        tight[i, :n] = tb
        all_planes.append(pl.reshape(n, HW))
    keep, cnt = nms_expected(tight, scores, counts, R, nms_thresh, K, mut=mut if mut in ("nms_ge", "cols48", "no_clamp") else None,
                             init_keep=keep_before(images, K, R))
    planes = np.full((images, K, HW), SENT_F, dtype=np.float32)
    packed = np.full((images, K, pack_words(HW)), SENT_W, dtype=np.int64)
    kb, ks = np.zeros((images, K, 4), np.float32), np.zeros((images, K), np.float32)
    rois = np.zeros((images * K, 5), np.float32)
    rois[:, 0] = -1.0
    for i in range(images):
        for k in range(int(cnt[i])):
            r = int(keep[i, k])
            if r >= len(all_planes[i]):                        # (only the no-clamp mutant indexes past the image's rows)
                continue
            planes[i, k] = all_planes[i][r]
            packed[i, k] = pack_bits(all_planes[i][r], ge=mut == "mask_ge")
            kb[i, k], ks[i, k] = tight[i, r], scores[i, r]
            rois[i * K + k] = (base + i,) + tuple(tight[i, r])
        if mut == "dead_cleared":
            planes[i, int(cnt[i]):] = 0.0
            packed[i, int(cnt[i]):] = 0
    return Prep(tight, keep, cnt, planes, kb, ks, rois, packed)


# ---- the frame step's epilogue ----------------------------------------------------------------------------------------------
Finish = collections.namedtuple("Finish", "full bound exact hist hist_written packed_flat bits bits_decided labels labels_decided")


def _clear(diff, e):
    """The sign of ``diff`` is the device's too: |diff| above the error ``e``, or no error at all (exact rows)."""
    return (np.abs(diff) > e) | (e == 0.0)


def finish_ref(Rb, planes, keep_count, m_valid, o_valid, commit, want_packed=True, mut=None):
    """Rb [B, M, Pp] float32, planes [B, K, HW] float32 (the oracle's; only n < keep_count[b] is read), m_valid / o_valid /
    commit: [B] or None -> Finish: full [B, M, HW] float64 with its elementwise bound and the exact rows [B, M]; hist as
    the entry leaves a buffer of ``SENT_F``; packed_flat = the int64 words of a [B, M, words] buffer of ``SENT_W`` WITH its
    two guard bands, flat; bits / labels with their decided masks.  ``mut``: see MUTANTS."""
    Rb = np.asarray(Rb, dtype=np.float32)
    B, M, Pp = Rb.shape
    K, HW = planes.shape[1], planes.shape[2]
    words = pack_words(HW)
    full, bound = np.zeros((B, M, HW)), np.zeros((B, M, HW))
    exact = np.ones((B, M), dtype=bool)                        # rows without a weight are zero: exact
    labels = np.zeros((B, HW), dtype=np.uint8)
    ldec = np.ones((B, HW), dtype=bool)
    for b in range(B):
        Nb = min(max(int(keep_count[b]), 0), K)
        Mb = M if m_valid is None else min(max(int(m_valid[b]), 0), M)
        if Nb == 0:
            Mb = 0
        rows = M if mut == "no_mb" and Nb > 0 else Mb
        cols = np.arange(Nb)
        if mut == "chunk16":                                   # only the first 16 used columns are ever staged
            used = np.nonzero((Rb[b, :Mb, :Nb] != 0).any(axis=0))[0]
            cols = used[:16]
        P64 = planes[b, cols].astype(np.float64)
        for m in range(rows):
            w = Rb[b, m, cols]
            nz = np.nonzero(w != 0)[0]
            k = len(nz)
            if k == 1:
                full[b, m] = (F(w[nz[0]]) * planes[b, cols[nz[0]]].astype(np.float32)).astype(np.float64)
            elif k > 1:
                terms = w[nz].astype(np.float64)[:, None] * P64[nz]
                full[b, m] = terms.sum(axis=0)
                bound[b, m] = float(gamma(k)) * np.abs(terms).sum(axis=0)
            exact[b, m] = k <= 1
        Ob = M if o_valid is None else min(max(int(o_valid[b]), 0), M)
        if Ob > 0:
            v, e = full[b, :Ob], bound[b, :Ob]
            if mut == "last_max":
                arg = Ob - 1 - np.argmax(v[::-1], axis=0)
            else:
                arg = np.argmax(v, axis=0)                     # first maximum
            px = np.arange(HW)
            best, eb = v[arg, px], e[arg, px]
            labels[b] = np.where(best > 0.5, arg + 1, 0).astype(np.uint8)
            others = np.arange(Ob)[:, None] != arg[None, :]
            unamb = (~others | _clear(best[None] - v, eb[None] + e)).all(axis=0)
            all_below = ((v + e < 0.5) | ((e == 0.0) & (v <= 0.5))).all(axis=0)
            ldec[b] = all_below | (unamb & _clear(best - 0.5, eb))
    bits = (full >= 0.5) if mut == "mask_ge" else (full > 0.5)
    bdec = _clear(full - 0.5, bound)
    hist = np.full((B, M, HW), SENT_F, dtype=np.float32)
    written = np.zeros(B, dtype=bool)
    flat = np.full(B * M * words + 2 * GUARD, SENT_W, dtype=np.int64)
    for b in range(B):
        if commit is not None and int(commit[b]) != 0:
            hist[b] = full[b].astype(np.float32)               # (compared through ``full`` and its bound, not through this)
            written[b] = True
            if want_packed:
                flat[GUARD + b * M * words:GUARD + (b + 1) * M * words] = pack_bits(bits[b].astype(np.float32)).reshape(-1)
    if mut == "unbounded_store" and want_packed:
        # every wave of the last workgroup stores its four words, also the waves whose 256 pixels start at or after i_end
        i_end = ((HW + 255) // 256) * 256
        i_last = ((HW - 1) // 1024) * 1024
        for b in range(B):
            if written[b]:
                for m in range(M):
                    for wv in range(4):
                        i0 = i_last + 256 * wv
                        if i0 >= i_end:
                            o = GUARD + (b * M + m) * words + i0 // 64
                            flat[o:o + 4] = 0
    return Finish(full, bound, exact, hist, written, flat, bits, bdec, labels, ldec)


def emulate_finish32(Rb, planes, keep_count, m_valid):
    """The kernel's chain in float32: acc = fma(w, v, acc) over the non-zero weights of the live block in ascending column
    order.  The fma is done in float64 (the product of two float32 is exact there) and rounded once to float32."""
    Rb = np.asarray(Rb, dtype=np.float32)
    B, M, _ = Rb.shape
    K, HW = planes.shape[1], planes.shape[2]
    out = np.zeros((B, M, HW), dtype=np.float32)
    for b in range(B):
        Nb = min(max(int(keep_count[b]), 0), K)
        Mb = M if m_valid is None else min(max(int(m_valid[b]), 0), M)
        for m in range(Mb if Nb else 0):
            acc = np.zeros(HW, dtype=np.float32)
            for n in range(Nb):
                w = Rb[b, m, n]
                if w != 0:
                    acc = (np.float64(w) * planes[b, n].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
            out[b, m] = acc
    return out


def compare_finish(ref, full, hist, packed_flat, labels, has_packed=True, has_labels=True):
    """The one comparison of a dmm_step_finish_f32 result (device arrays, or a mutant's) with ``finish_ref`` -> (failures,
    achieved): full / hist inside the bound on EVERY element (exact rows: equal), the uncommitted videos' hist and words and
    the guard bands untouched, bits and labels equal where decided."""
    fails = []
    err = np.abs(np.asarray(full, dtype=np.float64) - ref.full)
    bad = ~(err <= ref.bound)
    if bad.any():
        fails.append(f"full: {int(bad.sum())} of {bad.size} elements over their bound (|err| up to {float(np.nanmax(err)):.3g})")
    pos = ref.bound > 0
    ratio = float((err[pos] / ref.bound[pos]).max()) if pos.any() else 0.0
    B, M, HW = ref.full.shape
    for b in range(B):
        if ref.hist_written[b]:
            if not np.array_equal(np.asarray(hist[b]), np.asarray(full[b])):
                fails.append(f"hist[{b}] differs from full[{b}] in a committed video")
        elif not np.array_equal(np.asarray(hist[b]), ref.hist[b]):
            fails.append(f"hist[{b}] of an uncommitted video was written")
    if has_packed:
        got = np.asarray(packed_flat).reshape(-1)
        words = pack_words(HW)
        exp_bits = unpack_bits(ref.packed_flat[GUARD:-GUARD].reshape(B, M, words), HW)
        got_bits = unpack_bits(got[GUARD:-GUARD].reshape(B, M, words), HW)
        for b in range(B):
            sl = slice(GUARD + b * M * words, GUARD + (b + 1) * M * words)
            if ref.hist_written[b]:
                wrong = (exp_bits[b] != got_bits[b]) & ref.bits_decided[b]
                if wrong.any():
                    fails.append(f"packed_hist[{b}]: {int(wrong.sum())} decided bits differ")
                pad = got[sl].reshape(M, words).copy()
                pad ^= pack_bits(got_bits[b].astype(np.float32))
                if pad.any():
                    fails.append(f"packed_hist[{b}]: pad bits set")
            elif not np.array_equal(got[sl], ref.packed_flat[sl]):
                fails.append(f"packed_hist[{b}] of an uncommitted video was written "
                             f"({int((got[sl] != ref.packed_flat[sl]).sum())} words)")
        if not np.array_equal(got[:GUARD], ref.packed_flat[:GUARD]) or not np.array_equal(got[-GUARD:], ref.packed_flat[-GUARD:]):
            fails.append("packed_hist: a guard band was written")
    if has_labels:
        wrong = (np.asarray(labels) != ref.labels) & ref.labels_decided
        if wrong.any():
            fails.append(f"labels: {int(wrong.sum())} decided pixels differ")
    return fails, ratio


def undecided_share(ref):
    """-> (share of bits, share of labels) the reference leaves undecided."""
    return 1.0 - float(ref.bits_decided.mean()), 1.0 - float(ref.labels_decided.mean())


# ---- cases of dmm_step_finish_f32 -------------------------------------------------------------------------------------------
# weights: "onehot" (test mode: exact), "dense" with U = the used columns per video.  None for m_valid / o_valid / commit = NULL.
FCase = collections.namedtuple("FCase", "name H W B M K R Mm pad T step weights U m_valid o_valid commit packed labels count")


def _fc(name, H, W, B, M, K, weights, U=None, R=None, Mm=28, pad=1, T=1, step=None, m_valid="full", o_valid="full",
        commit="mixed", packed=True, labels=True, count=None):
    R = R or K
    mv = None if m_valid is None else ([M] * B if m_valid == "full" else list(m_valid))
    ov = None if o_valid is None else ([M] * B if o_valid == "full" else list(o_valid))
    cm = None if commit is None else ([1, 0, 1][:B] if commit == "mixed" else list(commit))
    return FCase(name, H, W, B, M, K, R, Mm, pad, T, step, weights, U, mv, ov, cm, packed, labels, count)


FINISH_CASES = [
    # the sizes that put out-of-range waves into the last workgroup (33 x 40: two, 57 x 83: one, 25 x 41: three), test mode
    _fc("onehot_33x40", 33, 40, 3, 5, 12, "onehot", m_valid=(5, 3, 5), o_valid=(5, 2, 0)),
    _fc("onehot_57x83", 57, 83, 2, 8, 50, "onehot", T=3, step=2, commit=(1, 0)),
    _fc("onehot_25x41", 25, 41, 3, 1, 1, "onehot", commit=(1, 0, 0), o_valid=None),           # Pp = 2 > K
    _fc("onehot_k5_m8", 7, 37, 2, 8, 5, "onehot", m_valid=None, commit=(0, 1)),               # Pp = 9 > K
    # dense rows: the chunk of 16 used columns from both sides, zero weights interleaved
    _fc("dense_u0_1_15", 33, 40, 3, 5, 40, "dense", U=(0, 1, 15), m_valid=(5, 4, 3), o_valid=(5, 4, 2)),
    _fc("dense_u16_17_33", 33, 40, 3, 8, 50, "dense", U=(16, 17, 33), m_valid=(8, 6, 8), o_valid=None, commit=(0, 1, 0)),
    _fc("dense_u33_57x83", 57, 83, 2, 5, 50, "dense", U=(33, 17), T=3, step=1, commit=(1, 0), R=60),
    _fc("dense_67x129", 67, 129, 1, 8, 20, "dense", U=(17,), commit=(1,)),
    # NULL arguments, an empty video
    _fc("no_commit", 33, 40, 2, 5, 20, "dense", U=(5, 17), commit=None),
    _fc("no_packed", 33, 40, 2, 5, 20, "dense", U=(5, 17), packed=False, commit=(1, 0)),
    _fc("no_labels", 33, 40, 2, 5, 12, "onehot", labels=False, commit=(0, 1)),
    _fc("empty_video", 33, 40, 3, 5, 20, "dense", U=(6, 0, 17), count=(20, 0, 19), commit=(1, 1, 0), R=24),
    # small planes
    _fc("tiny_1x1", 1, 1, 2, 5, 6, "dense", U=(3, 2), commit=(1, 0)),
    _fc("tiny_3x5", 3, 5, 2, 5, 6, "onehot", commit=(0, 1)),
    _fc("col_300x1", 300, 1, 2, 5, 8, "dense", U=(4, 8), commit=(1, 0)),
    _fc("narrow_100x3", 100, 3, 2, 5, 8, "onehot", commit=(1, 0)),
    _fc("block_16x16", 16, 16, 2, 8, 8, "dense", U=(8, 3), commit=(1, 0)),
    _fc("under_9x28", 9, 28, 2, 1, 8, "dense", U=(8, 3), commit=(1, 0)),
    _fc("band_65x63", 65, 63, 1, 5, 18, "dense", U=(17,), commit=(1,)),
    _fc("band_64x64", 64, 64, 2, 5, 8, "onehot", commit=(1, 0)),
    # mask sizes: Mp = 1 and the largest legal 32
    _fc("mp1", 33, 40, 2, 5, 20, "dense", U=(5, 17), Mm=1, pad=0, commit=(1, 0)),
    _fc("mp32", 33, 40, 2, 5, 20, "dense", U=(5, 17), Mm=30, pad=1, commit=(1, 0)),
]
FINISH_BY_NAME = {c.name: c for c in FINISH_CASES}


@functools.lru_cache(maxsize=None)
def finish_inputs(name):
    """Seeded host inputs of one case, never modified: the clip-resident raw proposals, a fabricated keep table (any raw
    indices in any order are legal input of the entry), keep_count, Rb, and the oracle's planes of the kept proposals."""
    c = FINISH_BY_NAME[name]
    seed = sum(map(ord, name)) * 7919 + c.K
    gen = np.random.default_rng(seed)
    prob, boxes, scores = raw_proposals(c.H, c.W, c.T, c.B, c.R, c.Mm, seed + 1)
    t = c.step or 0
    keep = np.stack([gen.permutation(c.R)[:c.K] for _ in range(c.B)]).astype(np.int32)
    count = np.asarray(c.count if c.count is not None else [c.K] * c.B, dtype=np.int32)
    Pp = c.K if c.K > c.M else c.M + 1                           # ops.padded_width
    Rb = np.zeros((c.B, c.M, Pp), dtype=np.float32)
    HW = c.H * c.W
    planes = np.zeros((c.B, c.K, HW), dtype=np.float32)
    for b in range(c.B):
        pl, _ = oracle.paste_masks(prob[t, b, keep[b]], boxes[t, b, keep[b]], c.H, c.W, 0.4, c.pad)
        planes[b] = pl.reshape(c.K, HW)
    ones = [[k for k in range(c.K) if keep[b, k] % 14 == ALL_ONE] for b in range(c.B)]
    for b in range(c.B):
        Nb = int(count[b])
        Mb = c.M if c.m_valid is None else c.m_valid[b]
        if c.weights == "onehot":
            # rows 0 and 1 share their column and weight (a tie: the first wins), row 2 at most 0.5 (background), row 3
            # negative, the others 1.0; one row of video 0 puts 0.5 on an all-one proposal: values exactly 0.5
            col = gen.integers(0, max(Nb, 1), c.M)
            wt = np.ones(c.M, dtype=np.float32)
            if c.M > 1:
                col[1] = col[0]
            if c.M > 2:
                wt[2] = F(0.45)
            if c.M > 3:
                wt[3] = F(-0.75)
            if c.M > 4 and ones[b] and ones[b][0] < Nb:
                col[4], wt[4] = ones[b][0], F(0.5)
            for m in range(c.M):
                if Nb:
                    Rb[b, m, col[m]] = wt[m]
        else:
            U_b = c.U[b]
            used = np.sort(gen.permutation(Nb)[:U_b]) if Nb else np.zeros(0, dtype=np.int64)
            assert len(used) == U_b or Nb == 0
            for u, n in enumerate(used):
                rows = [m for m in range(Mb) if gen.uniform() < 0.6] or [int(gen.integers(0, Mb))]
                rows[0] = rows[0] if u else 0                   # (row 0 sees the first used column)
                for m in rows:
                    Rb[b, m, n] = F(gen.uniform(0.2, 1.0) * (-1.0 if gen.uniform() < 0.25 else 1.0))
            if U_b:                                             # the LAST used column reaches row 0: dropping it shows
                Rb[b, 0, used[-1]] = F(0.8)
            free = [n for n in range(Nb) if n not in set(used.tolist())]
            if free and Mb < c.M:                               # a column whose only weight sits in a row >= m_valid[b]
                Rb[b, c.M - 1, free[0]] = F(0.9)
            if Mb < c.M and U_b:                                # and a used column that also carries one there
                Rb[b, c.M - 1, used[0]] = F(0.7)
        Rb[b, :, Nb:] = F(0.6)                                  # outside the live block: never read
    for a in (prob, boxes, scores, keep, count, Rb, planes):
        a.setflags(write=False)
    return dict(prob=prob, boxes=boxes, scores=scores, keep=keep, count=count, Rb=Rb, planes=planes, Pp=Pp)


@functools.lru_cache(maxsize=None)
def finish_expected(name, mut=None):
    c, d = FINISH_BY_NAME[name], finish_inputs(name)
    return finish_ref(d["Rb"], d["planes"], d["count"], c.m_valid, c.o_valid, c.commit, want_packed=c.packed, mut=mut)


# ---- cases of the three preparation entries -----------------------------------------------------------------------------------
SIZES = [(1, 1), (3, 5), (300, 1), (100, 3), (9, 28), (16, 16), (7, 37), (25, 41), (33, 40), (65, 63), (64, 64), (57, 83),
         (67, 129)]
PCase = collections.namedtuple("PCase", "name H W images R K Mm pad T step counts base stride_extra")


def _prep_cases():
    out = []
    for j, (H, W) in enumerate(SIZES):
        clip = j % 2 == 1                                       # every other size: clip resident (T = 3), step 2, img_base
        out.append(PCase(f"{H}x{W}", H, W, 3, 17, 6, 28, 1, 3 if clip else 1, 2 if clip else None,
                         (17, 0, 4) if j % 3 else (15, 3, 0), 7 if clip else None, (0, 5, 256)[j % 3]))
    out.append(PCase("mp1_33x40", 33, 40, 2, 14, 6, 1, 0, 1, None, (14, 5), None, 0))
    out.append(PCase("mp32_33x40", 33, 40, 2, 14, 6, 30, 1, 1, None, None, None, 3))            # counts == NULL
    out.append(PCase("mp64_33x40", 33, 40, 2, 14, 20, 62, 1, 3, 0, (14, 9), 3, 0))
    return out


PREP_CASES = _prep_cases()
PREP_BY_NAME = {c.name: c for c in PREP_CASES}
NMS_T, MASK_T = 0.5, 0.4


@functools.lru_cache(maxsize=None)
def prep_inputs(name):
    c = PREP_BY_NAME[name]
    prob, boxes, scores = raw_proposals(c.H, c.W, c.T, c.images, c.R, c.Mm, sum(map(ord, name)) * 104729 + c.R)
    counts = None
    if c.counts is not None:
        counts = np.zeros((c.T, c.images), dtype=np.int32) + 1
        counts[c.step or 0] = c.counts
    for a in (prob, boxes, scores):
        a.setflags(write=False)
    return dict(prob=prob, boxes=boxes, scores=scores, counts=counts)


@functools.lru_cache(maxsize=None)
def prep_expected(name, mut=None):
    c, d = PREP_BY_NAME[name], prep_inputs(name)
    t = c.step or 0
    base = 0 if c.base is None else c.base + t                  # img_base[t] = base + t in the tests
    return prepare_expected(d["prob"][t], d["boxes"][t], d["scores"][t], None if d["counts"] is None else d["counts"][t],
                            c.H, c.W, MASK_T, c.pad, NMS_T, c.K, base=base, mut=mut)


def compare_prep(exp, got):
    """Field by field, bit for bit (sentinels included) -> failures."""
    return [f"{f}: {int((np.asarray(getattr(got, f)) != getattr(exp, f)).sum())} elements differ"
            for f in Prep._fields if getattr(got, f) is not None and not np.array_equal(np.asarray(getattr(got, f)), getattr(exp, f))]


# ---- mutants: Python variants of the reference, each one plausible kernel error ------------------------------------------------
# name: (what, the family it applies to)
MUTANTS = {
    "unbounded_store": ("packed-history store not bounded by i_end", "finish"),
    "chunk16": ("the 17th used column dropped", "finish"),
    "no_mb": ("rows >= Mb not zeroed", "finish"),
    "last_max": ("last maximum wins instead of first", "finish"),
    "mask_ge": (">= in place of > at the mask threshold", "finish+prep"),
    "nms_ge": (">= in place of > at the NMS threshold", "nms"),
    "cols48": ("suppression columns 48..63 dropped", "nms"),
    "dead_cleared": ("a dead slot's plane cleared", "prep"),
    "no_clamp": ("counts not clamped to R", "nms"),
}
NMS_SIZES = (0, 1, 2, 16, 17, 32, 33, 47, 48, 49, 63, 64)


@functools.lru_cache(maxsize=None)
def nms_inputs(n, R=64, images=2):
    """tight [images, R, 4], scores [images, R], counts [images] = n: the first n rows of image i are ``nms_boxes(n, i)``; the
    rows past n hold boxes with HIGHER scores than any live one (a kernel that reads them shows)."""
    gen = np.random.default_rng(77 + n + R)
    tight = gen.integers(0, 40, (images, R, 4)).astype(np.float32)
    tight[..., 2:] += tight[..., :2] + 5
    scores = gen.uniform(2.0, 3.0, (images, R)).astype(np.float32)
    for i in range(images):
        tight[i, :n], scores[i, :n] = nms_boxes(n, i)
    counts = np.full(images, n, dtype=np.int32)
    for a in (tight, scores, counts):
        a.setflags(write=False)
    return tight, scores, counts


def nms_ks(n):
    return sorted({k for k in (1, n - 1, n, n + 5) if k > 0})
