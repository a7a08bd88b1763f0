"""Cases for the device-side proposal selection (step_select_train, step_amd.ops.select_train, step_amd.selection.DeviceSelector), driven
on the host interpreter by tests/test_emul_select.py and on the real library by tests/test_gpu_select.py.

The reference of every kernel comparison is `restate` below: the rule of include/step_amd.h ("The rule, per clip") written again in
numpy / plain Python from the header's text, drawing from tests/dropout_cases.philox_words.  sel, tgt, mask, inv and counts are
compared for EQUALITY: the rule is comparisons, fp32 IoU arithmetic in a fixed order and double sums in a fixed order.  The one place
where the device and libm may differ in the last bit is exp() of the softmax weights; `restate` reports how close any draw came to a
running sum (relative to the total), and the softmax cases first assert that no draw landed within 1e-9 of one.

Kernel cases take a backend of tests/backends.py; module cases take a device string ("cpu" under the interpreter patch, "cuda")."""
import math
from types import SimpleNamespace as NS

import numpy as np
import torch

from tests.dropout_cases import philox_words

f32 = np.float32
u64 = np.uint64
SAMPLING = {"uniform": 0, "random": 1, "softmax": 2}
E_SHAPE, E_NULL, E_UNSUPPORTED = -2, -3, -4


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def draw(seed, offset, b, phase, k):
    """u in [0, 1): 53 bits from words 0 and 1 of block (b << 20) | (phase << 16) | k at (seed, offset)"""
    w = philox_words(seed, offset, (b << 20) | (phase << 16) | k, 1)[0]
    return float((int(w[0]) << 21) | (int(w[1]) >> 11)) * 2.0 ** -53


def floor_draw(u, n):
    return min(int(math.floor(u * n)), n - 1)


def box_iou_f32(q, a):
    """fp32, the operation order of select_prepare_kernel: 0 for an all-zero box, no +1 convention"""
    q, a = [f32(v) for v in q], [f32(v) for v in a]
    if (((q[0] + q[1]) + q[2]) + q[3]) == 0 or (((a[0] + a[1]) + a[2]) + a[3]) == 0:
        return f32(0)
    iw = max(min(q[2], a[2]) - max(q[0], a[0]), f32(0))
    ih = max(min(q[3], a[3]) - max(q[1], a[1]), f32(0))
    inter = iw * ih if (iw > 0 and ih > 0) else f32(0)
    uni = (q[2] - q[0]) * (q[3] - q[1]) + (a[2] - a[0]) * (a[3] - a[1]) - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        return f32(inter / uni)


def restate(inp, prm, seed, offset):
    """-> (sel, tgt, mask, inv, counts, margin): the outputs of step_select_train and the smallest |running sum - t| / total any
    negative draw saw (inf when nothing was drawn)."""
    cand, first, last, score, iou = inp["cand"], inp.get("first"), inp.get("last"), inp.get("score"), inp.get("iou")
    clip_start, gt, gt_count, pad = inp["clip_start"], inp["gt"], inp["gt_count"], inp["pad"]
    B = len(clip_start) - 1
    Tc = cand.shape[1]
    Tw = first.shape[1] if first is not None else 0
    Tout = Tc + 2 * Tw
    NC = gt.shape[3] - 4
    budget, mid, before, after = prm["budget"], prm["mid"], prm["before"], prm["after"]
    topk, max_pos, neg_ratio, sampling = prm["topk"], prm["max_pos_num"], prm["neg_ratio"], prm["sampling"]
    cls_thresh, reg_thresh = f32(prm["cls_thresh"]), f32(prm["reg_thresh"])
    sel = np.zeros((B * budget, Tout, 5), f32)
    tgt = np.zeros((B * budget, 3, 6 + NC), f32)
    mask = np.zeros((B * budget, 1), f32)
    counts = np.zeros((B, 2), np.int32)
    margin = float("inf")
    for b in range(B):
        lo = int(clip_start[b])
        A = min(int(clip_start[b + 1]) - lo, prm.get("amax", 1024))
        G = int(gt_count[b])
        pos, neg = [], []                                       # (ground truth, candidate position)
        if A > 0 and G > 0:
            # candidates, in order
            if score is None:
                order = list(range(A))
            else:
                s = score[lo:lo + A]
                keep = 2 * (topk // NC) if topk > 0 else A
                best = {}
                for a in range(A):
                    for c in range(NC):
                        ahead = sum(1 for o in range(A) if s[o, c] > s[a, c] or (s[o, c] == s[a, c] and o < a))
                        if ahead < keep:
                            best[a] = max(best.get(a, s[a, c]), s[a, c])
                order = sorted(best, key=lambda a: (-float(best[a]), a))
                if topk > 0:
                    order = order[:topk]
            n = len(order)
            if iou is None:
                tab = np.array([[box_iou_f32(gt[b, g, mid, :4], cand[lo + a, Tc // 2]) for a in order] for g in range(G)], f32).reshape(G, n)
            else:
                tab = np.array([[iou[lo + a, g] for a in order] for g in range(G)], f32).reshape(G, n)
            cscore = tab.max(axis=0) if score is None else np.array([best[a] for a in order], f32)
            owner = [int(np.argmax(tab[:, k])) for k in range(n)]       # first arg-max
            # first positives
            taken = [False] * n
            rowmax = [float(tab[g].max()) for g in range(G)]
            for _ in range(G):
                g = max(range(G), key=lambda h: (rowmax[h], -h))
                free = [k for k in range(n) if not taken[k]]
                if not free:
                    continue
                k = max(free, key=lambda k_: (float(tab[g, k_]), k_))    # equal values: the higher position
                taken[k] = True
                pos.append((g, k))
                rowmax[g] = -1.0
            if len(pos) > max_pos:
                for i in range(len(pos) - 1, 0, -1):
                    j = floor_draw(draw(seed, offset, b, 0, i), i + 1)
                    pos[i], pos[j] = pos[j], pos[i]
                pos = pos[:max_pos]
            # more positives
            above = [k for k in range(n) if not taken[k] and bool((tab[:, k] > cls_thresh).any())]
            if above and len(pos) < max_pos:
                remaining = list(above)
                for d in range(min(len(above), max_pos - len(pos))):
                    k = remaining.pop(floor_draw(draw(seed, offset, b, 1, d), len(remaining)))
                    pos.append((owner[k], k))
            for k in above:
                taken[k] = True
            # negatives
            rest = [k for k in range(n) if not taken[k]]
            if sampling == 0:
                wgt = {k: float(cscore[k]) + 1e-6 for k in rest}
            elif sampling == 1:
                wgt = {k: 1.0 for k in rest}
            else:
                wgt = {k: math.exp(float(cscore[k])) for k in rest}
            for d in range(min(len(pos) * neg_ratio, len(rest))):
                total = 0.0
                for k in rest:
                    total += wgt[k]
                t = draw(seed, offset, b, 2, d) * total
                run, pick = 0.0, rest[-1]
                for k in rest:
                    run += wgt[k]
                    margin = min(margin, abs(run - t) / total)
                    if run > t:
                        pick = k
                        break
                rest.remove(pick)
                neg.append((owner[pick], pick))
        # the clip's rows
        rows = pos + neg
        assert len(rows) <= budget
        counts[b] = (len(pos), len(neg))
        for r in range(budget):
            o = b * budget + r
            sel[o, :, 0] = b * Tout + np.arange(Tout)
            if r >= len(rows):
                sel[o, :, 1:] = pad[b]
                continue
            g, k = rows[r]
            tube = lo + order[k]
            sel[o, :, 1:] = cand[tube] if first is None else np.concatenate((first[tube], cand[tube], last[tube]))
            mask[o] = 1
            positive = r < len(pos)
            if positive or tab[g, k] >= reg_thresh:
                tgt[o, 1, :4] = gt[b, g, mid, :4]
                tgt[o, 1, 6:] = gt[b, g, mid, 4:]
                tgt[o, 1, 5] = 1
                tgt[o, 1, 4] = 1 if positive else 0
            if positive and before >= 0:
                for row, frame in ((0, before), (2, after)):
                    q = gt[b, g, frame]
                    tgt[o, row, :4] = q[:4]
                    tgt[o, row, 5] = 1 if (((q[0] + q[1]) + q[2]) + q[3]) > 0 else 0
                    tgt[o, row, 6:] = q[4:]
    inv = np.array([1.0 / (max(int(counts.sum()), 1) * NC)], f32)
    return sel, tgt, mask, inv, counts, margin


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def rand_boxes(rs, n, lo=0.0, hi=400.0):
    xy = rs.uniform(lo, hi - 120, (n, 2))
    return np.concatenate([xy, xy + rs.uniform(60, 110, (n, 2))], 1).astype(f32)


def make_inputs(rs, tubes, gts, NC=4, Tc=3, Tw=0, F=3, score=False, near=0.6, Gmax=None):
    """tubes / gts: per clip.  Ground-truth boxes jitter from frame to frame; a share `near` of the tubes sits close to a ground truth
    (so that IoUs above the thresholds exist), the others anywhere.  score: uniform class scores [N,NC]."""
    B, N = len(tubes), int(sum(tubes))
    Gmax = Gmax or max(max(gts), 1)
    gt = np.zeros((B, Gmax, F, 4 + NC), f32)
    for b in range(B):
        base = rand_boxes(rs, gts[b])
        for g in range(gts[b]):
            for fr in range(F):
                gt[b, g, fr, :4] = base[g] + rs.uniform(-4, 4, 4).astype(f32)
            gt[b, g, :, 4:] = (rs.rand(NC) < 0.4).astype(f32)
    cand = np.zeros((N, Tc, 4), f32)
    n = 0
    for b in range(B):
        for _ in range(tubes[b]):
            if gts[b] and rs.rand() < near:
                box = gt[b, rs.randint(gts[b]), F // 2, :4] + rs.uniform(-15, 15, 4).astype(f32)
            else:
                box = rand_boxes(rs, 1)[0]
            for t in range(Tc):
                cand[n, t] = box + rs.uniform(-3, 3, 4).astype(f32)
            n += 1
    inp = {"cand": cand, "clip_start": np.concatenate(([0], np.cumsum(tubes))).astype(np.int32), "gt": gt,
           "gt_count": np.asarray(gts, np.int32), "pad": np.tile(rand_boxes(rs, B)[:, None, :], (1, Tc + 2 * Tw, 1)).astype(f32)}
    if Tw:
        inp["first"] = (cand[:, :1] + rs.uniform(-6, 6, (N, Tw, 4))).astype(f32)
        inp["last"] = (cand[:, -1:] + rs.uniform(-6, 6, (N, Tw, 4))).astype(f32)
    if score:
        inp["score"] = rs.rand(N, NC).astype(f32)
    return inp


def params(**kw):
    prm = dict(mid=1, before=-1, after=-1, topk=-1, cls_thresh=0.5, reg_thresh=0.5, max_pos_num=5, neg_ratio=2, sampling=2, budget=15, amax=1024)
    prm.update(kw)
    return prm


def _state(bk, seed, offset):
    return bk.dev(np.array([seed, offset], u64).view(np.int64))


def _read_state(st):
    s = st.get().view(u64)
    return int(s[0]), int(s[1])


def call(bk, inp, prm, st, expect_status=0, **override):
    """one step_select_train call -> (sel, tgt, mask, inv, counts) as numpy, or the status when expect_status != 0"""
    g = lambda k: inp.get(k)
    B = len(inp["clip_start"]) - 1
    N, Tc = inp["cand"].shape[:2]
    Tw = g("first").shape[1] if g("first") is not None else 0
    Tout = Tc + 2 * Tw
    Gmax, F, NC = inp["gt"].shape[1], inp["gt"].shape[2], inp["gt"].shape[3] - 4
    K = max(B * prm["budget"], 1)
    bufs = {k: bk.dev(np.ascontiguousarray(g(k))) if g(k) is not None else bk.dev(None) for k in
            ("cand", "first", "last", "score", "iou", "clip_start", "gt", "gt_count", "pad")}
    out = [bk.dev(np.full((K, Tout, 5), 7, f32)), bk.dev(np.full((K, 3, 6 + NC), 7, f32)), bk.dev(np.full((K, 1), 7, f32)),
           bk.dev(np.full((1,), 7, f32)), bk.dev(np.full((max(B, 1), 2), 7, np.int32))]
    a = dict(N=N, Tc=Tc, Tw=Tw, NC=NC, B=B, Gmax=Gmax, F=F, rng=st.ptr, **prm)
    a.update(override)
    rc = bk.lib.step_select_train(bufs["cand"].ptr, bufs["first"].ptr, bufs["last"].ptr, bufs["score"].ptr, bufs["iou"].ptr, a["N"], a["Tc"], a["Tw"],
                                  a["NC"], bufs["clip_start"].ptr, a["B"], a["amax"], bufs["gt"].ptr, bufs["gt_count"].ptr, a["Gmax"], a["F"],
                                  bufs["pad"].ptr, a["rng"], a["mid"], a["before"], a["after"], a["topk"], a["cls_thresh"], a["reg_thresh"],
                                  a["max_pos_num"], a["neg_ratio"], a["sampling"], a["budget"], out[0].ptr, out[1].ptr, out[2].ptr, out[3].ptr,
                                  out[4].ptr, bk.stream)
    assert rc == expect_status, (rc, expect_status)
    got = [o.get().copy() for o in out]
    if expect_status != 0:
        assert all(np.all(o == 7) for o in got), "a refused call wrote something"
        return rc
    return got[0][:B * prm["budget"]], got[1][:B * prm["budget"]], got[2][:B * prm["budget"]], got[3], got[4][:B]


NAMES = ("sel", "tgt", "mask", "inv", "counts")


def check(bk, inp, prm, seed=0x1_0000_0007, offset=0x2_0000_0003, softmax_margin=True):
    """kernel == restatement on (inp, prm) at (seed, offset); the offset ends one further.  -> the restatement's outputs"""
    want = restate(inp, prm, seed, offset)
    if prm["sampling"] == 2 and softmax_margin:
        assert want[5] > 1e-9, ("a softmax draw within 1e-9 of a running sum: pick another seed", want[5])
    st = _state(bk, seed, offset)
    got = call(bk, inp, prm, st)
    for nm, a, b in zip(NAMES, got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, (nm, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(a, b), (nm, np.argwhere(a != b)[:5], got[4], want[4])
    assert _read_state(st) == (seed, offset + 1)
    return want


# ---- kernel cases --------------------------------------------------------------------------------------------------------------
def case_select_small_clips(bk, golden):
    """Step 1 (score and iou NULL): three clips with different tube counts in one call -- A = 1 with G = 1; A = 2 < G = 4 (the later
    rounds find every candidate taken); G = 0 (nothing selected, every slot padded) -- and a call whose middle clip has no tubes."""
    rs = np.random.RandomState(1)
    inp = make_inputs(rs, [1, 2, 5], [1, 4, 0], near=1.0)
    _, _, mask, _, counts, _ = check(bk, inp, params(cls_thresh=0.2, reg_thresh=0.2))
    assert counts[0].sum() == 1 and counts[1, 0] == 2 and counts[1, 1] == 0 and counts[2].sum() == 0 and mask[30:].sum() == 0
    inp = make_inputs(rs, [3, 0, 4], [2, 2, 1], near=1.0)
    counts = check(bk, inp, params(cls_thresh=0.2, reg_thresh=0.2))[4]
    assert counts[1].sum() == 0 and counts[0, 0] >= 2


def case_select_shuffle(bk, golden):
    """G = 7 ground truths and max_pos_num = 5: seven greedy picks, the shuffle (phase 0), the first five; the two dropped stay taken."""
    rs = np.random.RandomState(2)
    inp = make_inputs(rs, [12, 9], [7, 7], near=0.9)
    for off in (0, 1, 5):
        counts = check(bk, inp, params(cls_thresh=0.9, reg_thresh=0.3), seed=77, offset=off)[4]
        assert np.all(counts[:, 0] == 5)


def case_select_no_overlap_tie(bk, golden):
    """A ground truth that overlaps nothing (a table row of zeros): its pick is the HIGHEST untaken position; equal IoUs elsewhere too."""
    rs = np.random.RandomState(3)
    inp = make_inputs(rs, [6], [3], near=0.0)
    iou = np.zeros((6, 3), f32)
    iou[:, 0] = [0.1, 0.7, 0.7, 0.2, 0.0, 0.0]                   # equal maxima: position 2 wins over 1
    iou[:, 2] = [0.3, 0.3, 0.1, 0.3, 0.0, 0.0]                   # row 1 stays all-zero
    inp["iou"] = iou
    sel, _, _, _, counts, _ = check(bk, inp, params(cls_thresh=0.9, reg_thresh=0.9, neg_ratio=0, budget=5, sampling=1))
    assert counts[0, 0] == 3
    picked = [int(np.flatnonzero((inp["cand"][:, 0] == sel[r, 0, 1:]).all(1))[0]) for r in range(3)]
    assert picked == [2, 3, 5], picked                            # row 0 -> 2 (tie, higher); row 2 -> 3 (tie among 0, 1, 3); row 1 (zeros) -> 5


def case_select_above_and_rest(bk, golden):
    """`above` larger than the free slots (one ground truth, ten tubes on top of it, max_pos_num = 5: four uniform draws out of nine,
    the other five never negatives) and `rest` smaller than the wanted negatives (3 left for 10 wanted), in the three samplings."""
    rs = np.random.RandomState(4)
    inp = make_inputs(rs, [13, 13], [1, 1], near=0.0)
    for b in range(2):
        for a in range(10):
            inp["cand"][13 * b + a] = inp["gt"][b, 0, 1, :4] + rs.uniform(-4, 4, (3, 4)).astype(f32)
    for sampling in (0, 1, 2):
        counts = check(bk, inp, params(cls_thresh=0.35, reg_thresh=0.35, sampling=sampling), seed=5 + sampling, offset=9)[4]
        assert np.all(counts == [[5, 3], [5, 3]]), counts


def case_select_samplings_and_reg_thresh(bk, golden):
    """Scores handed in (a later step), many negatives to draw from, the three samplings; IoUs handed in so that the negatives fall on
    either side of reg_thresh (regression flag, box and labels only at or above it)."""
    rs = np.random.RandomState(5)
    inp = make_inputs(rs, [20, 17, 23], [2, 1, 3], score=True)
    N = 60
    iou = rs.uniform(0.0, 0.3, (N, 3)).astype(f32)
    iou[rs.rand(N) < 0.15, 0] = 0.8                               # a few above cls_thresh
    iou[5, 0] = iou[5, 1] = f32(0.2)                              # exactly at reg_thresh, and an owner tie (first arg-max)
    inp["iou"] = iou
    for sampling in (0, 1, 2):
        _, tgt, mask, _, counts, _ = check(bk, inp, params(cls_thresh=0.5, reg_thresh=0.2, sampling=sampling), seed=31, offset=sampling)
        neg = (mask[:, 0] == 1) & (tgt[:, 1, 4] == 0)
        assert counts[:, 1].sum() == neg.sum() > 6
        assert (tgt[neg, 1, 5] == 1).any() and (tgt[neg, 1, 5] == 0).any(), "negatives on both sides of reg_thresh"
        assert not tgt[neg & (tgt[:, 1, 5] == 0)].any()


def case_select_topk_and_ties(bk, golden):
    """topk = 8 with NC = 4 (the best 4 per class, merged, at most 8 candidates); topk = -1 with NC = 60; scores quantised to five values,
    so that equal scores across tubes decide both the per-class ranks and the merged order (lower index first)."""
    rs = np.random.RandomState(6)
    inp = make_inputs(rs, [14, 3, 11], [2, 2, 1], score=True, near=0.8)
    check(bk, inp, params(topk=8, cls_thresh=0.3, reg_thresh=0.2), seed=8)
    inp["score"] = (np.floor(inp["score"] * 5) / 5).astype(f32)
    check(bk, inp, params(topk=8, cls_thresh=0.3, reg_thresh=0.2), seed=9)
    check(bk, inp, params(topk=-1, cls_thresh=0.3, reg_thresh=0.2), seed=10)
    inp = make_inputs(rs, [9, 6], [2, 1], NC=60, score=True, near=0.8)
    check(bk, inp, params(topk=-1, cls_thresh=0.3, reg_thresh=0.2, sampling=0), seed=11)
    check(bk, inp, params(topk=120, cls_thresh=0.3, reg_thresh=0.2, sampling=0), seed=12)


def case_select_neighbours_and_growing(bk, golden):
    """Neighbour targets (before = 0, after = 2) with one ground truth whose `before` box is all zeros (padding: no regression flag) and
    growing tubes (Tout = 9: first | cand | last), with and without scores."""
    rs = np.random.RandomState(7)
    inp = make_inputs(rs, [8, 5], [2, 2], Tw=3, score=True, near=0.8)
    inp["gt"][0, 1, 0, :4] = 0
    sel, tgt, mask, _, counts, _ = check(bk, inp, params(before=0, after=2, cls_thresh=0.3, reg_thresh=0.2), seed=13)
    assert sel.shape[1] == 9
    pos = tgt[:, 1, 4] == 1
    assert (tgt[pos, 0, 5] == 0).any() and (tgt[pos, 0, 5] == 1).any() and np.all(tgt[pos, 2, 5] == 1)
    assert not tgt[~pos][:, (0, 2)].any()
    del inp["score"]
    check(bk, inp, params(before=0, after=2, cls_thresh=0.3, reg_thresh=0.2), seed=14)
    del inp["first"], inp["last"]
    inp["pad"] = inp["pad"][:, :3].copy()
    check(bk, inp, params(before=0, after=2, cls_thresh=0.3, reg_thresh=0.2), seed=14)


def case_select_iou_null_against_prepare(bk, golden):
    """iou == NULL (the kernel's own table) against the table step_select_prepare computes for the same boxes (inside the frame, so its
    clamp changes nothing): the two calls select the same rows."""
    rs = np.random.RandomState(8)
    tubes, gts = [9, 1, 14], [2, 1, 3]
    inp = make_inputs(rs, tubes, gts, near=0.7)
    inp["cand"] = np.clip(inp["cand"], 1, 399).astype(f32)
    N, B = 24, 3
    prob = bk.dev(np.zeros((N, 3, 4), f32))
    outs = [bk.dev(np.zeros(s, f32)) for s in ((N, 4), (N, 3, 4), (N, 3))]
    clip_of = bk.dev(np.repeat(np.arange(B), tubes).astype(np.int32))
    loc, gt_mid, gt_count = bk.dev(inp["cand"]), bk.dev(np.ascontiguousarray(inp["gt"][:, :, 1, :4])), bk.dev(inp["gt_count"])
    rc = bk.lib.step_select_prepare(prob.ptr, loc.ptr, None, None, N, 3, 0, 4, clip_of.ptr, gt_mid.ptr, gt_count.ptr, 3, 400.0, 400.0,
                                    outs[0].ptr, outs[1].ptr, None, None, outs[2].ptr, bk.stream)
    assert rc == 0
    assert np.array_equal(outs[1].get(), inp["cand"])
    prm = params(cls_thresh=0.3, reg_thresh=0.2)
    a = check(bk, inp, prm, seed=15)
    inp["iou"] = outs[2].get().copy()
    b = check(bk, inp, prm, seed=15)
    for x, y in zip(a[:5], b[:5]):
        assert np.array_equal(x, y)
    assert a[4].sum() > 6


def case_select_errors(bk, golden):
    """budget < max_pos_num * (1 + neg_ratio) and 0 < topk < NC: STEP_E_SHAPE; Amax > 1024 and Gmax > 64: STEP_E_UNSUPPORTED; a missing
    generator state: STEP_E_NULL.  A refused call writes nothing and leaves the offset where it was."""
    rs = np.random.RandomState(9)
    inp = make_inputs(rs, [4, 3], [1, 2], score=True)
    st = _state(bk, 3, 11)
    assert call(bk, inp, params(budget=14), st, expect_status=E_SHAPE) == E_SHAPE
    assert call(bk, inp, params(topk=3), st, expect_status=E_SHAPE) == E_SHAPE
    assert call(bk, inp, params(amax=1025), st, expect_status=E_UNSUPPORTED) == E_UNSUPPORTED
    assert call(bk, inp, params(), st, expect_status=E_UNSUPPORTED, Gmax=65) == E_UNSUPPORTED
    assert call(bk, inp, params(), st, expect_status=E_NULL, rng=None) == E_NULL
    assert call(bk, inp, params(sampling=3), st, expect_status=E_SHAPE) == E_SHAPE
    assert _read_state(st) == (3, 11)
    call(bk, inp, params(budget=15, topk=4), st)
    assert _read_state(st) == (3, 12)


# ---- distribution and state ----------------------------------------------------------------------------------------------------
DIST_B = 2048


def _dist_negatives():
    """B identical clips: one ground truth, tube 0 on top of it (the positive), six tubes that overlap nothing with scores 0 .. 2.5
    (softmax weights e^0 .. e^2.5), max_pos_num = 1, neg_ratio = 2: two of the six drawn per clip."""
    NC, B = 2, DIST_B
    cand1 = np.zeros((7, 3, 4), f32)
    cand1[0] = [100, 100, 200, 200]
    for a in range(1, 7):
        cand1[a] = [300 + a, 10, 340 + a, 60]                    # x1 names the tube
    score1 = np.zeros((7, NC), f32)
    score1[:, 0] = [3.0, 0.0, 0.5, 1.0, 1.5, 2.0, 2.5]
    gt = np.zeros((B, 1, 3, 4 + NC), f32)
    gt[:, 0, :, :4] = [102, 98, 203, 199]
    gt[:, 0, :, 4] = 1
    inp = {"cand": np.tile(cand1, (B, 1, 1)), "score": np.tile(score1, (B, 1)), "clip_start": (np.arange(B + 1) * 7).astype(np.int32),
           "gt": gt, "gt_count": np.ones(B, np.int32), "pad": np.zeros((B, 3, 4), f32)}
    iou1 = np.array([box_iou_f32(gt[0, 0, 1, :4], cand1[a, 1]) for a in range(7)], f32)
    inp["iou"] = np.tile(iou1[:, None], (B, 1))
    prm = params(max_pos_num=1, neg_ratio=2, budget=3, sampling=2, cls_thresh=0.5, reg_thresh=0.5)
    w = np.exp(score1[1:, 0].astype(np.float64))
    W = w.sum()
    incl = np.array([w[i] / W + sum(w[j] / W * w[i] / (W - w[j]) for j in range(6) if j != i) for i in range(6)])
    return inp, prm, incl


def _dist_positives():
    """B identical clips: one ground truth, six tubes above cls_thresh (the greedy pick takes the best), max_pos_num = 3: two of the other
    five drawn uniformly per clip; no negatives."""
    NC, B = 2, DIST_B
    cand1 = np.zeros((6, 3, 4), f32)
    for a in range(6):
        cand1[a] = [100 + 3 * a, 100, 200 + 3 * a, 200]
    gt = np.zeros((B, 1, 3, 4 + NC), f32)
    gt[:, 0, :, :4] = [100, 100, 200, 200]
    gt[:, 0, :, 5] = 1
    inp = {"cand": np.tile(cand1, (B, 1, 1)), "clip_start": (np.arange(B + 1) * 6).astype(np.int32), "gt": gt,
           "gt_count": np.ones(B, np.int32), "pad": np.zeros((B, 3, 4), f32)}
    prm = params(max_pos_num=3, neg_ratio=0, budget=3, sampling=1, cls_thresh=0.5, reg_thresh=0.5)
    return inp, prm, np.full(5, 2.0 / 5.0)


def _inclusion(sel, mask, rows, x1_of):
    """share of the clips in which each named tube occupies one of `rows` (slots of the clip)"""
    B = DIST_B
    s = sel.reshape(B, -1, sel.shape[1], 5)[:, rows, 0, 1]
    m = mask.reshape(B, -1)[:, rows]
    assert np.all(m == 1)
    return np.array([(s == x).any(axis=1).mean() for x in x1_of])


def _assert_share(who, got, want):
    bound = 5.0 * np.sqrt(want * (1 - want) / DIST_B)
    print("selection distribution %s: shares %s, exact %s, 5 sigma %s" % (who, np.round(got, 4), np.round(want, 4), np.round(bound, 4)))
    assert np.all(np.abs(got - want) <= bound), (who, got, want, bound)


_DIST_CACHE = {}


def _dist_reference(kind, seed, offset):
    """the restatement on a distribution input, once per session (shared by the emulator and the state cases)"""
    key = (kind, seed, offset)
    if key not in _DIST_CACHE:
        inp, prm, incl = _dist_negatives() if kind == "neg" else _dist_positives()
        _DIST_CACHE[key] = (inp, prm, incl, restate(inp, prm, seed, offset))
    return _DIST_CACHE[key]


def case_select_distribution(bk, golden):
    """One launch with 2048 identical clips at a fixed seed.  Negatives: two of six drawn by softmax weight -- the inclusion frequency of
    every tube within 5 standard deviations sqrt(p (1 - p) / 2048) of its exact successive-sampling probability p_i + sum_j p_j w_i /
    (W - w_j).  Positives: two of five drawn uniformly -- every tube within 5 standard deviations of 2 / 5.  Asserted of the restatement
    first, then of the kernel, whose outputs also equal the restatement's."""
    for kind, rows, x1 in (("neg", [1, 2], [300.0 + a for a in range(1, 7)]), ("pos", [1, 2], None)):
        inp, prm, incl, want = _dist_reference(kind, 2024, 0)
        if kind == "neg":
            assert want[5] > 1e-9, want[5]
        else:
            order = np.argsort([-box_iou_f32(inp["gt"][0, 0, 1, :4], inp["cand"][a, 1]) for a in range(6)])
            assert order[0] == 0                                   # tube 0 is the greedy pick; the other five are drawn from
            x1 = [float(inp["cand"][a, 0, 0]) for a in range(1, 6)]
        _assert_share("restatement " + kind, _inclusion(want[0], want[2], rows, x1), incl)
        st = _state(bk, 2024, 0)
        got = call(bk, inp, prm, st)
        _assert_share(bk.name + " " + kind, _inclusion(got[0], got[2], rows, x1), incl)
        for nm, a, b in zip(NAMES, got, want):
            assert np.array_equal(a, b), nm


def case_select_state(bk, golden):
    """The offset advances by exactly 1 per call, also with B = 0 (inv = 1 / NC then); the same (seed, offset) gives identical outputs;
    the next offset gives another selection on the distribution input, equal to the restatement's at that offset."""
    inp, prm, _, want0 = _dist_reference("neg", 2024, 0)
    st = _state(bk, 2024, 0)
    a = call(bk, inp, prm, st)
    assert _read_state(st) == (2024, 1)
    b = call(bk, inp, prm, st)
    assert _read_state(st) == (2024, 2)
    assert not np.array_equal(a[0], b[0])
    want1 = _dist_reference("neg", 2024, 1)[3]
    assert np.array_equal(a[0], want0[0]) and np.array_equal(b[0], want1[0]) and np.array_equal(b[1], want1[1])
    st = _state(bk, 2024, 0)
    c = call(bk, inp, prm, st)
    for x, y in zip(a, c):
        assert np.array_equal(x, y)
    empty = {"cand": np.zeros((0, 3, 4), f32), "clip_start": np.zeros(1, np.int32), "gt": np.zeros((0, 1, 3, 6), f32),
             "gt_count": np.zeros(0, np.int32), "pad": np.zeros((0, 3, 4), f32)}
    st = _state(bk, 5, 0xFFFF_FFFF)
    out = call(bk, empty, params(), st)
    assert _read_state(st) == (5, 0x1_0000_0000)
    assert out[3][0] == f32(1.0 / 2)


KERNEL_CASES = ["case_select_small_clips", "case_select_shuffle", "case_select_no_overlap_tie", "case_select_above_and_rest",
                "case_select_samplings_and_reg_thresh", "case_select_topk_and_ties", "case_select_neighbours_and_growing",
                "case_select_iou_null_against_prepare", "case_select_errors", "case_select_distribution", "case_select_state"]


# ---- module cases --------------------------------------------------------------------------------------------------------------
def cfg(**kw):
    """the selection's share of the reference's argparse namespace (config.py:64-76, scripts/train_step.sh:43-48), NC = 6"""
    base = dict(T=3, num_classes=6, max_iter=3, NUM_CHUNKS={1: 1, 2: 1, 3: 3, 4: 3}, temporal_mode="predict", image_size=(400, 400),
                topk=-1, cls_thresh=[0.2, 0.35, 0.5], reg_thresh=[0.2, 0.35, 0.5], max_pos_num=5, neg_ratio=2, selection_sampling="softmax")
    base.update(kw)
    return NS(**base)


def np_(t):
    return t.detach().cpu().numpy()


def _module_inputs(rs, tubes, gts, NC, near, spread):
    """ground truths [B,G,3,4+NC] per clip (host arrays, as train_select takes them), initial tubes per clip and a history per step:
    pred_loc / pred_first_loc / pred_last_loc around the initial tubes, class scores random"""
    B, N = len(tubes), int(sum(tubes))
    inp = make_inputs(rs, tubes, gts, NC=NC, near=near, Gmax=max(gts))
    gt_list = [inp["gt"][b, :gts[b]].copy() for b in range(B)]
    init = [np.clip(inp["cand"][inp["clip_start"][b]:inp["clip_start"][b + 1]], 1, 399).astype(f32) for b in range(B)]
    flat = np.concatenate(init)
    hist = []
    for _ in range(2):
        hist.append({"pred_prob": torch.from_numpy(np.repeat(rs.rand(N, 1, NC).astype(f32), 3, axis=1)),
                     "pred_loc": torch.from_numpy((flat + rs.uniform(-spread, spread, flat.shape)).astype(f32)),
                     "pred_first_loc": torch.from_numpy((flat + rs.uniform(-spread, spread, flat.shape)).astype(f32)),
                     "pred_last_loc": torch.from_numpy((flat + rs.uniform(-spread, spread, flat.shape)).astype(f32)),
                     "tubes_nums": list(tubes)})
    return inp, gt_list, init, flat, hist


def _device_args(dev, inp, flat, hist, a):
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    pads = {i: to(np.tile(inp["pad"][:, :1], (1, a.NUM_CHUNKS[i] * a.T, 1))) for i in (1, 2, 3)}
    hist = [{k: (v.to(dev) if hasattr(v, "to") else v) for k, v in h.items()} for h in hist]
    return to(inp["gt"]), to(inp["gt_count"]), to(flat), to(inp["clip_start"]), pads, hist


def case_selector_matches_restatement(dev, golden):
    """DeviceSelector.select for the three steps of the default NUM_CHUNKS (1, 1, 3 chunks: step 2 writes neighbour targets, step 3 grows
    the tubes to 9 frames) against the restatement fed with step_select_prepare's outputs; one offset per step; the returned tensors are
    the selector's static buffers; temporal_mode "extrapolate" is refused before any launch."""
    import step_amd
    from step_amd import ops
    from step_amd.selection import DeviceSelector

    rs = np.random.RandomState(21)
    tubes, gts = [9, 4, 12], [2, 1, 3]
    a = cfg()
    inp, _, _, flat, hist = _module_inputs(rs, tubes, gts, a.num_classes, near=0.7, spread=12)
    rng = step_amd.DeviceRNG(dev, seed=41)
    selr = DeviceSelector(a, 3, 15, dev, rng)
    gt, gt_count, init_flat, clip_start, pads, dhist = _device_args(dev, inp, flat, hist, a)
    clip_of = torch.from_numpy(np.repeat(np.arange(3), tubes).astype(np.int32)).to(dev)
    for step in (1, 2, 3):
        out = selr.select(step, dhist[step - 2] if step > 1 else None, gt, gt_count, init_flat, clip_start, pads[step], max_tubes=12)
        assert all(o is s for o, s in zip(out, selr.out[step]))
        assert rng.offset() == step
        r = dict(inp, cand=flat, pad=np_(pads[step]))
        prm = params(cls_thresh=a.cls_thresh[step - 1], reg_thresh=a.reg_thresh[step - 1], before=0 if step == 2 else -1, after=2 if step == 2 else -1)
        if step > 1:
            h = dhist[step - 2]
            score, vloc, vfirst, vlast, iou = ops.select_prepare(h["pred_prob"], h["pred_loc"], h["pred_first_loc"], h["pred_last_loc"], clip_of,
                                                                 gt[:, :, 1, :4].contiguous(), gt_count, 400.0, 400.0)
            r.update(cand=np_(vloc), score=np_(score), iou=np_(iou))
            if step == 3:
                r.update(first=np_(vfirst), last=np_(vlast))
        want = restate(r, prm, 41, step - 1)
        assert want[5] > 1e-9, want[5]
        assert out[0].shape[1] == (9 if step == 3 else 3)
        for nm, g_, w_ in zip(NAMES, out, want):
            assert np.array_equal(np_(g_), w_), (step, nm)
        assert want[4].sum() > 10
    try:
        DeviceSelector(cfg(temporal_mode="extrapolate"), 3, 15, dev, rng)
    except NotImplementedError:
        pass
    else:
        raise AssertionError("DeviceSelector accepted temporal_mode 'extrapolate'")
    assert rng.offset() == 3


def case_selector_agrees_with_host_selection(dev, golden):
    """Inputs where no draw decides anything -- G = 2 <= max_pos_num, nothing above cls_thresh once the greedy picks are gone, rest (4) no
    longer than the wanted negatives (2 x 2), no equal scores or IoUs: selection.train_select (the host code tests/golden/
    selection_golden.npz pins to the reference) and DeviceSelector agree on the positive rows in order, on the SET of negative rows and on
    their targets, for steps 1, 2 and 3."""
    import step_amd
    from step_amd.selection import DeviceSelector, train_select

    rs = np.random.RandomState(22)
    a = cfg(selection_sampling="uniform")
    B, A, G = 2, 6, 2
    inp, gt_list, init, flat, hist = _module_inputs(rs, [A] * B, [G] * B, a.num_classes, near=0.0, spread=2)
    for b in range(B):                                           # tubes 0 and 1 on the two ground truths, the others far from both
        for g in range(G):
            init[b][g] = gt_list[b][g, 1, :4] + rs.uniform(-5, 5, (3, 4)).astype(f32)
        for k in range(G, A):
            box = rand_boxes(rs, 1)[0]
            while max(box_iou_f32(gt_list[b][g, 1, :4], box) for g in range(G)) > 0.05:
                box = rand_boxes(rs, 1)[0]
            init[b][k] = box
        init[b] = np.clip(init[b], 1, 399).astype(f32)
    flat = np.concatenate(init)
    for h in hist:
        for key in ("pred_loc", "pred_first_loc", "pred_last_loc"):
            h[key] = torch.from_numpy((flat + rs.uniform(-2, 2, flat.shape)).astype(f32))
    rng = step_amd.DeviceRNG(dev, seed=43)
    selr = DeviceSelector(a, B, 15, dev, rng)
    gt, gt_count, init_flat, clip_start, pads, dhist = _device_args(dev, inp, flat, hist, a)
    for step in (1, 2, 3):
        h_sel, h_tgt = train_select(step, dhist[step - 2] if step > 1 else None, gt_list, init, a, device=True if step > 1 else None)
        sel, tgt, mask, _, counts = [np_(t) for t in selr.select(step, dhist[step - 2] if step > 1 else None, gt, gt_count, init_flat, clip_start,
                                                                pads[step], max_tubes=A)]
        for b in range(B):
            P, R = int(counts[b, 0]), int(counts[b].sum())
            assert (P, R) == (G, A) == (G, len(h_sel[b])), (step, b, P, R, len(h_sel[b]))
            rows = slice(b * 15, b * 15 + R)
            d_sel, d_tgt = sel[rows][:, :, 1:], tgt[rows]
            assert np.array_equal(d_sel[:P], h_sel[b][:P]) and np.array_equal(d_tgt[:P], h_tgt[b][:P]), (step, b, "positives")
            key = lambda s_: sorted(range(P, R), key=lambda r: tuple(s_[r].reshape(-1)))
            kd, kh = key(d_sel), key(h_sel[b])
            assert np.array_equal(d_sel[kd], h_sel[b][kh]) and np.array_equal(d_tgt[kd], h_tgt[b][kh]), (step, b, "negatives")
            assert mask[rows].all() and not mask[b * 15 + R:(b + 1) * 15].any()


MODULE_CASES = ["case_selector_matches_restatement", "case_selector_agrees_with_host_selection"]
