"""Cases for the classification pre-training stage (train_cls.py): step_anchor_sample, step_amd.ops.anchor_sample,
step_amd.selection.sample_anchors / cls_select / DeviceClsSelector, the fused tail of a cls_only head and step_amd.driver.classified_rows
-- driven on the host interpreter by tests/test_emul_cls.py and on the real library by tests/test_gpu_cls.py.

The reference of every kernel comparison is `restate` below: the rule of include/step_amd.h ("The rule, per pair") written again in
Python on float64 scalars from the header's text, drawing from tests/dropout_cases.philox_words (select_cases.draw is the same draw, one
at a time; `_draws` is checked against it).  tubes, clip_start and counts are compared for EQUALITY: the rule is float64 arithmetic in a
fixed order, comparisons, and one rounding to fp32.

Kernel cases take a backend of tests/backends.py; module cases take a device string ("cpu" under the interpreter patch, "cuda")."""
import random

import numpy as np
import torch

from tests.dropout_cases import philox_words
from tests.select_cases import box_iou_f32, draw

f32, f64, u64 = np.float32, np.float64, np.uint64
E_SHAPE, E_NULL, E_UNSUPPORTED = -2, -3, -4
W, H = 320.0, 240.0
TRIALS = 50


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def _draws(seed, offset, q, phase):
    """u [50, 16] of blocks (q << 20) | (phase << 16) | k, k = 16 j + slot"""
    w = philox_words(seed, offset, (q << 20) | (phase << 16), 16 * TRIALS)
    u = ((w[:, 0] << u64(21)) | (w[:, 1] >> u64(11))).astype(f64) * 2.0 ** -53
    return u.reshape(TRIALS, 16)


def _uniform(a, b, u):
    return a + (b - a) * u


def _box(cx, cy, bw, bh):
    return [cx - 0.5 * bw, cy - 0.5 * bh, cx + 0.5 * bw, cy + 0.5 * bh]


def _ious(boxes, c):
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for a in boxes:
            iw = (a[2] if a[2] < c[2] else c[2]) - (a[0] if a[0] > c[0] else c[0])
            ih = (a[3] if a[3] < c[3] else c[3]) - (a[1] if a[1] > c[1] else c[1])
            iw = f64(0) if iw < 0 else iw
            ih = f64(0) if ih < 0 else ih
            inter = iw * ih
            out.append(inter / ((a[2] - a[0]) * (a[3] - a[1]) + (c[2] - c[0]) * (c[3] - c[1]) - inter))
    return out


def accept(boxes, g, c, pos_thresh, neg_thresh):
    """(P, N) of a candidate for ground truth g among `boxes` (float64, normalised)"""
    iou = _ious(boxes, c)
    below = sum(1 for v in iou if v < neg_thresh)
    return bool(iou[g] > pos_thresh) and below == len(boxes) - 1, below == len(boxes)


def pair_rows(boxes, g, q, prm, seed, offset):
    """-> (positives, negatives): the candidates (float64, normalised) the pair takes, in row order"""
    pos_num, neg_num = prm["pos_num"], prm["pos_num"] * prm["neg_ratio"]
    pt, nt = f64(f32(prm["pos_thresh"])), f64(f32(prm["neg_thresh"]))
    a = boxes[g]
    w, h = a[2] - a[0], a[3] - a[1]
    x, y = a[0] + 0.5 * w, a[1] + 0.5 * h
    pos, neg = [], []
    if prm["mode"] == 0:
        u = _draws(seed, offset, q, 0)
        for j in range(TRIALS):
            bw = _uniform(0.8 * w, min(f64(1), 1.2 * w), u[j, 0])
            bh = _uniform(0.8 * h, min(f64(1), 1.2 * h), u[j, 1])
            cx = _uniform(max(0.5 * bw, x - 0.2 * w), min(1 - 0.5 * bw, x + 0.2 * w), u[j, 2])
            cy = _uniform(max(0.5 * bh, y - 0.2 * h), min(1 - 0.5 * bh, y + 0.2 * h), u[j, 3])
            c = _box(cx, cy, bw, bh)
            P, N = accept(boxes, g, c, pt, nt)
            if P:
                pos.append(c)
            elif N and len(neg) < neg_num:
                neg.append(c)
            if len(pos) == pos_num:
                break
    u = _draws(seed, offset, q, 1)
    for j in range(TRIALS):
        pick = lambda k, first, second: first if u[j, k] < 0.5 else second
        bw = pick(2, _uniform(0.3 * w, 0.7 * w, u[j, 0]), min(f64(1), _uniform(1.5 * w, 2 * w, u[j, 1])))
        bh = pick(5, _uniform(0.3 * h, 0.7 * h, u[j, 3]), min(f64(1), _uniform(1.5 * h, 2 * h, u[j, 4])))
        cx = pick(8, _uniform(max(0.5 * bw, x - w), max(0.5 * bw, x - 0.3 * w), u[j, 6]),
                  _uniform(min(1 - 0.5 * bw, x + 0.3 * w), min(1 - 0.5 * bw, x + w), u[j, 7]))
        cy = pick(11, _uniform(max(0.5 * bh, x - h), max(0.5 * bh, y - 0.3 * h), u[j, 9]),
                  _uniform(min(1 - 0.5 * bh, y + 0.3 * h), min(1 - 0.5 * bh, y + h), u[j, 10]))
        c = _box(cx, cy, bw, bh)
        if len(neg) < neg_num and accept(boxes, g, c, pt, nt)[1]:
            neg.append(c)
    return pos, neg


def restate(gt, gt_count, prm, seed, offset):
    """-> (tubes [B*Gmax*S,T,4], clip_start [B+1], counts [B*Gmax,2], kinds): the outputs of step_anchor_sample and, per live pair,
    (sampled positives, negatives)"""
    B, Gmax = gt.shape[:2]
    S, T = prm["pos_num"] * (1 + prm["neg_ratio"]), prm["T"]
    whwh = np.array([W, H, W, H], f64)
    tubes = np.zeros((B * Gmax * S, T, 4), f32)
    clip_start = np.zeros(B + 1, np.int32)
    counts = np.zeros((B * Gmax, 2), np.int32)
    kinds = {}
    row = 0
    for b in range(B):
        clip_start[b] = row
        G = int(gt_count[b])
        boxes = [[f64(gt[b, o, prm["mid"], k]) / whwh[k] for k in range(4)] for o in range(G)]
        for g in range(G):
            q = b * Gmax + g
            pos, neg = pair_rows(boxes, g, q, prm, seed, offset)
            kinds[q] = (len(pos), len(neg))
            counts[q] = (1 if prm["mode"] else len(pos), len(neg))
            if prm["mode"] or not pos:
                tubes[row] = gt[b, g, prm["mid"], :4]
                row += 1
                pos = []
            for c in pos + neg:
                tubes[row] = [f32(c[k] * whwh[k]) for k in range(4)]
                row += 1
    clip_start[B] = row
    return tubes, clip_start, counts, kinds


# ---- inputs --------------------------------------------------------------------------------------------------------------------
SITUATIONS = {"isolated": [96.0, 84.0, 176.0, 192.0], "identical": [64.0, 60.0, 160.0, 168.0], "border": [0.0, 0.0, 70.4, 98.4],
              "full": [6.4, 7.2, 310.4, 237.6], "far": [236.0, 150.0, 306.0, 232.0], "left": [16.0, 24.0, 96.0, 144.0],
              "middle": [128.0, 36.0, 198.4, 180.0], "right": [211.2, 72.0, 297.6, 216.0]}
LAYOUTS = {"A": ([1, 4, 0], [["full"], ["identical", "identical", "border", "far"], []]),
           "B": ([0, 2, 3], [[], ["isolated", "far"], ["left", "middle", "right"]])}


def make_gt(layout, Gmax=4, F=2, NC=4, mid=1):
    """gt [3,Gmax,F,4+NC]: the named boxes at frame `mid`; every other frame and every slot past the clip's count holds other boxes, which
    the kernel must not read"""
    cnt, names = LAYOUTS[layout]
    rs = np.random.RandomState(5)
    gt = rs.uniform(10, 200, (len(cnt), Gmax, F, 4 + NC)).astype(f32)
    gt[..., 2:4] += 30
    gt[..., 4:] = (rs.rand(len(cnt), Gmax, F, NC) < 0.4)
    for b, row in enumerate(names):
        for g, nm in enumerate(row):
            gt[b, g, mid, :4] = SITUATIONS[nm]
    return gt, np.asarray(cnt, np.int32)


def params(**kw):
    prm = dict(mid=1, T=3, pos_num=1, neg_ratio=3, pos_thresh=0.75, neg_thresh=0.2, mode=0)
    prm.update(kw)
    return prm


def _state(bk, seed, offset):
    return bk.dev(np.array([seed, offset], u64).view(np.int64))


def _read_state(st):
    s = st.get().view(u64)
    return int(s[0]), int(s[1])


def call(bk, gt, gt_count, prm, st, expect_status=0, **override):
    """one step_anchor_sample call -> (tubes, clip_start, counts) as numpy, or the status when expect_status != 0"""
    B, Gmax, F, NC = gt.shape[0], gt.shape[1], gt.shape[2], gt.shape[3] - 4
    a = dict(B=B, Gmax=Gmax, F=F, NC=NC, rng=st.ptr, **prm)
    a.update(override)
    S = max(a["pos_num"] * (1 + max(a["neg_ratio"], 0)), 1)
    rows = max(B * Gmax * S, 1)
    out = [bk.dev(np.full((rows, max(prm["T"], 1), 4), 7, f32)), bk.dev(np.full((B + 1,), 7, np.int32)), bk.dev(np.full((max(B * Gmax, 1), 2), 7, np.int32))]
    d_gt, d_cnt = bk.dev(gt), bk.dev(gt_count)
    rc = bk.lib.step_anchor_sample(d_gt.ptr, d_cnt.ptr, a["B"], a["Gmax"], a["F"], a["NC"], a["mid"], W, H, a["T"], a["pos_num"], a["neg_ratio"],
                                   a["pos_thresh"], a["neg_thresh"], a["mode"], a["rng"], out[0].ptr, out[1].ptr, out[2].ptr, bk.stream)
    assert rc == expect_status, (rc, expect_status)
    got = [o.get().copy() for o in out]
    if expect_status != 0:
        assert all(np.all(o == 7) for o in got), "a refused call wrote something"
        return rc
    return got[0][:B * Gmax * S], got[1], got[2][:B * Gmax]


_RESTATED = {}


def restated(layout, prm, seed, offset):
    """the restatement, once per session and input (shared by the two backends and by the cases)"""
    key = (layout, tuple(sorted(prm.items())), seed, offset)
    if key not in _RESTATED:
        gt, cnt = make_gt(layout)
        _RESTATED[key] = restate(gt, cnt, prm, seed, offset)
    return _RESTATED[key]


def check(bk, layout, prm, seed, offset):
    gt, cnt = make_gt(layout)
    want = restated(layout, prm, seed, offset)
    st = _state(bk, seed, offset)
    got = call(bk, gt, cnt, prm, st)
    for nm, a, b in zip(("tubes", "clip_start", "counts"), got, want[:3]):
        assert a.shape == b.shape and a.dtype == b.dtype, (nm, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), (nm, np.argwhere(a != b)[:5], got[2].tolist(), want[2].tolist())
    assert _read_state(st) == (seed, offset + 1)
    return got, want


# ---- kernel cases --------------------------------------------------------------------------------------------------------------
SEED, OFFSET = 0x1_0000_0007, 0x2_0000_0003
SETTINGS = [params(), params(mode=1), params(pos_num=2, neg_ratio=2), params(neg_ratio=0), params(pos_num=2, neg_ratio=4)]


def case_anchor_draws_are_select_train_s():
    """the vectorised draws of the restatement are select_cases.draw, block by block"""
    u = _draws(SEED, OFFSET, 5, 1)
    for j, s_ in ((0, 0), (3, 11), (49, 15)):
        assert u[j, s_] == draw(SEED, OFFSET, 5, 1, 16 * j + s_)


def case_anchor_matches_restatement(bk, golden):
    """Bit equality of tubes, clip_start and counts with the restatement, train and eval mode, pos_num = 2 (with 4 and with 8 negatives
    wanted) and neg_ratio = 0, on the two
    layouts gt_count = [1, 4, 0] (a box that nearly fills the frame alone; two identical boxes, a box in the frame's corner and a far one;
    an EMPTY clip last) and [0, 2, 3] (an empty clip first; an isolated pair; three boxes side by side), at seed 0x100000007, offset
    0x200000003 (both above 2^32: the high words of key and counter matter).  At that seed the set holds, asserted below from the
    restatement: pairs with a sampled positive (the far, isolated and side-by-side boxes), pairs that fall back to their own box (the two
    identical boxes: no candidate can overlap one by more than 0.75 and the other by less than 0.2) and pairs that end with fewer than
    pos_num * neg_ratio negatives (the box that nearly fills the frame with 8 negatives wanted: only a candidate of less than a fifth of its
    area stays below 0.2, about one trial in eleven)."""
    case_anchor_draws_are_select_train_s()                       # precondition: the restatement's vectorised draws are select_cases.draw
    seen = dict(sampled=0, fallback=0, short=0)
    for layout in ("A", "B"):
        for prm in SETTINGS:
            got, want = check(bk, layout, prm, SEED, OFFSET)
            if prm["mode"] == 0:
                for q, (npos, nneg) in want[3].items():
                    seen["sampled"] += npos > 0
                    seen["fallback"] += npos == 0
                    seen["short"] += nneg < prm["pos_num"] * prm["neg_ratio"]
            else:
                assert np.all(got[2][:, 0] == (np.arange(12) % 4 < np.repeat(make_gt(layout)[1], 4)))
    assert all(v > 0 for v in seen.values()), seen
    tubes, clip_start, counts = restated("A", SETTINGS[0], SEED, OFFSET)[:3]
    assert clip_start[2] == clip_start[3] and counts[4, 0] == 0 and counts[5, 0] == 0, (clip_start, counts)     # empty clip last; the identical pair


def case_anchor_properties(bk, golden):
    """For other draws (three offsets, not compared with the restatement's rows): every row is its pair's own ground-truth box or satisfies
    its acceptance predicate recomputed in float64 from the fp32 row -- P for the first `positives` rows of a pair, N for the others, with
    1e-5 of slack on the IoUs: the fp32 rounding of a pixel coordinate (2^-24 relative) moves an IoU by less than that; rows from
    clip_start[B] on are zero; the frames of a row are identical; clip_start is the running sum of max(positives, 1) + negatives over the
    live pairs."""
    whwh = np.array([W, H, W, H], f64)
    for layout, prm, off in (("A", params(), 1), ("B", params(pos_num=2, neg_ratio=2), 2), ("B", params(mode=1), 3)):
        gt, cnt = make_gt(layout)
        tubes, clip_start, counts = call(bk, gt, cnt, prm, _state(bk, 99, off))
        assert np.array_equal(tubes, np.repeat(tubes[:, :1], prm["T"], axis=1))
        assert not tubes[clip_start[3]:].any() and clip_start[0] == 0
        row = 0
        for b in range(3):
            assert clip_start[b] == row
            boxes = [[f64(v) / whwh[k] for k, v in enumerate(gt[b, o, 1, :4])] for o in range(cnt[b])]
            for g in range(4):
                npos, nneg = counts[b * 4 + g]
                if g >= cnt[b]:
                    assert npos == 0 and nneg == 0
                    continue
                assert 0 <= npos <= prm["pos_num"] and 0 <= nneg <= prm["pos_num"] * prm["neg_ratio"]
                own = npos == 0 or prm["mode"] == 1
                for r in range(max(npos, 1) + nneg):
                    box = tubes[row, 0]
                    if r == 0 and own:
                        assert np.array_equal(box, gt[b, g, 1, :4])
                    else:
                        iou = _ious(boxes, [f64(v) / whwh[k] for k, v in enumerate(box)])
                        if r < npos:
                            assert iou[g] > 0.75 - 1e-5 and all(v < 0.2 + 1e-5 for o, v in enumerate(iou) if o != g), (layout, b, g, r, iou)
                        else:
                            assert all(v < 0.2 + 1e-5 for v in iou), (layout, b, g, r, iou)
                    row += 1
        assert clip_start[3] == row


def case_anchor_state(bk, golden):
    """The offset advances by exactly 1 per launch, also with B = 0; the same (seed, offset) gives the same output; the next launch on the
    same state gives other boxes, equal to the restatement's at the next offset."""
    gt, cnt = make_gt("B")
    prm = params()
    st = _state(bk, SEED, OFFSET)
    a = call(bk, gt, cnt, prm, st)
    assert _read_state(st) == (SEED, OFFSET + 1)
    b = call(bk, gt, cnt, prm, st)
    assert _read_state(st) == (SEED, OFFSET + 2)
    assert not np.array_equal(a[0], b[0])
    c = call(bk, gt, cnt, prm, _state(bk, SEED, OFFSET))
    for x, y in zip(a, c):
        assert np.array_equal(x, y)
    want = restated("B", prm, SEED, OFFSET + 1)
    assert np.array_equal(b[0], want[0]) and np.array_equal(b[1], want[1]) and np.array_equal(b[2], want[2])
    st = _state(bk, 5, 0xFFFF_FFFF)
    out = call(bk, np.zeros((0, 4, 2, 8), f32), np.zeros(0, np.int32), prm, st)
    assert _read_state(st) == (5, 0x1_0000_0000) and out[1].tolist() == [0]


def case_anchor_errors(bk, golden):
    """Gmax > 64 and Gmax * S > 1024: STEP_E_UNSUPPORTED; pos_num < 1, neg_ratio < 0, T < 1: STEP_E_SHAPE; a missing generator state:
    STEP_E_NULL.  A refused call writes nothing and leaves the offset where it was."""
    gt, cnt = make_gt("A")
    st = _state(bk, 3, 11)
    assert call(bk, gt, cnt, params(), st, expect_status=E_UNSUPPORTED, Gmax=65) == E_UNSUPPORTED
    assert call(bk, gt, cnt, params(pos_num=65, neg_ratio=3), st, expect_status=E_UNSUPPORTED) == E_UNSUPPORTED      # 4 * 260 > 1024
    assert call(bk, gt, cnt, params(pos_num=0), st, expect_status=E_SHAPE) == E_SHAPE
    assert call(bk, gt, cnt, params(neg_ratio=-1), st, expect_status=E_SHAPE) == E_SHAPE
    assert call(bk, gt, cnt, params(T=0), st, expect_status=E_SHAPE) == E_SHAPE
    assert call(bk, gt, cnt, params(), st, expect_status=E_NULL, rng=None) == E_NULL
    assert _read_state(st) == (3, 11)
    call(bk, gt, cnt, params(pos_num=64, neg_ratio=3), st)                                                            # 4 * 256 = 1024: the limit itself
    assert _read_state(st) == (3, 12)


KERNEL_CASES = ["case_anchor_matches_restatement", "case_anchor_properties", "case_anchor_state", "case_anchor_errors"]


# ---- host cases (no kernel) ----------------------------------------------------------------------------------------------------
def case_sample_anchors_golden(golden):
    """selection.sample_anchors against every case of tests/golden/cls_golden.npz (recorded from the reference's function): the same boxes
    as float64 BITS, in the same order, and the same next random.random() -- the stream is left where the reference leaves it."""
    from step_amd.selection import sample_anchors

    g = golden("cls_golden")
    assert len(g["cases"]) >= 40
    for k in g["cases"]:
        k = str(k)
        pos_num, neg_ratio, seed = (int(v) for v in g[k + "_args"])
        random.seed(seed)
        out = sample_anchors(g[k + "_in"].copy(), pos_num=pos_num, neg_ratio=neg_ratio, mode=str(g[k + "_mode"]))
        nxt = random.random()
        want = g[k + "_out"]
        assert out.dtype == np.float64 and out.shape == want.shape, (k, out.shape, want.shape)
        assert np.array_equal(out.view(np.uint64), want.view(np.uint64)), k
        assert nxt == float(g[k + "_next"]), k


def case_cls_select_literal(golden):
    """cls_select on a hand-made clip under random.seed(3) / numpy.random.seed(3): two ground truths; tubes 0 and 1 sit on them (IoU 1 and
    0.81: the greedy positives, in the order of the ground truths' best IoU), tube 2 overlaps ground truth 0 by 0.78 > 0.75 (the drawn
    positive: the only one above the threshold), tubes 3-5 overlap nothing and become the negatives, all three of them (9 wanted), in the
    order numpy.random.choice gives under that seed behind the one-element draw of the third positive: tubes 5, 3, 4 -- transcribed below
    as the literal rows."""
    from step_amd.selection import cls_select

    NC = 3
    gt = np.zeros((2, 1, 4 + NC), f32)
    gt[0, 0] = [100, 100, 200, 200, 1, 0, 1]
    gt[1, 0] = [250, 50, 350, 150, 0, 1, 0]
    boxes = np.array([[100, 100, 200, 200], [255, 55, 355, 145], [100, 100, 200, 178], [10, 300, 60, 380], [300, 300, 380, 390], [20, 20, 60, 70]], f32)
    tubes = np.tile(boxes[:, None, :], (1, 3, 1))
    random.seed(3)
    np.random.seed(3)
    sel, tgt = cls_select([gt], [tubes])
    assert len(sel) == 1 and sel[0].shape == (6, 3, 4) and tgt[0].shape == (6, 3, 6 + NC) and sel[0].dtype == f32 and tgt[0].dtype == f32
    want_rows = [0, 1, 2, 5, 3, 4]
    assert np.array_equal(sel[0], tubes[want_rows]), (want_rows, sel[0][:, 0])
    want_tgt = np.zeros((6, 6 + NC), f32)
    want_tgt[0] = [100, 100, 200, 200, 1, 0, 1, 0, 1]
    want_tgt[1] = [250, 50, 350, 150, 1, 0, 0, 1, 0]
    want_tgt[2] = [100, 100, 200, 200, 1, 0, 1, 0, 1]
    want_tgt[3:, 4] = 1
    for fr in range(3):
        assert np.array_equal(tgt[0][:, fr], want_tgt), fr


HOST_CASES = ["case_sample_anchors_golden", "case_cls_select_literal"]


# ---- module cases --------------------------------------------------------------------------------------------------------------
def np_(t):
    return t.detach().cpu().numpy()


def case_classified_rows(dev, golden):
    """driver.classified_rows and detections_csv against a loop over (clip, class, tube) as train_cls.py:508-543 runs it: 2 clips with 2 and
    3 tubes, 4 classes, scores on both sides of the threshold (one equal to it: not kept), a class without any row; no NMS -- two
    identical boxes both stay."""
    from types import SimpleNamespace as NS

    from step_amd import driver

    args = NS(image_size=(400, 300), conf_thresh=0.3, num_classes=4)
    nums = [2, 3]
    rs = np.random.RandomState(11)
    prob = rs.uniform(0.05, 0.95, (5, 4)).astype(f32)
    prob[:, 2] = 0.1                                             # a class without rows
    prob[1, 0] = f32(0.3)                                        # equal to the threshold: `gt` drops it
    prob[0, 1], prob[3, 1] = 0.9, 0.05
    tubes = np.zeros((5, 3, 5), f32)
    mids = np.array([[40, 30, 200, 260], [40, 30, 200, 260], [10, 20, 390, 290], [120.5, 33.25, 300.75, 140], [0, 0, 399, 299]], f32)
    tubes[:, :, 1:] = mids[:, None, :] + np.array([-3, 0, 3], f32)[None, :, None]     # only the middle frame is the box written
    tubes[:, :, 0] = np.arange(15).reshape(5, 3)
    dets = driver.classified_rows(args, torch.from_numpy(prob).to(dev), torch.from_numpy(tubes).to(dev), nums)
    want, lines = [], []
    infos = [{"video_name": "vidA", "fid": 7}, {"video_name": "vidB", "fid": 1234}]
    start = 0
    for b, n in enumerate(nums):
        rows = []
        for c in range(4):
            for j in range(n):
                s_ = prob[start + j, c]
                if s_ > f32(0.3):
                    box = tubes[start + j, 1, 1:] / np.array([400, 300, 400, 300], f32)
                    rows.append((box, s_, c, j))
                    lines.append("{0},{1:04},{2:.4},{3:.4},{4:.4},{5:.4},{6},{7:.4}\n".format(infos[b]["video_name"], infos[b]["fid"], box[0], box[1],
                                                                                              box[2], box[3], c + 1, s_))
        want.append(rows)
        start += n
    assert len(dets) == 2
    for b in range(2):
        d = dets[b]
        assert len(d["scores"]) == len(want[b]) > 2, (b, len(d["scores"]), len(want[b]))
        assert np.array_equal(np_(d["boxes"]), np.array([r[0] for r in want[b]], f32))
        assert np.array_equal(np_(d["scores"]), np.array([r[1] for r in want[b]], f32))
        assert np_(d["labels"]).tolist() == [r[2] for r in want[b]] and np_(d["tubes"]).tolist() == [r[3] for r in want[b]]
        assert 2 not in np_(d["labels"]).tolist()
    assert driver.detections_csv(dets, infos) == lines
    empty = driver.classified_rows(args, torch.zeros((0, 4), device=dev), torch.zeros((0, 3, 5), device=dev), [0, 0])
    assert [len(d["scores"]) for d in empty] == [0, 0]


def _cls_cfg(**kw):
    from tests.select_cases import cfg
    return cfg(max_iter=1, NUM_CHUNKS={1: 1}, **kw)


def case_device_cls_selector(dev, golden):
    """DeviceClsSelector on hand-made ground truths (3 clips with 2, 3 and 0 boxes, Gmax 3, NC 6), two select() calls: per clip at most 5
    positives and at most 3 x positives negatives, at least one positive per ground truth's clip; real rows first (mask 1), then padding
    (mask 0, the pad box, all-zero targets); inv = 1 / (rows * NC); a positive row's centre target is the box and labels of the ground
    truth its tube overlaps most, a negative row's is zero, column 4 is 1 on every real row (column 5 is not compared); every selected
    tube is one of the sampled tubes of its clip; two offsets per call, and the second call selects other boxes."""
    import step_amd
    from step_amd.selection import DeviceClsSelector

    a = _cls_cfg()
    NC, B, Gmax, Bu = a.num_classes, 3, 3, 20
    rs = np.random.RandomState(31)
    gt = np.zeros((B, Gmax, 1, 4 + NC), f32)
    boxes = [[[40, 60, 140, 220], [230, 80, 330, 260]], [[20, 30, 110, 150], [150, 200, 260, 340], [280, 20, 380, 130]], []]
    for b, row in enumerate(boxes):
        for g, bx in enumerate(row):
            gt[b, g, 0, :4] = bx
            gt[b, g, 0, 4:] = rs.rand(NC) < 0.5
            gt[b, g, 0, 4 + g] = 1
    cnt = np.array([2, 3, 0], np.int32)
    pad = np.tile(np.array([[5, 5, 100, 100]], f32), (B, 3, 1))
    rng = step_amd.DeviceRNG(dev, seed=77)
    selr = DeviceClsSelector(a, B, Gmax, dev, rng)
    d_gt, d_cnt, d_pad = (torch.from_numpy(x).to(dev) for x in (gt, cnt, pad))
    seen = []
    for it in range(2):
        out = selr.select(d_gt, d_cnt, d_pad)
        assert all(o is s_ for o, s_ in zip(out, selr.out)) and rng.offset() == 2 * (it + 1)
        sel, tgt, mask, inv, counts = (np_(t) for t in out)
        sampled, clip_start = np_(selr.sampled[0]), np_(selr.sampled[1])
        assert sel.shape == (B * Bu, 3, 5) and tgt.shape == (B * Bu, 3, 6 + NC)
        rows = int(counts.sum())
        assert inv[0] == f32(1.0 / (rows * NC))
        for b in range(B):
            P, N = counts[b]
            assert (P, N) == (0, 0) if cnt[b] == 0 else (cnt[b] <= P <= 5 and 0 <= N <= 3 * P), (b, P, N)
            m = mask[b * Bu:(b + 1) * Bu, 0]
            assert np.all(m[:P + N] == 1) and not m[P + N:].any()
            mine = sampled[clip_start[b]:clip_start[b + 1]]
            for r in range(Bu):
                o = b * Bu + r
                assert np.array_equal(sel[o, :, 0], b * 3 + np.arange(3, dtype=f32))
                if r >= P + N:
                    assert np.array_equal(sel[o, :, 1:], pad[b]) and not tgt[o].any()
                    continue
                assert any(np.array_equal(sel[o, :, 1:], t) for t in mine), (b, r)
                assert tgt[o, 1, 4] == 1 and not tgt[o, 0].any() and not tgt[o, 2].any()
                if r < P:
                    ious = [box_iou_f32(gt[b, g, 0, :4], sel[o, 1, 1:]) for g in range(cnt[b])]
                    g = int(np.argmax(ious))
                    assert ious[g] > 0.75 and np.array_equal(tgt[o, 1, :4], gt[b, g, 0, :4]) and np.array_equal(tgt[o, 1, 6:], gt[b, g, 0, 4:]), (b, r, ious)
                else:
                    assert not tgt[o, 1, :4].any() and not tgt[o, 1, 5:].any()
        seen.append(sel.copy())
    assert not np.array_equal(seen[0], seen[1])


def case_cls_only_fused_against_chain(dev, golden):
    """TwoBranchNet(cls_only=True): the fused tail (step_head_outputs with reg == NULL) against its torch chain
    (heads.FUSED_HEAD_OUTPUTS = False), in the head's three branches -- training with gradients (heads._HeadOutputsFn), targets without
    gradients, and inference (no targets).  The PATH is asserted by counting the calls of ops.head_outputs / ops.head_outputs_backward
    around each forward and backward: fused, one forward launch per call, every one with reg None, and one backward launch for the
    training branch; chain, none at all -- a quiet fall-back to the chain fails here.  Values at the tolerance of
    module_cases.case_loss_masks_without_host_branches: outputs within 2e-6 * max(1, |chain|) (the launch sums in another, fixed order),
    the gradient's absolute sum within 1e-5 relative, here also the input gradient element-wise at 1e-5 of its largest entry; in every
    branch the returned shapes are the chain's; negatives (flag 1, no labels) are part of the targets."""
    import step_amd
    from step_amd import heads, ops
    from tests.module_cases import R, cfg, fill

    g = golden("head_golden")
    tubes, targets = torch.from_numpy(g["loss_tubes"]).to(dev), torch.from_numpy(g["loss_targets"]).to(dev).clone()
    targets[1, :, :4] = 0
    targets[1, :, 5:] = 0                                        # tube 1: a negative of the classification stage (flag 1, nothing else)
    targets[:, :, 4] = 1
    keep, fwd, bwd = heads.FUSED_HEAD_OUTPUTS, ops.head_outputs, ops.head_outputs_backward
    calls = {"fwd": [], "bwd": []}

    def spy_fwd(logits, reg, *a, **k):
        calls["fwd"].append(reg)
        return fwd(logits, reg, *a, **k)

    def spy_bwd(logits, reg, *a, **k):
        calls["bwd"].append(reg)
        return bwd(logits, reg, *a, **k)

    out = {}
    try:
        ops.head_outputs, ops.head_outputs_backward = spy_fwd, spy_bwd
        for fused in (True, False):
            heads.FUSED_HEAD_OUTPUTS = fused
            net = fill(step_amd.TwoBranchNet(cfg(), cls_only=True), "det0.").to(dev)
            net.set_device(dev)
            net.train()
            pf = R.fill_tensor("golden.det.pooled3", (2, 3, 832, 7, 7), "feat").to(dev).requires_grad_(True)
            cx = R.fill_tensor("golden.det.ctx3", (2, 1024, 3, 1, 1), "feat").to(dev)
            want = (1, 1) if fused else (0, 0)
            calls["fwd"], calls["bwd"] = [], []
            o = net(pf, context_feat=cx, tubes=tubes, targets=targets)
            assert (len(calls["fwd"]), len(calls["bwd"])) == (want[0], 0), (fused, "training forward", calls)
            o[4].mean().backward()
            assert (len(calls["fwd"]), len(calls["bwd"])) == want, (fused, "training backward", calls)
            gsum = sum(float(p.grad.abs().sum()) for p in net.parameters() if p.grad is not None)
            with torch.no_grad():
                o_ng = net(pf, context_feat=cx, tubes=tubes, targets=targets)
            net.eval()
            with torch.no_grad():
                o_inf = net(pf, context_feat=cx)
            assert (len(calls["fwd"]), len(calls["bwd"])) == (3 * want[0], want[1]), (fused, "no-grad and inference", calls)
            assert all(r is None for r in calls["fwd"] + calls["bwd"]), "a cls_only head handed a regressor to the launch"
            out[fused] = ([np_(t) for t in o], np_(pf.grad), gsum, [np_(t) for t in o_ng], [np_(t) for t in o_inf])
    finally:
        heads.FUSED_HEAD_OUTPUTS, ops.head_outputs, ops.head_outputs_backward = keep, fwd, bwd
    (fo, fg, fs, fng, finf), (co, cg, cs, cng, cinf) = out[True], out[False]
    for tag, f_, c_ in (("training", fo, co), ("no-grad", fng, cng), ("inference", finf, cinf)):
        for i in range(7):
            assert f_[i].shape == c_[i].shape, (tag, i, f_[i].shape, c_[i].shape)
        assert f_[0].shape == (2, 60) and all(f_[i].shape == (1,) and not f_[i].any() for i in (1, 2, 3, 5, 6)), tag
        for i in (0, 4):
            assert np.abs(f_[i] - c_[i]).max() <= 2e-6 * max(1.0, np.abs(c_[i]).max()), (tag, i, np.abs(f_[i] - c_[i]).max())
    assert fo[4].shape == fng[4].shape == (120,) and finf[4].shape == (1,) and not finf[4].any() and np.abs(co[4]).max() > 0
    assert cs > 0 and abs(fs - cs) <= 1e-5 * cs, (fs, cs)
    assert np.abs(cg).max() > 0 and np.abs(fg - cg).max() <= 1e-5 * np.abs(cg).max(), (np.abs(fg - cg).max(), np.abs(cg).max())


MODULE_CASES = ["case_classified_rows", "case_device_cls_selector", "case_cls_only_fused_against_chain"]
