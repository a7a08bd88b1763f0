"""Cases for detector proposals on the device path: ragged tubes per clip as PADDED slots with a device-side count (step_augment_plan_tubes,
step_select_train_counted, DeviceTubeAugmentation.apply(tubes=...), DeviceSelector.select(clip_count=...), driver.pad_tubes and the
"tubes_count" of a history, selection.read_proposals), driven on the host interpreter by tests/test_emul_proposals.py and on the real
library by tests/test_gpu_proposals.py.

The references.  The planner's proposals: TubeAugmentation.plan(shape, tubes, proposals=float64(inputs)) -- the host rule that
tests/augment_cases.py pins to the reference bit for bit -- fed the device's draws through tests/augplan_cases' feeder, then
scale_tubes_abs (utils/tube_utils.py:202-212) in float64 and ONE rounding to fp32; the plan block and the ground truths: augplan_cases'
restatement, i.e. step_augment_plan's own results at the same state.  The counted selection: tests/select_cases.restate on the COMPACTED
inputs (the real rows alone).  The padded post-processing: driver.postprocess on the history sliced to its real rows.  Everything is
compared for equality, floats as bits.

Kernel cases take a backend of tests/backends.py; module cases take a device string ("cpu" under the interpreter patch, "cuda")."""
import os

import numpy as np

from step_amd.augment import TubeAugmentation
from tests import augplan_cases as PC
from tests import select_cases as SC

f32, f64 = np.float32, np.float64
E_SHAPE, E_NULL, E_UNSUPPORTED = -2, -3, -4
FLIP, CROP, PHOTO, ERASE, ALL = PC.FLIP, PC.CROP, PC.PHOTO, PC.ERASE, PC.ALL
SWITCHES = (0, CROP, FLIP, CROP | FLIP, ALL)

# ---- the planner with tubes ----------------------------------------------------------------------------------------------------------------
PMAX, TP = 5, 3
PCOUNTS = (0, 3, 5)
FILL = np.array([[0.125, 0.25, 0.5, 0.75], [0.3, 0.1, 0.95, 0.8]], f32)         # two anchors


def make_props():
    """tubes_in [3,PMAX,TP,4] percent boxes and their counts.  Clip 0 has none (the fill stands in); clip 1 -- the one whose crops are
    accepted: augplan_cases gives clip 2 no ground truths -- holds a box entirely outside any plausible crop (a corner sliver that also
    leaves [0, 1]), a box under 2 px wide in its 28 px frame and a box covering the frame; clip 2 holds a box with coordinates outside
    [0, 1] among ordinary ones.  Boxes jitter from frame to frame; slots past a clip's count hold other numbers, which the kernel must
    not use."""
    rs = np.random.RandomState(17)
    p = rs.uniform(0.05, 0.55, (3, PMAX, TP, 4)).astype(f32)
    p[..., 2:4] = p[..., 0:2] + rs.uniform(0.15, 0.4, (3, PMAX, TP, 2)).astype(f32)
    for t in range(TP):
        p[1, 0, t] = (-0.2, -0.1, 0.03 + 0.001 * t, 0.04)
        p[1, 1, t] = (0.5, 0.2 + 0.01 * t, 0.5 + 1.5 / 28.0, 0.8)
        p[1, 2, t] = (0.0, 0.0, 1.0, 1.0)
        p[2, 0, t] = (-0.1, -0.25, 1.2 + 0.01 * t, 1.1)
    return p, np.asarray(PCOUNTS, np.int32)


def scale_tubes_abs(tubes, width, height):
    """utils/tube_utils.py:202-212 on a float64 array"""
    tubes = np.minimum(np.maximum(np.asarray(tubes, f64), 0.0), 1.0)
    for i in range(4):
        tubes[:, :, i] *= float(width) if i % 2 == 0 else float(height)
    return tubes


def host_plan(aug, dims, tubes, proposals, rec):
    """augplan_cases.host_plan with proposals: TubeAugmentation.plan fed the draws the restatement consumed -> the transformed proposals"""
    feed = PC._Feeder(rec["log"], rec["patches"])
    saved = (np.random.uniform, np.random.randint)
    np.random.uniform, np.random.randint = feed.uniform, feed.randint
    try:
        _, _, out = aug.plan((PC.T, dims[0], dims[1]), tubes, proposals=proposals)
    finally:
        np.random.uniform, np.random.randint = saved
    assert feed.at == len(rec["log"]) and feed.pk == len(rec["patches"]), "the host rule consumed fewer draws than the restatement"
    return out


def usable(want, switches, clips=(0, 1, 2)):
    """a restated state the host rule has an answer for: no cap hit, and a clip without ground truths draws `None` as its first crop mode
    (numpy raises on the minimum over no boxes: augplan_cases' header)"""
    cnt = PC.COUNTS
    for n in clips:
        r = want[4][n]
        if r["crop_cap"] or r["erase_cap"] or ((switches & CROP) and cnt[n] == 0 and r["mode_first"] != 0):
            return False
    return True


_OWN = set()


def restated(switches, seed, offset, keep=True):
    """augplan_cases.restated, with the entries THIS module adds to its session cache tracked: a state that is only looked at by a search
    is dropped again at once (keep=False), the others by release() -- the suite runs in one process, and a search over hundreds of states
    would otherwise stay resident under every test that follows"""
    key = (switches, seed, offset, False)
    had = key in PC._RESTATED
    want = PC.restated(switches, seed, offset)
    if not had:
        if keep:
            _OWN.add(key)
        else:
            del PC._RESTATED[key]
    return want


def release():
    """drop this module's entries of augplan_cases' cache"""
    for key in _OWN:
        PC._RESTATED.pop(key, None)
    _OWN.clear()


def _kind(r, dims):
    return (r["crop"] != (0, 0, dims[1], dims[0]), bool(r["mirror"]))


# Found by a CPU search with the restatement alone (find_states below), committed as constants the way augplan_cases commits its cap
# states: the search looks at some 300 states, whose records would stay resident in a suite that runs in one process.
STATES = {0: [(0, 0)], CROP: [(1, 3), (32, 96)], FLIP: [(1, 3), (0, 0)], CROP | FLIP: [(1, 3), (13, 39), (32, 96), (129, 387)],
          ALL: [(1, 3), (13, 39), (32, 96), (129, 387)]}
GRAPH_STATE = (1, 0)


def states():
    """{switches: [(seed, offset), ...]}: per switch combination one usable state for every (cropped, mirrored) outcome of clip 1, the clip
    with real proposals whose crops can be accepted; case_plan_tubes asserts the coverage, so stale constants cannot pass"""
    return STATES


def find_states(limit=400):
    """the search behind STATES: per switch combination the first usable state (seed, 3 seed) of every outcome of clip 1"""
    out = {}
    for sw in SWITCHES:
        kinds, found = 1 << (bool(sw & CROP) + bool(sw & FLIP)), {}
        for seed in range(limit):
            want = restated(sw, seed, 3 * seed, keep=False)
            if usable(want, sw) and _kind(want[4][1], PC.DIMS[1]) not in found:
                found[_kind(want[4][1], PC.DIMS[1])] = (seed, 3 * seed)
            if len(found) == kinds:
                break
        out[sw] = [found[k] for k in sorted(found)]
    return out


def find_graph_state(limit=400):
    """the search behind GRAPH_STATE: the first (seed, 0) whose offsets 0, 2, 4 are all usable for clips 0 and 1 with the four switches on
    and give clip 1 three different (crop, mirror) decisions, so that the HOST rule's three answers differ"""
    for seed in range(limit):
        recs = [restated(ALL, seed, 2 * k, keep=False) for k in range(3)]
        if all(usable(r, ALL, clips=(0, 1)) for r in recs) and len({(r[4][1]["crop"], r[4][1]["mirror"]) for r in recs}) == 3:
            return seed, 0
    raise AssertionError("no seed with three usable, different offsets in a row")


def expected_tubes(switches, seed, offset, props, counts, fill, Wn=PC.WN, Hn=PC.HN, clips=(0, 1, 2)):
    """-> (tubes_out [len(clips),PMAX,TP,4] fp32, tube_count_out): the rule of include/step_amd.h through the HOST rule"""
    gt, cnt = PC.make_gt()
    want = restated(switches, seed, offset)
    assert usable(want, switches, clips), (switches, seed, offset)
    aug = TubeAugmentation((Wn, Hn), PC.MEAN, PC.STDS, bool(switches & FLIP), bool(switches & CROP), bool(switches & PHOTO), bool(switches & ERASE),
                           scale=PC.SCALE)
    Pmax = props.shape[1]
    out = np.empty((len(clips), Pmax, props.shape[2], 4), f32)
    out[:] = (0, 0, Wn, Hn)
    cnt_out = np.zeros(len(clips), np.int32)
    for k, n in enumerate(clips):
        P = min(max(int(counts[n]), 0), Pmax)
        if P == 0 and fill is not None:
            rows = np.repeat(np.asarray(fill[:Pmax], f64)[:, None, :], props.shape[2], axis=1)         # not transformed
        elif P == 0:
            continue
        else:
            rows = host_plan(aug, PC.DIMS[n], gt[n, :int(cnt[n])], props[n, :P].astype(f64), want[4][n])
            assert rows.dtype == f64
        cnt_out[k] = rows.shape[0]
        out[k, :rows.shape[0]] = scale_tubes_abs(rows, Wn, Hn).astype(f32)
    return out, cnt_out


class TubeCall(PC.Call):
    """augplan_cases.Call plus the buffers of step_augment_plan_tubes"""

    def __init__(self, bk, props, counts, fill=FILL):
        gt, cnt = PC.make_gt()
        super().__init__(bk, PC.DIMS, gt, cnt)
        self.Pmax, self.Tp = props.shape[1], props.shape[2]
        self.tubes, self.tcnt = bk.dev(props), bk.dev(np.asarray(counts, np.int32))
        self.fill, self.n_fill = (bk.dev(None), 0) if fill is None else (bk.dev(fill), len(fill))
        self.fresh()

    def fresh(self):
        super().fresh()
        if hasattr(self, "Pmax"):
            self.tubes_out = self.bk.dev(np.full((self.N, self.Pmax, self.Tp, 4), 7, f32))
            self.tcnt_out = self.bk.dev(np.full(self.N, 7, np.int32))

    def untouched(self):
        return super().untouched() and bool(np.all(self.tubes_out.get() == 7) and np.all(self.tcnt_out.get() == 7))

    def run_tubes(self, st, switches, **o):
        a = dict(src=self.src.ptr, dims=self.dims.ptr, gt=self.gt.ptr, cnt=self.cnt.ptr, N=self.N, Gmax=self.Gmax, F=self.F, NC=self.NC,
                 switches=switches, scale=PC.SCALE, Wn=PC.WN, Hn=PC.HN, max_hw=self.max_hw, rng=st.ptr, block=self.block.ptr, gt_out=self.gt_out.ptr,
                 cnt_out=self.cnt_out.ptr, tubes=self.tubes.ptr, tcnt=self.tcnt.ptr, Pmax=self.Pmax, Tp=self.Tp, fill=self.fill.ptr, n_fill=self.n_fill,
                 tubes_out=self.tubes_out.ptr, tcnt_out=self.tcnt_out.ptr)
        a.update(o)
        return self.bk.lib.step_augment_plan_tubes(a["src"], a["dims"], a["gt"], a["cnt"], a["N"], a["Gmax"], a["F"], a["NC"], a["switches"],
                                                   a["scale"], a["Wn"], a["Hn"], a["max_hw"], a["rng"], a["block"], a["gt_out"], a["cnt_out"],
                                                   a["tubes"], a["tcnt"], a["Pmax"], a["Tp"], a["fill"], a["n_fill"], a["tubes_out"], a["tcnt_out"],
                                                   self.bk.stream)


def same_tubes(call, want, what):
    got, cnt = call.tubes_out.get(), call.tcnt_out.get()
    assert np.array_equal(cnt, want[1]), (what, "tube_count_out", cnt, want[1])
    bad = np.argwhere(got.view(np.int32) != want[0].view(np.int32))
    assert bad.size == 0, (what, "tubes_out", bad[:6].tolist(), got[tuple(bad[0][:3])], want[0][tuple(bad[0][:3])])


def case_plan_tubes(bk):
    """switches none / crop / flip / crop + flip / all four, each at the states of `states()`: tubes_out and tube_count_out equal the host
    rule's answer bit for bit; the block, gt_out, gt_count_out and the state are step_augment_plan's at the same state.  The states make a
    clip with real proposals crop, mirror, do both and keep its frame (asserted: a planner that never crops cannot pass), and among the
    cropped ones valid_tubes replaces a proposal by the crop's window somewhere."""
    props, counts = make_props()
    call = TubeCall(bk, props, counts)
    seen, windows = set(), 0
    for sw in SWITCHES:
        for seed, offset in states()[sw]:
            call.fresh()
            st = PC._state(bk, seed, offset)
            assert call.run_tubes(st, sw) == 0
            want = restated(sw, seed, offset)
            PC.same_outputs(call, want, (sw, seed, offset))
            assert PC._read_state(st) == (seed, offset + 2)
            exp = expected_tubes(sw, seed, offset, props, counts, FILL)
            same_tubes(call, exp, (sw, seed, offset))
            assert exp[1].tolist() == [2, 3, 5]
            for n in (1, 2):
                seen.add(_kind(want[4][n], PC.DIMS[n]))
            r = want[4][1]
            if r["crop"] != (0, 0, PC.DIMS[1][1], PC.DIMS[1][0]):               # the sliver in the corner: outside the crop, so the crop's window
                b = exp[0][1, 0, 0]
                windows += int(b[2] - b[0] > 0.9 * PC.WN and b[3] - b[1] > 0.9 * PC.HN)
    assert seen == {(False, False), (True, False), (False, True), (True, True)}, seen
    assert windows >= 2, windows


def case_plan_tubes_null_is_plan(bk):
    """tubes_in == NULL is step_augment_plan: the same block, ground truths and offset from both entries, the tube outputs untouched"""
    props, counts = make_props()
    call = TubeCall(bk, props, counts)
    for sw in (ALL, CROP):
        seed, offset = states()[sw][0]
        want = restated(sw, seed, offset)
        st = PC._state(bk, seed, offset)
        call.fresh()
        assert call.run_tubes(st, sw, tubes=None) == 0
        PC.same_outputs(call, want, "tubes_in NULL")
        assert PC._read_state(st) == (seed, offset + 2)
        assert np.all(call.tubes_out.get() == 7) and np.all(call.tcnt_out.get() == 7)
        blk = call.block.get().copy()
        st = PC._state(bk, seed, offset)
        call.fresh()
        assert call.run(st, sw) == 0
        PC.same_outputs(call, want, "step_augment_plan")
        head = call.L["patch_base"]
        assert np.array_equal(call.block.get()[:head], blk[:head])
        assert call.run_tubes(st, sw, tubes=None, tcnt=None, Pmax=-1, Tp=0, fill=None, n_fill=-1, tubes_out=None, tcnt_out=None) == 0     # (not read)


def case_plan_tubes_counts_and_fill(bk):
    """counts outside [0, Pmax] are clamped; a fill longer than Pmax is cut to Pmax rows; without a fill a clip without proposals gets
    count 0 and whole-frame rows only; another network resolution"""
    props, _ = make_props()
    sw = CROP | FLIP
    seed, offset = states()[sw][-1]
    long_fill = np.concatenate([FILL] * 4)[:7].copy()
    long_fill[2:] += f32(0.01)
    for counts, fill in (((-3, 9, 5), FILL), ((0, 3, 0), long_fill), ((0, 3, 5), None)):
        call = TubeCall(bk, props, counts, fill)
        st = PC._state(bk, seed, offset)
        assert call.run_tubes(st, sw) == 0
        exp = expected_tubes(sw, seed, offset, props, counts, fill)
        same_tubes(call, exp, (counts, None if fill is None else len(fill)))
        PC.same_outputs(call, restated(sw, seed, offset), counts)
    assert exp[1].tolist() == [0, 3, 5] and np.array_equal(exp[0][0], np.tile(np.array([0, 0, PC.WN, PC.HN], f32), (PMAX, TP, 1)))
    call = TubeCall(bk, props, PCOUNTS)
    st = PC._state(bk, seed, offset)
    assert call.run_tubes(st, sw, Wn=400, Hn=320) == 0
    same_tubes(call, expected_tubes(sw, seed, offset, props, PCOUNTS, FILL, 400, 320), "400 x 320")


def case_plan_tubes_refusals(bk):
    """Pmax < 0, Tp < 1, n_fill < 0 -> STEP_E_SHAPE; Pmax > 1024 -> STEP_E_UNSUPPORTED; tubes_in with tube_count, tubes_out or
    tube_count_out NULL -> STEP_E_NULL; step_augment_plan's own refusals still come first.  Nothing is written, the offset stays."""
    props, counts = make_props()
    call = TubeCall(bk, props, counts)
    st = PC._state(bk, 5, 9)
    for want, o in ((E_SHAPE, dict(Pmax=-1)), (E_SHAPE, dict(Tp=0)), (E_SHAPE, dict(n_fill=-1)), (E_UNSUPPORTED, dict(Pmax=1025)),
                    (E_NULL, dict(tcnt=None)), (E_NULL, dict(tubes_out=None)), (E_NULL, dict(tcnt_out=None)), (E_SHAPE, dict(switches=16)),
                    (E_NULL, dict(rng=None)), (E_NULL, dict(block=None))):
        assert call.run_tubes(st, o.pop("switches", ALL), **o) == want, (want, o)
        assert call.untouched() and PC._read_state(st) == (5, 9), o


PLAN_CASES = ["case_plan_tubes", "case_plan_tubes_null_is_plan", "case_plan_tubes_counts_and_fill", "case_plan_tubes_refusals"]


# ---- the counted selection -------------------------------------------------------------------------------------------------------------------
SB, SK, SG, SNC = 3, 6, 2, 4
SCOUNTS = (0, 2, 6)


def padded_inputs(seed, counts=SCOUNTS, score=False, iou=False, Tw=0):
    """-> (padded, compact): B = 3 clips of K = 6 slots, G = 2, NC = 4.  The slots past a clip's count are DECOYS: a copy of one of the
    clip's ground-truth boxes with the highest score of the clip (and IoU 1 in a prepared table) -- a kernel that ignores the count
    selects them first.  `compact` holds the real rows alone, clip_start their running sum: what select_cases.restate is run on."""
    rs = np.random.RandomState(seed)
    inp = SC.make_inputs(rs, [SK] * SB, [SG] * SB, NC=SNC, Tw=Tw, score=score, near=0.7)
    N = SB * SK
    if iou:
        inp["iou"] = np.array([[SC.box_iou_f32(inp["gt"][n // SK, g, 1, :4], inp["cand"][n, 1]) for g in range(SG)] for n in range(N)], f32)
    real = np.zeros(N, bool)
    for b in range(SB):
        c = min(max(int(counts[b]), 0), SK)
        real[b * SK:b * SK + c] = True
        for a in range(c, SK):
            n, g = b * SK + a, a % SG
            inp["cand"][n] = inp["gt"][b, g, 1, :4]
            if Tw:
                inp["first"][n] = inp["gt"][b, g, 1, :4]
                inp["last"][n] = inp["gt"][b, g, 1, :4]
            if score:
                inp["score"][n] = inp["score"][b * SK:(b + 1) * SK].max() + f32(0.25)
            if iou:
                inp["iou"][n] = 0.0
                inp["iou"][n, g] = 1.0
    compact = dict(inp)
    for k in ("cand", "first", "last", "score", "iou"):
        if k in inp:
            compact[k] = np.ascontiguousarray(inp[k][real])
    kept = [int(real[b * SK:(b + 1) * SK].sum()) for b in range(SB)]
    compact["clip_start"] = np.concatenate(([0], np.cumsum(kept))).astype(np.int32)
    return inp, compact


def call_counted(bk, inp, prm, st, counts, use_plain=False):
    """one step_select_train_counted call (clip_count = counts, None: NULL; use_plain: step_select_train itself) -> the five outputs"""
    g = lambda k: inp.get(k)
    B = len(inp["clip_start"]) - 1
    N, Tc = inp["cand"].shape[:2]
    Tw = g("first").shape[1] if g("first") is not None else 0
    Tout = Tc + 2 * Tw
    Gmax, F, NC = inp["gt"].shape[1], inp["gt"].shape[2], inp["gt"].shape[3] - 4
    K = B * prm["budget"]
    bufs = {k: bk.dev(np.ascontiguousarray(g(k))) if g(k) is not None else bk.dev(None) for k in
            ("cand", "first", "last", "score", "iou", "clip_start", "gt", "gt_count", "pad")}
    cc = bk.dev(None if counts is None else np.asarray(counts, np.int32))
    out = [bk.dev(np.full((K, Tout, 5), 7, f32)), bk.dev(np.full((K, 3, 6 + NC), 7, f32)), bk.dev(np.full((K, 1), 7, f32)),
           bk.dev(np.full((1,), 7, f32)), bk.dev(np.full((B, 2), 7, np.int32))]
    head = (bufs["cand"].ptr, bufs["first"].ptr, bufs["last"].ptr, bufs["score"].ptr, bufs["iou"].ptr, N, Tc, Tw, NC, bufs["clip_start"].ptr, B,
            prm["amax"], bufs["gt"].ptr, bufs["gt_count"].ptr, Gmax, F, bufs["pad"].ptr, st.ptr, prm["mid"], prm["before"], prm["after"], prm["topk"],
            prm["cls_thresh"], prm["reg_thresh"], prm["max_pos_num"], prm["neg_ratio"], prm["sampling"], prm["budget"], out[0].ptr, out[1].ptr,
            out[2].ptr, out[3].ptr, out[4].ptr)
    rc = bk.lib.step_select_train(*head, bk.stream) if use_plain else bk.lib.step_select_train_counted(*head, cc.ptr, bk.stream)
    assert rc == 0, rc
    return [o.get().copy() for o in out]


def check_counted(bk, padded, compact, prm, counts, seed, offset, cprm=None):
    """counted kernel on the padded inputs == restatement on the compacted ones; the offset ends one further -> the restatement"""
    want = SC.restate(compact, cprm or prm, seed, offset)
    if prm["sampling"] == 2:
        assert want[5] > 1e-9, ("a softmax draw within 1e-9 of a running sum: pick another seed", want[5])
    st = SC._state(bk, seed, offset)
    got = call_counted(bk, padded, prm, st, counts)
    for nm, a, b in zip(SC.NAMES, got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, (nm, a.shape, b.shape)
        assert np.array_equal(a, b), (nm, np.argwhere(a != b)[:5].tolist(), got[4].tolist(), want[4].tolist())
    assert SC._read_state(st) == (seed, offset + 1)
    return want


def no_decoy(sel, padded, counts):
    """no selected row (column 1-4 of its middle frame) is a padded slot's box"""
    budget = sel.shape[0] // SB
    for b in range(SB):
        c = min(max(int(counts[b]), 0), SK)
        decoys = {padded["cand"][b * SK + a, 1].tobytes() for a in range(c, SK)}
        for r in range(budget):
            assert sel[b * budget + r, sel.shape[1] // 2, 1:].tobytes() not in decoys, (b, r)


def case_counted_forms(bk):
    """step 1 (score and iou NULL), a later step with scores and the prepared IoU table in the three samplings, and a growing step (Tout =
    9): outputs and state equal the restatement on the compacted inputs; clip 0 (count 0) selects nothing, no decoy is ever selected."""
    prm = SC.params(cls_thresh=0.3, reg_thresh=0.2)
    padded, compact = padded_inputs(31)
    want = check_counted(bk, padded, compact, prm, SCOUNTS, 0x1_0000_0007, 5)
    assert want[4][0].sum() == 0 and want[4][1, 0] == 2 and want[4][2].sum() >= 4
    no_decoy(want[0], padded, SCOUNTS)
    for sampling in (0, 1, 2):
        padded, compact = padded_inputs(32, score=True, iou=True)
        want = check_counted(bk, padded, compact, dict(prm, sampling=sampling, before=0, after=2), SCOUNTS, 77 + sampling, sampling)
        no_decoy(want[0], padded, SCOUNTS)
    padded, compact = padded_inputs(33, score=True, iou=True, Tw=3)
    want = check_counted(bk, padded, compact, prm, SCOUNTS, 91, 2)
    assert want[0].shape[1] == 9 and want[4][2].sum() >= 4
    no_decoy(want[0], padded, SCOUNTS)


def case_counted_null_is_select_train(bk):
    """clip_count == NULL is step_select_train on the same (padded) inputs -- which selects decoys, so the count is what keeps them out"""
    prm = SC.params(cls_thresh=0.3, reg_thresh=0.2)
    padded, compact = padded_inputs(32, score=True, iou=True)
    outs = []
    for plain in (False, True):
        st = SC._state(bk, 12, 3)
        outs.append(call_counted(bk, padded, prm, st, None, use_plain=plain))
        assert SC._read_state(st) == (12, 4)
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    want = SC.restate(padded, prm, 12, 3)
    for nm, a, b in zip(SC.NAMES, outs[0], want):
        assert np.array_equal(a, b), nm
    counted = call_counted(bk, padded, prm, SC._state(bk, 12, 3), SCOUNTS)
    assert outs[0][4][0].sum() > 0 and counted[4][0].sum() == 0                 # clip 0: all decoys against nothing


def case_counted_clamps(bk):
    """a count above the segment is the segment, a negative count selects nothing, and Amax cuts a count like it cuts a segment"""
    prm = SC.params(cls_thresh=0.3, reg_thresh=0.2)
    padded, compact = padded_inputs(34, counts=(6, 6, 0), score=True, iou=True)
    want = check_counted(bk, padded, compact, prm, (9, 7, -3), 21, 0)
    assert want[4][0].sum() >= 4 and want[4][2].sum() == 0
    padded, compact = padded_inputs(35, counts=(4, 2, 4), score=True, iou=True)
    want = check_counted(bk, padded, compact, dict(prm, amax=4), (6, 2, 5), 22, 1, cprm=prm)
    no_decoy(want[0], padded, (4, 2, 4))


SELECT_CASES = ["case_counted_forms", "case_counted_null_is_select_train", "case_counted_clamps"]
KERNEL_CASES = PLAN_CASES + SELECT_CASES


def run_kernel_case(name, bk):
    return globals()[name](bk)


# ---- the host ----------------------------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "proposals_golden.npz")


def case_read_proposals(tmp_path):
    """selection.read_proposals == the reference's get_proposals on the fixture's text (tools/make_proposals_golden.py): the `<` of the score
    filter, one copy of a box repeated in its frame, first-seen order, the score in the last column whatever stands before it"""
    from step_amd.selection import read_proposals

    g = np.load(GOLDEN)
    path = os.path.join(str(tmp_path), "proposals.csv")
    with open(path, "w") as f:
        f.write(str(g["text"]))
    res = read_proposals(path)
    rows = [(v, k, b) for v, frames in res.items() for k, boxes in frames.items() for b in boxes]
    assert [r[0] for r in rows] == g["video"].tolist() and [r[1] for r in rows] == g["fid"].tolist()
    assert np.array_equal(np.array([r[2] for r in rows], f64), g["box"])
    assert len(rows) == 7 and set(res) == {"vidA", "vidB"} and all(isinstance(v, float) for r in rows for v in r[2])
    assert sum(len(b) for fr in read_proposals(path, min_score=0.0).values() for b in fr.values()) == 8     # only the in-frame repeats go


# ---- the modules ---------------------------------------------------------------------------------------------------------------------------------
def module_selector_counted(device):
    """DeviceSelector.select(clip_count=...) for the three steps of the default NUM_CHUNKS on padded clips (K = 12 slots, counts 9, 0, 12;
    decoys behind the counts in the initial tubes and in the history) against the restatement fed with the REAL rows of
    step_select_prepare's outputs, which runs over all slots"""
    import torch

    import step_amd
    from step_amd import ops
    from step_amd.selection import DeviceSelector

    rs = np.random.RandomState(23)
    K, counts, gts = 12, [9, 0, 12], [2, 1, 3]
    a = SC.cfg()
    inp, _, _, flat, hist = SC._module_inputs(rs, [K] * 3, gts, a.num_classes, near=0.7, spread=12)
    real = np.zeros(3 * K, bool)
    for b in range(3):
        real[b * K:b * K + counts[b]] = True
        for s in range(counts[b], K):
            n = b * K + s
            flat[n] = inp["gt"][b, s % gts[b], 1, :4]
            for h in hist:
                h["pred_prob"][n] = 1.0
                for key in ("pred_loc", "pred_first_loc", "pred_last_loc"):
                    h[key][n] = torch.from_numpy(inp["gt"][b, s % gts[b], 1, :4])
    rng = step_amd.DeviceRNG(device, seed=41)
    selr = DeviceSelector(a, 3, 15, device, rng)
    gt, gt_count, init_flat, clip_start, pads, dhist = SC._device_args(device, inp, flat, hist, a)
    clip_count = torch.tensor(counts, dtype=torch.int32, device=device)
    clip_of = torch.from_numpy(np.repeat(np.arange(3), K).astype(np.int32)).to(device)
    cstart = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    decoys = {flat[n, 1].tobytes() for n in np.flatnonzero(~real)}
    for step in (1, 2, 3):
        out = selr.select(step, dhist[step - 2] if step > 1 else None, gt, gt_count, init_flat, clip_start, pads[step], max_tubes=K,
                          clip_count=clip_count)
        assert all(o is s for o, s in zip(out, selr.out[step])) and rng.offset() == step
        r = dict(inp, cand=flat[real], pad=SC.np_(pads[step]), clip_start=cstart)
        prm = SC.params(cls_thresh=a.cls_thresh[step - 1], reg_thresh=a.reg_thresh[step - 1], before=0 if step == 2 else -1, after=2 if step == 2 else -1)
        if step > 1:
            h = dhist[step - 2]
            score, vloc, vfirst, vlast, iou = ops.select_prepare(h["pred_prob"], h["pred_loc"], h["pred_first_loc"], h["pred_last_loc"], clip_of,
                                                                 gt[:, :, 1, :4].contiguous(), gt_count, 400.0, 400.0)
            r.update(cand=SC.np_(vloc)[real], score=SC.np_(score)[real], iou=SC.np_(iou)[real])
            if step == 3:
                r.update(first=SC.np_(vfirst)[real], last=SC.np_(vlast)[real])
        want = SC.restate(r, prm, 41, step - 1)
        assert want[5] > 1e-9, want[5]
        for nm, g_, w_ in zip(SC.NAMES, out, want):
            assert np.array_equal(SC.np_(g_), w_), (step, nm)
        assert want[4][1].sum() == 0 and want[4].sum() > 8
        if step == 1:
            sel = SC.np_(out[0])
            assert not any(sel[k, 1, 1:].tobytes() in decoys for k in range(sel.shape[0]))
    with_null = [SC.np_(t).copy() for t in selr.select(1, None, gt, gt_count, init_flat, clip_start, pads[1], max_tubes=K)]
    assert with_null[4][1].sum() > 0                                            # without the count clip 1's decoys are tubes like any other


def apply_inputs(device, clips=(0, 1, 2)):
    import torch

    gt, cnt, frames, d_gt, d_cnt = PC.module_inputs(device)
    props, counts = make_props()
    k = list(clips)
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)
    return ([frames[n] for n in k], d_gt[k].contiguous(), d_cnt[k].contiguous(), to(props[k]), to(counts[k]), to(FILL)), (props, counts)


def module_apply_tubes(device):
    """DeviceTubeAugmentation.apply(tubes=...) with all four switches at a state of the kernel case: five tensors come back, the last two
    equal the kernel case's expectation, the first three are what apply() returns without tubes (block, pixels and ground truths checked
    by augplan_cases.check_apply); tubes_out= / tube_count_out= are filled in place; the stray arguments of a call without tubes raise"""
    import pytest
    import torch

    import step_amd
    (clips, d_gt, d_cnt, d_props, d_pcnt, d_fill), (props, counts) = apply_inputs(device)
    gt, cnt = PC.make_gt()
    seed, offset = states()[ALL][-1]
    rng = step_amd.DeviceRNG(device, seed=seed)
    rng.set_state((seed, offset))
    aug = step_amd.DeviceTubeAugmentation((PC.WN, PC.HN), PC.MEAN, PC.STDS, True, True, True, True, scale=PC.SCALE, rng=rng)
    res = aug.apply(clips, d_gt, d_cnt, tubes=d_props, tube_count=d_pcnt, fill=d_fill)
    assert len(res) == 5 and rng.get_state() == (seed, offset + 2)
    PC.check_apply(aug, res[:3], seed, offset, PC._frames(), gt, cnt)
    exp = expected_tubes(ALL, seed, offset, props, counts, FILL)
    assert np.array_equal(res[3].cpu().numpy().view(np.int32), exp[0].view(np.int32)) and np.array_equal(res[4].cpu().numpy(), exp[1])
    t_out, c_out = torch.full_like(d_props, 7.0), torch.full_like(d_pcnt, 7)
    rng.set_state((seed, offset))
    res = aug.apply(clips, d_gt, d_cnt, tubes=d_props, tube_count=d_pcnt, fill=d_fill, tubes_out=t_out, tube_count_out=c_out)
    assert res[3] is t_out and res[4] is c_out and np.array_equal(t_out.cpu().numpy().view(np.int32), exp[0].view(np.int32))
    assert len(aug.apply(clips, d_gt, d_cnt)) == 3
    state = rng.get_state()
    for bad in (lambda: aug.apply(clips, d_gt, d_cnt, tube_count=d_pcnt), lambda: aug.apply(clips, d_gt, d_cnt, fill=d_fill),
                lambda: aug.apply(clips, d_gt, d_cnt, tubes=d_props), lambda: aug.apply(clips, d_gt, d_cnt, tubes=d_props.double(), tube_count=d_pcnt),
                lambda: aug.apply(clips, d_gt, d_cnt, tubes=d_props, tube_count=d_pcnt.long()),
                lambda: aug.apply(clips, d_gt, d_cnt, tubes=d_props, tube_count=d_pcnt, tubes_out=t_out[:, :2])):
        with pytest.raises(RuntimeError):
            bad()
    assert rng.get_state() == state


def padded_history(rs, K, counts, NC=6, Tl=3, iters=2):
    """a synthetic padded history (no network): random pred_prob / pred_loc over B * K slots, the slots behind a clip's count DECOYS with
    score 1 on a box of their own -> (padded history as numpy dicts, the same history sliced to its real rows with tubes_nums = counts)"""
    B = len(counts)
    N = B * K
    real = np.zeros(N, bool)
    for b in range(B):
        real[b * K:b * K + counts[b]] = True
    pad, cut = [], []
    for _ in range(iters):
        prob = rs.rand(N, 1, NC).astype(f32) ** 3
        loc = (SC.rand_boxes(rs, N)[:, None, :] + rs.uniform(-3, 3, (N, Tl, 4))).astype(f32)
        loc[::3, :, :] -= 40.0                                                  # some boxes leave the frame: valid_tubes clamps them
        prob[~real] = 1.0
        prob = np.repeat(prob, Tl, axis=1)
        pad.append({"pred_prob": prob, "pred_loc": loc, "tubes_nums": [K] * B})
        cut.append({"pred_prob": np.ascontiguousarray(prob[real]), "pred_loc": np.ascontiguousarray(loc[real]), "tubes_nums": list(counts)})
    return pad, cut


def module_postprocess_padded(device):
    """postprocess and postprocess_merged on a padded history (B = 2, K = 5, counts (2, 5) and then (0, 3) through the SAME count tensor
    rewritten in place, decoy slots with score 1) equal, bit for bit, the existing functions on the history sliced to its real rows with
    tubes_nums = counts; the `tubes` they return are slot numbers, the real tubes' own indices.  train_select refuses such a history."""
    import pytest
    import torch
    from types import SimpleNamespace as NS

    from step_amd import driver
    from step_amd.selection import train_select

    args = NS(image_size=(400, 400), conf_thresh=0.05, nms_thresh=0.4, evaluate_topk=-1, topk=-1)
    rs = np.random.RandomState(5)
    K = 5
    count = torch.zeros(2, dtype=torch.int32, device=device)
    rows = 0
    for counts in ((2, 5), (0, 3)):
        pad, cut = padded_history(rs, K, counts)
        to = lambda h: {k: (torch.from_numpy(v).to(device) if isinstance(v, np.ndarray) else v) for k, v in h.items()}
        pad, cut = [to(h) for h in pad], [to(h) for h in cut]
        count.copy_(torch.tensor(counts, dtype=torch.int32))
        for h in pad:
            h["tubes_count"] = count
        for kw in (dict(), dict(evaluate_topk=1, topk=6)):
            got, want = driver.postprocess(args, pad, **kw), driver.postprocess(args, cut, **kw)
            for gi, wi in zip(got, want):
                for gd, wd, c in zip(gi, wi, counts):
                    for key in ("boxes", "scores", "labels", "tubes"):
                        assert torch.equal(gd[key], wd[key]), (counts, kw, key)
                    assert gd["boxes"].dtype == torch.float32 and (gd["tubes"] < c).all()
                    rows += int(gd["tubes"].numel())
            got, want = driver.postprocess_merged(args, pad, **kw), driver.postprocess_merged(args, cut, **kw)
            for gi, wi in zip(got, want):
                for gd, wd in zip(gi, wi):
                    for key in ("boxes", "cluster", "labels", "scores", "tubes"):
                        assert torch.equal(gd[key], wd[key]), (counts, kw, key)
        plain = driver.postprocess(args, [{k: v for k, v in pad[0].items() if k != "tubes_count"}])
        assert sum(int((d["tubes"] >= c).sum()) for d, c in zip(plain[0], counts)) > 0       # without the count the decoys are detections
    assert rows > 20, rows
    with pytest.raises(ValueError):
        train_select(2, pad[0], None, None, NS(temporal_mode="predict"))


def module_pad_tubes(device):
    """driver.pad_tubes: the slots of a ragged list -- real tubes first, then the whole frame, the frame-index column of _flat_tubes --
    and the count; an empty clip may be an empty list; more tubes than slots raise ValueError"""
    import pytest
    import torch

    from step_amd import driver

    rs = np.random.RandomState(2)
    tubes = [rs.uniform(0, 300, (3, 4, 4)).astype(f32), np.zeros((0, 4, 4), f32), rs.uniform(0, 300, (5, 4, 4)).astype(f32)]
    flat, count = driver.pad_tubes(tubes, 5, device, 400, 320)
    assert tuple(flat.shape) == (15, 4, 5) and flat.dtype == torch.float32 and count.dtype == torch.int32 and count.tolist() == [3, 0, 5]
    ref, nums = driver._flat_tubes([torch.from_numpy(t) for t in tubes], "cpu")
    flat = flat.cpu().numpy().reshape(3, 5, 4, 5)
    assert np.array_equal(flat[0, :3], ref[:3].numpy()) and np.array_equal(flat[2], ref[3:].numpy())
    whole = np.array([0, 0, 400, 320], f32)
    assert np.all(flat[0, 3:, :, 1:] == whole) and np.all(flat[1, :, :, 1:] == whole)
    assert np.array_equal(flat[1, :, :, 0], np.tile(np.arange(4, 8, dtype=f32), (5, 1)))
    assert driver.pad_tubes([tubes[0], [], tubes[2]], 5, device, 400, 320)[1].tolist() == [3, 0, 5]
    with pytest.raises(ValueError):
        driver.pad_tubes(tubes, 4, device, 400, 320)


MODULE_CASES = ["module_selector_counted", "module_apply_tubes", "module_postprocess_padded", "module_pad_tubes"]
