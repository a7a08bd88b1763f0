"""Cases for the fused detection tail on clips of MORE than 64 tubes (step_detect_nms' workgroup form, 64 < kmax <= 1024, and its routing
in step_amd.driver.postprocess / postprocess_merged / classified_rows), driven on the host interpreter by tests/test_emul_detect.py and
on the real library by tests/test_gpu_detect.py.  References: a numpy restatement around oracle.nms_batched (bit-exact to the
reference's C++ operator) for the kernel, tests/golden/detect_block_golden.npz (the reference's own test.py loop on a seeded history
of 84 / 65 / 0 / 109 tubes per clip, tools/make_detect_golden.py) and the general path of the driver for the modules.

Kernel cases take a backend of tests/backends.py; module cases take a device string ("cpu" under the interpreter patch, "cuda").
Everything is exactly specified (fp32 operations rounded one by one), so every comparison is equality."""
import contextlib
import ctypes
import types

import numpy as np
import torch

import oracle
from tests import merge_cases as MG

f32 = np.float32
W, H = 400.0, 300.0
CONF, THR = 0.01, 0.4


# ---- the numpy restatement -----------------------------------------------------------------------------------------------------------
def np_valid_boxes(loc, width, height):
    """valid_tubes on [n,4] fp32 boxes: clamp with NaN propagation (np.maximum / np.minimum), then the whole frame where the box is under
    3 px in either direction -- a NaN coordinate fails the `<` test, so such a box becomes the whole frame too"""
    loc = np.asarray(loc, f32)
    with np.errstate(invalid="ignore"):
        x1, y1 = np.maximum(f32(0), loc[:, 0]), np.maximum(f32(0), loc[:, 1])
        x2, y2 = np.minimum(f32(width), loc[:, 2]), np.minimum(f32(height), loc[:, 3])
        ok = (x1 < x2 - f32(2)) & (y1 < y2 - f32(2))
    out = np.stack([x1, y1, x2, y2], 1).astype(f32)
    out[~ok] = np.asarray([0, 0, width, height], f32)
    return out


def np_detect(prob, loc, nums, kmax, NC, conf=CONF, thr=THR, width=W, height=H):
    """keep [B,NC,kmax] uint8 and the clamped boxes [N,4]: mask `> conf`, valid_tubes, oracle.nms_batched on the COMPACTED masked boxes
    (their order kept), scattered back to the original slots.  Also returns the masked and kept counts per group [B,NC]."""
    B = len(nums)
    start = np.cumsum([0] + list(nums))
    keep = np.zeros((B, NC, kmax), np.uint8)
    boxes = np_valid_boxes(loc, width, height)
    masked = np.zeros((B, NC), np.int64)
    for b in range(B):
        n = min(nums[b], kmax)
        rows = np.arange(start[b], start[b] + n)
        for c in range(NC):
            s = prob[rows, c]
            with np.errstate(invalid="ignore"):
                idx = np.flatnonzero(s > f32(conf))                                # (a NaN score is never masked)
            masked[b, c] = len(idx)
            if len(idx):
                k = oracle.nms_batched(boxes[rows[idx]][None], s[idx][None], [len(idx)], thr)[0]
                keep[b, c, idx[k.astype(bool)]] = 1
    return keep, boxes, masked, keep.sum(2)


def detect_inputs(seed, nums, NC, prob_cols=None):
    """Seeded tubes shaped like oracle.make_golden.postprocess_history: coordinates outside the frame, sizes under 3 px and negative, clusters
    of overlapping boxes, two NaN coordinates; scores that are multiples of 1/6 (many exact ties, many zeros under conf); class 1: every
    tube at 0.5 (all masked, all tied); class 2 (where there is one): nothing above conf; one NaN score.  prob [N, prob_cols] (columns
    past NC hold a score that must not be read: 1.0), loc3 [N,3,4] whose MIDDLE frame is the one that counts."""
    rs = np.random.RandomState(seed)
    N = int(sum(nums))
    cols = NC if prob_cols is None else prob_cols
    xy = rs.uniform(-30, 330, (N, 2))
    wh = rs.uniform(-5, 90, (N, 2))                                      # (smaller than postprocess_history: ~100 tubes keep > 64 of a tied class)
    mid = np.concatenate([xy, xy + wh], 1).astype(f32)
    mid[rs.rand(N) < 0.3] += rs.uniform(0, 120, (1, 4)).astype(f32)
    prob = np.ones((N, cols), f32)
    prob[:, :NC] = (rs.randint(0, 7, (N, NC)) / 6.0 * (rs.rand(N, NC) < 0.6)).astype(f32)
    if NC > 1:
        prob[:, 1] = 0.5
    if NC > 2:
        prob[:, 2] = rs.choice([0.0, 0.005, 0.01], N).astype(f32)                 # (0.01 rounded to fp32 is not > fp32(0.01))
    if N:
        mid[rs.randint(N), 0] = np.nan
        mid[rs.randint(N), 3] = np.nan
        prob[rs.randint(N), 0] = np.nan
    loc3 = np.stack([mid + f32(7), mid, mid - f32(5)], 1).astype(f32)
    return prob, loc3


def _ptr_at(buf, nbytes):
    p = buf.ptr
    if isinstance(p, ctypes.c_void_p):
        return ctypes.c_void_p(p.value + nbytes)
    return p + nbytes


def run_detect(bk, prob, loc, nums, kmax, NC, conf=CONF, thr=THR, loc_stride=4, loc_off=0, width=W, height=H):
    """step_detect_nms through the C ABI; keep and boxes_out are pre-filled with 9 / -9 so that every slot is seen to be written.
    loc: the buffer of box rows, row stride loc_stride floats, first box at float loc_off."""
    B, N = len(nums), int(sum(nums))
    start = (np.cumsum(nums) - np.asarray(nums)).astype(np.int32) if B else np.zeros(0, np.int32)
    dp, dl = bk.dev(prob), bk.dev(loc)
    ds, dn = bk.dev(start), bk.dev(np.asarray(nums, np.int32))
    keep, out = bk.dev(np.full((B, NC, kmax), 9, np.uint8)), bk.dev(np.full((max(N, 1), 4), -9, f32))
    rc = bk.lib.step_detect_nms(dp.ptr, prob.shape[1], NC, _ptr_at(dl, 4 * loc_off), loc_stride, ds.ptr, dn.ptr, B, kmax, conf, thr, width, height,
                                keep.ptr, out.ptr, bk.stream)
    assert rc == 0, rc
    return keep.get(), out.get()[:N]


# ---- kernel cases --------------------------------------------------------------------------------------------------------------------
SHAPES = (((65, 0, 109), 109, 5), ((256, 255), 256, 3), ((257, 1), 257, 3), ((1024,), 1024, 2), ((64, 40, 3), 128, 4))


def case_detect_block_restatement(bk, golden):
    """The workgroup form against the numpy restatement, keep flags and clamped boxes bit for bit: 65 / 109 tubes with an empty clip, 256
    (every thread one slot) and 255, 257 (one slot in the second round) next to a clip of one tube, 1024 (the limit: sixteen bitmap words,
    four slots per thread), few tubes under a large kmax.  Wherever a clip has more than 64 tubes the inputs are held to give a group with
    more than 64 masked tubes AND a group that keeps more than 64, so the case cannot pass on wave-sized work."""
    for k, (nums, kmax, NC) in enumerate(SHAPES):
        prob, loc3 = detect_inputs(40 + k, nums, NC)
        mid = np.ascontiguousarray(loc3[:, 1])
        want, wbox, masked, kept = np_detect(prob, mid, nums, kmax, NC)
        print("shape", nums, kmax, NC, "masked per group: max %d, kept per group: max %d, groups without a masked tube %d"
              % (masked.max(), kept.max(), int((masked == 0).sum())))
        if max(nums) > 64:
            assert masked.max() > 64 and kept.max() > 64, (nums, masked.max(), kept.max())
        else:
            assert masked.max() == 64                                               # (the all-tied class of the 64-tube clip)
        if NC > 2:
            assert (masked[:, 2] == 0).all()
        got, gbox = run_detect(bk, prob, mid, nums, kmax, NC)
        assert np.array_equal(got, want), (nums, kmax, NC, np.argwhere(got != want)[:8])
        assert np.array_equal(gbox, wbox, equal_nan=True) and not np.isnan(gbox).any(), (nums, kmax, NC)
        # more tubes than kmax: the slots past kmax are not looked at
        if kmax == 109:
            got2, _ = run_detect(bk, prob, mid, nums, 80, NC)
            want2 = np_detect(prob, mid, nums, 80, NC)[0]
            assert np.array_equal(got2, want2)


def case_detect_wave_and_block_agree(bk, golden):
    """The same clips of at most 64 tubes at kmax = 64 (one wavefront per group) and at kmax = 65 and 128 (one workgroup per group): the
    flags of the first 64 slots and the clamped boxes are identical, the slots past 64 are cleared."""
    nums, NC = (64, 33, 0, 1, 17), 4
    prob, loc3 = detect_inputs(50, nums, NC)
    mid = np.ascontiguousarray(loc3[:, 1])
    k64, b64 = run_detect(bk, prob, mid, nums, 64, NC)
    assert np.array_equal(k64, np_detect(prob, mid, nums, 64, NC)[0]) and k64.sum() > 40
    for kmax in (65, 128):
        k, b_ = run_detect(bk, prob, mid, nums, kmax, NC)
        assert np.array_equal(k[:, :, :64], k64), kmax
        assert not k[:, :, 64:].any(), kmax
        assert np.array_equal(b_, b64), kmax


def case_detect_block_strided(bk, golden):
    """Rows as the driver hands them over: prob_stride = NC + 3 (the columns past NC hold 1.0 and must not be read as a class) and
    loc_stride = 12 from the middle frame of a [N,3,4] tensor."""
    nums, kmax, NC = (70, 5, 100), 100, 5
    prob, loc3 = detect_inputs(66, nums, NC, prob_cols=NC + 3)
    mid = np.ascontiguousarray(loc3[:, 1])
    want, wbox, masked, kept = np_detect(prob, mid, nums, kmax, NC)
    assert masked.max() > 64 and kept.max() > 64
    got, gbox = run_detect(bk, prob, loc3, nums, kmax, NC, loc_stride=12, loc_off=4)
    assert np.array_equal(got, want) and np.array_equal(gbox, wbox)


def case_detect_block_status(bk, golden):
    """status codes: kmax = 1024 is accepted, 1025 is STEP_E_UNSUPPORTED; a NULL keep with work to do is STEP_E_NULL; B = 0 is STEP_OK
    and writes nothing."""
    nums, NC = (3,), 2
    prob, loc3 = detect_inputs(70, nums, NC)
    mid = np.ascontiguousarray(loc3[:, 1])
    k, _ = run_detect(bk, prob, mid, nums, 1024, NC)
    assert np.array_equal(k, np_detect(prob, mid, nums, 1024, NC)[0])
    dp, dl, ds, dn = bk.dev(prob), bk.dev(mid), bk.dev(np.zeros(1, np.int32)), bk.dev(np.asarray(nums, np.int32))
    keep, out = bk.dev(np.full((1, NC, 1025), 9, np.uint8)), bk.dev(np.full((3, 4), -9, f32))
    fn = bk.lib.step_detect_nms
    assert fn(dp.ptr, NC, NC, dl.ptr, 4, ds.ptr, dn.ptr, 1, 1025, CONF, THR, W, H, keep.ptr, out.ptr, bk.stream) == -4
    assert fn(dp.ptr, NC, NC, dl.ptr, 4, ds.ptr, dn.ptr, 1, 100, CONF, THR, W, H, None, out.ptr, bk.stream) == -3
    assert fn(dp.ptr, NC, NC, dl.ptr, 4, ds.ptr, dn.ptr, 0, 100, CONF, THR, W, H, keep.ptr, out.ptr, bk.stream) == 0
    assert fn(None, NC, NC, None, 4, None, None, 0, 100, CONF, THR, W, H, None, None, bk.stream) == 0
    assert (keep.get() == 9).all() and (out.get() == -9).all()


KERNEL_CASES = ["case_detect_block_restatement", "case_detect_wave_and_block_agree", "case_detect_block_strided", "case_detect_block_status"]


# ---- module cases --------------------------------------------------------------------------------------------------------------------
ROW_KEYS = ("boxes", "scores", "labels", "tubes")
MERGED_KEYS = ("boxes", "cluster", "labels", "scores", "tubes")


@contextlib.contextmanager
def detect_block(on):
    from step_amd import driver
    saved = driver.DETECT_BLOCK
    driver.DETECT_BLOCK = on
    try:
        yield
    finally:
        driver.DETECT_BLOCK = saved


def _args(**kw):
    return types.SimpleNamespace(image_size=(400, 400), num_classes=12, nms_thresh=0.4, **kw)


def golden_history(g, dev):
    nums = [int(v) for v in g["nums"]]
    hist = []
    for i in range(3):
        loc = torch.from_numpy(g["hist%d_loc" % i]).to(dev)
        prob = torch.from_numpy(g["hist%d_prob" % i]).to(dev)
        hist.append({"pred_prob": prob.unsqueeze(1).expand(-1, loc.shape[1], -1), "pred_loc": loc, "tubes_nums": nums})
    return hist, nums


def check_fixture(golden):
    """the fixture is the one the cases expect: clips of 84 / 65 / 0 / 109 tubes, and in every iteration a (clip, class) group that keeps
    more than 64 boxes (so more than 64 were masked)"""
    g = golden("detect_block_golden")
    assert [int(v) for v in g["nums"]] == [84, 65, 0, 109] and [float(v) for v in g["cfg"]] == [CONF, THR]
    meta = g["all_meta"]
    for it in range(3):
        m = meta[meta[:, 0] == it]
        assert np.bincount(m[:, 1] * 12 + m[:, 2]).max() > 64


def case_postprocess_block_golden(dev, golden):
    """driver.postprocess on the fixture's history: rows, order, boxes and scores bit-identical to what the reference's loop wrote, for
    `all` and `top20`; and each result identical to driver._postprocess_general on the same history."""
    from step_amd import driver
    check_fixture(golden)
    g = golden("detect_block_golden")
    hist, nums = golden_history(g, dev)
    for tag, kw in (("all", dict(evaluate_topk=-1, topk=-1)), ("top20", dict(evaluate_topk=1, topk=20))):
        dets = driver.postprocess(_args(conf_thresh=CONF, **kw), hist)
        assert len(dets) == 3 and all(len(d) == len(nums) for d in dets)
        meta, box, score = [], [], []
        for it, clips in enumerate(dets):
            for b, d in enumerate(clips):
                meta += [[it, b, int(c)] for c in d["labels"].cpu()]
                box.append(d["boxes"].cpu().numpy().reshape(-1, 4))
                score.append(d["scores"].cpu().numpy())
                assert bool((d["tubes"] < max(nums[b], 1)).all())
            gen = driver._postprocess_general(hist[it], nums, CONF, THR, kw["evaluate_topk"], kw["topk"], 400.0, 400.0)
            for a_, b_ in zip(gen, clips):
                assert all(torch.equal(a_[k], b_[k]) for k in ROW_KEYS), (tag, it)
        assert np.array_equal(np.asarray(meta, np.int32), g[tag + "_meta"]), tag
        assert np.array_equal(np.concatenate(box), g[tag + "_box"]), tag
        assert np.array_equal(np.concatenate(score), g[tag + "_score"]), tag


def case_postprocess_merged_block(dev, golden):
    """driver.postprocess_merged on the same history, conf 0.4 and global_thresh 0.8, with and without top-k: equal, key for key, to the
    result with DETECT_BLOCK = False (the general path's rows scattered into segments), and the merge of postprocess()'s rows."""
    from step_amd import driver
    g = golden("detect_block_golden")
    hist, nums = golden_history(g, dev)
    for kw in (dict(evaluate_topk=-1, topk=-1), dict(evaluate_topk=1, topk=50)):
        args = _args(conf_thresh=0.4, **kw)
        dets = driver.postprocess_merged(args, hist, global_thresh=0.8)
        with detect_block(False):
            old = driver.postprocess_merged(args, hist, global_thresh=0.8)
        assert len(dets) == len(old) == 3
        rows = 0
        for ca, cb in zip(dets, old):
            assert len(ca) == len(cb) == len(nums)
            for a_, b_ in zip(ca, cb):
                assert all(torch.equal(a_[k], b_[k]) for k in MERGED_KEYS), kw
                rows += int(a_["scores"].numel())
        assert rows > 100
        MG.check_against_rows(dets, driver.postprocess(args, hist), 0.8, "block %r" % (kw,))


def case_classified_rows_block(dev, golden):
    """driver.classified_rows at 100 and 7 tubes per clip (three clips, one of them empty): identical to the result with
    DETECT_BLOCK = False (the nonzero / gather form at 100 tubes; the same launch at 7)."""
    from step_amd import driver
    rs = np.random.RandomState(81)
    for per in (100, 7):
        nums = [per, 0, per - 3]
        N, NC = sum(nums), 9
        prob = torch.from_numpy((rs.randint(0, 7, (N, NC)) / 6.0 * (rs.rand(N, NC) < 0.5)).astype(f32)).to(dev)
        flat = torch.from_numpy(np.concatenate([np.zeros((N, 3, 1)), rs.uniform(0, 400, (N, 3, 4))], 2).astype(f32)).to(dev)
        args = _args(conf_thresh=0.01)
        new = driver.classified_rows(args, prob, flat, nums)
        with detect_block(False):
            old = driver.classified_rows(args, prob, flat, nums)
        assert len(new) == len(old) == 3 and int(new[0]["scores"].numel()) > per
        for a_, b_ in zip(new, old):
            assert all(torch.equal(a_[k], b_[k]) for k in ROW_KEYS), per


MODULE_CASES = ["case_postprocess_block_golden", "case_postprocess_merged_block", "case_classified_rows_block"]
