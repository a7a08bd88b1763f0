"""Cases for the cross-class merge of detections (step_detect_merge, step_amd.driver.postprocess_merged / merged_csv), driven on the
host interpreter by tests/test_emul_merge.py and on the real library by tests/test_gpu_merge.py.  The reference of every comparison is
tests/golden/merge_golden.npz: what the reference's own demo.py:140-217 did with seeded histories (tools/make_merge_golden.py).

Kernel cases take a backend of tests/backends.py; module cases take a device string ("cpu" under the interpreter patch, "cuda").
Everything is exactly specified (fp32 operations rounded one by one, sums in list order), so every comparison is equality."""
import types

import numpy as np
import torch

f32 = np.float32


# ---- a plain numpy restatement of the merge, written from its description (the host-side pin: fixture vs kernel) ---------------------
def np_iou(a, b):
    """IoU of the normalised fp32 box a with box(es) b ([4] or [n,4]): no "+1", intersection only where both extents are > 0, every
    operation rounded to fp32 on its own (numpy's fp32 element-wise operations do not contract)"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    iw = np.maximum(np.minimum(a[2], b[..., 2]) - np.maximum(a[0], b[..., 0]), f32(0))
    ih = np.maximum(np.minimum(a[3], b[..., 3]) - np.maximum(a[1], b[..., 1]), f32(0))
    inter = np.where((iw > 0) & (ih > 0), iw * ih, f32(0)).astype(f32)
    union = ((a[2] - a[0]) * (a[3] - a[1]) + (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])) - inter
    assert inter.dtype == f32 and union.dtype == f32
    return inter / union


def np_merge(boxes, thr):
    """boxes [n,4] fp32 in list order -> (leader [n]: list position of every row's leader, merged [K,4]: the clusters' boxes in leader
    order).  A row joins the FIRST leader before it that it overlaps (IoU with the leader's box > fp32(thr), strict), else leads; the
    cluster's box is the fp32 sum of its members in list order divided by their number."""
    boxes = np.asarray(boxes, f32).reshape(-1, 4)
    n = len(boxes)
    t = f32(thr)
    leader = np.full(n, -1, np.int32)
    for i in range(n):
        if leader[i] >= 0:
            continue
        leader[i] = i
        later = np.arange(n) > i
        leader[later & (leader < 0) & (np_iou(boxes[i], boxes) > t)] = i
    merged = []
    for i in np.flatnonzero(leader == np.arange(n)):
        s = np.zeros(4, f32)
        for j in np.flatnonzero(leader == i):
            s = (s + boxes[j]).astype(f32)
        merged.append((s / f32((leader == i).sum())).astype(f32))
    return leader, np.asarray(merged, f32).reshape(-1, 4)


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
def case_names(g):
    return [str(c) for c in g["cases"]]


def case_cfg(g, tag):
    conf, thr, etopk, topk = g[tag + "_cfg"]
    return float(conf), float(thr), int(etopk), int(topk)


def case_groups(g, tag):
    """per (iteration, clip) group of a case, in list order: dict(it, clip, cls [n], leader [n], box [n,4], score [n], merged [K,4], lines)"""
    groups, rows, box, score, merged = g[tag + "_groups"], g[tag + "_rows"], g[tag + "_box"], g[tag + "_score"], g[tag + "_merged"]
    lines = g[tag + "_lines"].tobytes().decode().splitlines(keepends=True)
    out, r0, k0 = [], 0, 0
    for it, b, n, K in groups:
        out.append(dict(it=int(it), clip=int(b), cls=rows[r0:r0 + n, 0], leader=rows[r0:r0 + n, 1], box=box[r0:r0 + n], score=score[r0:r0 + n],
                        merged=merged[k0:k0 + K], lines=lines[r0:r0 + n]))
        r0 += n
        k0 += K
    assert r0 == len(rows) == len(lines) and k0 == len(merged)
    return out


def fixture_history(g, name, dev):
    nums = [int(v) for v in g["hist%s_nums" % name]]
    hist = []
    i = 0
    while "hist%s_%d_loc" % (name, i) in g.files:
        loc = torch.from_numpy(g["hist%s_%d_loc" % (name, i)]).to(dev)
        prob = torch.from_numpy(g["hist%s_%d_prob" % (name, i)]).to(dev)
        hist.append({"pred_prob": prob.unsqueeze(1).expand(-1, loc.shape[1], -1), "pred_loc": loc, "tubes_nums": nums})
        i += 1
    return hist, nums


HIST_OF = {"all08": "A", "all05": "A", "top08": "A", "topm1_05": "A", "big08": "B", "general08": "C", "general_top075": "C"}


def check_numpy_restatement(golden):
    """np_merge on the fixture's rows == what the reference recorded (leaders, merged boxes bit for bit), every case; and the fixture is
    the one the cases below expect (case list, a group over 256 rows, empty and one-row groups, a pair at exactly the threshold)."""
    g = golden("merge_golden")
    assert case_names(g) == list(HIST_OF)
    sizes, exact = [], 0
    for tag in case_names(g):
        thr = case_cfg(g, tag)[1]
        for grp in case_groups(g, tag):
            leader, merged = np_merge(grp["box"], thr)
            assert np.array_equal(leader, grp["leader"]), (tag, grp["it"], grp["clip"])
            assert np.array_equal(merged, grp["merged"]), (tag, grp["it"], grp["clip"])
            sizes.append(len(leader))
            if thr == 0.5:
                for p in range(len(leader)):
                    for q in range(p):
                        if np_iou(grp["box"][q], grp["box"][p]) == f32(0.5):
                            assert leader[p] != q and leader[q] != p and grp["cls"][p] != grp["cls"][q]
                            exact += 1
    assert exact >= 1                                                            # the fixture does hold a pair at exactly the threshold
    assert max(sizes) > 256 and 0 in sizes and 1 in sizes
    assert not (f32(0.8) > 0.8) and float(f32(0.8)) > 0.8                        # numpy compares with the threshold rounded to fp32; in double it would differ


# ---- kernel cases --------------------------------------------------------------------------------------------------------------------
def run_merge(bk, segs, thr, cap=None, scramble=None):
    """step_detect_merge on a list of [n,4] row lists (list order).  scramble: a RandomState -- the rows are stored in a shuffled order
    inside their segment (behind a few rows that the list does not name) and `order` / `sel_counts` name the list.
    Returns per group (leader [n], merged [K,4]) and the raw outputs."""
    G = len(segs)
    cap = max([len(s) for s in segs] + [1]) + 9 if cap is None else cap
    boxes = np.zeros((G, cap, 4), f32)
    boxes[:] = np.asarray([0.1, 0.1, 0.2, 0.2], f32)                             # rows past a count: never read
    counts = np.asarray([len(s) for s in segs], np.int32)
    order = sel = None
    if scramble is not None:
        order = np.zeros((G, cap), np.int32)
        sel = counts.copy()
        counts = np.minimum(counts + 5, cap).astype(np.int32)                    # more rows than the list selects
        for k, s in enumerate(segs):
            slot = scramble.permutation(int(counts[k]))[:len(s)]
            boxes[k, slot] = s
            order[k, :len(s)] = slot
    else:
        for k, s in enumerate(segs):
            boxes[k, :len(s)] = s
    db, dc = bk.dev(boxes), bk.dev(counts)
    do, ds = bk.dev(order), bk.dev(sel)
    cl, lp, mg, nc = bk.dev(np.full((G, cap), -7, np.int32)), bk.dev(np.full((G, cap), -7, np.int32)), bk.dev(np.zeros((G, cap, 4), f32)), bk.dev(np.full(G, -7, np.int32))
    rc = bk.lib.step_detect_merge(db.ptr, dc.ptr, do.ptr, ds.ptr, G, cap, float(thr), cl.ptr, lp.ptr, mg.ptr, nc.ptr, bk.stream)
    assert rc == 0, rc
    cl, lp, mg, nc = cl.get(), lp.get(), mg.get(), nc.get()
    res = []
    for k, s in enumerate(segs):
        n, K = len(s), int(nc[k])
        assert 0 <= K <= n and np.all(cl[k, n:] == -1) and np.all((cl[k, :n] >= 0) & (cl[k, :n] < max(K, 1)))
        res.append((lp[k][cl[k, :n]] if n else np.zeros(0, np.int32), mg[k, :K].copy()))
    return res


def case_merge_fixture_segments(bk, golden):
    """step_detect_merge on every case's row segments, all groups of a case in one launch: leaders, cluster counts equal and the merged
    boxes BIT-equal to what the reference recorded -- in identity order, and with the rows scrambled inside their segments behind `order`."""
    g = golden("merge_golden")
    rs = np.random.RandomState(5)
    for tag in case_names(g):
        thr = case_cfg(g, tag)[1]
        groups = case_groups(g, tag)
        for scramble in (None, rs):
            res = run_merge(bk, [grp["box"] for grp in groups], thr, scramble=scramble)
            for grp, (leader, merged) in zip(groups, res):
                where = (tag, grp["it"], grp["clip"], scramble is not None)
                assert np.array_equal(leader, grp["leader"]), where
                assert merged.shape == grp["merged"].shape and np.array_equal(merged, grp["merged"]), where


def _box(x1, y1, x2, y2):
    return np.asarray([x1, y1, x2, y2], f32)


def case_merge_hand_made(bk, golden):
    """Hand-made segments.  A chain a-b-c: b overlaps a and c above the threshold, a and c do not -- b joins a, c leads its own cluster
    (it is compared with leaders only).  A row that overlaps two leaders joins the earlier one.  Two rows at exactly the threshold do not
    merge; just above it they do.  A full segment (count == cap), a group of one row and an empty group in the same launch."""
    a, b, c = _box(0, 0, .40, .5), _box(.04, 0, .44, .5), _box(.08, 0, .48, .5)                       # IoU(a,b) = IoU(b,c) = 9/11, IoU(a,c) = 2/3
    assert np_iou(a, b) > f32(0.8) and np_iou(b, c) > f32(0.8) and not np_iou(a, c) > f32(0.8)
    chain = np.stack([a, b, c])
    l1, l2, both = _box(0, 0, .5, .5), _box(.2, 0, .7, .5), _box(.1, 0, .6, .5)                       # IoU(l1,l2) = 3/7, `both` overlaps each by 2/3
    assert not np_iou(l1, l2) > f32(0.5) and np_iou(l1, both) > f32(0.5) and np_iou(l2, both) > f32(0.5)
    two = np.stack([l1, l2, both, l2])
    (lead, merged), = run_merge(bk, [chain], 0.8)
    assert lead.tolist() == [0, 0, 2] and np.array_equal(merged, np_merge(chain, 0.8)[1]) and np.array_equal(merged[1], c)
    (lead, merged), = run_merge(bk, [two], 0.5)
    assert lead.tolist() == [0, 1, 0, 1] and np.array_equal(merged, np_merge(two, 0.5)[1])
    e1, e2 = _box(0, 0, .5, .5), _box(0, 0, .5, .25)
    assert np_iou(e1, e2) == f32(0.5)
    (lead, merged), = run_merge(bk, [np.stack([e1, e2])], 0.5)
    assert lead.tolist() == [0, 1] and np.array_equal(merged, np.stack([e1, e2]))
    (lead, merged), = run_merge(bk, [np.stack([e1, e2])], float(np.nextafter(f32(0.5), f32(0))))
    assert lead.tolist() == [0, 0]
    segs = [chain, np.zeros((0, 4), f32), a.reshape(1, 4), two[:3]]
    for (lead, merged), s in zip(run_merge(bk, segs, 0.8, cap=3), segs):
        want = np_merge(s, 0.8)
        assert np.array_equal(lead, want[0]) and np.array_equal(merged, want[1])


def case_merge_long_lists(bk, golden):
    """Row counts past one wave, past 64 bitmap words' worth of one search step and past the rows the kernel keeps in LDS (2048): 2600
    and 4300 rows of jittered person-like boxes, and 700 rows that all lead (no overlap: as many clusters as rows), against np_merge."""
    rs = np.random.RandomState(11)
    segs = []
    for n, people in ((2600, 90), (4300, 25)):
        base = rs.uniform(0.0, 0.6, (people, 2))
        wh = rs.uniform(0.15, 0.4, (people, 2))
        who = rs.randint(0, people, n)
        b = np.concatenate([base[who], base[who] + wh[who]], 1) + rs.uniform(-0.015, 0.015, (n, 4))
        segs.append(b.astype(f32))
    k = np.arange(700)
    segs.append(np.stack([(k % 30) / 32.0, (k // 30) / 32.0, (k % 30) / 32.0 + 1 / 64.0, (k // 30) / 32.0 + 1 / 64.0], 1).astype(f32))
    for scramble in (None, rs):
        for (lead, merged), s in zip(run_merge(bk, segs, 0.8, scramble=scramble), segs):
            want = np_merge(s, 0.8)
            assert np.array_equal(lead, want[0]) and np.array_equal(merged, want[1])
    assert np.array_equal(np_merge(segs[2], 0.8)[0], k)


def case_merge_errors(bk, golden):
    """status codes: negative sizes -> STEP_E_SHAPE; G == 0 or cap == 0 -> STEP_OK without touching a pointer; null pointers ->
    STEP_E_NULL (also `order` without `sel_counts` and the reverse); more rows than the bitmap is sized for -> STEP_E_UNSUPPORTED"""
    G, cap = 2, 8
    b, c = bk.dev(np.zeros((G, cap, 4), f32)), bk.dev(np.zeros(G, np.int32))
    o, s = bk.dev(np.zeros((G, cap), np.int32)), bk.dev(np.zeros(G, np.int32))
    cl, lp, mg, nc = bk.dev(np.zeros((G, cap), np.int32)), bk.dev(np.zeros((G, cap), np.int32)), bk.dev(np.zeros((G, cap, 4), f32)), bk.dev(np.zeros(G, np.int32))
    fn = bk.lib.step_detect_merge
    assert fn(b.ptr, c.ptr, None, None, -1, cap, 0.8, cl.ptr, lp.ptr, mg.ptr, nc.ptr, bk.stream) == -2
    assert fn(b.ptr, c.ptr, None, None, G, -1, 0.8, cl.ptr, lp.ptr, mg.ptr, nc.ptr, bk.stream) == -2
    assert fn(None, None, None, None, 0, cap, 0.8, None, None, None, None, bk.stream) == 0
    assert fn(None, None, None, None, G, 0, 0.8, None, None, None, None, bk.stream) == 0
    full = [b.ptr, c.ptr, o.ptr, s.ptr, G, cap, 0.8, cl.ptr, lp.ptr, mg.ptr, nc.ptr, bk.stream]
    for k in (0, 1, 7, 8, 9, 10):
        a = list(full)
        a[k] = None
        assert fn(*a) == -3, k
    for k in (2, 3):                                                               # order and sel_counts go together
        a = list(full)
        a[k] = None
        assert fn(*a) == -3, k
    assert fn(b.ptr, c.ptr, None, None, 1, 65537, 0.8, cl.ptr, lp.ptr, mg.ptr, nc.ptr, bk.stream) == -4
    assert fn(*full) == 0 and fn(b.ptr, c.ptr, None, None, G, cap, 0.8, cl.ptr, lp.ptr, mg.ptr, nc.ptr, bk.stream) == 0
    assert nc.get().tolist() == [0, 0]


KERNEL_CASES = ["case_merge_fixture_segments", "case_merge_hand_made", "case_merge_long_lists", "case_merge_errors"]


# ---- module cases --------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    return types.SimpleNamespace(image_size=(400, 400), num_classes=60, nms_thresh=0.4, **kw)


def check_merged(dets, groups, nums, tag):
    """postprocess_merged's result for one case against the recorded groups"""
    from step_amd.driver import merged_csv
    by = {(grp["it"], grp["clip"]): grp for grp in groups}
    assert len(dets) * len(nums) == len(groups) and all(len(d) == len(nums) for d in dets)
    lines, want_lines = [], []
    for it, clips in enumerate(dets):
        for b, d in enumerate(clips):
            grp = by[(it, b)]
            where = (tag, it, b)
            heads = np.flatnonzero(grp["leader"] == np.arange(len(grp["leader"])))
            cluster = np.searchsorted(heads, grp["leader"])                      # cluster number of every list position
            out = np.argsort(cluster, kind="stable")                             # the reference writes cluster after cluster, list order inside
            assert d["boxes"].dtype == torch.float32 and tuple(d["boxes"].shape) == (len(heads), 4), where
            assert d["cluster"].dtype == torch.int64 and d["labels"].dtype == torch.int64 and d["tubes"].dtype == torch.int64, where
            assert np.array_equal(d["boxes"].cpu().numpy(), grp["merged"]), where
            assert np.array_equal(d["cluster"].cpu().numpy(), cluster[out]), where
            assert np.array_equal(d["labels"].cpu().numpy(), grp["cls"][out]), where
            assert np.array_equal(d["scores"].cpu().numpy(), grp["score"][out]), where
            assert d["tubes"].numel() == len(out) and bool((d["tubes"] >= 0).all()) and bool((d["tubes"] < max(nums[b], 1)).all()), where
            want_lines += grp["lines"]
        lines += merged_csv(clips, [{"video_name": "vid%d" % b, "fid": 900 + b} for b in range(len(nums))])
    assert lines == want_lines, tag


def check_against_rows(dets, plain, thr, tag):
    """postprocess_merged's result against np_merge on the rows postprocess() returns for the same history (its list order): the same
    rows regrouped -- labels, scores AND tubes -- and the merged boxes, exactly"""
    assert len(dets) == len(plain)
    for it, (clips, pclips) in enumerate(zip(dets, plain)):
        assert len(clips) == len(pclips)
        for b, (d, p_) in enumerate(zip(clips, pclips)):
            leader, merged = np_merge(p_["boxes"].cpu().numpy(), thr)
            cluster = np.searchsorted(np.flatnonzero(leader == np.arange(len(leader))), leader)
            out = np.argsort(cluster, kind="stable")
            where = (tag, it, b)
            assert np.array_equal(d["boxes"].cpu().numpy(), merged), where
            assert np.array_equal(d["cluster"].cpu().numpy(), cluster[out]), where
            for k in ("labels", "scores", "tubes"):
                assert np.array_equal(d[k].cpu().numpy(), p_[k].cpu().numpy()[out]), where + (k,)


def case_postprocess_merged_golden(dev, golden):
    """driver.postprocess_merged on the fixture's histories, every case (the three top-k settings, thresholds 0.8 / 0.5 / 0.75, a group
    over 256 rows, a clip over 64 tubes = the general path, empty and one-row clips): clusters, merged boxes (bit for bit), labels,
    scores in the reference's output order, and merged_csv's text string for string.  The rows (tubes included) are those postprocess()
    returns for the same history, regrouped."""
    from step_amd.driver import postprocess, postprocess_merged
    g = golden("merge_golden")
    for tag in case_names(g):
        conf, thr, etopk, topk = case_cfg(g, tag)
        hist, nums = fixture_history(g, HIST_OF[tag], dev)
        args = _args(conf_thresh=conf, evaluate_topk=etopk, topk=topk)
        dets = postprocess_merged(args, hist, global_thresh=thr)
        check_merged(dets, case_groups(g, tag), nums, tag)
        check_against_rows(dets, postprocess(args, hist), thr, tag)
    # thresholds from args / explicit arguments, one iteration only, demo.py's defaults
    hist, nums = fixture_history(g, "A", dev)
    one = postprocess_merged(_args(conf_thresh=0.01, evaluate_topk=-1, topk=-1), hist, conf_thresh=0.4, iterations=(1,))
    assert len(one) == 1
    check_merged(one, [dict(grp, it=0) for grp in case_groups(g, "all08") if grp["it"] == 1], nums, "iterations=(1,)")
    # a history without tubes
    h0 = {"pred_prob": hist[0]["pred_prob"][:0], "pred_loc": hist[0]["pred_loc"][:0], "tubes_nums": [0, 0]}
    e = postprocess_merged(_args(conf_thresh=0.4, evaluate_topk=-1, topk=-1), [h0])[0]
    assert len(e) == 2 and tuple(e[0]["boxes"].shape) == (0, 4) and e[1]["cluster"].numel() == 0


def case_postprocess_unchanged(dev, golden):
    """postprocess() itself still returns what the reference's evaluation loop recorded (the existing case, as it stands)"""
    from tests import module_cases as MC
    MC.case_postprocess_golden(dev, golden)


MODULE_CASES = ["case_postprocess_merged_golden", "case_postprocess_unchanged"]
