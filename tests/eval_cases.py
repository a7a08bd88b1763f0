"""Cases for the frame-mAP evaluation (step_round_sig4, step_eval_match, step_eval_ap, step_amd.evaluate.FrameMAP), driven on the host
interpreter by tests/test_emul_eval.py and on the real library by tests/test_gpu_eval.py.  The reference of every comparison is
tests/golden/eval_golden.npz: what the reference's own PascalDetectionEvaluator did with seeded rows (tools/make_eval_golden.py), or the
numpy restatement below, which is itself held to that fixture (check_numpy_restatement).

Kernel cases take a backend of tests/backends.py; module cases take a device string ("cpu" under the interpreter patch, "cuda").
Labels, matches, lists, counts, precision and recall are exactly specified, so they are compared for equality.  AP is a sum of K terms
(K = true positives of the class, each term in [0, 1], total <= 1) taken in another order than numpy's pairwise sum: both lie within
K * 2^-53 of the exact sum, hence the bound (K + 2) * 2^-52 per class, and (NC + 2) * 2^-52 on top for the mean over the classes."""
import io
import warnings

import numpy as np
import torch

f64 = np.float64
CASES = ("A", "B", "C")


# ---- a plain numpy restatement, written from the description of the semantics (the host-side pin: fixture vs kernels) ----------------
def np_round_sig4(v):
    """float("{:.4}".format(x)) of every fp32 value"""
    v = np.asarray(v, np.float32)
    return np.asarray([float("{:.4}".format(x)) for x in v.ravel()], f64).reshape(v.shape)


def np_labelling_order(scores):
    """descending score, among equal scores the LATER row first: a stable ascending sort, reversed"""
    return np.argsort(np.asarray(scores), kind="stable")[::-1]


def np_match_image(boxes, cls, gboxes, gcls, thr):
    """One image, rows ALREADY in labelling order (position = rank): boxes [n,4] f64 (x1,y1,x2,y2), cls [n], ground truth gboxes [m,4],
    gcls [m] -> (label [n] uint8: 0 / 1 / 2 = removed, match [n] int32).  Every valid row takes the FIRST ground-truth box of its class
    with the largest IoU; where that IoU >= thr it claims the box, and the claimant of lowest rank per box is the true positive."""
    boxes, gboxes = np.asarray(boxes, f64).reshape(-1, 4), np.asarray(gboxes, f64).reshape(-1, 4)
    cls, gcls = np.asarray(cls), np.asarray(gcls)
    n, m = len(boxes), len(gboxes)
    label, match = np.zeros(n, np.uint8), np.full(n, -1, np.int32)
    with np.errstate(invalid="ignore"):
        valid = (boxes[:, 1] < boxes[:, 3]) & (boxes[:, 0] < boxes[:, 2])
    label[~valid] = 2
    if n == 0 or m == 0:
        return label, match
    x1, y1, x2, y2 = (boxes[:, k:k + 1] for k in range(4))
    gx1, gy1, gx2, gy2 = (gboxes[None, :, k] for k in range(4))
    with np.errstate(invalid="ignore", divide="ignore"):
        ih = np.maximum(0.0, np.minimum(y2, gy2) - np.maximum(y1, gy1))
        iw = np.maximum(0.0, np.minimum(x2, gx2) - np.maximum(x1, gx1))
        inter = ih * iw
        iou = inter / (((y2 - y1) * (x2 - x1) + (gy2 - gy1) * (gx2 - gx1)) - inter)
    same = (cls[:, None] == gcls[None, :]) & valid[:, None]
    iou = np.where(same, iou, -1.0)
    best = np.argmax(iou, axis=1)                                    # first maximum
    has = same.any(axis=1)
    match[has] = best[has]
    ok = has & (iou[np.arange(n), best] >= thr)
    claim = np.full(m, n, np.int64)
    np.minimum.at(claim, best[ok], np.flatnonzero(ok))
    label[ok & (claim[best] == np.arange(n))] = 1
    return label, match


def np_precision_recall_ap(labels, num_gt):
    """labels [n] 0 / 1 in descending score order -> (precision, recall, ap); the sum of AP sequential in list order"""
    labels = np.asarray(labels).astype(np.int64)
    if num_gt == 0:
        return np.full(len(labels), np.nan), np.full(len(labels), np.nan), float("nan")
    ctp = np.cumsum(labels)
    precision = ctp.astype(f64) / np.arange(1, len(labels) + 1)
    recall = ctp.astype(f64) / num_gt
    env = np.maximum.accumulate(precision[::-1])[::-1] if len(labels) else precision
    ap = 0.0
    for i in np.flatnonzero(labels == 1):
        ap += (recall[i] - f64(ctp[i] - 1) / num_gt) * env[i]
    return precision, recall, float(ap)


def np_evaluate(rows, thr=0.5):
    """rows = evaluated_rows(...) -> dict(scores, labels: per class, score-descending; num_gt [NC]; ap [NC]; map; per image `order`,
    `label`, `match` in labelling order)"""
    NC = rows["num_class"]
    per_cls_s, per_cls_l = [[] for _ in range(NC)], [[] for _ in range(NC)]
    images = []
    for im in rows["images"]:
        order = np_labelling_order(im["score"])
        gb, gc = rows["gt"].get(im["key"], (np.zeros((0, 4)), np.zeros(0, np.int32)))
        label, match = np_match_image(im["box"][order], im["cls"][order], gb, gc, thr)
        images.append(dict(order=order, label=label, match=match))
        cl, sc = im["cls"][order], im["score"][order]
        for c in np.unique(cl[label != 2]):
            sel = (cl == c) & (label != 2)
            per_cls_s[c].append(sc[sel])
            per_cls_l[c].append(label[sel])
    num_gt = np.zeros(NC, np.int64)
    for gb, gc in rows["gt"].values():
        num_gt += np.bincount(gc, minlength=NC)
    scores, labels, ap = [], [], np.full(NC, np.nan)
    for c in range(NC):
        s = np.concatenate(per_cls_s[c]) if per_cls_s[c] else np.zeros(0)
        l = np.concatenate(per_cls_l[c]) if per_cls_l[c] else np.zeros(0, np.uint8)
        o = np.argsort(s, kind="stable")[::-1]
        scores.append(s[o])
        labels.append(l[o])
        ap[c] = np_precision_recall_ap(l[o], num_gt[c])[2]
    have = ap[~np.isnan(ap)]
    return dict(scores=scores, labels=labels, num_gt=num_gt, ap=ap, map=float(have.sum() / len(have)) if len(have) else float("nan"),
                images=images)


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
def load_case(g, X):
    p = X + "_"
    ids = [int(v) for v in g[p + "ids"]]
    c = dict(ids=ids, names=[str(v) for v in g[p + "names"]], vids=[str(v) for v in g[p + "vids"]], ts=[int(v) for v in g[p + "ts"]],
             excl=[int(v) for v in g[p + "excl"]])
    c["keys"] = ["%s,%04d" % (v, t) for v, t in zip(c["vids"], c["ts"])]
    for k in ("gt_img", "gt_box", "gt_id", "det_img", "det_box32", "det_score32", "det_box64", "det_score64", "det_id", "ref_cls_start",
              "ref_scores", "ref_labels", "ref_num_gt", "ref_ap", "ref_map", "ref_dict_vals"):
        c[k] = g[p + k]
    c["ref_dict_keys"] = [str(v) for v in g[p + "ref_dict_keys"]]
    c["categories"] = [{"id": i, "name": n} for i, n in zip(ids, c["names"])]
    return c


def evaluated_rows(c, rounded="fixture"):
    """the rows the evaluator sees: label-map and exclusion filters applied, detections per image in file order (images in the order of
    their first row), boxes / scores = the text-rounded float64 of the fixture (or np_round_sig4 of the fp32 rows: rounded="numpy")"""
    ids, excl = set(c["ids"]), {c["keys"][k] for k in c["excl"]}
    box = c["det_box64"] if rounded == "fixture" else np_round_sig4(c["det_box32"])
    score = c["det_score64"] if rounded == "fixture" else np_round_sig4(c["det_score32"])
    images, gt = {}, {}
    for r in range(len(c["det_id"])):
        key = c["keys"][int(c["det_img"][r])]
        if int(c["det_id"][r]) in ids and key not in excl:
            images.setdefault(key, []).append(r)
    for r in range(len(c["gt_id"])):
        key = c["keys"][int(c["gt_img"][r])]
        if int(c["gt_id"][r]) in ids and key not in excl:
            gt.setdefault(key, []).append(r)
    return dict(num_class=max(ids),
                images=[dict(key=k, box=box[v], score=score[v], cls=c["det_id"][v].astype(np.int32) - 1) for k, v in images.items()],
                gt={k: (c["gt_box"][v].astype(f64), c["gt_id"][v].astype(np.int32) - 1) for k, v in gt.items()})


def ref_lists(c):
    cs = c["ref_cls_start"]
    return ([c["ref_scores"][cs[k]:cs[k + 1]] for k in range(len(cs) - 1)], [c["ref_labels"][cs[k]:cs[k + 1]] for k in range(len(cs) - 1)])


def ap_bounds(labels, NC):
    """(per-class bound [NC], bound of the mean) from the true positives of every class"""
    K = np.asarray([int(np.sum(np.asarray(l) == 1)) for l in labels], f64)
    per = (K + 2) * 2.0 ** -52
    return per, float(per.max()) + (NC + 2) * 2.0 ** -52


def assert_ap(ap, mean, c, labels, where):
    per, bm = ap_bounds(labels, len(c["ref_ap"]))
    ref = c["ref_ap"]
    assert np.array_equal(np.isnan(ap), np.isnan(ref)), where
    d = np.abs(np.where(np.isnan(ref), 0, np.asarray(ap) - ref))
    print("%s: largest |AP - reference| %.3g (bound %.3g), |mAP - reference| %.3g (bound %.3g)"
          % (where, d.max(), per.max(), abs(mean - float(c["ref_map"])), bm))
    assert np.all(d <= per), (where, d.max())
    assert abs(mean - float(c["ref_map"])) <= bm, where


def check_numpy_restatement(golden):
    """np_evaluate on the fixture's rows == what the reference recorded: the (score, label) list of every class and num_gt exactly, AP
    and mAP within the derived bound; np_round_sig4 of the fp32 rows == the float64 the reference parsed from the text; and the fixture
    holds what the cases expect (ties only between equal labels, NaN and 0 classes, excluded keys, unlisted classes, invalid boxes)."""
    g = golden("eval_golden")
    for X in CASES:
        c = load_case(g, X)
        assert np.array_equal(np_round_sig4(c["det_box32"]), c["det_box64"]) and np.array_equal(np_round_sig4(c["det_score32"]), c["det_score64"])
        rows = evaluated_rows(c)
        res = np_evaluate(rows)
        rs, rl = ref_lists(c)
        assert len(rs) == rows["num_class"] == len(c["ref_ap"])
        for k in range(rows["num_class"]):
            assert np.array_equal(res["scores"][k], rs[k]) and np.array_equal(res["labels"][k], rl[k]), (X, k)
            for s in np.unique(rs[k]):
                assert len(np.unique(rl[k][rs[k] == s])) == 1, (X, k, s)             # the reference's result does not hang on its unstable sort
        assert np.array_equal(res["num_gt"], c["ref_num_gt"])
        assert_ap(res["ap"], res["map"], c, rl, "restatement " + X)
    a, b, cc = (load_case(g, X) for X in CASES)
    bx = a["det_box64"]
    assert np.any(~((bx[:, 1] < bx[:, 3]) & (bx[:, 0] < bx[:, 2])))                   # invalid boxes
    assert max(b["ids"]) > len(b["ids"]) and len(b["excl"]) > 0                      # a label map with gaps, excluded keys
    assert np.any(~np.isin(b["det_id"], b["ids"])) and np.any(~np.isin(b["gt_id"], b["ids"]))
    listed = np.asarray(b["ids"]) - 1
    assert np.any(b["ref_ap"][listed] == 0) and np.any(np.isnan(b["ref_ap"][listed]))
    assert any(len(np.unique(s)) < len(s) for s in ref_lists(cc)[0])                 # case C has score ties


# ---- kernel cases --------------------------------------------------------------------------------------------------------------------
def run_round(bk, v):
    v = np.ascontiguousarray(v, np.float32).ravel()
    i, o, st = bk.dev(v), bk.dev(np.zeros(len(v), f64)), bk.dev(np.zeros(1, np.int32))
    rc = bk.lib.step_round_sig4(i.ptr, len(v), o.ptr, st.ptr, bk.stream)
    assert rc == 0, rc
    return o.get(), int(st.get()[0])


def round_values(n=120000, seed=3):
    rs = np.random.RandomState(seed)
    edge = [0.03125, 0.15625, 0.99995, 1.0, 0.0, 1e-5, 0.5, 0.12345, 0.12355, 0.00010005, 9999.4, 9999.5, 9999.7, 1.5e-9, 1.00049995, 1000.5, 2.5e-7,
            -0.25, -0.123456, 0.1, 0.2, 0.3, 999.95, 99.995, 9.9995, 0.99985, 1e-8, 3e-9]
    ties = (rs.randint(1000, 10000, 4000) + 0.5) / rs.choice([1.0, 16.0, 256.0, 4096.0], 4000)            # exact halves of the fourth digit where fp32 holds them
    return np.concatenate([rs.uniform(0, 1, n // 2), np.exp(rs.uniform(np.log(1e-8), np.log(8e3), n // 2)), ties, edge]).astype(np.float32)


def case_round_sig4(bk, golden):
    """step_round_sig4 == float("{:.4}".format(np.float32(v))), bit for bit, on > 1e5 seeded values (uniform in [0, 1), log-uniform in
    [1e-8, 8e3), exact decimal halves, edge values) and on the fixture's fp32 rows; the status word stays 0 on them and is set, with a
    NaN result, for values out of range, inf and NaN; n == 0 and null pointers."""
    v = round_values()
    assert len(v) >= 100000
    out, st = run_round(bk, v)
    want = np_round_sig4(v)
    assert st == 0 and np.array_equal(out.view(np.int64), want.view(np.int64)), int(np.sum(out != want))
    c = load_case(golden("eval_golden"), "A")
    out, st = run_round(bk, c["det_box32"])
    assert st == 0 and np.array_equal(out.reshape(-1, 4), c["det_box64"])
    for bad in (1e4, 12345.0, 5e-10, np.inf, -np.inf, np.nan, 1e-40):
        out, st = run_round(bk, [0.5, bad, 0.25])
        assert st == 1 and np.isnan(out[1]) and out[0] == 0.5 and out[2] == 0.25, bad
    fn = bk.lib.step_round_sig4
    i, o, s = bk.dev(np.zeros(4, np.float32)), bk.dev(np.zeros(4, f64)), bk.dev(np.zeros(1, np.int32))
    assert fn(None, 0, None, None, bk.stream) == 0 and fn(i.ptr, -1, o.ptr, s.ptr, bk.stream) == -2
    for k in range(3):
        a = [i.ptr, 4, o.ptr, s.ptr, bk.stream]
        a[(0, 2, 3)[k]] = None
        assert fn(*a) == -3


def run_match(bk, images, thr=0.5, gt_max=None):
    """images: list of (boxes [n,4], cls [n], gboxes [m,4], gcls [m]) with rows in labelling order -> (rc, label, match) over all rows"""
    cat = lambda k, tail, dt: np.concatenate([np.zeros((0,) + tail, dt)] + [np.asarray(im[k], dt).reshape((-1,) + tail) for im in images])
    db, dc = cat(0, (4,), f64), cat(1, (), np.int32)
    gb, gc = cat(2, (4,), f64), cat(3, (), np.int32)
    ds = np.cumsum([0] + [len(im[1]) for im in images]).astype(np.int64)
    gs = np.cumsum([0] + [len(im[3]) for im in images]).astype(np.int64)
    gmax = max([len(im[3]) for im in images] + [0]) if gt_max is None else gt_max
    R = len(dc)
    lab, mt = bk.dev(np.full(R, 9, np.uint8)), bk.dev(np.full(R, -7, np.int32))
    bufs = [bk.dev(a) for a in (db, dc, ds, gb, gc, gs)]
    rc = bk.lib.step_eval_match(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, bufs[5].ptr, len(images), R, len(gc), gmax, thr,
                                lab.ptr, mt.ptr, bk.stream)
    return rc, lab.get(), mt.get()


def case_match_fixture(bk, golden):
    """step_eval_match on every fixture case, all images in one launch: label and match of every row == the restatement's, which
    check_numpy_restatement holds to the reference's lists; the lists built from the kernel's labels == the reference's."""
    g = golden("eval_golden")
    for X in CASES:
        c = load_case(g, X)
        rows = evaluated_rows(c)
        res = np_evaluate(rows)
        ims = []
        for im, r in zip(rows["images"], res["images"]):
            gb, gc = rows["gt"].get(im["key"], (np.zeros((0, 4)), np.zeros(0, np.int32)))
            ims.append((im["box"][r["order"]], im["cls"][r["order"]], gb, gc))
        rc, lab, mt = run_match(bk, ims)
        assert rc == 0
        assert np.array_equal(lab, np.concatenate([r["label"] for r in res["images"]])), X
        assert np.array_equal(mt, np.concatenate([r["match"] for r in res["images"]])), X
        # the reference's per-class lists from the kernel's labels
        sc = np.concatenate([np.zeros(0)] + [im["score"][r["order"]] for im, r in zip(rows["images"], res["images"])])
        cl = np.concatenate([im[1] for im in ims])
        rs, rl = ref_lists(c)
        for k in range(rows["num_class"]):
            sel = (cl == k) & (lab != 2)
            o = np.argsort(sc[sel], kind="stable")[::-1]
            assert np.array_equal(sc[sel][o], rs[k]) and np.array_equal(lab[sel][o], rl[k]), (X, k)


def _b(x1, y1, x2, y2):
    return [x1, y1, x2, y2]


def case_match_hand_made(bk, golden):
    """Two detections of equal score on one box: in labelling order the LATER input row stands first and wins.  A row whose best box
    is taken does not fall back to its second-best.  First maximum among equal IoUs.  IoU exactly at the threshold counts.  An image of
    3 000 rows (chunks of 256), an empty image, an image without ground truth, invalid and NaN boxes, NI = 0."""
    g1 = _b(0.1, 0.1, 0.5, 0.5)
    d_a, d_b = _b(0.1, 0.1, 0.5, 0.52), _b(0.1, 0.1, 0.52, 0.5)
    score = np.asarray([0.9, 0.9])
    order = np_labelling_order(score)
    assert order.tolist() == [1, 0]
    rc, lab, mt = run_match(bk, [(np.asarray([d_a, d_b])[order], [3, 3], [g1], [3])])
    assert rc == 0 and lab.tolist() == [1, 0] and mt.tolist() == [0, 0]           # position 0 = input row 1 (the later one)
    # no fall-back: rows 0 and 1 both prefer box 0; row 1 overlaps box 1 above the threshold as well, and stays a false positive
    ga, gb_ = _b(0.0, 0.0, 0.4, 0.4), _b(0.1, 0.0, 0.5, 0.4)
    rc, lab, mt = run_match(bk, [([_b(0.0, 0.0, 0.4, 0.4), _b(0.02, 0.0, 0.42, 0.4)], [7, 7], [ga, gb_], [7, 7])])
    assert rc == 0 and lab.tolist() == [1, 0] and mt.tolist() == [0, 0]
    # two identical ground-truth boxes: the FIRST maximum, so the second row finds box 0 taken; another class's box is not looked at
    rc, lab, mt = run_match(bk, [([ga, ga, ga], [2, 2, 5], [ga, ga, ga], [2, 2, 9])])
    assert rc == 0 and lab.tolist() == [1, 0, 0] and mt.tolist() == [0, 0, -1]
    # exactly the threshold: [0,0,.5,.5] against [0,0,.5,.25] is IoU 0.5
    rc, lab, mt = run_match(bk, [([_b(0, 0, 0.5, 0.25)], [0], [_b(0, 0, 0.5, 0.5)], [0])])
    assert rc == 0 and lab.tolist() == [1]
    rc, lab, mt = run_match(bk, [([_b(0, 0, 0.5, 0.25)], [0], [_b(0, 0, 0.5, 0.5)], [0])], thr=float(np.nextafter(0.5, 1)))
    assert rc == 0 and lab.tolist() == [0] and mt.tolist() == [0]
    # a large image next to an empty one, one without ground truth, and invalid / NaN boxes
    rs = np.random.RandomState(21)
    n, m = 3000, 40
    gxy = rs.uniform(0, 0.7, (m, 2))
    gbx = np.concatenate([gxy, gxy + rs.uniform(0.1, 0.3, (m, 2))], 1)
    gcl = rs.randint(0, 6, m)
    who = rs.randint(0, m, n)
    dbx = gbx[who] + rs.uniform(-0.04, 0.04, (n, 4))
    dcl = np.where(rs.rand(n) < 0.8, gcl[who], rs.randint(0, 8, n))
    dbx[5] = [0.5, 0.5, 0.5, 0.7]
    dbx[700] = [0.6, 0.5, 0.4, 0.7]
    dbx[2999] = [np.nan, 0.1, 0.5, 0.5]
    ims = [(dbx, dcl, gbx, gcl), (np.zeros((0, 4)), [], np.zeros((0, 4)), []), (dbx[:300], dcl[:300], np.zeros((0, 4)), []),
           (np.zeros((0, 4)), [], gbx[:3], gcl[:3])]
    rc, lab, mt = run_match(bk, ims)
    want = [np_match_image(*im, 0.5) for im in ims]
    assert rc == 0 and np.array_equal(lab, np.concatenate([w[0] for w in want])) and np.array_equal(mt, np.concatenate([w[1] for w in want]))
    assert lab[5] == 2 and lab[700] == 2 and lab[2999] == 2 and 10 < int((lab[:3000] == 1).sum()) <= m and not (lab[3000:] == 1).any()
    rc, lab, mt = run_match(bk, [])
    assert rc == 0 and len(lab) == 0


def case_match_limits(bk, golden):
    """An image with 1 024 ground-truth rows is evaluated (against the restatement); with 1 025: STEP_E_UNSUPPORTED.  Status codes for
    negative sizes and null pointers."""
    rs = np.random.RandomState(22)
    m = 1025
    k = np.arange(m)
    gbx = np.stack([(k % 40) / 41.0, (k // 40) / 41.0, (k % 40) / 41.0 + 1 / 50.0, (k // 40) / 41.0 + 1 / 50.0], 1)
    gcl = rs.randint(0, 3, m)
    who = rs.randint(0, m, 600)
    dbx = gbx[who] + rs.uniform(-0.002, 0.002, (600, 4))
    dcl = gcl[who]
    im = (dbx, dcl, gbx[:1024], gcl[:1024])
    rc, lab, mt = run_match(bk, [im])
    want = np_match_image(*im, 0.5)
    assert rc == 0 and np.array_equal(lab, want[0]) and np.array_equal(mt, want[1]) and int((lab == 1).sum()) > 100 and mt.max() > 900
    rc, lab, mt = run_match(bk, [(dbx, dcl, gbx, gcl)])
    assert rc == -4 and np.all(lab == 9)                                           # nothing was launched
    # a gt_max that understates gt_start: the launch goes ahead, and the image is marked, not matched against a cut list; its neighbour is untouched
    rc, lab, mt = run_match(bk, [im, (dbx, dcl, gbx, gcl), im], gt_max=1024)
    assert rc == 0 and np.all(lab[600:1200] == 255) and np.all(mt[600:1200] == -2)
    assert np.array_equal(lab[:600], want[0]) and np.array_equal(lab[1200:], want[0]) and np.array_equal(mt[1200:], want[1])
    fn = bk.lib.step_eval_match
    d = [bk.dev(a) for a in (np.zeros((2, 4), f64), np.zeros(2, np.int32), np.asarray([0, 2], np.int64), np.zeros((1, 4), f64) + [0, 0, 1, 1],
                             np.zeros(1, np.int32), np.asarray([0, 1], np.int64))]
    lab, mt = bk.dev(np.zeros(2, np.uint8)), bk.dev(np.zeros(2, np.int32))
    full = [d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, d[5].ptr, 1, 2, 1, 1, 0.5, lab.ptr, mt.ptr, bk.stream]
    assert fn(*full) == 0
    for pos in (0, 1, 2, 3, 4, 5, 11, 12):
        a = list(full)
        a[pos] = None
        assert fn(*a) == -3, pos
    for pos, v in ((6, -1), (7, -1), (8, -1), (9, -1), (9, 2)):
        a = list(full)
        a[pos] = v
        assert fn(*a) == -2, pos
    assert fn(None, None, None, None, None, None, 0, 0, 0, 0, 0.5, None, None, bk.stream) == 0


def run_ap(bk, labels, num_gt, pad=0):
    """labels: per class arrays -> (precision, recall per class, ap [NC]); `pad` rows behind the last class belong to no class"""
    NC = len(labels)
    cs = np.cumsum([0] + [len(l) for l in labels]).astype(np.int64)
    lab = np.concatenate([np.asarray(l, np.uint8) for l in labels] + [np.zeros(pad, np.uint8)])
    R = len(lab)
    b = [bk.dev(a) for a in (cs, lab, np.asarray(num_gt, np.int64), np.full(R, -1.0), np.full(R, -1.0), np.full(NC, -1.0))]
    rc = bk.lib.step_eval_ap(b[0].ptr, b[1].ptr, b[2].ptr, NC, R, b[3].ptr, b[4].ptr, b[5].ptr, bk.stream)
    assert rc == 0, rc
    pr, rec, ap = b[3].get(), b[4].get(), b[5].get()
    return [pr[cs[k]:cs[k + 1]] for k in range(NC)], [rec[cs[k]:cs[k + 1]] for k in range(NC)], ap


def case_ap_fixture(bk, golden):
    """step_eval_ap on the reference's own lists of every case: AP per class and the mean within the derived bound, NaN exactly where
    the reference has NaN, precision and recall equal to the restatement's (quotients of integers, one rounding each)."""
    g = golden("eval_golden")
    for X in CASES:
        c = load_case(g, X)
        rs, rl = ref_lists(c)
        pr, rec, ap = run_ap(bk, rl, c["ref_num_gt"], pad=3)
        have = ap[~np.isnan(ap)]
        assert_ap(ap, float(have.sum() / len(have)), c, rl, "step_eval_ap " + X)
        for k in range(len(rl)):
            wp, wr, _ = np_precision_recall_ap(rl[k], int(c["ref_num_gt"][k]))
            assert np.array_equal(pr[k], wp, equal_nan=True) and np.array_equal(rec[k], wr, equal_nan=True), (X, k)


def case_ap_long(bk, golden):
    """A class of 1e5 rows (391 chunks) next to an empty class with ground truth (AP 0), a class without ground truth (NaN), a short
    one and one of exactly 256 rows, against the restatement; two launches on the same input are bit-equal.  Status codes."""
    rs = np.random.RandomState(23)
    n = 100000
    big = (rs.rand(n) < np.linspace(0.9, 0.05, n)).astype(np.uint8)
    labels = [big, np.zeros(0, np.uint8), np.asarray([1, 0, 1], np.uint8), np.asarray([0, 1, 1, 0, 0, 1], np.uint8), (rs.rand(256) < 0.5).astype(np.uint8),
              np.zeros(300, np.uint8)]
    num_gt = [int(big.sum()) + 17, 4, 0, 5, 256, 9]
    pr, rec, ap = run_ap(bk, labels, num_gt)
    per, _ = ap_bounds(labels, len(labels))
    for k in range(len(labels)):
        wp, wr, wa = np_precision_recall_ap(labels[k], num_gt[k])
        assert np.array_equal(pr[k], wp, equal_nan=True) and np.array_equal(rec[k], wr, equal_nan=True), k
        assert (np.isnan(ap[k]) and np.isnan(wa)) or abs(ap[k] - wa) <= per[k], (k, ap[k], wa)
    print("class of 1e5 rows: AP %.17g, |kernel - sequential| %.3g (bound %.3g)" % (ap[0], abs(ap[0] - np_precision_recall_ap(big, num_gt[0])[2]), per[0]))
    assert ap[1] == 0.0 and np.isnan(ap[2]) and ap[5] == 0.0 and 0.3 < ap[0] < 1.0
    pr2, rec2, ap2 = run_ap(bk, labels, num_gt)
    assert np.array_equal(ap.view(np.int64), ap2.view(np.int64))
    for k in range(len(labels)):
        assert np.array_equal(pr[k].view(np.int64), pr2[k].view(np.int64)) and np.array_equal(rec[k].view(np.int64), rec2[k].view(np.int64)), k
    fn = bk.lib.step_eval_ap
    cs, lab, ng = bk.dev(np.asarray([0, 2], np.int64)), bk.dev(np.asarray([1, 0], np.uint8)), bk.dev(np.asarray([2], np.int64))
    p, r, a = bk.dev(np.zeros(2)), bk.dev(np.zeros(2)), bk.dev(np.zeros(1))
    full = [cs.ptr, lab.ptr, ng.ptr, 1, 2, p.ptr, r.ptr, a.ptr, bk.stream]
    assert fn(*full) == 0 and a.get()[0] == 0.5
    for pos in (0, 1, 2, 5, 6, 7):
        x = list(full)
        x[pos] = None
        assert fn(*x) == -3, pos
    assert fn(cs.ptr, lab.ptr, ng.ptr, -1, 2, p.ptr, r.ptr, a.ptr, bk.stream) == -2 and fn(None, None, None, 0, 0, None, None, None, bk.stream) == 0


KERNEL_CASES = ["case_round_sig4", "case_match_fixture", "case_match_hand_made", "case_match_limits", "case_ap_fixture", "case_ap_long"]


# ---- module cases --------------------------------------------------------------------------------------------------------------------
def csv_text(c):
    """the three files of a case as text: ground truth, detections (test.py:213's format on the fp32 rows), exclusions"""
    gt = "".join("%s,%04d,%r,%r,%r,%r,%d\n" % ((c["vids"][k], c["ts"][k]) + tuple(float(v) for v in b) + (i,))
                 for k, b, i in zip(c["gt_img"], c["gt_box"], c["gt_id"]))
    det = "".join("{0},{1:04},{2:.4},{3:.4},{4:.4},{5:.4},{6},{7:.4}\n".format(c["vids"][k], c["ts"][k], b[0], b[1], b[2], b[3], i, s)
                  for k, b, i, s in zip(c["det_img"], c["det_box32"], c["det_id"], c["det_score32"]))
    ex = "".join("%s,%04d\n" % (c["vids"][k], c["ts"][k]) for k in c["excl"])
    return gt, det, ex


def labelmap_text(c):
    return "".join('item {\n  name: "%s"\n  id: %d\n}\n' % (n, i) for i, n in zip(c["ids"], c["names"]))


def frame_map_csv(c, dev):
    from step_amd.evaluate import FrameMAP, read_labelmap
    gt, det, ex = csv_text(c)
    cats, ids = read_labelmap(io.StringIO(labelmap_text(c)))
    assert cats == c["categories"] and ids == set(c["ids"])
    ev = FrameMAP(cats, device=dev)
    ev.add_groundtruth_csv(io.StringIO(gt), io.StringIO(ex))
    ev.add_detections_csv(io.StringIO(det), io.StringIO(ex))
    return ev


def frame_map_rows(c, dev, clips_per_call=7):
    """the same case through add_groundtruth + add_detections on the fp32 rows as device tensors, a few images per call"""
    from step_amd.evaluate import FrameMAP
    ev = FrameMAP(c["categories"], device=dev, exclusions={c["keys"][k] for k in c["excl"]})
    for k in dict.fromkeys(int(v) for v in c["gt_img"]):
        sel = c["gt_img"] == k
        ev.add_groundtruth(c["keys"][k], c["gt_box"][sel], c["gt_id"][sel])
    imgs = list(dict.fromkeys(int(v) for v in c["det_img"]))
    for i0 in range(0, len(imgs), clips_per_call):
        dets, infos = [], []
        for k in imgs[i0:i0 + clips_per_call]:
            sel = c["det_img"] == k
            dets.append({"boxes": torch.from_numpy(c["det_box32"][sel]).to(dev), "scores": torch.from_numpy(c["det_score32"][sel]).to(dev),
                         "labels": torch.from_numpy(c["det_id"][sel].astype(np.int64) - 1).to(dev)})
            infos.append({"video_name": c["vids"][k], "fid": c["ts"][k]})
        ev.add_detections(dets, infos)
    return ev


def check_frame_map(ev, c, where):
    metrics, full = ev.evaluate(full=True)
    rs, rl = ref_lists(c)
    for k in range(len(rs)):
        assert np.array_equal(full["scores"][k], rs[k]) and np.array_equal(full["labels"][k], rl[k]), (where, k)
        wp, wr, _ = np_precision_recall_ap(rl[k], int(c["ref_num_gt"][k]))
        assert np.array_equal(full["precision"][k], wp, equal_nan=True) and np.array_equal(full["recall"][k], wr, equal_nan=True), (where, k)
    assert np.array_equal(full["num_gt"], c["ref_num_gt"]), where
    assert list(metrics) == c["ref_dict_keys"], where
    vals = np.asarray(list(metrics.values()), f64)
    assert all(type(v) is float for v in metrics.values())
    assert np.array_equal(np.isnan(vals), np.isnan(c["ref_dict_vals"])) and np.array_equal(vals == 0, c["ref_dict_vals"] == 0), where
    assert_ap(full["ap"], metrics[c["ref_dict_keys"][0]], c, rl, where)
    assert repr(metrics) == repr(ev.evaluate())                                   # a second call gives the same dict (NaN != NaN, so the text is compared)
    return full


def case_frame_map_golden(dev, golden):
    """FrameMAP on every fixture case, through the CSV text and through add_groundtruth + add_detections on the fp32 rows (rounded on
    the device): both give the reference's (score, label) lists, num_gt, dict keys, NaN / 0 classes, and AP / mAP within the bound."""
    g = golden("eval_golden")
    for X in CASES:
        c = load_case(g, X)
        a = check_frame_map(frame_map_csv(c, dev), c, "FrameMAP csv " + X)
        b = check_frame_map(frame_map_rows(c, dev), c, "FrameMAP rows " + X)
        for k in range(len(a["scores"])):
            assert np.array_equal(a["scores"][k], b["scores"][k]) and np.array_equal(a["labels"][k], b["labels"][k])
        assert np.array_equal(a["ap"].view(np.int64), b["ap"].view(np.int64))


def case_frame_map_behaviours(dev, golden):
    """A detection key added twice: the second is ignored with a warning.  A ground-truth key added twice raises.  A score <= -10, more
    than 10 000 detections of one class in one image, a value the rounding does not cover, a ground-truth box without area: raise.  No
    detections at all: AP 0 for the classes with ground truth.  ava_evaluation reads the reference's file names."""
    import os
    import tempfile

    from step_amd.evaluate import FrameMAP, ava_evaluation
    c = load_case(golden("eval_golden"), "C")
    gt, det, ex = csv_text(c)
    ev = frame_map_csv(c, dev)
    want = ev.evaluate()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        ev.add_detections_csv(io.StringIO(det))
        k = int(c["det_img"][0])
        ev.add_detections([{"boxes": torch.zeros(1, 4).to(dev), "scores": torch.ones(1).to(dev), "labels": torch.zeros(1).long().to(dev)}],
                          [{"video_name": c["vids"][k], "fid": c["ts"][k]}])
    assert len([x for x in w if "already been added" in str(x.message)]) >= 2
    assert repr(ev.evaluate()) == repr(want)
    try:
        ev.add_groundtruth(c["keys"][int(c["gt_img"][0])], [[0, 0, 1, 1]], [c["ids"][0]])
        raise AssertionError("a ground-truth key added twice must raise")
    except ValueError:
        pass
    cats = c["categories"]

    def raises(build):
        e = FrameMAP(cats, device=dev)
        e.add_groundtruth("v,0001", [[0.1, 0.1, 0.5, 0.5]], [c["ids"][0]])
        try:
            build(e)
            e.evaluate()
        except ValueError:
            return True
        return False

    one = lambda box, score, n=1: [{"boxes": torch.tensor([box] * n, dtype=torch.float32).to(dev), "scores": torch.full((n,), score).to(dev),
                                    "labels": torch.zeros(n).long().to(dev)}]
    info = [{"video_name": "v", "fid": 1}]
    assert not raises(lambda e: e.add_detections(one([0.1, 0.1, 0.5, 0.5], 0.9), info))
    assert raises(lambda e: e.add_detections_csv(io.StringIO("v,0001,0.1,0.1,0.5,0.5,%d,-10\n" % c["ids"][0])))
    assert raises(lambda e: e.add_detections(one([0.1, 0.1, 0.5, 0.5], 0.9, n=10001), info))
    assert not raises(lambda e: e.add_detections(one([0.1, 0.1, 0.5, 0.5], 0.9, n=10000), info))
    assert raises(lambda e: e.add_detections(one([0.1, 0.1, 0.5, float("nan")], 0.9), info))
    assert raises(lambda e: e.add_detections(one([0.1, 0.1, 0.5, 0.5], 1e-12), info))
    assert raises(lambda e: e.add_groundtruth("v,0002", [[0.5, 0.1, 0.5, 0.5]], [c["ids"][0]]))
    # an exclusion that arrives AFTER the key's ground truth and detections: evaluate() gives what it gives when the exclusions come first
    b = load_case(golden("eval_golden"), "B")
    gtb, detb, exb = csv_text(b)
    late = FrameMAP(b["categories"], device=dev)
    late.add_groundtruth_csv(io.StringIO(gtb))
    late.add_detections_csv(io.StringIO(detb))
    assert repr(late.evaluate()) != repr(frame_map_csv(b, dev).evaluate())
    late.add_groundtruth_csv(io.StringIO(""), io.StringIO(exb))
    check_frame_map(late, b, "FrameMAP B, exclusions last")
    # the label map reader does not hang on indentation or line breaks
    from step_amd.evaluate import read_labelmap
    assert read_labelmap(io.StringIO('item {\n name: "a (b)"\n    id: 7\n}\nlabel {\n\tname: "c/d"\n\tlabel_id: 12\n\tlabel_type: X\n}\nitem { name: "e" id: 3 }\n')) == (
        [{"id": 7, "name": "a (b)"}, {"id": 12, "name": "c/d"}, {"id": 3, "name": "e"}], {3, 7, 12})
    e = FrameMAP(cats, device=dev)
    e.add_groundtruth("v,0001", [[0.1, 0.1, 0.5, 0.5]], [c["ids"][0]])
    m = e.evaluate()
    assert m["PascalBoxes_Precision/mAP@0.5IOU"] == 0.0 and sum(1 for v in m.values() if v == 0.0) == 2
    with tempfile.TemporaryDirectory() as root:
        root = root + os.sep
        for name, text in (("ava_action_list_v2.1_for_activitynet_2018.pbtxt", labelmap_text(c)), ("ava_val_excluded_timestamps_v2.1.csv", ex),
                           ("ava_val_v2.1.csv", gt), ("other_gt.csv", gt), ("result.csv", det)):
            with open(root + name, "w") as f:
                f.write(text)
        assert repr(ava_evaluation(root, root + "result.csv", device=dev)) == repr(want)
        assert repr(ava_evaluation(root, root + "result.csv", root + "other_gt.csv", device=dev)) == repr(want)


MODULE_CASES = ["case_frame_map_golden", "case_frame_map_behaviours"]
