"""tools/make_eval_golden.py -- writes tests/golden/eval_golden.npz: what the reference's frame-mAP evaluator (utils/eval_utils.py:12-23 ->
external/ActivityNet/Evaluation/get_ava_performance.py run_evaluation -> PascalDetectionEvaluator) does with seeded rows.

Method: the reference's evaluator package is imported from where the reference lies at generation time; the four files of a case are
written as text (the detections in test.py:213's `{:.4}` format) and handed to the reference's run_evaluation, which is called as it
stands: its own readers, its own loops, its own PascalDetectionEvaluator -- for the call the class's __init__ is wrapped to keep the
instance, so that the evaluator's per-class lists can be recorded next to the dict it returns.  This file holds no copy of the
reference's code.  The vendored evaluator uses `np.float` and `np.NAN`, which numpy 2 no longer has: the two names are set on the numpy
module before the import, nothing else is adapted.

Recorded per case: the input rows (ground truth; detections as fp32 BEFORE the text and as the float64 the reference parsed from it; video
names, timestamps, label map, exclusions) and from the reference: per class the concatenated (score, label) lists, sorted descending by
score, num_gt_instances_per_class, AP per class, mAP, the returned dict.  Asserted here, counts printed: no two rows of one class have
equal score and different labels (so the reference's result does not hang on its unstable sort), and the reference's lists equal those of
the tie rule (tests/eval_cases.py np_evaluate).  Needs the reference tree; not run by the tests, which read only the .npz.

    python tools/make_eval_golden.py
"""
import contextlib
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import OUT, REF  # noqa: E402

f32 = np.float32
GRID = np.arange(100, 10000) / 10000.0            # the four-digit score grid: drawn per class WITHOUT replacement -> no ties inside a class


def jitter(rs, box, amount):
    w, h = box[2] - box[0], box[3] - box[1]
    return box + rs.uniform(-amount, amount, 4) * np.asarray([w, h, w, h])


def seeded_case(seed, n_img, ids, extra_ids=(), n_excl=0, silent_gt_id=None, gtless_det_id=None):
    """ground truth: 0-4 people per image with 1-3 actions each (the same box under several ids, as AVA has it); detections: per person
    a few jittered boxes with the person's actions and others, and free boxes; some images without ground truth, some without
    detections, a few invalid boxes.  silent_gt_id: an id that only ground truth uses; gtless_det_id: an id only detections use."""
    rs = np.random.RandomState(seed)
    ids = list(ids)
    draw_ids = [i for i in ids if i not in (silent_gt_id, gtless_det_id)]
    pool = {i: list(rs.permutation(GRID)) for i in set(ids) | set(extra_ids)}
    vids = ["vid%02d" % (k % 7) for k in range(n_img)]
    ts = [902 + k for k in range(n_img)]
    gt, det = [], []
    for k in range(n_img):
        people = []
        for _ in range(0 if k % 9 == 4 else rs.randint(1, 5)):
            x1, y1 = rs.uniform(0, 0.6, 2)
            people.append(np.asarray([x1, y1, x1 + rs.uniform(0.12, 0.38), y1 + rs.uniform(0.2, 0.4)]))
        acts = [list(rs.choice(draw_ids, rs.randint(1, 4), replace=False)) for _ in people]
        for b, a in zip(people, acts):
            for i in a:
                gt.append((k, b, i))
            if extra_ids and rs.rand() < 0.3:
                gt.append((k, b, int(rs.choice(extra_ids))))
            if silent_gt_id is not None and rs.rand() < 0.2:
                gt.append((k, b, silent_gt_id))
        if k % 11 == 7:
            continue                                                   # ground truth without detections
        for b, a in zip(people, acts):
            for _ in range(rs.randint(2, 7)):
                box = jitter(rs, b, rs.choice([0.03, 0.08, 0.25]))
                for i in set(a) | set(rs.choice(draw_ids, rs.randint(1, 5), replace=False)):
                    if rs.rand() < 0.75:
                        det.append((k, box, int(i)))
        for _ in range(rs.randint(2, 9)):
            x1, y1 = rs.uniform(0, 0.7, 2)
            box = np.asarray([x1, y1, x1 + rs.uniform(0.05, 0.3), y1 + rs.uniform(0.05, 0.3)])
            if rs.rand() < 0.06:
                box[2] = box[0] if rs.rand() < 0.5 else box[0] - 0.1   # invalid: empty or reversed
            for i in rs.choice(draw_ids, rs.randint(1, 4), replace=False):
                det.append((k, box, int(i)))
            if extra_ids and rs.rand() < 0.3:
                det.append((k, box, int(rs.choice(extra_ids))))
            if gtless_det_id is not None and rs.rand() < 0.3:
                det.append((k, box, gtless_det_id))
    gt_order = np.concatenate([np.flatnonzero(np.asarray([g[0] for g in gt]) == k) for k in rs.permutation(n_img)])   # another image order than the detections'
    gt = [gt[j] for j in gt_order]
    case = dict(vids=vids, ts=ts, ids=ids, excl=sorted(int(v) for v in rs.choice(n_img, n_excl, replace=False)),
                gt_img=np.asarray([g[0] for g in gt], np.int32), gt_box=np.round(np.asarray([g[1] for g in gt]), 3),
                gt_id=np.asarray([g[2] for g in gt], np.int32),
                det_img=np.asarray([d[0] for d in det], np.int32), det_box32=np.clip(np.asarray([d[1] for d in det]), 0.001, 1.0).astype(f32),
                det_id=np.asarray([d[2] for d in det], np.int32))
    case["det_score32"] = np.asarray([pool[int(i)].pop() for i in case["det_id"]], f32)
    return case


def tie_case():
    """Case C, by hand: score ties only between rows of a class that receive the SAME label -- false positives of one score inside an
    image and across images, true positives of one score in different images (each on its own box), and a class where everything ties."""
    P, Q = [0.1, 0.1, 0.4, 0.6], [0.5, 0.2, 0.9, 0.8]
    near = lambda b, d: [b[0] + d, b[1], b[2] + d, b[3]]
    far = [0.05, 0.7, 0.2, 0.95]
    gt = [(0, P, 3), (0, Q, 3), (1, P, 3), (2, Q, 5), (3, P, 5), (3, Q, 9), (4, P, 3)]
    det = [(0, near(P, 0.01), 3, 0.9), (0, near(Q, 0.01), 3, 0.9), (0, far, 3, 0.5), (0, far, 3, 0.5), (0, near(far, 0.01), 3, 0.5),
           (1, near(P, 0.02), 3, 0.9), (1, far, 3, 0.5), (1, near(P, 0.03), 3, 0.25),
           (2, near(Q, 0.01), 5, 0.75), (2, far, 7, 0.3125), (2, far, 7, 0.3125),
           (3, near(P, 0.01), 5, 0.75), (3, far, 7, 0.3125), (3, near(Q, 0.02), 9, 0.6), (3, near(Q, 0.3), 9, 0.7),
           (5, far, 3, 0.5), (5, P, 7, 0.3125), (5, Q, 5, 0.125), (5, far, 5, 0.125)]
    return dict(vids=["tie%d" % (k % 2) for k in range(6)], ts=[1000 + k for k in range(6)], ids=list(range(1, 11)), excl=[],
                gt_img=np.asarray([g[0] for g in gt], np.int32), gt_box=np.asarray([g[1] for g in gt], np.float64), gt_id=np.asarray([g[2] for g in gt], np.int32),
                det_img=np.asarray([d[0] for d in det], np.int32), det_box32=np.asarray([d[1] for d in det], f32), det_id=np.asarray([d[2] for d in det], np.int32),
                det_score32=np.asarray([d[3] for d in det], f32))


def named(text, name):
    f = io.StringIO(text)
    f.name = name
    return f


def run_reference(case, gap):
    """the four files as text -> the reference's run_evaluation, called as it stands; for the call the evaluator class's __init__ is
    wrapped to keep the instance (and two methods to note when the first detections arrive and when evaluate() returns: the time of the
    evaluator proper, without the parsing of the text); returns the evaluator and the dict"""
    from tests import eval_cases as EC
    c = dict(case, names=["action %02d (%s)" % (i, "abc"[i % 3]) for i in case["ids"]],
             keys=["%s,%04d" % (v, t) for v, t in zip(case["vids"], case["ts"])])
    gt_text, det_text, ex_text = EC.csv_text(c)
    cls, kept = gap.object_detection_evaluation.PascalDetectionEvaluator, {}
    init, add, evaluate = cls.__init__, cls.add_single_detected_image_info, cls.evaluate

    def keeping_init(self, *a, **kw):
        init(self, *a, **kw)
        kept["ev"] = self

    def timed_add(self, *a, **kw):
        kept.setdefault("t0", time.time())
        return add(self, *a, **kw)

    def timed_evaluate(self):
        out = evaluate(self)
        kept["t1"] = time.time()
        return out

    cls.__init__, cls.add_single_detected_image_info, cls.evaluate = keeping_init, timed_add, timed_evaluate
    try:
        with contextlib.redirect_stdout(io.StringIO()):               # (run_evaluation pretty-prints the dict)
            metrics = gap.run_evaluation(named(EC.labelmap_text(c), "labelmap.pbtxt"), named(gt_text, "gt.csv"), named(det_text, "det.csv"),
                                         named(ex_text, "excluded.csv"))
    finally:
        cls.__init__ = init
        del cls.add_single_detected_image_info, cls.evaluate          # (inherited: the class itself never had them)
    ev, dt = kept["ev"], kept["t1"] - kept["t0"]
    rows = int(np.isin(case["det_id"], case["ids"]).sum())
    # the float64 the reference parsed from the text, row for row (read once more without the label-map filter)
    boxes, _, scores = gap.read_csv(named(det_text, "det.csv"), None)
    parsed_box = np.zeros((len(case["det_id"]), 4), np.float64)
    parsed_score = np.zeros(len(case["det_id"]), np.float64)
    seen = {}
    for r, k in enumerate(case["det_img"]):
        key = "%s,%04d" % (case["vids"][k], case["ts"][k])
        j = seen.get(key, 0)
        seen[key] = j + 1
        y1, x1, y2, x2 = boxes[key][j]
        parsed_box[r] = [x1, y1, x2, y2]
        parsed_score[r] = scores[key][j]
    return c, ev, metrics, parsed_box, parsed_score, rows, dt


def main():
    np.float, np.NAN = float, np.nan                                   # numpy 2 dropped the two aliases the vendored evaluator uses
    sys.path.insert(0, REF)
    import external.ActivityNet.Evaluation.get_ava_performance as gap   # reference
    from tests import eval_cases as EC

    ava_like = [i for i in range(1, 81) if i % 4 != 2]                 # 60 of 1..80, like AVA's evaluated subset
    cases = {
        "A": seeded_case(41, 120, range(1, 61)),
        "B": seeded_case(42, 40, ava_like, extra_ids=[2, 6, 18, 50], n_excl=5, silent_gt_id=ava_like[7], gtless_det_id=ava_like[30]),
        "C": tie_case(),
    }
    g = {}
    for X, case in cases.items():
        c, ev, metrics, pbox, pscore, rows, dt = run_reference(case, gap)
        E = ev._evaluation
        NC = E.num_class
        scores, labels = [], []
        for k in range(NC):
            s = np.concatenate(E.scores_per_class[k]) if E.scores_per_class[k] else np.zeros(0)
            l = np.concatenate(E.tp_fp_labels_per_class[k]) if E.tp_fp_labels_per_class[k] else np.zeros(0, bool)
            o = np.argsort(s, kind="stable")[::-1]
            scores.append(s[o])
            labels.append(l[o].astype(np.uint8))
        mixed = sum(1 for k in range(NC) for s in np.unique(scores[k]) if len(np.unique(labels[k][scores[k] == s])) > 1)
        ties = sum(len(s) - len(np.unique(s)) for s in scores)
        assert mixed == 0, "%s: %d score values of a class carry both labels: the reference's result would hang on its unstable sort" % (X, mixed)
        c.update(det_box64=pbox, det_score64=pscore)
        res = EC.np_evaluate(EC.evaluated_rows(c))
        differ = sum(1 for k in range(NC) if not (np.array_equal(res["scores"][k], scores[k]) and np.array_equal(res["labels"][k], labels[k])))
        assert differ == 0 and np.array_equal(res["num_gt"], E.num_gt_instances_per_class), (X, differ)
        ap = np.asarray(E.average_precision_per_class, np.float64)
        d_ap = np.nanmax(np.abs(res["ap"] - ap))
        assert np.array_equal(EC.np_round_sig4(c["det_box32"]), pbox) and np.array_equal(EC.np_round_sig4(c["det_score32"]), pscore)
        invalid = int(np.sum(~((pbox[:, 1] < pbox[:, 3]) & (pbox[:, 0] < pbox[:, 2]))))
        claims = sum(int(np.sum(np.bincount(r["match"][r["match"] >= 0]) > 1)) for r in res["images"] if np.any(r["match"] >= 0))
        listed = np.asarray(c["ids"]) - 1
        print("%s: images %d, ground-truth rows %d, detection rows %d (%d evaluated, %d invalid boxes), classes with ground truth %d, "
              "AP == 0: %d, NaN among the listed: %d, tied rows %d (mixed labels %d), boxes claimed by several rows %d, classes whose lists "
              "differ from the tie rule's %d, max |AP restatement - reference| %.3g, mAP %.6f; reference: %.2f s, %.0f rows/s"
              % (X, len(c["vids"]), len(c["gt_id"]), len(c["det_id"]), rows, invalid, int(np.sum(E.num_gt_instances_per_class > 0)),
                 int(np.sum(ap[listed] == 0)), int(np.sum(np.isnan(ap[listed]))), ties, mixed, claims, differ, d_ap, metrics[list(metrics)[0]],
                 dt, rows / max(dt, 1e-9)))
        if X == "A":
            assert invalid >= 3 and claims >= 20
        if X == "B":
            assert np.sum(ap[listed] == 0) >= 1 and np.sum(np.isnan(ap[listed])) >= 1
        if X == "C":
            assert ties >= 6
        p = X + "_"
        for k in ("gt_img", "gt_id", "det_img", "det_id", "det_box32", "det_score32", "det_box64", "det_score64"):
            g[p + k] = c[k]
        g[p + "gt_box"] = c["gt_box"].astype(np.float64)
        g[p + "ids"], g[p + "names"] = np.asarray(c["ids"], np.int32), np.asarray(c["names"])
        g[p + "vids"], g[p + "ts"], g[p + "excl"] = np.asarray(c["vids"]), np.asarray(c["ts"], np.int32), np.asarray(c["excl"], np.int32)
        g[p + "ref_cls_start"] = np.cumsum([0] + [len(s) for s in scores]).astype(np.int64)
        g[p + "ref_scores"] = np.concatenate(scores)
        g[p + "ref_labels"] = np.concatenate(labels)
        g[p + "ref_num_gt"] = np.asarray(E.num_gt_instances_per_class, np.int64)
        g[p + "ref_ap"] = ap
        g[p + "ref_map"] = np.float64(metrics[list(metrics)[0]])
        g[p + "ref_dict_keys"] = np.asarray(list(metrics))
        g[p + "ref_dict_vals"] = np.asarray([float(v) for v in metrics.values()], np.float64)
    path = os.path.join(OUT, "eval_golden.npz")
    np.savez_compressed(path, **g)
    print("eval_golden.npz: %d arrays, %d bytes" % (len(g), os.path.getsize(path)))


if __name__ == "__main__":
    main()
