"""tools/eval_map_bench.py -- timing of the frame-mAP evaluation on the device (step_amd.evaluate.FrameMAP) at the fixture's size and on
a seeded case scaled towards AVA's validation set, beside the numpy restatement of tests/eval_cases.py on the same rows on the host CPU.

Device events around repeated launches for step_eval_match, step_eval_ap and the two pairs of sorts; the host clock around evaluate()
calls, which end in their one synchronisation; medians and the spread (min .. max).  One process.

    python tools/eval_map_bench.py [--images 4000] [--rows 1000] [--out profiles/eval_map_timing.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from step_amd import ops  # noqa: E402
from step_amd.evaluate import FrameMAP  # noqa: E402
from tests import eval_cases as EV  # noqa: E402
from tools import abkit  # noqa: E402

NC = 60


def scaled_case(n_img, n_rows, seed=5):
    """per image 4-10 people with 1-3 actions each; detections: jittered copies of the people's boxes under their actions and others,
    and free boxes; boxes on the 1/1000 grid and scores on the 1/10000 grid, so that the fp32 rows round to themselves"""
    rs = np.random.RandomState(seed)
    images, gt = [], {}
    for k in range(n_img):
        m = rs.randint(4, 11)
        xy = rs.randint(0, 600, (m, 2))
        pb = np.concatenate([xy, xy + rs.randint(120, 400, (m, 2))], 1)
        acts = [rs.choice(NC, rs.randint(1, 4), replace=False) for _ in range(m)]
        gb = np.repeat(pb, [len(a) for a in acts], axis=0)
        key = "v%03d,%04d" % (k // 900, 902 + k % 900)
        gt[key] = (gb / 1000.0, np.concatenate(acts).astype(np.int32))
        n = n_rows + rs.randint(-n_rows // 10, n_rows // 10 + 1)
        who = rs.randint(0, m, n)
        db = pb[who] + rs.randint(-40, 41, (n, 4))
        free = rs.rand(n) < 0.3
        fxy = rs.randint(0, 700, (n, 2))
        db[free] = np.concatenate([fxy, fxy + rs.randint(50, 300, (n, 2))], 1)[free]
        cl = np.where(rs.rand(n) < 0.5, np.asarray([a[0] for a in acts])[who], rs.randint(0, NC, n)).astype(np.int32)
        images.append(dict(key=key, box=np.clip(db, 0, 1000) / 1000.0, score=rs.randint(100, 10000, n) / 10000.0, cls=cl))
    return dict(num_class=NC, images=images, gt=gt)


def build(rows, dev, per_call=200):
    ev = FrameMAP([{"id": i + 1, "name": "action %d" % (i + 1)} for i in range(NC)], device=dev)
    for key, (gb, gc) in rows["gt"].items():
        ev.add_groundtruth(key, gb, gc + 1)
    ims = rows["images"]
    for i0 in range(0, len(ims), per_call):
        dets = [{"boxes": torch.from_numpy(im["box"].astype(np.float32)).to(dev), "scores": torch.from_numpy(im["score"].astype(np.float32)).to(dev),
                 "labels": torch.from_numpy(im["cls"].astype(np.int64)).to(dev)} for im in ims[i0:i0 + per_call]]
        infos = [{"video_name": im["key"].split(",")[0], "fid": int(im["key"].split(",")[1])} for im in ims[i0:i0 + per_call]]
        ev.add_detections(dets, infos)
    return ev


def events(fn, reps):
    """`reps` single calls, each between device events of its own, after three warm calls (the list: fmt() reports median, min .. max)"""
    return [abkit.event_ms(fn, 1, warm=3 if r == 0 else 0) for r in range(reps)]            # (abkit's timer; the per-call list is this tool's)


def fmt(ts):
    return "median %9.3f ms  (min %9.3f .. max %9.3f, %d runs)" % (float(np.median(ts)), min(ts), max(ts), len(ts))


def measure(tag, rows, dev, reps, out):
    n_rows = sum(len(im["score"]) for im in rows["images"])
    out.append("%s: %d images, %d detection rows, %d ground-truth rows, %d classes" % (tag, len(rows["images"]), n_rows, sum(len(g[1]) for g in rows["gt"].values()), NC))
    ev = build(rows, dev)
    metrics, full = ev.evaluate(full=True)
    c = ev._prepare()
    boxes, score, cls, img = c["det"]
    o, det_start = ev._labelling_order(c)
    bo, cls_a, score_a = boxes[o].contiguous(), cls[o], score[o]
    match = lambda: ops.eval_match(bo, cls_a, det_start, c["gt_boxes"], c["gt_cls"], c["gt_start"], c["gt_max"], 0.5)
    label, _ = match()
    key, p, cls_start = ev._class_order(c, label, cls_a, score_a)
    label_b = label[p]
    out.append("  step_eval_match (one launch, %d workgroups)        %s" % (c["NI"], fmt(events(match, reps))))
    out.append("  step_eval_ap    (one launch, %d workgroups)          %s" % (NC, fmt(events(lambda: ops.eval_ap(cls_start, label_b, c["num_gt"]), reps))))
    out.append("  sorts: labelling order (score, image)              %s" % fmt(events(lambda: ev._labelling_order(c), reps)))
    out.append("  sorts: class-major order (score, class)            %s" % fmt(events(lambda: ev._class_order(c, label, cls_a, score_a), reps)))
    ts = [abkit.wall_ms(ev.evaluate, 1) for _ in range(reps)]
    out.append("  evaluate() (host clock, ends in its one copy)      %s" % fmt(ts))
    t_dev = float(np.median(ts))
    t0 = time.perf_counter()
    want = EV.np_evaluate(rows)
    t_np = (time.perf_counter() - t0) * 1e3
    out.append("  numpy restatement on the same rows, host CPU       %9.3f ms (one run; %.0f rows/s)" % (t_np, n_rows / t_np * 1e3))
    same = all(np.array_equal(full["labels"][k], want["labels"][k]) and np.array_equal(full["scores"][k], want["scores"][k]) for k in range(NC))
    d = float(np.nanmax(np.abs(full["ap"] - want["ap"])))
    out.append("  lists equal to the restatement's: %s; max |AP - restatement| %.3g; mAP %.6f; true positives %d"
               % (same, d, metrics["PascalBoxes_Precision/mAP@0.5IOU"], sum(int(l.sum()) for l in full["labels"])))
    out.append("  evaluate() is %.1fx %s than the numpy restatement (%.0f rows/s)" % (max(t_np / t_dev, t_dev / t_np), "faster" if t_dev < t_np else "SLOWER", n_rows / t_dev * 1e3))
    out.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4000)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_map_timing.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = ["frame-mAP evaluation on %s (tools/eval_map_bench.py --images %d --rows %d)" % (torch.cuda.get_device_name(0), a.images, a.rows), ""]
    measure("fixture size", scaled_case(120, 35, seed=4), dev, a.reps, out)
    measure("scaled case", scaled_case(a.images, a.rows), dev, a.reps, out)
    text = "\n".join(out)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
