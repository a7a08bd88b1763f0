"""tools/make_merge_golden.py -- writes tests/golden/merge_golden.npz: what the reference's demo.py does with a clip's detections
behind the per-class NMS (demo.py:140-198 and the rows of :210-217), recorded for seeded histories.

Method (as oracle.make_golden.postprocess_main): demo.py is read where the reference lies at generation time; the lines between
`# do NMS first` and `# visualize results`, and the write loop behind `# write to files`, are compiled and executed once per
(iteration, clip) with the reference's own nms, valid_tubes and compute_box_iou.  This file holds no copy of that code.  Which row
joined which leader is recorded from the reference's own comparisons: compute_box_iou is wrapped, and a call (leader row, later row)
whose result is `> global_thresh` IS a join in the loop (demo.py:190-194); a row that joined nobody leads a cluster.

The fixture holds the input histories, and per case and (iteration, clip) group in list order: class, score and box of every row, the
list position of its leader, the merged boxes in cluster order and the text lines.  The conditions the tests rely on are asserted here
and their counts printed.  Needs the reference tree and its operators (oracle/_ref, built by __graft_entry__.build()); it is not run
by the tests, which read only the .npz.

    python tools/make_merge_golden.py
"""
import os
import sys
import textwrap
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import OUT, REF, import_reference  # noqa: E402

NC = 60


def person_history(seed, nums, frames, groups, active, special=None):
    """A seeded `history` of person-like detections: every clip has a few groups (people) of tubes whose middle-frame boxes are one box
    jittered by +-6 px and scaled x0.9-1.1; some groups stand next to an earlier one (shifted by a fraction of its width), so rows of
    different clusters overlap too.  Every tube scores in `active` classes: multiples of 1/16 (exact ties across classes) or free values,
    some under the confidence threshold; the rest of its classes stay under 0.01."""
    rs = np.random.RandomState(seed)
    N = int(sum(nums))
    hist = []
    for Tl in frames:
        mid = np.zeros((N, 4), np.float32)
        prob = (rs.randint(0, 8, (N, NC)) / 1024.0).astype(np.float32)          # (few distinct values: the file stays small)
        t0 = 0
        for b, n in enumerate(nums):
            ng = groups[b]
            base = []
            for k in range(ng):
                if k % 2 == 1 and rs.rand() < 0.7:                       # next to the group before: partial overlap between people
                    x1, y1, w, h = base[k - 1]
                    x1 = x1 + w * rs.uniform(0.12, 0.3) * rs.choice([-1, 1])
                    y1 = y1 + h * rs.uniform(-0.05, 0.05)
                else:
                    w, h = rs.uniform(70, 170), rs.uniform(130, 300)
                    x1, y1 = rs.uniform(-15, 400 - w + 15), rs.uniform(-15, 400 - h + 15)
                base.append((x1, y1, w, h))
            for j in range(n):
                x1, y1, w, h = base[j % ng]
                s = rs.uniform(0.9, 1.1, 2)
                d = rs.uniform(-6, 6, 4)
                cx, cy = x1 + w / 2, y1 + h / 2
                mid[t0 + j] = [cx - w * s[0] / 2 + d[0], cy - h * s[1] / 2 + d[1], cx + w * s[0] / 2 + d[2], cy + h * s[1] / 2 + d[3]]
                for c in rs.choice(NC, active, replace=False):
                    u = rs.uniform(0.25, 1.0)
                    prob[t0 + j, c] = np.round(u * 16) / 16 if rs.rand() < 0.6 else u
            t0 += n
        if special is not None:
            special(mid, prob, nums)
        loc = np.repeat(mid[:, None, :], Tl, axis=1) + rs.randint(-20, 21, (N, Tl, 1)).astype(np.float32)
        loc[:, Tl // 2] = mid
        hist.append({"pred_prob": np.repeat(prob[:, None, :], Tl, axis=1), "pred_loc": loc.astype(np.float32), "tubes_nums": list(nums)})
    return hist


NUMS_A = [34, 20, 11, 3, 2, 4]


def special_a(mid, prob, nums):
    """clip 3: no row; clip 4: exactly one row; clip 5: two rows in different classes whose IoU is exactly 0.5 ([0,0,.5,.5] and
    [0,0,.5,.25] once normalised) and two boxes under 3 px that valid_tubes replaces by the whole frame (one cluster of whole frames)"""
    s = np.cumsum([0] + list(nums))
    prob[s[3]:s[4]] = np.minimum(prob[s[3]:s[4]], 0.3)
    prob[s[4]:s[5]] = 0.002
    prob[s[4] + 1, 17] = 0.8125
    prob[s[5]:s[6]] = 0.002
    mid[s[5] + 0] = [0, 0, 200, 200]; prob[s[5] + 0, 3] = 0.75
    mid[s[5] + 1] = [0, 0, 200, 100]; prob[s[5] + 1, 11] = 0.75
    mid[s[5] + 2] = [50, 60, 51.5, 300]; prob[s[5] + 2, 20] = 0.625
    mid[s[5] + 3] = [120, 80, 330, 81]; prob[s[5] + 3, 41] = 0.9


HISTORIES = {
    "A": dict(seed=31, nums=NUMS_A, frames=(3, 9), groups=[5, 4, 3, 1, 1, 1], active=4, special=special_a),
    "B": dict(seed=32, nums=[64, 64], frames=(3,), groups=[14, 9], active=10),
    "C": dict(seed=33, nums=[70, 12], frames=(3,), groups=[14, 4], active=4),
}
# conf_thresh / global_thresh as demo.py:54-55 has them, one exactly representable threshold, the three top-k settings
CASES = {
    "all08": dict(hist="A", conf_thresh=0.4, global_thresh=0.8, evaluate_topk=-1, topk=-1),
    "all05": dict(hist="A", conf_thresh=0.4, global_thresh=0.5, evaluate_topk=-1, topk=-1),
    "top08": dict(hist="A", conf_thresh=0.4, global_thresh=0.8, evaluate_topk=1, topk=30),
    "topm1_05": dict(hist="A", conf_thresh=0.4, global_thresh=0.5, evaluate_topk=5, topk=-1),
    "big08": dict(hist="B", conf_thresh=0.01, global_thresh=0.8, evaluate_topk=-1, topk=-1),
    "general08": dict(hist="C", conf_thresh=0.4, global_thresh=0.8, evaluate_topk=-1, topk=-1),
    "general_top075": dict(hist="C", conf_thresh=0.4, global_thresh=0.75, evaluate_topk=1, topk=100),
}


def reference_slices():
    src = open(os.path.join(REF, "demo.py")).read().split("\n")
    find = lambda text, start=0: next(k for k, l in enumerate(src) if k >= start and l.strip() == text)
    a, b = find("# do NMS first"), find("# visualize results")
    c = find("# write to files")
    d = find("torch.cuda.synchronize()", c)
    comp = lambda lo, hi, tag: compile(textwrap.dedent("\n".join(src[lo:hi])), os.path.join(REF, "demo.py") + ":" + tag, "exec")
    return comp(a, b, "merge"), comp(c, d, "write")


def main():
    _, _, ref_nms, _ = import_reference()
    from utils.tube_utils import compute_box_iou as ref_iou, valid_tubes as ref_valid_tubes   # reference
    merge_code, write_code = reference_slices()
    g = {}
    hists = {}
    for name, kw in HISTORIES.items():
        hists[name] = person_history(**kw)
        g["hist%s_nums" % name] = np.asarray(kw["nums"], np.int32)
        for i, h in enumerate(hists[name]):
            g["hist%s_%d_prob" % (name, i)] = h["pred_prob"][:, 0].copy()
            g["hist%s_%d_loc" % (name, i)] = h["pred_loc"]
    g["cases"] = np.asarray(list(CASES))
    for tag, kw in CASES.items():
        nums = HISTORIES[kw["hist"]]["nums"]
        args = types.SimpleNamespace(num_classes=NC, nms_thresh=0.4, evaluate_topk=kw["evaluate_topk"], topk=kw["topk"],
                                     label_dict={c: c + 1 for c in range(NC)})
        thr = kw["global_thresh"]
        groups, rows, merged, lines = [], [], [], []
        distinct = leader_only = ties = clashes = 0
        for it, h in enumerate(hists[kw["hist"]]):
            prob = torch.from_numpy(h["pred_prob"].copy())
            loc = torch.from_numpy(h["pred_loc"].copy())
            prob, loc = prob[:, int(prob.shape[1] / 2)], loc[:, int(loc.shape[1] / 2)]                 # demo.py:124-127
            t0 = 0
            for b, n in enumerate(nums):
                joins = []

                def iou(box, box2):
                    r = ref_iou(box, box2)
                    joins.append((box.__array_interface__["data"][0], box2.__array_interface__["data"][0], bool(r > thr)))
                    return r

                ns = {"np": np, "nms": ref_nms, "valid_tubes": ref_valid_tubes, "compute_box_iou": iou, "args": args,
                      "conf_thresh": kw["conf_thresh"], "global_thresh": thr, "width": 400, "height": 400,
                      "cur_pred_prob": prob[t0:t0 + n], "cur_pred_tubes": loc[t0:t0 + n]}
                exec(merge_code, ns)
                t0 += n
                sl, all_boxes, mr = ns["scores_list"], ns["all_boxes"], ns["merged_result"]
                addr = {all_boxes[c][j].__array_interface__["data"][0]: p for p, (s, c, j) in enumerate(sl)}
                leader = np.arange(len(sl), dtype=np.int32)
                for a_, b_, joined in joins:
                    if joined:
                        assert leader[addr[b_]] == addr[b_] and leader[addr[a_]] == addr[a_] and addr[a_] < addr[b_]
                        leader[addr[b_]] = addr[a_]
                heads = [p for p in range(len(sl)) if leader[p] == p]
                assert len(heads) == len(mr), "two clusters share a merged box: the reference's dict kept one"
                assert [len(v) for v in mr.values()] == [int((leader == p).sum()) for p in heads]
                bx = np.asarray([all_boxes[c][j] for s, c, j in sl], np.float32).reshape(-1, 4)
                # a row that overlaps a MEMBER of an earlier cluster above the threshold (it did not overlap that cluster's leader, or it would be in it)
                M = ref_iou(bx, bx) if len(sl) else np.zeros((0, 0), np.float32)
                for p in range(len(sl)):
                    leader_only += any(leader[q] != q and leader[q] < leader[p] and M[q, p] > np.float32(thr) for q in range(len(sl)))
                for p in heads:
                    distinct += len({bx[q].tobytes() for q in range(len(sl)) if leader[q] == p}) >= 2
                sc = np.asarray([s for s, c, j in sl], np.float32)
                cls = np.asarray([c for s, c, j in sl], np.int32)
                ties += sum(1 for p in range(1, len(sl)) if sc[p] == sc[p - 1] and cls[p] != cls[p - 1])
                clashes += sum(1 for p in range(len(sl)) for q in range(p) if cls[p] != cls[q] and M[q, p] == np.float32(thr))
                out = []
                ws = {"np": np, "merged_result": mr, "info": {"video_name": "vid%d" % b, "fid": 900 + b},
                      "fout": types.SimpleNamespace(write=out.append)}
                exec(write_code, ws)
                groups.append([it, b, len(sl), len(heads)])
                rows.append(np.stack([cls, leader], 1))
                g.setdefault(tag + "_box", []).append(bx)
                g.setdefault(tag + "_score", []).append(sc)
                merged.append(np.asarray([k.split(",") for k in mr], np.float32).reshape(-1, 4))
                lines += out
        groups = np.asarray(groups, np.int32)
        g[tag + "_groups"] = groups                                   # (iteration, clip, rows, clusters) per group
        g[tag + "_rows"] = np.concatenate(rows).astype(np.int32)      # (class, list position of the leader) per row, list order
        g[tag + "_box"] = np.concatenate(g[tag + "_box"])
        g[tag + "_score"] = np.concatenate(g[tag + "_score"])
        g[tag + "_merged"] = np.concatenate(merged)
        g[tag + "_lines"] = np.frombuffer("".join(lines).encode(), np.uint8)            # (every line ends in "\n": one text, split by the tests)
        g[tag + "_cfg"] = np.asarray([kw["conf_thresh"], thr, kw["evaluate_topk"], kw["topk"]], np.float64)
        sizes = np.concatenate([np.bincount(r[:, 1], minlength=len(r))[np.unique(r[:, 1])] for r in rows if len(r)])
        print("%-14s groups %2d rows %4d (largest group %3d) clusters %3d (>= 2 distinct boxes: %3d, >= 3 members: %3d) leader-only rows %3d "
              "cross-class score ties next to each other %3d, cross-class pairs at exactly the threshold %d, empty groups %d, one-row groups %d"
              % (tag, len(groups), groups[:, 2].sum(), groups[:, 2].max(), groups[:, 3].sum(), distinct, int((sizes >= 3).sum()), leader_only,
                 ties, clashes, int((groups[:, 2] == 0).sum()), int((groups[:, 2] == 1).sum())))
        assert distinct >= 10 and leader_only >= 5, tag
        if kw["hist"] == "A":
            assert (groups[:, 2] == 0).any()
            assert (groups[:, 2] == 1).any() or (kw["evaluate_topk"] > 0 and kw["topk"] == -1)     # (`[:-1]` empties the one-row clip)
            whole = np.all(g[tag + "_merged"] == np.asarray([0, 0, 1, 1], np.float32), axis=1).sum()
            assert whole >= 1, "no cluster of whole-frame boxes"
            if thr == 0.5:
                assert clashes >= 1
            if kw["evaluate_topk"] > 0:
                assert ties >= 1
                if kw["topk"] > 0:
                    assert (groups[:, 2] == kw["topk"]).any()        # the cut really cuts
        if kw["hist"] == "B":
            assert groups[:, 2].max() > 256
        if kw["hist"] == "C":
            assert max(HISTORIES["C"]["nums"]) > 64
    path = os.path.join(OUT, "merge_golden.npz")
    np.savez_compressed(path, **g)
    print("merge_golden.npz: %d arrays, %d bytes" % (len(g), os.path.getsize(path)))


if __name__ == "__main__":
    main()
