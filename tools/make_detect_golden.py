"""tools/make_detect_golden.py -- writes tests/golden/detect_block_golden.npz: what the reference's evaluation loop (test.py:157-218)
does with clips of MORE than 64 tubes -- 84 and 109 are the tube counts of --anchor_mode 3 and 4 -- recorded for a seeded history.

Method (as oracle.make_golden.postprocess_main, whose seeded history generator and reference import are used): test.py is read where the
reference lies at generation time; the lines of its evaluation loop are compiled and executed with the reference's own nms and
valid_tubes.  This file holds no copy of that code.  Every row the loop writes is recorded as (iteration, clip, class), box, score in
the order written; the text lines are not stored (postprocess_golden pins the CSV text already).

The conditions the tests rely on are asserted here: some (clip, class) group has more than 64 tubes above the confidence threshold,
and some group KEEPS more than 64 boxes after the NMS, so the survivors of one group span more than one wavefront.  Needs the reference
tree and its operators (oracle/_ref, built by __graft_entry__.build()); it is not run by the tests, which read only the .npz.

TIE ORDER.  The reference's operator orders the boxes with scores.sort(0, descending=True) (cpu/nms_cpu.cpp:48), which is not a stable
sort: which of two boxes with the SAME score comes first is unspecified, and the torch build decides (2.10 keeps the original order up
to 16 elements and scrambles equal scores beyond -- clips of at most 64 tubes with few ties never showed it).  This project pins "the
lower original index first" (oracle/step_oracle.c), and so does this generator: the loop gets the reference's own nms behind
a wrapper that hands it strictly decreasing surrogate scores in the stable descending order of the real ones -- same boxes, same
operator, same threshold, the order fixed.  How many of the operator's calls the pin changed is printed.

    python tools/make_detect_golden.py
"""
import os
import sys
import textwrap
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import OUT, REF, import_reference, postprocess_history  # noqa: E402

SEED, NUMS, NC = 2025, [84, 65, 0, 109], 12
CONF, NMS = 0.01, 0.4
CASES = {"all": dict(evaluate_topk=-1, topk=-1), "top20": dict(evaluate_topk=1, topk=20)}


def main():
    _, _, ref_nms, _ = import_reference()
    from utils.tube_utils import valid_tubes as ref_valid_tubes   # reference
    src = open(os.path.join(REF, "test.py")).read().split("\n")
    beg = next(k for k, l in enumerate(src) if l.strip() == "# loop for each  iteration")
    end = next(k for k, l in enumerate(src) if k > beg and l.strip() == "fout.close()")
    code = compile(textwrap.dedent("\n".join(src[beg:end])), os.path.join(REF, "test.py") + ":eval-loop", "exec")
    hist_np = postprocess_history(SEED, NUMS, num_classes=NC)
    calls = {"all": 0, "changed": 0}

    def pinned_nms(boxes, scores, thr):
        n = int(scores.shape[0])
        order = torch.sort(scores, dim=0, descending=True, stable=True).indices
        surrogate = torch.empty_like(scores)
        surrogate[order] = torch.arange(n, 0, -1, dtype=scores.dtype)           # exact in fp32, no two equal
        keep = ref_nms(boxes, surrogate, thr)
        calls["all"] += 1
        calls["changed"] += not torch.equal(keep, ref_nms(boxes, scores, thr))
        return keep

    g = {"nums": np.asarray(NUMS, np.int32), "cfg": np.asarray([CONF, NMS], np.float64)}
    for i, h in enumerate(hist_np):
        g["hist%d_prob" % i] = h["pred_prob"][:, 0].copy()
        g["hist%d_loc" % i] = h["pred_loc"]
    for tag, kw in CASES.items():
        args = types.SimpleNamespace(num_classes=NC, conf_thresh=CONF, nms_thresh=NMS, **kw)
        history = [{"pred_prob": torch.from_numpy(h["pred_prob"].copy()), "pred_loc": torch.from_numpy(h["pred_loc"].copy()),
                    "tubes_nums": list(NUMS)} for h in hist_np]
        rows = []

        class Sink:
            def __init__(self, ns):
                self.ns = ns

            def write(self, text):
                ns = self.ns                                     # the loop's own variables at the moment it writes a row
                rows.append([ns["i"], ns["b"], ns["cl_ind"]] + [float(v) for v in ns["box"]] + [float(ns["s"])])

        ns = {"np": np, "nms": pinned_nms, "valid_tubes": ref_valid_tubes, "args": args, "history": history,
              "infos": [{"video_name": "vid%d" % b, "fid": 900 + b} for b in range(len(NUMS))],
              "label_dict": {c: c + 1 for c in range(NC)}, "width": 400, "height": 400}
        ns["fouts"] = [Sink(ns) for _ in history]
        exec(code, ns)
        r = np.asarray(rows, np.float64)
        g[tag + "_meta"] = r[:, :3].astype(np.int32)
        g[tag + "_box"] = r[:, 3:7].astype(np.float32)
        g[tag + "_score"] = r[:, 7].astype(np.float32)
        print("detect_block", tag, "rows per iteration", np.bincount(g[tag + "_meta"][:, 0], minlength=len(hist_np)).tolist())
    # the properties the block form is tested on
    start = np.cumsum([0] + NUMS)
    meta = g["all_meta"]
    for i, h in enumerate(hist_np):
        masked = [int((h["pred_prob"][start[b]:start[b + 1], 0, c] > np.float32(CONF)).sum()) for b in range(len(NUMS)) for c in range(NC)]
        kept = np.bincount((meta[meta[:, 0] == i, 1] * NC + meta[meta[:, 0] == i, 2]), minlength=len(NUMS) * NC)
        print("iteration %d: groups over 64 masked %d (largest %d), largest kept %d" % (i, sum(m > 64 for m in masked), max(masked), kept.max()))
        assert max(masked) > 64, "no group with more than 64 masked tubes"
        assert kept.max() > 64, "no group keeps more than 64 boxes"
        assert all(k <= m for k, m in zip(kept, masked))
    print("nms calls %d, of which the tie-order pin changed the result of %d" % (calls["all"], calls["changed"]))
    path = os.path.join(OUT, "detect_block_golden.npz")
    np.savez_compressed(path, **g)
    print("detect_block_golden.npz: %d arrays, %d bytes" % (len(g), os.path.getsize(path)))
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()
