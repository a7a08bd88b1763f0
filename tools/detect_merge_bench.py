"""tools/detect_merge_bench.py -- what the cross-class merge costs on the GPU (profiles/detect_merge_timing.txt):
  (a) C3 history of 4 clips x 34 tubes x 3 iterations (hipGraph replay, bf16), conf_thresh 0.4, top-k 300
  (b) the fixture's largest group (tests/golden/merge_golden.npz, case big08: two clips of 64 tubes at conf_thresh 0.01)
per configuration: the step_detect_merge launch alone (device events around many back-to-back launches), the whole postprocess_merged
call and postprocess alone on the same history (host clock around calls that end in their own synchronisation, alternating), and the
numpy restatement of the host loop (tests.merge_cases.np_merge, vectorised per leader) on the same rows.  `--tree DIR` imports step_amd
from another checkout (a build of the commit before the merge: only postprocess is timed there).

    python tools/detect_merge_bench.py [--reps 200] [--skip-c3] [--tree DIR]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_ms(fn, reps):
    """median / min / max over `reps` calls, each ending in a device synchronise (the statistics are this tool's, the clock abkit's)"""
    from tools import abkit                        # (after main() has put --tree's step_amd first)
    ts = [abkit.wall_ms(fn, 1) for _ in range(reps)]
    return statistics.median(ts), min(ts), max(ts)


def measure(name, args, hist, kw, gthr, reps):
    from step_amd import driver, ops
    from tests import merge_cases as MG
    from tools import abkit

    merged = hasattr(driver, "postprocess_merged")
    plain = lambda: driver.postprocess(args, hist, **kw)
    both = (lambda: driver.postprocess_merged(args, hist, global_thresh=gthr, **kw)) if merged else None
    for _ in range(5):
        plain()
        if merged:
            both()
    # alternate the two calls, three rounds: the spread between rounds is the noise a difference has to beat
    for rnd in range(3):
        p = host_ms(plain, reps)
        line = "%s round %d: postprocess %.3f ms (min %.3f max %.3f)" % (name, rnd, *p)
        if merged:
            m = host_ms(both, reps)
            line += "   postprocess_merged %.3f ms (min %.3f max %.3f)   difference of medians %.3f ms" % (*m, m[0] - p[0])
        print(line, flush=True)
    if not merged:
        return
    # the launch alone, on the segments the call feeds it
    rows = driver.postprocess(args, hist, **kw)
    n = [int(d["scores"].numel()) for clips in rows for d in clips]
    cap = max(max(n), 1)
    G = len(n)
    seg = torch.zeros((G, cap, 4), device="cuda")
    for g, d in enumerate(d for clips in rows for d in clips):
        seg[g, :n[g]] = d["boxes"]
    cnt = torch.tensor(n, dtype=torch.int32, device="cuda")
    call = lambda: ops.detect_merge(seg, cnt, gthr)
    abkit.event_ms(call, 10)
    per = [abkit.event_ms(call, reps) * 1e3 for _ in range(5)]
    K = call()[3].tolist()
    print("%s: step_detect_merge, %d groups, rows per group %s, clusters per group %s: %.1f us per launch incl. its four output "
          "allocations, back to back (five windows: %s)" % (name, G, n, K, statistics.median(per), ", ".join("%.1f" % v for v in per)), flush=True)
    boxes = [d["boxes"].cpu().numpy() for clips in rows for d in clips]
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        for b in boxes:
            MG.np_merge(b, gthr)
        ts.append((time.perf_counter() - t0) * 1e3)
    print("%s: numpy restatement of the host loop on the same rows (all %d groups, after their copy to the host): %.2f ms (of 3: %s)"
          % (name, G, statistics.median(ts), ", ".join("%.2f" % v for v in ts)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--skip-c3", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)                       # tests.merge_cases (the fixture's accessors, np_merge)
    sys.path.insert(0, os.path.abspath(a.tree))    # step_amd
    import step_amd
    from step_amd import driver
    from tests import merge_cases as MG

    assert torch.cuda.is_available(), "needs the GPU"
    print("device %s, step_amd from %s, postprocess_merged present: %s"
          % (torch.cuda.get_device_name(0), os.path.relpath(os.path.dirname(step_amd.__file__), ROOT), hasattr(driver, "postprocess_merged")))
    g = np.load(os.path.join(ROOT, "tests", "golden", "merge_golden.npz"))
    hist, nums = MG.fixture_history(g, "B", "cuda")
    conf, thr, etopk, topk = MG.case_cfg(g, "big08")
    measure("(b) fixture big08 (2 clips x 64 tubes, conf 0.01)", MG._args(conf_thresh=conf, evaluate_topk=etopk, topk=topk), hist, {}, thr, a.reps)
    if not a.skip_c3:
        from step_amd import workloads
        w = workloads.C3Inference(torch.device("cuda:0"), torch.bfloat16, batch=4, tubes=34, graph=True)
        with torch.no_grad():
            hist = w.launch()
        torch.cuda.synchronize()
        measure("(a) C3 4 clips x 34 tubes x 3 iterations, conf 0.4, top-k 300", w.args, hist, dict(conf_thresh=0.4, evaluate_topk=1, topk=300), 0.8, a.reps)


if __name__ == "__main__":
    main()
