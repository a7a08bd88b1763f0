#!/usr/bin/env python
"""tools/cls_bench.py -- the classification pre-training iteration (workloads.C4ClsTrainStep; train_cls.py, stage 1) in its four forms,
interleaved in one process, at 1 and 4 clips per GPU (4 is scripts/train_cls.sh's batch size):

  (a) step()                     the ragged eager iteration with the head's torch chain tail (heads.FUSED_HEAD_OUTPUTS = False): the
                                 reference-shaped program from the pieces that existed before the stage was built -- the baseline
  (b) step_padded()              static shapes, eager, host sampling and selection
  (c) capture(), selection host  ONE graph; sampling and selection drawn on the host before each replay
  (d) capture(), selection device ONE graph with step_anchor_sample + step_select_train inside

plus the host cost of selection.sample_anchors per clip and the duration of the step_anchor_sample launch.  Every form is warmed up, then
timed in `--rounds` interleaved rounds of `--iters` iterations each, host clock around work that ends in a device synchronise; median
[min .. max] over the rounds.  Writes profiles/cls_train_timing.txt (or --out).

    python tools/cls_bench.py [--batches 1,4] [--rounds 5] [--iters 40] [--out PATH]
"""
import argparse
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40, help="iterations per timed round (40: 0.3-0.7 s of work per round and form)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cls_train_timing.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/cls_bench.py needs a ROCm device (a timing without one says nothing)")
    from step_amd import heads, ops, workloads
    from step_amd import rng as srng
    from step_amd.selection import sample_anchors

    dev = torch.device("cuda:0")
    lines = ["tools/cls_bench.py --batches %s --rounds %d --iters %d   (%s)" % (a.batches, a.rounds, a.iters, torch.cuda.get_device_name(0))]

    def emit(s_):
        print(s_, flush=True)
        lines.append(s_)

    for batch in (int(v) for v in a.batches.split(",")):
        random.seed(1)
        np.random.seed(1)
        mk = lambda **kw: workloads.C4ClsTrainStep(dev, batch=batch, seed=123, dtype=torch.bfloat16, rng_seed=3, **kw)
        wa, wb = mk(selection="host"), mk(selection="host")
        wc, wd = mk(selection="host", capturable=True), mk(selection="device", capturable=True)

        def ragged_chain():
            keep = heads.FUSED_HEAD_OUTPUTS
            heads.FUSED_HEAD_OUTPUTS = False
            try:
                return wa.step()
            finally:
                heads.FUSED_HEAD_OUTPUTS = keep

        wc.capture(warmup=a.warmup)
        wd.capture(warmup=a.warmup)
        forms = [("(a) ragged eager step(), chain tail", ragged_chain, "eager"), ("(b) step_padded(), eager", wb.step_padded, "eager"),
                 ("(c) captured, host selection", wc.step, wc.graph_mode), ("(d) captured, device selection", wd.step, wd.graph_mode)]
        for _, fn, _ in forms:
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _, _ in forms}
        for _ in range(a.rounds):
            for name, fn, _ in forms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.iters):
                    fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / a.iters * 1e3)
        emit("classification pre-training iteration, bf16, %d clip(s): ms per iteration, median [min .. max] of %d interleaved rounds x %d iterations"
             % (batch, a.rounds, a.iters))
        base = statistics.median(times[forms[0][0]])
        for name, _, mode in forms:
            t = times[name]
            med = statistics.median(t)
            emit("  %-40s %8.3f  [%8.3f .. %8.3f]   %-8s %+6.1f %% against (a)" % (name, med, min(t), max(t), mode, (med - base) / base * 100.0))
        emit("  rows per clip in the last iteration: (c) %s, (d) %s; final losses (a) %.4f (b) %.4f (c) %.4f (d) %.4f"
             % (wc.selected, wd.selected, float(wa.loss), float(wb.loss), float(wc.loss), float(wd.loss)))
        # the host's sampling alone: what the loader pays per clip (2 boxes, one positive + three negatives each)
        anchors = wa.gt[0][:, 0, :4].astype(np.float64) / 400.0
        n = 200
        t0 = time.perf_counter()
        for _ in range(n):
            sample_anchors(anchors, neg_ratio=3, mode="train")
        host_us = (time.perf_counter() - t0) / n * 1e6
        t0 = time.perf_counter()
        for _ in range(20):
            wa._host_selection()
        sel_us = (time.perf_counter() - t0) / 20 * 1e6
        per_clip = len(sample_anchors(anchors, neg_ratio=3, mode="train"))
        emit("  host: selection.sample_anchors %.0f us per clip of 2 boxes = %.1f us per sampled box (%d per clip); sampling + cls_select for the "
             "batch %.0f us per iteration" % (host_us, host_us / per_clip, per_clip, sel_us))
        # the launch alone: back-to-back launches between a device-event pair
        g = srng.DeviceRNG(dev, seed=5)
        out = tuple(torch.empty_like(t) for t in wd.selector.sampled)
        reps = 200
        for _ in range(10):
            ops.anchor_sample(wd.d_gt, wd.d_gt_count, g, 0, 400.0, 400.0, wd.Tl, 1, 3, out=out)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        dur = []
        for _ in range(5):
            e0.record()
            for _ in range(reps):
                ops.anchor_sample(wd.d_gt, wd.d_gt_count, g, 0, 400.0, 400.0, wd.Tl, 1, 3, out=out)
            e1.record()
            torch.cuda.synchronize()
            dur.append(e0.elapsed_time(e1) / reps * 1e3)
        emit("  step_anchor_sample, %d clip(s) x 2 boxes, %d back-to-back launches per device-event pair: %.1f us per launch  [%.1f .. %.1f] "
             "(launch-bound: includes the enqueue gap)" % (batch, reps, statistics.median(dur), min(dur), max(dur)))
        del wa, wb, wc, wd, forms
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
