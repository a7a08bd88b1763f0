"""Timing of the proposals recipe (padded slots with a device-side count) -- ONE process, forms alternated round by round, each form's own
spread (min .. max of the rounds) beside its median:

  * the training iteration, captured: C4SelectTrainStep(selection="device", proposals=34) against the anchor form at 34 tubes, the latter
    both on this tree's library and -- with tools/libstep_amd_prev.so present (tools/build_prev.sh) -- recorded on the PARENT's library
    (`--prev`: the parent's two entries stand in for the counted / tubes forms, whose new pointers are NULL on that path), at 1 and 8
    clips per GPU;
  * inference: GraphedInference(capacity=34) replayed on ragged lists of a given mean fill against the eager ragged driver.inference on
    the same lists (host wall time per batch up to the device's completion), for several fills.

    python tools/proposals_bench.py [--prev] [--out profiles/proposals_timing.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from step_amd import _lib, driver, workloads
from tools import abkit

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=10, help="timed iterations per form and round")
ap.add_argument("--prev", action="store_true", help="also record the anchor form on tools/libstep_amd_prev.so")
ap.add_argument("--batches", default="1,8")
ap.add_argument("--fills", default="0.25,0.5,0.75,1.0")
ap.add_argument("--skip-train", action="store_true")
ap.add_argument("--skip-inference", action="store_true")
a = ap.parse_args()
assert torch.cuda.is_available(), "tools/proposals_bench.py needs a ROCm device"
dev = torch.device("cuda:0")
say = abkit.tee(a.out)
wall = abkit.wall_ms


def prev_library():
    """the parent's library behind this tree's host layer: the two new entries fall back to the parent's own (their new pointers are NULL
    wherever the anchor form calls them)"""
    L = abkit.load_build("prev")
    L.step_select_train_counted = lambda *v: L.step_select_train(*v[:-2], v[-1])
    L.step_augment_plan_tubes = lambda *v: L.step_augment_plan(*v[:17], v[-1])
    return L


res = {}
if not a.skip_train:
    for batch in [int(v) for v in a.batches.split(",")]:
        forms = {}

        def build(**kw):
            torch.manual_seed(7)
            w = workloads.C4SelectTrainStep(dev, batch=batch, seed=123, dtype=torch.bfloat16, capturable=True, rng_seed=9, selection="device", **kw)
            return w.capture(warmup=3)

        if a.prev:
            with _lib.use(prev_library()):
                forms["anchors x 34, parent's library"] = build(tubes_per_clip=34)
        forms["anchors x 34, this library"] = build(tubes_per_clip=34)
        wp = build(proposals=34)
        forms["proposals=34 (counts %s)" % (wp.d_count.tolist(),)] = wp
        ms = {k: [] for k in forms}
        for w in forms.values():
            wall(w.step, 3)
        for _ in range(a.rounds):
            for k, w in forms.items():
                ms[k].append(wall(w.step, a.iters))
        say("C4SelectTrainStep, bf16, selection on the device, ONE graph per iteration, %d clip(s) per GPU; %d rounds x %d replays, alternated:" % (batch, a.rounds, a.iters))
        for k, v in ms.items():
            say("  %-60s median %.3f ms per iteration (min %.3f .. max %.3f)" % (k, float(np.median(v)), min(v), max(v)))
        res["train_%d" % batch] = ms
        del forms
        torch.cuda.empty_cache()

if not a.skip_inference:
    K, B = 34, 4
    w = workloads.C3Inference(dev, torch.bfloat16, batch=B, tubes=K, graph=False)
    rs = np.random.RandomState(5)

    def lists(fill):
        out = []
        for _ in range(B):
            n = int(np.clip(round(rs.normal(fill * K, 0.1 * K)), 0, K)) if fill < 1.0 else K
            xy = rs.uniform(10, 250, (n, 1, 2))
            out.append((np.concatenate([xy, xy + rs.uniform(60, 140, (n, 1, 2))], 2) + rs.uniform(-4, 4, (n, 3, 4))).astype(np.float32))
        return out

    gi = driver.GraphedInference(w.args, w.base, w.ctx, w.nets, w.x, lists(1.0), capacity=K)
    say("C3 inference, bf16, %d clips, capacity %d: GraphedInference(capacity) replay (copy of the slots + replay) against the eager ragged driver.inference "
        "on the same lists; wall time per batch, %d rounds x %d calls, alternated:" % (B, K, a.rounds, a.iters))
    for fill in [float(v) for v in a.fills.split(",")]:
        batches = [lists(fill) for _ in range(a.iters)]
        at = [0, 0]

        def padded():
            with torch.no_grad():
                gi(None, batches[at[0] % len(batches)])
            at[0] += 1

        def ragged():
            with torch.no_grad():
                cf = w.base(w.x)
                driver.inference(w.args, cf, w.ctx(cf), w.nets, 3, batches[at[1] % len(batches)])
            at[1] += 1

        forms = {"padded replay": padded, "eager ragged": ragged}
        for fn in forms.values():
            wall(fn, 3)
        ms = {k: [] for k in forms}
        for _ in range(a.rounds):
            for k, fn in forms.items():
                ms[k].append(wall(fn, a.iters))
        mean = float(np.mean([len(t) for b_ in batches for t in b_]))
        say("  mean fill %.2f (%.1f tubes per clip): " % (mean / K, mean) +
            "; ".join("%s median %.3f ms (min %.3f .. max %.3f)" % (k, float(np.median(v)), min(v), max(v)) for k, v in ms.items()))
        res["inference_fill_%.2f" % fill] = ms
say(json.dumps(res))
say.close()
