"""Timing of the tube growth per temporal_mode (predict | extrapolate | mean) -- ONE process, variants interleaved round by round on
abkit's timers, each variant's own spread (min .. max of its rounds) beside its median:

  * inference, 4 clips x 34 tubes, bf16, three refinement steps: the eager driver.inference_flat on a resident backbone feature (host wall
    time per call up to the device's completion) and the GraphedInference replay (backbone + ContextNet + the three steps), each with
    driver.TUBE_KERNEL True (step_tube_update / step_tube_update_mode: one launch per step) and False (the tensor-op restatement);
  * the training iteration, one clip, bf16, captured: C4SelectTrainStep(selection="device") -- ONE graph -- against the host selection's
    split form of the same mode.

    python tools/tube_mode_bench.py [--out profiles/tube_modes_timing.txt]      (the default)
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from step_amd import driver, workloads
from tools import abkit

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tube_modes_timing.txt"))
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=30, help="timed calls per variant, leg and round")
ap.add_argument("--modes", default="predict,extrapolate,mean")
ap.add_argument("--skip-train", action="store_true")
ap.add_argument("--skip-inference", action="store_true")
a = ap.parse_args()
assert torch.cuda.is_available(), "tools/tube_mode_bench.py needs a ROCm device"
dev = torch.device("cuda:0")
say = abkit.tee(a.out)
modes = [m for m in a.modes.split(",") if m]
res = {}


def line(name, t):
    return "  %-46s median %8.3f ms (min %8.3f .. max %8.3f)" % (name, t.median, t.min, t[-1])


def verdict(on, off):
    """the kernel variant against the off variant's own spread over its interleaved repeats"""
    spread = off[-1] - off.min
    d = on.median - off.median
    return "kernel %+.3f ms against off (off's spread %.3f ms): %s" % (d, spread, "slower beyond the spread" if d > spread else "not slower")


if not a.skip_inference:
    B, K = 4, 34
    w = workloads.C3Inference(dev, torch.bfloat16, batch=B, tubes=K, graph=False)
    flat, nums = driver._flat_tubes(w.tubes, dev)
    clip_of = torch.as_tensor(np.repeat(np.arange(B), nums), device=dev)
    with torch.no_grad():
        cf = w.base(w.x)
        cx = w.ctx(cf)

    class Form:
        def __init__(self, mode, kernel):
            self.mode, self.kernel = mode, kernel
            self.args = copy.copy(w.args)
            self.args.temporal_mode = mode
            driver.TUBE_KERNEL = kernel
            try:
                with torch.no_grad():
                    self.graphed = driver.GraphedInference(self.args, w.base, w.ctx, w.nets, w.x, w.tubes)
            finally:
                driver.TUBE_KERNEL = True

        def eager(self):
            driver.TUBE_KERNEL = self.kernel
            try:
                with torch.no_grad():
                    driver.inference_flat(self.args, cf, cx, w.nets, 3, flat, nums, clip_of, want_classes=False)
            finally:
                driver.TUBE_KERNEL = True

    forms = [Form(m, k) for m in modes for k in (True, False)]
    legs = {"eager": lambda f: abkit.wall_ms(f.eager, a.iters, warm=3), "replay": lambda f: abkit.wall_ms(f.graphed, a.iters, warm=3)}
    times = abkit.interleave(forms, legs, a.rounds)
    say("inference, bf16, %d clips x %d tubes, three refinement steps; %d rounds x %d calls, variants interleaved:" % (B, K, a.rounds, a.iters))
    for leg, what in (("eager", "eager inference_flat (the three steps on a resident feature)"), ("replay", "GraphedInference replay (backbone + ContextNet + the steps)")):
        say(" %s:" % what)
        for f, t in zip(forms, times):
            say(line("%s, TUBE_KERNEL %s" % (f.mode, f.kernel), t[leg]))
            res["%s_%s_kernel_%s" % (leg, f.mode, f.kernel)] = list(t[leg])
        for m in modes:
            on, off = [t[leg] for f, t in zip(forms, times) if f.mode == m]
            say("  %s: %s" % (m, verdict(on, off)))
    del forms, w
    torch.cuda.empty_cache()

if not a.skip_train:
    def build(mode, selection):
        torch.manual_seed(7)
        t = workloads.C4SelectTrainStep(dev, batch=1, seed=123, dtype=torch.bfloat16, capturable=True, rng_seed=9, selection=selection, temporal_mode=mode)
        t.capture(warmup=3)
        return t

    steps = [(m, s, build(m, s)) for m in modes for s in ("device", "host")]
    times = abkit.interleave(steps, {"step": lambda v: abkit.wall_ms(v[2].step, max(a.iters // 3, 5), warm=2)}, a.rounds)
    say("training iteration, C4SelectTrainStep, bf16, 1 clip, captured; %d rounds x %d iterations, variants interleaved:" % (a.rounds, max(a.iters // 3, 5)))
    for (m, s, t), tm in zip(steps, times):
        say(line("%s, selection %s (%s)" % (m, s, t.graph_mode), tm["step"]))
        res["train_%s_%s" % (m, s)] = list(tm["step"])
say(json.dumps(res))
say.close()
