"""tools/detect_block_bench.py -- what the workgroup form of step_detect_nms buys on clips of more than 64 tubes
(profiles/detect_block_timing.txt).  driver.postprocess over a three-iteration history of 4 clips x 84 tubes and 4 x 109 tubes (the
grids of --anchor_mode 3 and 4), NC = 60, conf_thresh 0.01, scores and boxes shaped like oracle.make_golden.postprocess_history; and
4 x 34 tubes, where the routing does not change.

Legs: driver.DETECT_BLOCK = False (the routing before the workgroup form: tensor operations around step_nms_batched) TWICE -- the
difference between the two identical legs is the spread a result has to beat -- and True.  ONE process, the legs interleaved round-robin
inside every round, warmed; per leg and round the median of `--calls` calls (host clock around a call that ends in a device
synchronise); reported: the median of the round medians with their min .. max.  Then, per leg, the device launches (kernels and copies,
torch.profiler) and the synchronising calls (torch.cuda.set_sync_debug_mode) of ONE call, and the launch alone: device events around
back-to-back ops.detect_nms calls at kmax = 109 and kmax = 1024.

    python tools/detect_block_bench.py [--rounds 5] [--calls 50] [--out profiles/detect_block_timing.txt]
"""
import argparse
import os
import statistics
import sys
import time
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import abkit  # noqa: E402

LEGS = (("False (a)", False), ("True", True), ("False (b)", False))


def history(seed, nums, dev):
    from oracle.make_golden import postprocess_history
    hist = []
    for h in postprocess_history(seed, nums, num_classes=60):
        hist.append({"pred_prob": torch.from_numpy(h["pred_prob"]).to(dev), "pred_loc": torch.from_numpy(h["pred_loc"]).to(dev),
                     "tubes_nums": list(nums)})
    return hist


def one_call(args, hist):
    from step_amd import driver
    driver.postprocess(args, hist)
    torch.cuda.synchronize()


def launches(fn):
    """device-side records (kernels, copies, fills) of one call"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA)


def syncs(fn):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return sum(1 for x in w if "synchronizing" in str(x.message) and "prototype" not in str(x.message))


def measure(say, name, nums, rounds, calls, dev):
    from step_amd import driver
    args = types.SimpleNamespace(image_size=(400, 400), num_classes=60, conf_thresh=0.01, nms_thresh=0.4, evaluate_topk=-1, topk=-1)
    hist = history(2025, nums, dev)
    rows = {}
    for leg, on in LEGS:                                         # warm: per-layout constants, workspaces, the allocator
        driver.DETECT_BLOCK = on
        for _ in range(10):
            res = driver.postprocess(args, hist)
        rows[leg] = [int(d["scores"].numel()) for clips in res for d in clips]
    assert rows["True"] == rows["False (a)"] == rows["False (b)"]
    med = {leg: [] for leg, _ in LEGS}
    for _ in range(rounds):
        for leg, on in LEGS:
            driver.DETECT_BLOCK = on
            ts = []
            for _ in range(calls):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                one_call(args, hist)
                ts.append((time.perf_counter() - t0) * 1e3)
            med[leg].append(statistics.median(ts))
    say("%s: %d rows over 3 iterations; postprocess, ms per call, median of %d round medians (min .. max), %d calls per leg and round"
        % (name, sum(rows["True"]), rounds, calls))
    for leg, on in LEGS:
        driver.DETECT_BLOCK = on
        say("    DETECT_BLOCK = %-9s  %.3f  (%.3f .. %.3f)   device launches per call %d, synchronising calls per call %d"
            % (leg, statistics.median(med[leg]), min(med[leg]), max(med[leg]), launches(lambda: one_call(args, hist)),
               syncs(lambda: driver.postprocess(args, hist))))
    fa, fb, tr = (statistics.median(med[leg]) for leg in ("False (a)", "False (b)", "True"))
    say("    spread between the two identical False legs %.3f ms; True against the mean of the False legs: %+.3f ms (x%.2f)"
        % (abs(fa - fb), tr - (fa + fb) / 2, (fa + fb) / 2 / tr))
    driver.DETECT_BLOCK = True


def kernel_alone(say, nums, dev, reps=200):
    from step_amd import ops
    h = history(2025, nums, dev)[0]
    B, kmax, NC = len(nums), max(nums), 60
    n = torch.as_tensor(nums, device=dev, dtype=torch.int32)
    start = (torch.cumsum(n, 0) - n).to(torch.int32)
    prob, loc = h["pred_prob"][:, 1].float(), h["pred_loc"][:, 1].float()
    keep = torch.empty((B, NC, kmax), dtype=torch.uint8, device=dev)
    call = lambda: ops.detect_nms(prob, loc, start, n, kmax, 0.01, 0.4, 400.0, 400.0, keep)
    abkit.event_ms(call, 10)
    per = [abkit.event_ms(call, reps) * 1e3 for _ in range(5)]
    masked = (prob > 0.01).sum(0)
    say("ops.detect_nms alone, %d clips x %d tubes, kmax %d, %d groups (kept %d of %d masked; most masked tubes in a class column %d): %.1f us per "
        "call incl. its box allocation, back to back (five windows: %s)"
        % (B, kmax, kmax, B * NC, int(keep.sum()), int((prob > 0.01).sum()), int(masked.max()), statistics.median(per),
           ", ".join("%.1f" % v for v in per)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect_block_timing.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    assert a.rounds >= 5 and a.calls >= 50, "at least 5 rounds x 50 calls"
    import step_amd  # noqa: F401
    dev = torch.device("cuda:0")
    say = abkit.tee(a.out)
    say("# tools/detect_block_bench.py on %s: driver.postprocess with and without the workgroup form of step_detect_nms" % torch.cuda.get_device_name(0))
    for name, nums in (("4 clips x 84 tubes (anchor mode 3)", [84] * 4), ("4 clips x 109 tubes (anchor mode 4)", [109] * 4),
                       ("4 clips x 34 tubes (the <= 64 path: same routing in every leg)", [34] * 4)):
        measure(say, name, nums, a.rounds, a.calls, dev)
    kernel_alone(say, [109] * 4, dev)
    kernel_alone(say, [1024] * 4, dev)
    say.close()


if __name__ == "__main__":
    main()
