"""tools/select_bench.py -- what the host's proposal selection costs inside the captured training iteration, and what the device-side
selection costs in its place (GPU only; writes profiles/select_device_timing.txt, quoted by DESIGN.md 3.12).

1. Iteration timing: C4SelectTrainStep (bf16) captured with selection="host" (graph F, train_select on the host, graph B -- twice: two
   identical legs give the run-to-run spread) and with selection="device" (ONE graph), interleaved round-robin in one process after
   warm-up; median and range over the rounds, for every --batches entry.
2. The host part alone: after a synchronised replay of graph F, the wall time of the host leg's selection (one launch and one
   device-to-host copy per later step, the sorts and draws, four pinned host-to-device copies per step) up to the synchronise behind it,
   and its share of the host leg's iteration.
3. The selection launches alone: the three DeviceSelector.select calls of one iteration recorded as a graph of their own on the static
   outputs of an eager front part, device events around its replays, and the number of library launches in it.

    python tools/select_bench.py [--batches 1,8] [--rounds 7] [--iters 10] [--out profiles/select_device_timing.txt]
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
from step_amd import ops, workloads  # noqa: E402


def build(dev, batch, selection):
    random.seed(1000)
    np.random.seed(1000)
    w = workloads.C4SelectTrainStep(dev, batch=batch, seed=123, dtype=torch.bfloat16, capturable=True, rng_seed=1, selection=selection)
    w.capture(warmup=3)
    return w


def iteration_timing(ws, names, a, lines, batch):
    times = [[] for _ in ws]
    for r in range(a.rounds + 1):
        for k, w in enumerate(ws):
            w.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                w.step()
            torch.cuda.synchronize()
            if r:
                times[k].append((time.perf_counter() - t0) / a.iters * 1e3)
    lines.append("captured iteration, bf16, %d clip(s): ms per iteration, median [min .. max] of %d interleaved rounds x %d iterations" % (batch, a.rounds, a.iters))
    for name, w, t in zip(names, ws, times):
        lines.append("  %-34s %8.3f  [%8.3f .. %8.3f]   %s" % (name, statistics.median(t), min(t), max(t), w.graph_mode))
    m = [statistics.median(t) for t in times]
    lines.append("  spread of the two identical host legs %.3f ms; device - host %+.3f ms (%+.1f %%)" % (abs(m[0] - m[1]), m[2] - min(m[0], m[1]),
                                                                                                      100 * (m[2] - min(m[0], m[1])) / min(m[0], m[1])))
    return m


def host_part(w, a, lines, iteration_ms):
    t = []
    for r in range(a.rounds * a.iters + 1):
        w._gF.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        w._select_part(w._front[2])
        torch.cuda.synchronize()
        if r:
            t.append((time.perf_counter() - t0) * 1e3)
        w._gB.replay()                                            # (keeps the trajectory that of a training run)
        torch.cuda.synchronize()
    med = statistics.median(t)
    lines.append("  host selection alone (graph F drained, then train_select x 3 and its copies, to the synchronise): %.3f ms  [%.3f .. %.3f]  = %.1f %% of the "
                 "host leg's iteration" % (med, min(t), max(t), 100 * med / iteration_ms))


def device_part(w, a, lines):
    calls = {"select_prepare": 0, "select_train": 0}
    orig = {k: getattr(ops, k) for k in calls}

    def counted(name):
        def f(*args, **kw):
            calls[name] += 1
            return orig[name](*args, **kw)
        return f
    with torch.no_grad():
        _, _, hist = w._front_part()
    torch.cuda.synchronize()
    for k in calls:
        setattr(ops, k, counted(k))
    try:
        w._select_part(hist)
    finally:
        for k in calls:
            setattr(ops, k, orig[k])
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        w._select_part(hist)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        w._select_part(hist)
    t, per = [], 50                                              # 50 replays per event pair: the selection, not the events' own cost
    for r in range(a.rounds + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        if r:
            t.append(e0.elapsed_time(e1) * 1e3 / per)
    lib = calls["select_prepare"] + 2 * calls["select_train"]
    lines.append("  device selection alone (3 steps as a graph of their own, 50 back-to-back replays per device-event pair): %.1f us per replay  [%.1f .. %.1f]; library launches per iteration %d "
                 "(%d x step_select_prepare, %d x step_select_train with its finishing kernel) + 2 torch copies per later step (pred_prob made dense, "
                 "the ground truths' middle frame)" % (statistics.median(t), min(t), max(t), lib, calls["select_prepare"], calls["select_train"]))
    lines.append("  rows selected in the last iteration per step: %s" % (w.selected,))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_device_timing.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/select_bench.py needs a ROCm device: it measures, and a measurement has no CPU fallback")
    dev = torch.device("cuda:0")
    lines = ["tools/select_bench.py --batches %s --rounds %d --iters %d   (%s)" % (a.batches, a.rounds, a.iters, torch.cuda.get_device_name(0))]
    names = ["host selection (graph F | host | graph B)", "host selection (again)", "device selection (one graph)"]
    for batch in (int(v) for v in a.batches.split(",")):
        ws = [build(dev, batch, "host"), build(dev, batch, "host"), build(dev, batch, "device")]
        m = iteration_timing(ws, names, a, lines, batch)
        host_part(ws[0], a, lines, m[0])
        device_part(ws[2], a, lines)
        lines.append("  host leg per iteration: 2 graph replays, 2 step_select_prepare launches, 2 device-to-host copies, 12 pinned host-to-device copies; "
                     "device leg: 1 graph replay, no copy")
        del ws
        torch.cuda.empty_cache()
    lines.append("record to compare with: 17.1 ms for the captured host-selection iteration at 1 clip (README)")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
