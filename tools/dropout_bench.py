"""tools/dropout_bench.py -- what the device-side dropout costs (GPU only; writes profiles/dropout_timing.txt, quoted by DESIGN.md 3.11).

1. Kernel rate: step_dropout_forward / step_dropout_backward at the C4 call-site sizes (8 clips x 15 tubes, Tl = 3 and Tl = 9 frames of
   12544 features; bf16 and fp32), as a HIP graph of back-to-back calls (what the captured step replays), over a ring of buffers larger
   than the last-level cache and again on ONE buffer pair (the call site's input was written by the launch before it), next to
   step_hbm_stream_probe's copy rate from the same process.  Bytes are the algorithm's: forward reads n and writes n elements + n / 8 mask
   bytes, backward reads n elements + n / 8 and writes n.
2. Step timing: the C4 bf16 step at dropout 0, dropout 0.3 on the device path (twice: two identical legs give the run-to-run spread) and
   dropout 0.3 with torch.nn.Dropout (heads.DEVICE_DROPOUT = False, what STEP_TORCH_DROPOUT=1 selects), interleaved round-robin in one
   process, as captured and as eager steps; median and range over the rounds.
3. Mask memory per step.

    python tools/dropout_bench.py [--batch 8] [--tubes 15] [--rounds 7] [--iters 10] [--out profiles/dropout_timing.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from step_amd import _capi, _lib, heads, ops, rng, workloads  # noqa: E402
from tools import abkit  # noqa: E402


def hbm_copy_rate(dev):
    L = _lib.lib()
    nbytes = 1 << 30
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev).random_(0, 255)
    dst = torch.empty_like(src)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    probe = lambda: _capi.check(L.step_hbm_stream_probe(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), nbytes, cus * 16, _lib.stream_ptr(dev)),
                                "step_hbm_stream_probe")
    probe()
    return 2 * nbytes / (min(abkit.event_ms(probe, 1) for _ in range(5)) * 1e-3)


def graph_time(fn, calls, reps=5):
    """microseconds per call of `fn(k)`, k = 0 .. calls - 1 recorded back to back in one graph; best of `reps` replays after a warm-up
    (its own: it builds the graph of indexed calls that it times, which abkit's timers do not)"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn(0)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for k in range(calls):
            fn(k)
    g.replay()
    return min(abkit.event_ms(g.replay, 1) for _ in range(reps)) * 1e3 / calls


def kernel_rates(dev, a, lines, copy_rate):
    g = rng.DeviceRNG(dev, seed=1)
    lines.append("kernel rate (HIP graph of back-to-back calls, best of 5 replays; the forward figure includes its one-thread offset kernel)")
    lines.append("  %-34s %10s %10s %10s %12s" % ("call", "us", "GB/s", "of copy", "buffers"))
    for Tl in (3, 9):
        n = a.batch * a.tubes * Tl * 12544
        for dt, es in ((torch.bfloat16, 2), (torch.float32, 4)):
            ring = max(2, int(768e6 // (2 * n * es)) + 1)                   # in + out of the ring > 3 x the 256 MB last-level cache
            for tag, nbuf in (("ring", ring), ("one", 1)):
                xs = [torch.randn(n, device=dev).to(dt) for _ in range(nbuf)]
                ys = [torch.empty_like(x) for x in xs]
                masks = [None] * nbuf

                def fwd(k):
                    _, masks[k % nbuf] = ops.dropout(xs[k % nbuf], 0.3, g, out=ys[k % nbuf])

                calls = max(20, 2 * nbuf)
                us_f = graph_time(fwd, calls)

                def bwd(k):
                    _capi.check(_lib.lib().step_dropout_backward(ops._dt(xs[0]), _lib.dptr(ys[k % nbuf]), _lib.dptr(xs[k % nbuf]), _lib.dptr(masks[k % nbuf]), n, 0.3,
                                                                 _lib.stream_ptr(dev)), "step_dropout_backward")
                for k in range(nbuf):
                    fwd(k)
                us_b = graph_time(bwd, calls)
                for name, us in (("forward", us_f), ("backward", us_b)):
                    rate = (2 * n * es + n // 8) / (us * 1e-6)
                    lines.append("  %-34s %10.2f %10.0f %9.0f%% %12s" % ("%s Tl=%d %s n=%d" % (name, Tl, str(dt).split(".")[1], n), us, rate / 1e9,
                                                                        100 * rate / copy_rate, "%s (%d)" % (tag, nbuf)))
                del xs, ys, masks
                torch.cuda.empty_cache()


def step_timing(dev, a, lines):
    legs = [("dropout 0", 0.0, True), ("dropout 0.3 device", 0.3, True), ("dropout 0.3 device (again)", 0.3, True), ("dropout 0.3 torch", 0.3, False)]
    ws = []
    for name, p, device_path in legs:
        heads.DEVICE_DROPOUT = device_path
        try:
            w = workloads.C4TrainStep(dev, batch=a.batch, tubes_per_clip=a.tubes, dtype=torch.bfloat16, capturable=True, dropout=p, rng_seed=1)
        finally:
            heads.DEVICE_DROPOUT = True
        want = (heads.Dropout if device_path else torch.nn.Dropout)
        assert type(w.heads[0].dropout) is want, (name, type(w.heads[0].dropout))
        w.capture(warmup=3)
        ws.append(w)
    for form in ("captured", "eager"):
        times = [[] for _ in legs]
        for r in range(a.rounds + 1):
            for k, w in enumerate(ws):
                ms = abkit.wall_ms(w.step if form == "captured" else w._eager_step, a.iters, warm=1)
                if r:
                    times[k].append(ms)
        lines.append("C4 bf16 step, %d clips x %d tubes, %s: ms per step, median [min .. max] of %d interleaved rounds x %d steps" % (a.batch, a.tubes, form, a.rounds, a.iters))
        for (name, _, _), t in zip(legs, times):
            lines.append("  %-30s %8.3f  [%8.3f .. %8.3f]" % (name, statistics.median(t), min(t), max(t)))
        m = [statistics.median(t) for t in times]
        lines.append("  spread of the two identical legs %.3f ms; device - torch %+.3f ms; device - dropout 0 %+.3f ms" % (abs(m[1] - m[2]), min(m[1], m[2]) - m[3], min(m[1], m[2]) - m[0]))
    lines.append("generator offset after the device legs: %d" % ws[1].rng.offset())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--tubes", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dropout_timing.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/dropout_bench.py needs a ROCm device: it measures, and a measurement has no CPU fallback")
    dev = torch.device("cuda:0")
    lines = ["tools/dropout_bench.py --batch %d --tubes %d --rounds %d --iters %d   (%s)" % (a.batch, a.tubes, a.rounds, a.iters, torch.cuda.get_device_name(0))]
    copy_rate = hbm_copy_rate(dev)
    lines.append("step_hbm_stream_probe (1 GiB read + 1 GiB written, best of 5, this process): %.0f GB/s" % (copy_rate / 1e9))
    kernel_rates(dev, a, lines, copy_rate)
    sites = [a.batch * a.tubes * Tl * (12544 + 1024 + 12544) for Tl in (3, 3, 9)]
    n = sum(sites)
    lines.append("mask memory per step (3 heads x 3 sites, %d elements): %.2f MB as bits (n / 8) against %.2f MB for one byte per element (torch's bool mask)"
                 % (n, n / 8 / 1e6, n / 1e6))
    if not a.skip_steps:
        step_timing(dev, a, lines)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
