"""tools/clip_bench.py -- what gradient-norm clipping and the device learning-rate schedule cost on the MI355X, in ONE process with the
legs alternated; every figure is median [min .. max] over the rounds.  Writes profiles/grad_clip_timing.txt (--out).

  1. the passes alone, on the C4 workload's own gradient arena layout (C4TrainStep's FlatAdam: its element count and segment table): the
     norm pass (streaming launch + finishing launch), the clip pass (active, and with a coefficient of 1), against
     step_hbm_stream_probe over the same bytes and against grad_scan_kernel over the same arena (reached through step_sgd_flat_amp on
     an arena that holds an inf: the scan, then an update that skips without touching memory, then the one-thread scale update).  The
     legs rotate over three arenas (~600 MB together) so that no pass finds its input in the 256 MB last-level cache;
  2. the captured C4 iteration at 1 and 8 clips: the parent form (host lr table, no clip) twice for its spread, norm pass only (a huge
     max_norm), clip active (a tiny max_norm), device schedule;
  3. the torch way, eager: torch.nn.utils.clip_grad_norm_ over the arena's views, for scale (host wall time, synchronised)."""
import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import step_amd  # noqa: E402
from step_amd import _capi, _lib, ops, workloads  # noqa: E402

def fmt(v):
    return "%8.3f [%8.3f .. %8.3f]" % (statistics.median(v), min(v), max(v))


def event_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(n):
        fn(k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def c4_layout(dev):
    """(elements, device seg_end table, [(offset, numel)] of the tensors) of the C4 training step's gradient arena"""
    w = workloads.C4TrainStep(dev, batch=1, tubes_per_clip=5, seed=123, dtype=torch.bfloat16)
    lay = (w.opt.numel, w.opt._seg_end.clone(), [(o, k) for _, _, o, k in w.opt._entries])
    del w
    torch.cuda.empty_cache()
    return lay


def passes(dev, rounds, iters, out):
    L = _lib.lib()
    st = _lib.stream_ptr(dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    n, ends, tensors = c4_layout(dev)
    nseg = len(tensors)
    torch.manual_seed(0)
    arenas = [torch.randn(n, device=dev) for _ in range(3)]
    dst = torch.empty(n, device=dev)
    ws = ops.grad_norm_workspace(n, nseg, dev)
    seg, stats = torch.zeros(nseg, device=dev), torch.zeros(4, device=dev)
    half, twice, one = (torch.tensor([1.0, c, 0.0, 0.0], device=dev) for c in (0.5, 2.0, 1.0))
    # grad_scan: an arena set whose first element is inf, so that the update behind the scan skips (no memory traffic of its own)
    bad = [a.clone() for a in arenas]
    for b in bad:
        b[0] = float("inf")
    lr, wd = torch.zeros(nseg, device=dev), torch.zeros(nseg, device=dev)
    cnt, amp = torch.zeros(1, dtype=torch.int64, device=dev), torch.tensor([1024.0, 0.0, 0.0, 0.0], device=dev)
    param, buf = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    params = [torch.nn.Parameter(torch.empty(k, device=dev)) for _, k in tensors]     # the torch way: one view of arena 0 per tensor as .grad
    for p, (o, k) in zip(params, tensors):
        p.grad = arenas[0][o:o + k]

    def probe(k):
        _capi.check(L.step_hbm_stream_probe(vp(arenas[k % 3]), vp(dst), 4 * n, 256 * 8, st), "probe")

    def scan(k):
        _capi.check(L.step_sgd_flat_amp(vp(param), vp(bad[k % 3]), vp(buf), n, vp(ends), vp(lr), vp(wd), nseg, 0.9, 0.0, 0, vp(cnt), 1.0, 0, vp(amp),
                                        2.0, 1.0, 1000, st), "scan")

    def norm(k):
        _capi.check(L.step_grad_norm_flat(vp(arenas[k % 3]), n, vp(ends), nseg, 1.0, None, 1e30, vp(ws), ws.numel() * 8, vp(seg), vp(stats), st), "norm")

    def clip(k):                                                 # x 0.5 and x 2 in turn over each arena: the values stay where they are
        _capi.check(L.step_grad_clip_flat(vp(arenas[k % 3]), n, vp(half if (k // 3) % 2 == 0 else twice), st), "clip")

    def clip_off(k):
        _capi.check(L.step_grad_clip_flat(vp(arenas[k % 3]), n, vp(one), st), "clip")

    legs = [("step_hbm_stream_probe, copy of the arena", probe, 8), ("grad_scan_kernel (+ skipped update, scale update)", scan, 4),
            ("norm pass: partial + finish launches", norm, 4), ("clip pass, active (read + write)", clip, 8), ("clip pass, coefficient 1", clip_off, 0)]
    iters6 = -(-iters // 6) * 6                                  # the clip leg restores the arenas every 6 calls
    for _, fn, _ in legs:
        for k in range(6):
            fn(k)
    torch.cuda.synchronize()
    t = {name: [] for name, _, _ in legs}
    for _ in range(rounds):
        for name, fn, _ in legs:
            t[name].append(event_ms(fn, iters6))
    out.append("1. the passes alone: %d elements (%.1f MB) in %d segments, %d rounds x %d calls, rotating over 3 arenas (%.0f MB)" % (n, 4 * n / 1e6, nseg, rounds, iters6, 12 * n / 1e6))
    for name, _, bpe in legs:
        med = statistics.median(t[name])
        rate = "%7.0f GB/s at %d B/element" % (bpe * n / med / 1e6, bpe) if bpe else ""
        out.append("   %-52s %s us   %s" % (name, fmt([v * 1e3 for v in t[name]]), rate))
    out.append("   norm pass / grad_scan (medians): %.2f" % (statistics.median(t[legs[2][0]]) / statistics.median(t[legs[1][0]])))
    # 3. torch, eager
    tt = []
    for r in range(max(rounds, 3)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch.nn.utils.clip_grad_norm_(params, 1e30)
        torch.cuda.synchronize()
        tt.append((time.perf_counter() - t0) * 1e3)
    out.append("3. torch.nn.utils.clip_grad_norm_ over the %d views, eager, wall: %s ms" % (nseg, fmt(tt[1:])))


SCHED = dict(milestones=[100000, 200000], min_ratio=0.01, cycle_decay=0.5, warmup_iters=1000, warmup_factor=0.1)


def iteration(dev, batch, rounds, iters, out):
    """ONE workload, one captured graph per leg (the re-pack launch of a step covers every live network, so several workloads side by side
    would pay for each other's weights): a leg is selected by putting its graph and its settings back on the workload."""
    w = workloads.C4TrainStep(dev, batch=batch, tubes_per_clip=5, seed=123, dtype=torch.bfloat16, capturable=True)
    sched = [None]

    def settings(max_grad_norm=None, scheduled=False):
        if scheduled and sched[0] is None:
            sched[0] = step_amd.DeviceWarmupCosineLR(w.opt, **SCHED)
        w.max_grad_norm = max_grad_norm
        w.sched = w.opt.lr_scheduler = sched[0] if scheduled else None
        w.opt._tables = None

    legs = [("parent form (host lr table, no clip) A", {}), ("parent form (host lr table, no clip) B", {}),
            ("norm pass only (max_grad_norm 1e30)", dict(max_grad_norm=1e30)), ("clip active (max_grad_norm 1e-3)", dict(max_grad_norm=1e-3)),
            ("device schedule (cosine)", dict(scheduled=True))]
    graphs = []
    for name, kw in legs:
        settings(**kw)
        w.graph = None
        w.capture(warmup=2)
        graphs.append(w.graph)
    t = {name: [] for name, _ in legs}
    norm = None
    for _ in range(rounds):
        for (name, kw), g in zip(legs, graphs):
            settings(**kw)
            w.graph = g
            w.step()                                             # (the switch may refresh the host lr table: not timed)
            torch.cuda.synchronize()
            t[name].append(event_ms(lambda k: w.step(), iters))
            if kw.get("max_grad_norm") == 1e-3:
                norm = w.opt.grad_norm.tolist()
    out.append("2. the captured C4 iteration, bf16, %d clip%s, %d rounds x %d replays" % (batch, "" if batch == 1 else "s", rounds, iters))
    for name, _ in legs:
        out.append("   %-45s %s ms" % (name, fmt(t[name])))
    out.append("   (clip-active leg: last total_norm %.4g, coefficient %.4g)" % (norm[0], norm[1]))
    del w, graphs
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "grad_clip_timing.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--batches", default="1,8")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/clip_bench.py needs a ROCm device")
    dev = torch.device("cuda:0")
    out = ["gradient-norm clipping and the device lr schedule on %s (tools/clip_bench.py): median [min .. max]" % torch.cuda.get_device_name(0)]
    passes(dev, a.rounds, a.iters, out)
    for b in (int(v) for v in a.batches.split(",") if v):
        iteration(dev, b, a.rounds, max(a.iters // 2, 6), out)
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
