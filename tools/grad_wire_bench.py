"""The bf16 gradient wire (step_grad_pack16 / step_grad_unpack16, step_amd.dist.GradWire) on ONE GPU, over the arena of the real C4 model:

  1. kernels: pack with a residual, pack without, unpack, and -- for scale -- step_adam_flat_dev over the same arena, alternated in one
     process, device events around blocks of launches (--rounds x --launches >= 200 timed repetitions each, after a warm-up); achieved
     bytes/s from the bytes each pass needs (14 / 6 / 6 / 32 B per element) against the 6.29 TB/s measured copy ceiling of the MI355X;
  2. the step: the C4 training step (bf16 activations, one clip) in a ONE-rank RCCL group with force_exchange=True, captured in the split
     form, fp32 wire against bf16 wire with feedback, interleaved -- the on-GPU cost of the feature when the link is free;
  3. numbers, recorded and not asserted: after 20 eager C4 steps in the one-rank forced exchange, the relative L2 distance of the parameter
     delta to the fp32-wire run, with and without feedback;
  4. a PROJECTION for 8 ranks, labelled as such: halved ring bytes at 153 GB/s per link against the measured pack + unpack time.

    python tools/grad_wire_bench.py [--out profiles/grad_wire_timing.txt]
"""
import argparse
import ctypes
import json
import os
import socket
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.distributed as dist

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "grad_wire_timing.txt"))
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--step-rounds", type=int, default=8)
ap.add_argument("--steps-per-round", type=int, default=10)
ap.add_argument("--numeric-steps", type=int, default=20)
a = ap.parse_args()
assert torch.cuda.is_available(), "tools/grad_wire_bench.py needs a ROCm device"
assert a.launches * a.rounds >= 200, "at least 200 timed repetitions per form"

from step_amd import _capi, _lib, workloads
from step_amd import dist as sdist
from tools import abkit

HBM_COPY_TBPS = 6.29                                             # measured copy ceiling of the MI355X
LINK_GBPS = 153.0                                                # per xGMI link
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
s = socket.socket()
s.bind(("127.0.0.1", 0))
port = s.getsockname()[1]
s.close()
dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1, device_id=dev)      # "nccl" IS RCCL on ROCm
say = abkit.tee(a.out)


def workload(grad_wire, feedback=True, capturable=True):
    torch.manual_seed(7)
    return workloads.C4TrainStep(dev, batch=1, seed=123, dtype=torch.bfloat16, capturable=capturable, force_exchange=True, grad_wire=grad_wire,
                                 wire_feedback=feedback)


# ---- 1. the kernels over the real arena ---------------------------------------------------------------------------------------
w = workload("bf16")
opt, wire = w.opt, w.wire
n = opt.numel
L = _lib.lib()
vp = lambda t: ctypes.c_void_p(t.data_ptr())
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
opt._refresh_tables()
w.forward_backward()                                             # real gradients in the arena
torch.cuda.synchronize()
g_keep = opt.flat_grad.clone()


def pack_res():
    _capi.check(L.step_grad_pack16(_capi.BF16, vp(opt.flat_grad), vp(wire.residual), vp(wire.wire), n, 1.0, stream), "step_grad_pack16")


def pack_plain():
    _capi.check(L.step_grad_pack16(_capi.BF16, vp(opt.flat_grad), None, vp(wire.wire), n, 1.0, stream), "step_grad_pack16")


def unpack():
    _capi.check(L.step_grad_unpack16(_capi.BF16, vp(wire.wire), vp(opt.flat_grad), n, stream), "step_grad_unpack16")


def adam():
    opt._launch(L, 1.0, 1, None)                                 # step_adam_flat_dev, gradient clear in the same pass: 16 B read + 16 B written


forms = (("pack16 + residual", pack_res, 14), ("pack16, no residual", pack_plain, 6), ("unpack16", unpack, 6), ("adam_flat_dev + clear", adam, 32))
for _, fn, _ in forms:
    for _ in range(5):
        fn()
torch.cuda.synchronize()
us = {k: [] for k, _, _ in forms}
for _ in range(a.rounds):
    for k, fn, _ in forms:
        if fn is not adam:
            opt.flat_grad.copy_(g_keep)
        us[k].append(abkit.event_ms(fn, a.launches) * 1e3)       # us per launch
say("bf16 gradient wire over the C4 arena: %d elements (%.1f MB fp32), %d rounds x %d launches per form, alternated, device events" % (n, n * 4e-6, a.rounds, a.launches))
say("%-24s %10s %22s %6s %8s %14s" % ("form", "median us", "min .. max us", "B/el", "TB/s", "of 6.29 TB/s"))
res = {"elements": n, "rounds": a.rounds, "launches": a.launches, "forms": {}}
for k, _, bpe in forms:
    med = float(np.median(us[k]))
    tbps = n * bpe / med * 1e-6
    res["forms"][k] = {"us": med, "us_min": min(us[k]), "us_max": max(us[k]), "bytes_per_element": bpe, "TB_per_s": tbps}
    say("%-24s %10.1f %10.1f .. %-9.1f %6d %8.2f %13.1f%%" % (k, med, min(us[k]), max(us[k]), bpe, tbps, 100 * tbps / HBM_COPY_TBPS))
both = res["forms"]["pack16 + residual"]["us"] + res["forms"]["unpack16"]["us"]
adam_us = res["forms"]["adam_flat_dev + clear"]["us"]
res["pack_plus_unpack_us"], res["adam_us"] = both, adam_us
say("pack + unpack = %.1f us against the Adam launch's %.1f us (20 B against 32 B per element): %s"
    % (both, adam_us, "no longer than Adam, as the bytes say" if both <= adam_us else "LONGER than Adam -- the vector path wants a look"))
w.reducer.close()
del w, opt, wire, g_keep
torch.cuda.empty_cache()

# ---- 2. the captured step, fp32 wire against bf16 wire, one-rank forced exchange, split form ------------------------------------------
ws = {"fp32": workload("fp32"), "bf16": workload("bf16")}
for k, wk in ws.items():
    wk.capture(warmup=2, mode="split")
    assert wk.graph_mode == "split" and (wk.wire is not None) == (k == "bf16")
for wk in ws.values():
    for _ in range(3):
        wk.step()
torch.cuda.synchronize()
ms = {k: [] for k in ws}
for _ in range(a.step_rounds):
    for k, wk in ws.items():
        ms[k].append(abkit.wall_ms(wk.step, a.steps_per_round))
say()
say("C4 step, bf16 activations, one clip, one-rank RCCL group with the exchange forced, split form (graph, eager flat all-reduce, graph);")
say("%d rounds x %d steps per wire, interleaved, host clock around synchronised blocks:" % (a.step_rounds, a.steps_per_round))
res["step_ms"] = {}
for k in ws:
    med = float(np.median(ms[k]))
    res["step_ms"][k] = {"ms": med, "min": min(ms[k]), "max": max(ms[k])}
    say("  %s wire   %.3f ms per step (min %.3f, max %.3f)" % (k, med, min(ms[k]), max(ms[k])))
d_ms = res["step_ms"]["bf16"]["ms"] - res["step_ms"]["fp32"]["ms"]
res["step_ms"]["bf16_minus_fp32"] = d_ms
say("  bf16 - fp32 = %+.3f ms per step with the link free (the fp32 form's own spread: %.3f ms); pack + unpack alone: %.3f ms, the other %+.3f ms are not attributed by this tool"
    % (d_ms, res["step_ms"]["fp32"]["max"] - res["step_ms"]["fp32"]["min"], both * 1e-3, d_ms - both * 1e-3))
for wk in ws.values():
    wk.reducer.close()
del ws, wk
torch.cuda.empty_cache()

# ---- 3. what the rounding does to the trajectory (recorded, not asserted) ---------------------------------------------------------------
deltas = {}
for k, (gw, fb) in (("fp32", ("fp32", True)), ("bf16 + feedback", ("bf16", True)), ("bf16, no feedback", ("bf16", False))):
    wk = workload(gw, fb, capturable=False)
    p0 = wk.opt.flat_param.clone()
    for _ in range(a.numeric_steps):
        wk.step()
    torch.cuda.synchronize()
    deltas[k] = (wk.opt.flat_param - p0).double().cpu().numpy()
    wk.reducer.close()
    del wk, p0
    torch.cuda.empty_cache()
say()
say("%d eager C4 steps (Adam, lr 1e-5) in the one-rank forced exchange: relative L2 distance of the parameter delta to the fp32-wire run" % a.numeric_steps)
res["delta_rel"] = {}
for k in ("bf16 + feedback", "bf16, no feedback"):
    rel = float(np.linalg.norm(deltas[k] - deltas["fp32"]) / np.linalg.norm(deltas["fp32"]))
    res["delta_rel"][k] = rel
    say("  %-18s %.3e" % (k, rel))

# ---- 4. projection ------------------------------------------------------------------------------------------------------------------
ring = lambda nbytes, ranks: 2.0 * (ranks - 1) / ranks * nbytes / (LINK_GBPS * 1e9) * 1e3      # ms: reduce-scatter + all-gather, per-link bound
r32, r16 = ring(n * 4, 8), ring(n * 2, 8)
res["projection_8_ranks_ms"] = {"fp32_ring": r32, "bf16_ring": r16, "pack_plus_unpack": both * 1e-3}
say()
say("PROJECTION (not measured: one GPU here), 8 ranks, ring all-reduce at %.0f GB/s per link:" % LINK_GBPS)
say("  fp32 ring %.2f ms, bf16 ring %.2f ms: %.2f ms less on the link per step, against %.3f ms of pack + unpack measured above"
    % (r32, r16, r32 - r16, both * 1e-3))
say("  (both run bucket by bucket on the communication stream under backward; the projection compares totals, not what stays exposed)")
say(json.dumps(res))
say.close()
dist.barrier()
dist.destroy_process_group()
