"""step_sgd_flat beside step_adam_flat on the 44.4 M-element arena of the C4 model (the sizes of tests/kernel_cases.py::big_adam_full_size),
ONE process, the two launches timed alternately: device events around 24 launches each, after a warm-up, five rounds; zero_grad = 1.
Prints bytes moved / time for both (SGD 12 B read + 12 B written per element with the clear, Adam 16 + 16) and one JSON line.

    python tools/sgd_bench.py [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from step_amd import _capi, _lib
from tools import abkit

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--launches", type=int, default=24)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
assert torch.cuda.is_available(), "tools/sgd_bench.py needs a ROCm device"
dev = torch.device("cuda:0")
L = _lib.lib()
sizes = [4_000_000 + 64 * i for i in range(11)]
n = sum(sizes)
torch.manual_seed(0)
P, G = torch.randn(n, device=dev) * 0.05, torch.randn(n, device=dev)
B, M, V = torch.zeros_like(P), torch.zeros_like(P), torch.zeros_like(P)
ends = torch.tensor(np.cumsum(sizes), dtype=torch.int64, device=dev)
LR = torch.tensor([1e-5 * (1 + i % 3) for i in range(len(sizes))], device=dev)
WD = torch.tensor([0.0 if i % 2 else 1e-7 for i in range(len(sizes))], device=dev)
vp = lambda t: ctypes.c_void_p(t.data_ptr())
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
step = [1]


def sgd():
    step[0] += 1
    _capi.check(L.step_sgd_flat(vp(P), vp(G), vp(B), n, vp(ends), vp(LR), vp(WD), len(sizes), 0.9, 0.0, 0, step[0], 1.0, 1, stream), "step_sgd_flat")


def sgd_first():                                             # the first-step form: the buffer is written, not read
    _capi.check(L.step_sgd_flat(vp(P), vp(G), vp(B), n, vp(ends), vp(LR), vp(WD), len(sizes), 0.9, 0.0, 0, 1, 1.0, 1, stream), "step_sgd_flat")


def adam():
    step[0] += 1
    _capi.check(L.step_adam_flat(vp(P), vp(G), vp(M), vp(V), n, vp(ends), vp(LR), vp(WD), len(sizes), 0.9, 0.999, 1e-8, step[0], 1.0, 1, stream),
                "step_adam_flat")


forms = (("sgd", sgd, 24), ("adam", adam, 32), ("sgd_first", sgd_first, 20))
for _, fn, _ in forms:
    for _ in range(5):
        fn()
torch.cuda.synchronize()
us = {k: [] for k, _, _ in forms}
for _ in range(a.rounds):
    for k, fn, _ in forms:
        us[k].append(abkit.event_ms(fn, a.launches) * 1e3)     # us per launch
res = {"elements": n, "launches": a.launches, "rounds": a.rounds}
for k, _, bpe in forms:
    med = float(np.median(us[k]))
    res[k] = {"us": round(med, 1), "us_min": round(min(us[k]), 1), "us_max": round(max(us[k]), 1), "bytes_per_element": bpe,
              "TB_per_s": round(n * bpe / med * 1e-6, 3)}
    print("%-9s %7.1f us (min %.1f, max %.1f)  %2d B/element  %.2f TB/s" % (k, med, min(us[k]), max(us[k]), bpe, n * bpe / med * 1e-6))
res["sgd_over_adam"] = round(res["sgd"]["us"] / res["adam"]["us"], 3)
print(json.dumps(res))
if a.out:
    json.dump(res, open(a.out, "w"), indent=1)
