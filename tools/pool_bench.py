"""tools/pool_bench.py -- the max pools of the C2 backbone (and the AVA-shaped maps with --set c3) one by one: us per launch and
algorithmic GB/s (input + output bytes); then branch_3 of Mixed_3b / 3c as pool + pointwise conv in two launches against the one launch
that never writes the pooled tensor (ops.pool_then_conv_forward).  GPU only, tuning aid."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from step_amd import _capi, _lib, ops  # noqa: E402
from tools import abkit  # noqa: E402

# (name, C, D, H, W, kernel, stride) per clip
C2 = [("pool2a", 64, 16, 112, 112, (1, 3, 3), (1, 2, 2)), ("pool3a", 192, 16, 56, 56, (1, 3, 3), (1, 2, 2)),
      ("3b_pool", 192, 16, 28, 28, (3, 3, 3), (1, 1, 1)), ("3c_pool", 256, 16, 28, 28, (3, 3, 3), (1, 1, 1)),
      ("pool4a", 480, 16, 28, 28, (3, 3, 3), (2, 2, 2)),
      ("4b_pool", 480, 8, 14, 14, (3, 3, 3), (1, 1, 1)), ("4c_pool", 512, 8, 14, 14, (3, 3, 3), (1, 1, 1)),
      ("4f_pool", 528, 8, 14, 14, (3, 3, 3), (1, 1, 1))]
C3 = [("pool2a", 64, 18, 200, 200, (1, 3, 3), (1, 2, 2)), ("pool3a", 192, 18, 100, 100, (1, 3, 3), (1, 2, 2)),
      ("3b_pool", 192, 18, 50, 50, (3, 3, 3), (1, 1, 1)), ("3c_pool", 256, 18, 50, 50, (3, 3, 3), (1, 1, 1)),
      ("pool4a", 480, 18, 50, 50, (3, 3, 3), (2, 2, 2)), ("4b_pool", 480, 9, 25, 25, (3, 3, 3), (1, 1, 1)),
      ("4f_pool", 528, 9, 25, 25, (3, 3, 3), (1, 1, 1))]


# branch_3 of the 28x28 / 50x50 blocks: (name, Cin, Cout, D, H, W) per clip
B3 = {"c2": [("3b_b3", 192, 32, 16, 28, 28), ("3c_b3", 256, 64, 16, 28, 28)],
      "c3": [("3b_b3", 192, 32, 18, 50, 50), ("3c_b3", 256, 64, 18, 50, 50)]}


def branch3(a, dev):
    bf = torch.bfloat16
    timed = lambda fn, iters: abkit.event_ms(fn, iters, warm=3) * 1e3          # us per launch
    for name, Cin, Cout, D, H, W in B3[a.set]:
        x = torch.randn(a.batch, D, H, W, Cin, device=dev).to(bf)
        w = ops.pack_conv_weight(torch.randn(Cout, Cin, 1, 1, 1, device=dev) / Cin ** 0.5, bf)
        sc, sh = torch.rand(Cout, device=dev) + 0.5, torch.randn(Cout, device=dev)
        p, y0, y1 = torch.empty_like(x), torch.empty(a.batch, D, H, W, Cout, device=dev, dtype=bf), torch.empty(a.batch, D, H, W, Cout, device=dev, dtype=bf)
        t_pool = timed(lambda: ops.maxpool_tf(x, (3, 3, 3), (1, 1, 1), p), a.iters)
        t_conv = timed(lambda: ops.conv_forward(p, w, Cout, (1, 1, 1), sc, sh, True, None, y0), a.iters)
        with _capi.options(_lib.lib(), pool_then_conv=2):
            ran = ops.pool_then_conv_forward(x, w, Cout, sc, sh, True, y1) is not None
            t_one = timed(lambda: ops.pool_then_conv_forward(x, w, Cout, sc, sh, True, y1), a.iters) if ran else float("nan")
        print("%-6s %3d -> %2d %2dx%2dx%2d  pool %6.1f us + conv %6.1f us = %6.1f us | one launch %6.1f us  (%5.0f GB/s of x + y)  identical %s" % (
            name, Cin, Cout, D, H, W, t_pool, t_conv, t_pool + t_conv, t_one, (x.numel() + y1.numel()) * 2 / t_one * 1e-3, bool(ran and torch.equal(y0, y1))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--set", default="c2")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--lib", default=None, help="NAME: time the experiment build NAME (abkit.load_build: make -C step_amd/csrc EXP=NAME EXPFLAGS=-D...)")
    ap.add_argument("--branch3-only", action="store_true")
    a = ap.parse_args()
    with _lib.use(abkit.load_build(a.lib) if a.lib else _lib.lib()):
        dev = torch.device("cuda:0")
        tot = 0.0
        for name, C, D, H, W, k, s in ([] if a.branch3_only else C2 if a.set == "c2" else C3):
            x = torch.randn(a.batch, D, H, W, C, device=dev).to(torch.bfloat16)
            y = ops.maxpool_tf(x, k, s)
            us = abkit.event_ms(lambda: ops.maxpool_tf(x, k, s, y), a.iters, warm=3) * 1e3
            tot += us
            print("%-8s C=%3d %2dx%3dx%3d k%s s%s  %7.1f us  %6.0f GB/s" % (name, C, D, H, W, "".join(map(str, k)), "".join(map(str, s)), us,
                                                                        (x.numel() + y.numel()) * 2 / us * 1e-3))
        print("total %.1f us" % tot)
        branch3(a, dev)


if __name__ == "__main__":
    main()
