"""tools/peaks.py -- achievable peaks of the box next to the datasheet values: a device-to-device stream copy
(HBM read + write) and a large bf16 / fp32 GEMM through torch (hipBLASLt / rocBLAS) for the matrix cores."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import abkit  # noqa: E402

dev = torch.device("cuda:0")
timed = lambda fn, n: abkit.event_ms(fn, n, warm=3) * 1e-3       # seconds per call


for mb in (256, 1024, 4096):
    x = torch.empty(mb << 20, dtype=torch.uint8, device=dev)
    y = torch.empty_like(x)
    t = timed(lambda: y.copy_(x), 20)
    print("stream copy %5d MiB: %7.1f GB/s (read + write)" % (mb, 2 * (mb << 20) / t / 1e9))
x = torch.zeros(1 << 30, dtype=torch.uint8, device=dev)
t = timed(lambda: x.zero_(), 20)
print("fill        1024 MiB: %7.1f GB/s (write only)" % ((1 << 30) / t / 1e9))
for dt, n in ((torch.bfloat16, 8192), (torch.float16, 8192), (torch.float32, 8192)):
    a = torch.randn(n, n, device=dev, dtype=dt)
    b = torch.randn(n, n, device=dev, dtype=dt)
    t = timed(lambda: torch.matmul(a, b), 10)
    print("GEMM %s %d^3: %7.1f TFLOP/s" % (str(dt).split(".")[-1], n, 2 * n ** 3 / t / 1e12))
