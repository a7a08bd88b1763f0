"""tools/skip_probe.py -- UPPER BOUND of what fusing a stand-alone pool into its producer could buy: the C2 step with maxPool3d_3a and / or
maxPool3d_4a simply NOT LAUNCHED (their consumers read a stale buffer of the right shape: wrong results, right timing of everything
else), one batch at a time and two batches in flight, variants interleaved.  Measurement aid, GPU only.  The patching of the net is this
tool's own; capture, replay and statistics are tools/abkit.py's."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from tools import abkit  # noqa: E402

ROUNDS, STEPS = 4, 300


def main():
    dev = torch.device("cuda:0")
    net = bench.build_net(dev)
    xs = [(torch.rand(8, 32, 3, 224, 224) * 2 - 1).to(dev).to(torch.bfloat16) for _ in range(2)]
    streams = abkit.streams(2)
    variants = {"baseline": (), "no_pool3a": (4,), "no_pool4a": (7,), "no_pool3a_4a": (4, 7)}
    caps = {}
    with torch.no_grad():
        # the pooled shapes, once
        keep = {}
        hooks = [net.base_model[i].register_forward_hook(lambda m, a, o, i=i: keep.__setitem__(i, o.detach().clone())) for i in (4, 7)]
        net(xs[0])
        for h in hooks:
            h.remove()
        torch.cuda.synchronize()
    orig = {i: net.base_model[i].forward for i in (4, 7)}
    try:
        for name, skip in variants.items():
            for i in (4, 7):
                net.base_model[i].forward = (lambda x, i=i: keep[i]) if i in skip else orig[i]
            caps[name] = abkit.capture_step(net, xs, streams)[0]
    finally:
        for i in (4, 7):
            net.base_model[i].forward = orig[i]
    torch.cuda.synchronize()
    legs = {n: (lambda v, n=n: abkit.replay_ms(caps[v], streams, n, STEPS)) for n in (1, 2)}
    for v, t in zip(caps, abkit.interleave(list(caps), legs, ROUNDS)):
        a, b = t[1].median, t[2].median
        print("%-16s one %.4f ms = %5.0f clips/s | two %.4f ms = %5.0f clips/s" % (v, a, 8 / a * 1e3, b, 8 / b * 1e3))


if __name__ == "__main__":
    main()
