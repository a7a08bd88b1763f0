"""tools/step_ab.py -- whole-step A/B of library builds, planner options and / or module switches on the C2 (or C5) backbone step, variants
interleaved in ONE process (boxes of the pool differ by 5-10 %: only same-process A/Bs are trusted).

    python tools/step_ab.py --var default --var lib=prev [--var conv_persist=0,lib=prev] [--config c2|c5] [--rounds 5] [--steps 300] [--in-flight 1,2[,3]]

A variant is a comma list (tools/abkit.py has the grammar): `option=value` planner options (step_set_option), `module.SWITCH=literal` module
switches of step_amd and at most one `lib=NAME` (tools/libstep_amd_NAME.so: `prev` from tools/build_prev.sh, experiment builds from
`make -C step_amd/csrc EXP=NAME EXPFLAGS=-D...`); `default` = the working tree's library, default options.  Each variant's step is captured
(HIP graph) once per batch under its own library / options / switches, then the variants' graphs are replayed round-robin: one batch at a
time and two (three) in flight.  Outputs are compared with the first variant's (bit-identity is reported, not required).

This tool also does what tools/plan_ab.py and tools/fuse_ab.py did:
    python tools/plan_ab.py "" "conv_nb_rule=1"    is    python tools/step_ab.py --var default --var conv_nb_rule=1
    python tools/fuse_ab.py                        is    python tools/step_ab.py --var default --var backbone.FUSE_CONV_POOL=False"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import abkit  # noqa: E402

LEG_NAMES = {1: "one", 2: "two", 3: "three"}


def in_flight_arg(text):
    n = tuple(int(v) for v in text.split(","))
    if not n or any(v not in LEG_NAMES for v in n):
        raise argparse.ArgumentTypeError("a comma list of 1, 2, 3")
    return n


def run(variants, config="c2", in_flight=(1, 2), rounds=5, steps=300):
    """-> (clips per step, [same_bits vs the first variant], [{n in flight: abkit.Times}])"""
    import torch

    import bench
    c = bench.CONFIGS[config]
    dev = torch.device("cuda:0")
    tdt = {"bf16": torch.bfloat16, "f16": torch.float16}[c["dtype"]]
    net = bench.build_net(dev)
    xs = [(torch.rand(c["clips"], c["T"], 3, c["HW"], c["HW"]) * 2 - 1).to(dev).to(tdt) for _ in range(max(in_flight))]
    with torch.no_grad():
        net(xs[0])                                               # weight packs (the packed format is the same for every build compared)
    torch.cuda.synchronize()
    return (c["clips"],) + abkit.ab_step(net, xs, variants, in_flight, rounds, steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--var", action="append", default=[], type=abkit.Variant.arg)
    ap.add_argument("--config", default="c2", choices=["c2", "c5"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--in-flight", type=in_flight_arg, default=(1, 2))
    a = ap.parse_args()
    variants = a.var or [abkit.Variant.parse("default"), abkit.Variant.parse("lib=prev")]
    n, same, times = run(variants, a.config, a.in_flight, a.rounds, a.steps)
    for v, (bits, d) in list(zip(variants, same))[1:]:
        print("%-40s vs %-20s bit-identical: %s (max abs diff %.3e)" % (v.text, variants[0].text, bits, d))
    for v, t in zip(variants, times):
        print("%-40s %s" % (v.text, " | ".join("%s %.4f ms (min %.4f) = %5.0f clips/s" % (LEG_NAMES[k], t[k].median, t[k].min, n / t[k].median * 1e3)
                                               for k in a.in_flight)))


if __name__ == "__main__":
    main()
