"""tools/bench_with.py -- bench.py under one variant of tools/abkit.py's grammar (module switches, planner options, lib=NAME), A/B aid on the GPU box:

    python tools/bench_with.py backbone.POOL_WITH_POINTWISE=False driver.TUBE_KERNEL=False -- --config c3 --steps 60
    python tools/bench_with.py lib=wgc3 -- --config c4 --dtype bf16          (an experiment build, `make -C step_amd/csrc EXP=wgc3 EXPFLAGS=...`)

Everything after `--` is bench.py's own command line."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import abkit  # noqa: E402


def main():
    argv = sys.argv[1:]
    cut = argv.index("--") if "--" in argv else len(argv)
    ap = argparse.ArgumentParser(usage="bench_with.py [item ...] -- [bench.py's arguments]")
    ap.add_argument("item", nargs="*", help="module.SWITCH=literal, option=value or lib=NAME")
    a = ap.parse_args(argv[:cut])
    try:
        variant = abkit.Variant.parse(",".join(a.item))
    except ValueError as e:
        ap.error(str(e))
    import bench
    sys.argv = ["bench.py"] + argv[cut + 1:]
    with variant.applied():
        bench.main()


if __name__ == "__main__":
    main()
