"""tools/two_in_flight.py -- C2 throughput with ONE captured step replayed back to back against N captured steps (N batches, N streams;
default 2) replayed alternately, so that the tail of one batch's launches overlaps the other's: tools/step_ab.py's run of the default
variant with the legs 1 and N (GPU only, measurement aid).     python tools/two_in_flight.py [N]

It prints ONE line, the median (element len // 2) and the minimum of three rounds of 200 steps per leg.  Before the harness it printed
three lines, one per round, with that round's two raw figures and every batch on a side stream: the lines quoted in DESIGN.md 3.2 and
bench.py's comments are of that form."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import abkit, step_ab  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=int, default=2, help="batches in flight beside the one-batch leg")
    a = ap.parse_args()
    clips, _, (t,) = step_ab.run([abkit.Variant.parse("default")], "c2", (1, a.n), rounds=3, steps=200)
    one, many = t[1], t[a.n]
    print("one batch in flight: %.4f ms/step (min %.4f) = %.0f clips/s | %d in flight: %.4f ms/step (min %.4f) = %.0f clips/s" % (
        one.median, one.min, clips / one.median * 1e3, a.n, many.median, many.min, clips / many.median * 1e3))


if __name__ == "__main__":
    main()
