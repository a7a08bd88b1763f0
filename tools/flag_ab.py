"""tools/flag_ab.py -- switches of the backbone A/B on the whole C2 step, one / two / three batches in flight, variants interleaved: tools/step_ab.py's
run with three legs and this tool's own line format (profiles/r05_ab_flags.txt).  One positional argument per variant, tools/abkit.py's grammar:
   python tools/flag_ab.py "" "ops.POOL_CONV_MAX_NB=3" "opt:conv_tail=0" """
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import abkit, step_ab  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("variant", nargs="*", type=abkit.Variant.arg, help="comma list of switches / options; \"\" = default")
    a = ap.parse_args()
    variants = a.variant or [abkit.Variant.parse("")]
    n, same, times = step_ab.run(variants, "c2", (1, 2, 3), rounds=5, steps=300)
    for v, (bits, _), t in zip(variants, same, times):
        m = [t[k].median for k in (1, 2, 3)]
        print("%-34s one %.4f ms = %5.0f | two %.4f ms = %5.0f | three %.4f ms = %5.0f clips/s | same bits: %s" % (
            "(default)" if v.text == "default" else v.text, m[0], n / m[0] * 1e3, m[1], n / m[1] * 1e3, m[2], n / m[2] * 1e3, bits))


if __name__ == "__main__":
    main()
